"""ocrfdet_amd — MI355X (gfx950) implementation of OcRFDet's OcRF-render + BEV-pool + HOA hot path.

Drop-in mirrors of the reference's Python surface for that path (and nothing else):

  ==============================================  =================================================
  reference import                                here
  ==============================================  =================================================
  mmdet3d.ops.bev_pool_v2.bev_pool                ocrfdet_amd.bevpool
  diff_gaussian_rasterization (w-depth fork)      ocrfdet_amd.diff_gaussian_rasterization
  ...MVSGaussian.lib.gaussian_renderer.render     ocrfdet_amd.gaussian_renderer.render
  HOA blocks of view_transformer_ocrf.py          ocrfdet_amd.hoa
  index preparation of view_transformer(_ocrf)    ocrfdet_amd.index_prep
  ...necks.view_transformer_ocrf                  ocrfdet_amd.view_transformer_ocrf (OcRFViewTransformerFull
                                                  and its sub-modules; kernels: ocrfdet_amd.neck_ops)
  ...backbones.resnet.CustomResNet,               ocrfdet_amd.bev_encoder (CustomResNet, FPN_LSS, BEVEncoder,
  ...necks.lss_fpn.FPN_LSS                        build_pre_process)
  mmdet ResNet, ...necks.fpn.CustomFPN,           ocrfdet_amd.image_encoder (ResNet, CustomFPN, ImageEncoder, also
  BEVDet.image_encoder                            exported here)
  mmdet BasicBlock / Bottleneck, mmcv ConvModule, ocrfdet_amd.blocks (shared by the two encoders, depthnet and
  build_norm_layer, kaiming_init                  center_head)
  (the encoders' fused passes between             ocrfdet_amd.plane_ops (add_relu, upsample_add, upsample_cat;
  convolutions)                                   re-exported by the encoder modules)
  nn.BatchNorm2d + ReLU (+ the residual           ocrfdet_amd.norm_ops (bn_act, bn_act_torch, bn_act_fusable; opt-in
  addition) inside the blocks                     through blocks.fuse_norms)
  BEVDet4D.gen_grid / shift_feature and the       ocrfdet_amd.temporal (feature_transform, shift_feature,
  cat of the aligned frames                       align_and_cat, gen_grid, shift_feature_method, also
                                                  exported here)
  torch.optim.AdamW + clip_grad_norm_ (mmcv's     ocrfdet_amd.optim (FusedAdamW, ModelEMA, paramwise_groups, also
  grad_clip), ...core.hook.ema.ModelEMA, mmcv's   exported here)
  DefaultOptimizerConstructor custom_keys
  ...detectors.ocrfdet.OcRFDet4D and              ocrfdet_amd.detector (OcRFDet4D, prepare_inputs, frame_poses,
  BEVDet4D.prepare_inputs                         frame_poses_torch, also exported here)
  (none: the reference's sequential test cannot   ocrfdet_amd.streaming (stream_step, StreamState, key_frame_inputs;
  run)                                            OcRFDet4D.stream_step / simple_test_stream) over
                                                  temporal.stream_align / stream_align_torch
  ...datasets.pipelines.loading                   ocrfdet_amd.inputs (sample_augmentation, post_homography,
  PrepareImageInputs (image and point-label       sample_bda_augmentation, bev_transform, assemble_img_inputs,
  stage), LoadAnnotationsBEVDepth.bev_transform   prepare_images, point_label_maps and their *_torch forms, also
                                                  exported here)
  mmcv.ops DeformConv2d, DeformConv2dPack         ocrfdet_amd.deform_conv (deform_conv2d, deform_conv2d_torch,
  (type 'DCN'), deform_conv2d                     DeformConv2d, DeformConv2dPack, build_dcn; opt-in in depthnet
                                                  through NATIVE_DCN, in center_head through DCNSeparateHead)
  ...detectors.ocrfdet_vggt.OcRFDet4DVGGT,        ocrfdet_amd.detector.OcRFDet4DVGGT and ocrfdet_amd.distill
  ...detectors.bevdet_vggt.CrossAttentionAlign    (build_cost_volume, group_corr_volume, group_corr_volume_torch,
                                                  kd_losses, kd_losses_torch, CrossAttentionAlign, resize_img,
                                                  get_pair_indices; the VGGT teacher itself is passed in)
  ...datasets.nuscenes_dataset                    ocrfdet_amd.detection_eval (EvalConfig, DetectionEval,
  NuScenesDataset.evaluate (the metrics, not the  evaluate_host, evaluate_stream; OcRFDet4D.evaluate_stream): AP,
  devkit's JSON submission)                       the TP errors, mAP and NDS from padded device tensors
  ==============================================  =================================================

Every op calls the C ABI of ``csrc/libocrf_hip.so`` (``include/ocrf_hip.h``) through ctypes with
raw device pointers; PyTorch is only the allocator / stream / ``torch.distributed`` provider.
"""
from . import _lib  # noqa: F401

__version__ = "0.1.0"
_LAZY = ('ResNet', 'CustomFPN', 'ImageEncoder')
_LAZY_TEMPORAL = ('feature_transform', 'shift_feature', 'shift_feature_torch', 'align_and_cat', 'gen_grid',
                  'shift_feature_method', 'stream_align', 'stream_align_torch')
_LAZY_OPTIM = ('FusedAdamW', 'ModelEMA', 'paramwise_groups')
_LAZY_DETECTOR = ('OcRFDet4D', 'OcRFDet4DVGGT', 'prepare_inputs', 'frame_poses', 'frame_poses_torch')
_LAZY_DISTILL = ('build_cost_volume', 'group_corr_volume', 'group_corr_volume_torch', 'kd_losses', 'kd_losses_torch',
                 'CrossAttentionAlign')
_LAZY_STREAMING = ('StreamState', 'stream_step', 'key_frame_inputs')
_LAZY_INPUTS = ('sample_augmentation', 'post_homography', 'sample_bda_augmentation', 'bev_transform',
                'assemble_img_inputs', 'prepare_images', 'prepare_images_torch', 'point_label_maps',
                'point_label_maps_torch')


def __getattr__(name):
    """``ocrfdet_amd.ResNet`` / ``CustomFPN`` / ``ImageEncoder``: the classes of ``ocrfdet_amd.image_encoder``, imported
    on first use, and the functions of ``ocrfdet_amd.temporal`` and the names of ``ocrfdet_amd.optim`` likewise.  There
    is no ``__all__``: ``from ocrfdet_amd import *`` yields what it yielded before."""
    if name in _LAZY:
        from . import image_encoder
        return getattr(image_encoder, name)
    if name in _LAZY_TEMPORAL:
        from . import temporal
        return getattr(temporal, name)
    if name in _LAZY_OPTIM:
        from . import optim
        return getattr(optim, name)
    if name in _LAZY_DETECTOR:
        from . import detector
        return getattr(detector, name)
    if name in _LAZY_DISTILL:
        from . import distill
        return getattr(distill, name)
    if name in _LAZY_STREAMING:
        from . import streaming
        return getattr(streaming, name)
    if name in _LAZY_INPUTS:
        from . import inputs
        return getattr(inputs, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
