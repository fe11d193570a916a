"""The detector: ``OcRFDet4D`` (mmdet3d/models/detectors/ocrfdet.py:141-386), a ``BEVStereo4D`` / ``BEVDet4D``
(bevdet.py:274-723), over this package's native modules, without mmcv, mmdet or mmdet3d.

* ``frame_poses_torch`` / ``frame_poses``: the pose algebra of ``BEVDet4D.prepare_inputs`` (bevdet.py:435-456) and the
  per-frame ``get_mlp_input`` of ``extract_img_feat`` (ocrfdet.py:229-231).  The reference runs two ``torch.inverse``
  calls on float64 4 x 4 stacks (a host synchronisation each) and one ``get_mlp_input`` per frame.  Here the same
  products are evaluated in float64 with the inverses in closed form (affine maps: adjugate / determinant of the 3 x 3
  block, as ``temporal._inverse3``), without a host read; on CUDA float32 inputs as ONE launch
  (``ocrf_frame_poses``, ``csrc/frame_poses.hip``).
* ``prepare_inputs``: ``BEVDet4D.prepare_inputs`` (bevdet.py:412-476) as a function: the 12-entry ``img_inputs`` split
  into per-frame lists.
* ``OcRFDet4D``: the class.  Constructor keys, attribute names and ``state_dict`` keys are the reference's.

**Precondition:** ``sensor2egos`` and ``ego2globals`` have the last row (0, 0, 0, 1), as the dataset's always have.  It
is not checked: a check would synchronise.  Nothing assumes an orthonormal rotation; a singular matrix gives inf / nan.

Out of scope: mmcv's ``Config`` and registries, ``DataContainer`` unwrapping, ``train_step``, the dataset pipeline,
``grid_mask``, ``extract_img_feat_sequential`` and ``pred_prev`` (both raise ``NotImplementedError``: neither can run in
the reference; streaming inference has its own names, ``OcRFDet4D.stream_step`` / ``simple_test_stream``,
``ocrfdet_amd/streaming.py``).
"""
import contextlib

import torch
from torch import nn

from . import _lib, temporal
from .blocks import build
from .temporal import _affine_inverse

LOSS_KEYS_NECK = ('loss_depth', 'loss_ce_semantic', 'loss_gs_color', 'loss_gs_ssim', 'loss_render_depth')


# ------------------------------------------------------------------------------------------------ frame poses
def mlp_input_torch(rots, trans, intrins, post_rots, post_trans, bda):
    """(F, B, N, 27): for every frame f what ``get_mlp_input(rots[:, 0], trans[:, 0], intrins[:, f], post_rots[:, f],
    post_trans[:, f], bda)`` returns (view_transformer.py:696-722), from (B, F, N, ...) inputs.  Copies only."""
    B, F, N = rots.shape[:3]
    a = bda.view(B, 1, 1, 3, 3).expand(B, F, N, 3, 3)
    v = torch.stack([intrins[..., 0, 0], intrins[..., 1, 1], intrins[..., 0, 2], intrins[..., 1, 2],
                     post_rots[..., 0, 0], post_rots[..., 0, 1], post_trans[..., 0], post_rots[..., 1, 0],
                     post_rots[..., 1, 1], post_trans[..., 1], a[..., 0, 0], a[..., 0, 1], a[..., 1, 0], a[..., 1, 1],
                     a[..., 2, 2]], dim=-1)
    s2e = torch.cat([rots[:, 0], trans[:, 0].reshape(B, N, 3, 1)], dim=-1).reshape(B, 1, N, 12).expand(B, F, N, 12)
    return torch.cat([v, s2e], dim=-1).permute(1, 0, 2, 3).contiguous()


def _check_pose_shapes(sensor2egos, ego2globals, rots, trans, intrins, post_rots, post_trans, bda, temporal_frame):
    if sensor2egos.dim() != 5 or sensor2egos.shape[-2:] != (4, 4):
        raise ValueError(f'sensor2egos must be (B, F, N, 4, 4), got {tuple(sensor2egos.shape)}')
    B, F, N = sensor2egos.shape[:3]
    want = dict(ego2globals=(B, F, N, 4, 4), rots=(B, F, N, 3, 3), trans=(B, F, N, 3), intrins=(B, F, N, 3, 3),
                post_rots=(B, F, N, 3, 3), post_trans=(B, F, N, 3), bda=(B, 3, 3))
    got = dict(ego2globals=ego2globals, rots=rots, trans=trans, intrins=intrins, post_rots=post_rots,
               post_trans=post_trans, bda=bda)
    for name, shape in want.items():
        if tuple(got[name].shape) != shape:
            raise ValueError(f'{name} must be {shape}, got {tuple(got[name].shape)}')
    if not 0 <= int(temporal_frame) < F:
        raise ValueError(f'temporal_frame must be in [0, {F}), got {temporal_frame}')
    return B, F, N


def frame_poses_torch(sensor2egos, ego2globals, rots, trans, intrins, post_rots, post_trans, bda, temporal_frame):
    """The frame poses in torch, on any device, for any floating dtype; differentiable, no ``torch.inverse``, no host
    read.  Inputs (B, F, N, ...) as ``include/ocrf_hip.h`` lists them; ``T = temporal_frame``.  Returns

    * ``sensor2keyegos`` (B, F, N, 4, 4) = inv(ego2globals[:, 0, 0]) . ego2globals . sensor2egos,
    * ``curr2adjsensor`` (B, T, N, 4, 4) = inv(ego2globals[:, 1:T+1] . sensor2egos[:, 1:T+1]) . ego2globals[:, :T] .
      sensor2egos[:, :T], or None when T = 0,
    * ``mlp_input`` (F, B, N, 27) (``mlp_input_torch``),

    the products evaluated in float64 and rounded once to the dtype of ``sensor2egos``."""
    T = int(temporal_frame)
    _check_pose_shapes(sensor2egos, ego2globals, rots, trans, intrins, post_rots, post_trans, bda, T)
    dtype = sensor2egos.dtype
    e2g, s2e = ego2globals.double(), sensor2egos.double()
    sensor2global = e2g @ s2e
    global2keyego = _affine_inverse(e2g[:, 0, 0])[:, None, None]
    sensor2keyegos = (global2keyego @ sensor2global).to(dtype)
    curr2adjsensor = None
    if T > 0:
        curr2adjsensor = (_affine_inverse(sensor2global[:, 1:T + 1]) @ sensor2global[:, :T]).to(dtype)
    return sensor2keyegos, curr2adjsensor, mlp_input_torch(rots, trans, intrins, post_rots, post_trans, bda)


def frame_poses_fusable(*tensors):
    """The kernel takes these: CUDA float32 tensors on one device, none of which records a gradient."""
    dev = tensors[0].device
    return all(t.is_cuda and t.dtype == torch.float32 and t.device == dev
               and not (t.requires_grad and torch.is_grad_enabled()) for t in tensors)


def frame_poses(sensor2egos, ego2globals, rots, trans, intrins, post_rots, post_trans, bda, temporal_frame, fused=True):
    """``frame_poses_torch`` with a dispatch: CUDA float32 inputs with ``fused=True`` take ``ocrf_frame_poses``, one
    launch without a host read (the outputs get no gradient); everything else, the CPU included, the torch formulation.
    The two agree within one float32 ulp in the poses (both round a float64 result once) and bit for bit in
    ``mlp_input``."""
    tensors = (sensor2egos, ego2globals, rots, trans, intrins, post_rots, post_trans, bda)
    if not (fused and frame_poses_fusable(*tensors)):
        return frame_poses_torch(*tensors, temporal_frame)
    T = int(temporal_frame)
    B, F, N = _check_pose_shapes(*tensors, T)
    tensors = [t.detach().contiguous() for t in tensors]
    dev = sensor2egos.device
    sensor2keyegos = torch.empty(B, F, N, 4, 4, dtype=torch.float32, device=dev)
    curr2adjsensor = torch.empty(B, T, N, 4, 4, dtype=torch.float32, device=dev) if T > 0 else None
    mlp_input = torch.empty(F, B, N, 27, dtype=torch.float32, device=dev)
    _lib.launch('ocrf_frame_poses', dev, B, F, N, T, *tensors, sensor2keyegos, curr2adjsensor, mlp_input)
    return sensor2keyegos, curr2adjsensor, mlp_input


# ------------------------------------------------------------------------------------------------ prepare_inputs
def _frames(t):
    return list(t.unbind(1))


def frame_split(inputs, num_frame):
    """(B, N) of a 12-entry ``img_inputs`` whose images (B, N * num_frame, ...) are ``num_frame`` frames of N cameras."""
    if len(inputs) != 12:
        raise ValueError(f'img_inputs has 12 entries, got {len(inputs)}')
    B, NF = inputs[0].shape[:2]
    if NF % num_frame:
        raise ValueError(f'{NF} images are not {num_frame} frames of the same cameras')
    return B, NF // num_frame


def prepare_inputs(inputs, num_frame, temporal_frame, extra_ref_frames, stereo=True, fused=True):
    """``BEVDet4D.prepare_inputs`` (bevdet.py:412-476) for the 12-entry ``img_inputs`` = (imgs (B, N * num_frame, C, H,
    W), rots, trans, intrins, post_rots, post_trans, bda, sensor2egos, ego2globals, imgs_wo_norm, imgs_wo_aug, c2w).
    Returns a pair:

    * the reference's 13-tuple ``(imgs, rots, trans, intrins, post_rots, post_trans, bda, sensor2keyegos, ego2globals,
      curr2adjsensor, imgs_wo_norm, imgs_wo_aug, c2w)``: every entry but ``bda`` a list over the frames;
      ``curr2adjsensor`` holds ``temporal_frame`` poses and ``extra_ref_frames`` times ``None`` (``stereo=True``), or is
      ``None`` (``stereo=False``);
    * the list over the frames of ``mlp_input`` (B, N, 27), what ``extract_img_feat`` gets from ``get_mlp_input``.

    The poses come from ``frame_poses(..., fused=fused)``."""
    B, N = frame_split(inputs, num_frame)
    C, H, W = inputs[0].shape[2:]
    imgs = _frames(inputs[0].view(B, N, num_frame, C, H, W).transpose(1, 2))
    rots, trans, intrins, post_rots, post_trans, bda, sensor2egos, ego2globals = inputs[1:9]
    imgs_wo_norm = _frames(inputs[9].view(B, N, num_frame, 3, H, W).transpose(1, 2))
    imgs_wo_aug = _frames(inputs[10].view(B, N, num_frame, 3, H, W).transpose(1, 2))
    sensor2egos = sensor2egos.view(B, num_frame, N, 4, 4)
    ego2globals = ego2globals.view(B, num_frame, N, 4, 4)
    rots, intrins, post_rots = (t.view(B, num_frame, N, 3, 3) for t in (rots, intrins, post_rots))
    trans, post_trans = (t.view(B, num_frame, N, 3) for t in (trans, post_trans))
    c2w = inputs[11].view(B, num_frame, N, 4, 4)
    T = temporal_frame if stereo else 0
    sensor2keyegos, curr2adj, mlp_input = frame_poses(sensor2egos, ego2globals, rots, trans, intrins, post_rots,
                                                      post_trans, bda, T, fused=fused)
    curr2adjsensor = None
    if stereo:
        curr2adjsensor = _frames(curr2adj) + [None] * extra_ref_frames
        assert len(curr2adjsensor) == num_frame
    out = (imgs, _frames(rots), _frames(trans), _frames(intrins), _frames(post_rots), _frames(post_trans), bda,
           _frames(sensor2keyegos), _frames(ego2globals), curr2adjsensor, imgs_wo_norm, imgs_wo_aug, _frames(c2w))
    return out, list(mlp_input.unbind(0))


# ------------------------------------------------------------------------------------------------ the detector
def _build(cfg, kind, factory):
    """A sub-module from its config dict, or the module itself when it is already built."""
    if cfg is None or isinstance(cfg, nn.Module):
        return cfg
    return build(cfg, kind, factory)


def _pts(cfg):
    """``train_cfg.pts`` / ``test_cfg.pts`` of a config (a dict, or anything with a ``pts`` attribute)."""
    if cfg is None:
        return None
    return cfg.get('pts') if isinstance(cfg, dict) else getattr(cfg, 'pts', None)


class OcRFDet4D(nn.Module):
    """``OcRFDet4D`` of the reference config (configs/ocrfdet/ocrfdet.py:44-154): ResNet + CustomFPN, the stereo
    ``OcRFViewTransformerFull``, ``pre_process``, the BEV encoder and ``CenterHead``, with the reference's constructor
    keys, attribute names (``img_backbone``, ``img_neck``, ``img_view_transformer``, ``img_bev_encoder_backbone``,
    ``img_bev_encoder_neck``, ``pre_process_net``, ``pts_bbox_head``) and therefore ``state_dict`` keys.

    Every sub-module is built from its config dict by this package's class of the dict's ``type``, or taken as it is
    when an ``nn.Module`` is passed.  ``train_cfg.pts`` and ``test_cfg.pts`` are merged into the head's dict, as the
    reference's ``MVXTwoStageDetector`` does.

    ``fused_poses`` (class attribute, default True): the frame poses and ``mlp_input`` of a forward come from one HIP
    launch when ``img_inputs`` is on the GPU; False takes ``frame_poses_torch``.  ``fused_align`` (default
    ``temporal.FUSED_ALIGN_DEFAULT``) is ``align_and_cat``'s flag.  ``bf16_inference()`` is the one switch for bfloat16
    inference: autocast plus the three bf16 opt-ins of the sub-modules, restored on exit."""

    fused_poses = True
    fused_align = None
    autocast_bf16 = False            # BEVEncoder's opt-in; False is the reference's @force_fp32

    def __init__(self, img_view_transformer, img_backbone=None, img_neck=None, img_bev_encoder_backbone=None,
                 img_bev_encoder_neck=None, pre_process=None, pts_bbox_head=None, num_adj=1,
                 align_after_view_transfromation=False, with_prev=True, train_cfg=None, test_cfg=None,
                 use_grid_mask=False, pretrained=None, init_cfg=None, type=None):
        super().__init__()
        if type not in (None, 'OcRFDet4D'):
            raise NotImplementedError(f'type {type}: only OcRFDet4D')
        if use_grid_mask:
            raise NotImplementedError('use_grid_mask: GridMask is not part of this package')
        from .bev_encoder import CustomResNet, FPN_LSS
        from .center_head import CenterHead
        from .image_encoder import CustomFPN, ResNet
        from .view_transformer_ocrf import OcRFViewTransformerFull
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.img_backbone = _build(img_backbone, 'ResNet', ResNet)
        if img_neck is not None:
            self.img_neck = _build(img_neck, 'CustomFPN', CustomFPN)
        self.img_view_transformer = _build(img_view_transformer, 'OcRFViewTransformerFull', OcRFViewTransformerFull)
        if img_bev_encoder_neck is not None and img_bev_encoder_backbone is not None:
            self.img_bev_encoder_backbone = _build(img_bev_encoder_backbone, 'CustomResNet', CustomResNet)
            self.img_bev_encoder_neck = _build(img_bev_encoder_neck, 'FPN_LSS', FPN_LSS)
        self.pre_process = pre_process is not None
        if self.pre_process:
            self.pre_process_net = _build(pre_process, 'CustomResNet', CustomResNet)
        if pts_bbox_head is not None:
            if isinstance(pts_bbox_head, dict):
                pts_bbox_head = dict(pts_bbox_head, train_cfg=_pts(train_cfg), test_cfg=_pts(test_cfg))
            self.pts_bbox_head = _build(pts_bbox_head, 'CenterHead', CenterHead)
        self.align_after_view_transfromation = align_after_view_transfromation
        self.with_prev = with_prev
        # BEVDet4D.__init__ (bevdet.py:300) and BEVStereo4D.__init__ (:596-598)
        self.num_frame = num_adj + 1
        self.extra_ref_frames = 1
        self.temporal_frame = self.num_frame
        self.num_frame += self.extra_ref_frames

    @property
    def with_img_neck(self):
        return getattr(self, 'img_neck', None) is not None

    @property
    def with_pts_bbox(self):
        return getattr(self, 'pts_bbox_head', None) is not None

    # ---------------------------------------------------------------- the stages: this package's native formulations
    def image_encoder(self, img, stereo=False):
        """``BEVDet.image_encoder`` (bevdet.py:44-64, no ``grid_mask``): ``ImageEncoder.image_encoder`` over this
        module's ``img_backbone`` / ``img_neck``."""
        from .image_encoder import ImageEncoder
        return ImageEncoder.image_encoder(self, img, stereo=stereo)

    def extract_stereo_ref_feat(self, x):
        """``BEVStereo4D.extract_stereo_ref_feat`` (bevdet.py:600-614) for a ResNet: the stem and ``layer1``."""
        from .image_encoder import ImageEncoder
        return ImageEncoder.extract_stereo_ref_feat(self, x)

    def bev_encoder(self, x):
        """``BEVDet.bev_encoder`` (bevdet.py:66-72): ``BEVEncoder.forward`` over this module's two attributes."""
        from .bev_encoder import BEVEncoder
        return BEVEncoder.forward(self, x)

    def prepare_inputs(self, inputs, stereo=False):
        return prepare_inputs(inputs, self.num_frame, self.temporal_frame, self.extra_ref_frames, stereo=stereo,
                              fused=self.fused_poses)

    # ---------------------------------------------------------------- bfloat16 inference
    @contextlib.contextmanager
    def bf16_inference(self):
        """bfloat16 inference on fused kernels from the images to the boxes: enters
        ``torch.autocast('cuda', dtype=torch.bfloat16)`` and turns on, where the sub-modules exist, ``self.autocast_bf16``
        (the BEV encoder stays bfloat16), ``img_view_transformer.depth_net.fused_cost_volume_bf16`` on that instance (the
        stereo cost volume reads bfloat16 features) and ``pts_bbox_head.fused_decode_bf16`` (the decode reads the
        bfloat16 head outputs in place).  All three are put back on exit, on an exception too: an instance attribute
        to its previous value, one that was only the class default is removed again.  Usable around ``simple_test``
        and the other test-time calls; ``stream_step(bf16=True)`` enters it itself."""
        targets = [(self, 'autocast_bf16')]
        depth_net = getattr(getattr(self, 'img_view_transformer', None), 'depth_net', None)
        if depth_net is not None:
            targets.append((depth_net, 'fused_cost_volume_bf16'))
        if self.with_pts_bbox:
            targets.append((self.pts_bbox_head, 'fused_decode_bf16'))
        missing = object()
        before = [vars(obj).get(name, missing) for obj, name in targets]
        try:
            for obj, name in targets:
                setattr(obj, name, True)
            with torch.autocast('cuda', dtype=torch.bfloat16):
                yield self
        finally:
            for (obj, name), value in zip(targets, before):
                if value is missing:
                    vars(obj).pop(name, None)
                else:
                    setattr(obj, name, value)

    # ---------------------------------------------------------------- ocrfdet.py:144-173
    def lift_to_bev(self, x, stereo_feat, img, rot, tran, intrin, post_rot, post_tran, bda, mlp_input, feat_prev_iv,
                    k2s_sensor, imgs_wo_norm, imgs_wo_aug, c2w, cv_feat_packed=None):
        """What follows the image encoder in ``prepare_bev_feat``: the view transformer on the image feature ``x`` with
        ``cv_feat_list = [feat_prev_iv, stereo_feat]``, then ``pre_process_net``.  ``(bev_feat, depth, bev_mask,
        extras)``.  ``cv_feat_packed``: ``[packed feat_prev_iv | None, packed stereo_feat | None]`` for the bfloat16 cost
        volume (``depthnet.stereo_cost_volume_hip_bf16``), from a caller that has them packed already."""
        vt = self.img_view_transformer
        metas = dict(k2s_sensor=k2s_sensor, intrins=intrin, post_rots=post_rot, post_trans=post_tran,
                     frustum=vt.cv_frustum.to(x), cv_downsample=4, downsample=vt.downsample,
                     grid_config=vt.grid_config, cv_feat_list=[feat_prev_iv, stereo_feat])
        if cv_feat_packed is not None:
            metas['cv_feat_packed'] = cv_feat_packed
        bev_feat, depth, bev_mask, extras = vt(
            [x, rot, tran, intrin, post_rot, post_tran, bda, mlp_input, img, imgs_wo_norm, imgs_wo_aug, c2w], metas)
        if self.pre_process:
            bev_feat = self.pre_process_net(bev_feat)[0]
        return bev_feat, depth, bev_mask, extras

    def prepare_bev_feat(self, img, rot, tran, sensor2keyego, ego2global, intrin, post_rot, post_tran, bda, mlp_input,
                         feat_prev_iv, k2s_sensor, extra_ref_frame, imgs_wo_norm, imgs_wo_aug, c2w):
        if extra_ref_frame:
            return None, None, None, self.extract_stereo_ref_feat(img), None
        x, stereo_feat = self.image_encoder(img, stereo=True)
        bev_feat, depth, bev_mask, extras = self.lift_to_bev(x, stereo_feat, img, rot, tran, intrin, post_rot, post_tran,
                                                             bda, mlp_input, feat_prev_iv, k2s_sensor, imgs_wo_norm,
                                                             imgs_wo_aug, c2w)
        return bev_feat, depth, bev_mask, stereo_feat, extras

    def extract_img_feat_sequential(self, inputs, feat_prev):
        raise NotImplementedError('extract_img_feat_sequential: the reference\'s sequential test cannot run (it calls '
                                  'prepare_bev_feat with 8 of its 16 arguments); streaming inference is stream_step')

    # ---------------------------------------------------------------- streaming inference (ocrfdet_amd/streaming.py)
    def stream_step(self, img_inputs, state=None, new_sequence=None, multi_frame=False, bf16=False):
        """One streaming step on ONE frame: ``(([x], depth, bev_mask), state)``.  ``streaming.stream_step``; ``bf16``:
        the step runs inside ``bf16_inference()`` with a bfloat16 ring."""
        from .streaming import stream_step
        return stream_step(self, img_inputs, state=state, new_sequence=new_sequence, multi_frame=multi_frame, bf16=bf16)

    def simple_test_stream(self, img_inputs, img_metas=None, state=None, new_sequence=None, rescale=False,
                           multi_frame=False, bf16=False):
        """``simple_test`` on a stream: ``stream_step``, then ``simple_test_pts``.  Returns ``(results, state)``,
        ``results`` the list over the samples of ``dict(pts_bbox=dict(boxes_3d, scores_3d, labels_3d))``.  ``bf16``:
        the step, the head and the decode run inside ``bf16_inference()``; the results are float32 as without it."""
        (img_feats, _, _), state = self.stream_step(img_inputs, state=state, new_sequence=new_sequence,
                                                    multi_frame=multi_frame, bf16=bf16)
        with torch.no_grad(), (self.bf16_inference() if bf16 else contextlib.nullcontext()):
            return self.pts_results(img_feats, img_metas, img_inputs[0].shape[0], rescale), state

    def track_stream(self, img_inputs, state=None, tracks=None, time_lag=0.5, new_sequence=None, multi_frame=False,
                     bf16=False, track_cfg=None):
        """Streaming detection with identities: ``stream_step``, the head, ``get_bboxes_padded`` and one
        ``tracking.track_step`` launch with camera 0's ``ego2global`` of the frame.  Returns ``(dict(boxes, scores,
        labels, counts, ids, hits), state, tracks)``, everything on the device and padded (``tracking.results_to_host``
        is the read-back); ``tracks`` is the ``tracking.TrackState`` to hand to the next step, ``time_lag`` the seconds
        since the previous frame.  Takes the BEV augmentation as the identity, as at test time."""
        from .tracking import track_stream
        return track_stream(self, img_inputs, state=state, tracks=tracks, time_lag=time_lag, new_sequence=new_sequence,
                            multi_frame=multi_frame, bf16=bf16, track_cfg=track_cfg)

    def evaluate_stream(self, frames_with_gt, evaluator, state=None, multi_frame=False, bf16=False):
        """Streaming detection into the nuScenes detection metrics: per ``(img_inputs, gt)`` one ``stream_step``, the
        head, ``get_bboxes_padded`` and one ``detection_eval.DetectionEval.update`` launch; ``gt``: ``dict(gt_boxes,
        gt_labels, gt_counts[, gt_attrs][, gt_valid][, new_sequence])`` on the device, in the key frame's ego.  Returns
        ``(evaluator, state)``: ``evaluator.results_to_host()`` is the one read-back, ``state`` the stream state for
        the next call.  Takes the BEV augmentation as the identity."""
        from .detection_eval import evaluate_stream
        return evaluate_stream(self, frames_with_gt, evaluator, state=state, multi_frame=multi_frame, bf16=bf16)

    # ---------------------------------------------------------------- what a subclass overrides
    def frame_args(self, key_frame):
        """Hook of the frame loop: the positional arguments of this class's ``prepare_bev_feat`` behind the sixteen of
        ``OcRFDet4D``'s, for one frame.  What ``prepare_bev_feat`` returns behind its five results for the key frame
        is returned behind ``extras`` by a training ``extract_img_feat`` and handed to ``losses_after_neck``."""
        return ()

    def losses_after_neck(self, *rest):
        """Hook of ``forward_train``: the losses that go right behind the neck's five, from what a training
        ``extract_img_feat`` returned behind ``extras``."""
        return {}

    def cat_history(self, bev_feat_list, sensor2keyegos=None, bda=None):
        """The BEV encoder's input from the frames' BEV maps, oldest first, key frame last.  ``with_prev=False``: the
        list holds the key frame alone, and the adjacent groups are zeros."""
        if not self.with_prev:
            key, n_adj = bev_feat_list[0], self.num_frame - self.extra_ref_frames - 1
            zeros = key.new_zeros((key.shape[0], key.shape[1] * n_adj) + tuple(key.shape[2:]))
            return torch.cat([zeros, key], dim=1)                # a warp of zeros is zeros: nothing to align
        if self.align_after_view_transfromation:
            vt = self.img_view_transformer
            frame_ids = [self.num_frame - 2 - k for k in range(self.num_frame - 2)] + [0]
            return temporal.align_and_cat(bev_feat_list, frame_ids, sensor2keyegos, bda, vt.grid_interval,
                                          vt.grid_lower_bound, fused=self.fused_align)
        return torch.cat(bev_feat_list, dim=1)

    # ---------------------------------------------------------------- ocrfdet.py:206-279
    def extract_img_feat(self, img, img_metas=None, pred_prev=False, sequential=False, **kwargs):
        """Frames ``num_frame - 1 ... 0``: the extra reference frame yields only the stereo feature, adjacent frames run
        under ``no_grad``, the key frame with gradients; the BEV features are concatenated oldest first, key frame last
        (``cat_history``).  Returns ``([x], depth, bev_mask, extras, ...)`` in training, with whatever the class's
        ``prepare_bev_feat`` returns behind ``extras``, and ``([x], depth, bev_mask)`` otherwise."""
        if sequential:
            return self.extract_img_feat_sequential(img, **kwargs)
        if pred_prev:
            raise NotImplementedError('pred_prev: the reference asserts False here')
        (imgs, rots, trans, intrins, post_rots, post_trans, bda, sensor2keyegos, ego2globals, curr2adjsensor,
         imgs_wo_norm, imgs_wo_aug, c2ws), mlp_inputs = self.prepare_inputs(img, stereo=True)
        bev_feat_list = []
        feat_prev_iv = None
        for fid in range(self.num_frame - 1, -1, -1):
            key_frame = fid == 0
            extra_ref_frame = fid == self.num_frame - self.extra_ref_frames
            if not (key_frame or self.with_prev):
                continue
            sensor2keyego, ego2global = sensor2keyegos[fid], ego2globals[fid]
            if self.align_after_view_transfromation:
                sensor2keyego, ego2global = sensor2keyegos[0], ego2globals[0]
            inputs_curr = (imgs[fid], rots[fid], trans[fid], sensor2keyego, ego2global, intrins[fid], post_rots[fid],
                           post_trans[fid], bda, mlp_inputs[fid], feat_prev_iv, curr2adjsensor[fid], extra_ref_frame,
                           imgs_wo_norm[fid], imgs_wo_aug[fid], c2ws[fid], *self.frame_args(key_frame))
            if key_frame:
                bev_feat, depth_key_frame, bev_mask_key_frame, feat_curr_iv, *rest = self.prepare_bev_feat(*inputs_curr)
            else:
                with torch.no_grad():
                    bev_feat, _, _, feat_curr_iv, *_ = self.prepare_bev_feat(*inputs_curr)
            if not extra_ref_frame:
                bev_feat_list.append(bev_feat)
            feat_prev_iv = feat_curr_iv
        x = self.bev_encoder(self.cat_history(bev_feat_list, sensor2keyegos, bda))
        if self.training:
            return [x], depth_key_frame, bev_mask_key_frame, *rest
        return [x], depth_key_frame, bev_mask_key_frame

    def extract_feat(self, points, img, img_metas=None, **kwargs):
        """ocrfdet.py:34-46: ``(img_feats, pts_feats = None, depth, bev_mask[, extras])``."""
        out = self.extract_img_feat(img, img_metas, **kwargs)
        return (out[0], None) + tuple(out[1:])

    def forward_pts_train(self, pts_feats, gt_bboxes_3d, gt_labels_3d, img_metas=None, gt_bboxes_ignore=None):
        """``CenterPoint`` / ``MVXTwoStageDetector.forward_pts_train``: the head, then its loss."""
        outs = self.pts_bbox_head(pts_feats)
        return self.pts_bbox_head.loss(gt_bboxes_3d, gt_labels_3d, outs)

    # ---------------------------------------------------------------- ocrfdet.py:331-386
    def forward_train(self, points=None, img_metas=None, gt_bboxes_3d=None, gt_labels_3d=None, gt_labels=None,
                      gt_bboxes=None, img_inputs=None, proposals=None, gt_bboxes_ignore=None, **kwargs):
        gt_depth, gt_semantic, gt_bev_mask = kwargs.pop('gt_depth'), kwargs.pop('gt_semantic'), kwargs.pop('gt_bev_mask')
        img_feats, _, depth, bev_mask, extras, *rest = self.extract_feat(points, img=img_inputs, img_metas=img_metas,
                                                                         **kwargs)
        (render_imgs, gt_images, render_image_G_all, render_image_N_all, opacity_alpha_view, cam_idx_list, render_depth,
         render_depth_G_all, render_depth_N_all) = extras
        vt = self.img_view_transformer
        values = vt.get_loss(depth, bev_mask[1], gt_depth, gt_semantic, gt_bboxes, cam_idx_list, render_imgs, gt_images,
                             render_image_G_all, render_image_N_all, render_depth, render_depth_G_all,
                             render_depth_N_all)
        losses = dict(zip(LOSS_KEYS_NECK, values))
        losses.update(self.losses_after_neck(*rest))
        if opacity_alpha_view is not None:
            losses.update(vt.prob.get_bev_opacity_loss(gt_bev_mask, opacity_alpha_view.squeeze(1)))
        losses.update(vt.prob.get_bev_mask_loss(gt_bev_mask, bev_mask[0]))
        losses.update(self.forward_pts_train(img_feats, gt_bboxes_3d, gt_labels_3d, img_metas, gt_bboxes_ignore))
        return losses

    def simple_test_pts(self, x, img_metas, rescale=False):
        """``CenterPoint.simple_test_pts``: the head, ``get_bboxes``, and ``bbox3d2result``'s dict on the host."""
        outs = self.pts_bbox_head(x)
        bbox_list = self.pts_bbox_head.get_bboxes(outs, img_metas, rescale=rescale)
        return [dict(boxes_3d=boxes.to('cpu'), scores_3d=scores.cpu(), labels_3d=labels.cpu())
                for boxes, scores, labels in bbox_list]

    def pts_results(self, img_feats, img_metas, B, rescale):
        """The result of ``simple_test`` / ``simple_test_stream`` for B samples: ``img_metas`` None is one empty dict
        per sample, and every sample's ``simple_test_pts`` dict goes under ``pts_bbox``."""
        if img_metas is None:
            img_metas = [dict() for _ in range(B)]
        return [dict(pts_bbox=pts_bbox) for pts_bbox in self.simple_test_pts(img_feats, img_metas, rescale=rescale)]

    def simple_test(self, points=None, img_metas=None, img=None, rescale=False, img_inputs=None, **kwargs):
        """ocrfdet.py:48-63: a list over the samples of ``dict(pts_bbox=dict(boxes_3d, scores_3d, labels_3d))``.
        ``img_metas``: a list of per-sample dicts, or None (then one empty dict per sample)."""
        img = img_inputs if img is None else img
        img_feats = self.extract_feat(points, img=img, img_metas=img_metas, **kwargs)[0]
        return self.pts_results(img_feats, img_metas, img[0].shape[0], rescale)

    def forward_dummy(self, points=None, img_metas=None, img_inputs=None, **kwargs):
        img_feats = self.extract_feat(points, img=img_inputs, img_metas=img_metas, **kwargs)[0]
        assert self.with_pts_bbox
        return self.pts_bbox_head(img_feats)

    def forward(self, return_loss=True, **kwargs):
        """mmdet3d's ``Base3DDetector.forward``: ``forward_train`` or ``simple_test`` (no test-time augmentation, no
        ``DataContainer`` unwrapping: ``img_inputs`` is the 12-entry list itself)."""
        if return_loss:
            return self.forward_train(**kwargs)
        return self.simple_test(**kwargs)


# ------------------------------------------------------------------------------------------------ geometry distillation
LOSS_KEYS_KD = ('loss_Smoothl1_KD', 'loss_cos_KD')


class OcRFDet4DVGGT(OcRFDet4D):
    """``OcRFDet4DVGGT`` of configs/ocrfdet/ocrfdet_vggt.py (mmdet3d/models/detectors/ocrfdet_vggt.py:148-498):
    ``OcRFDet4D`` plus a geometry-distillation branch on the key frame, in training only.  A frozen teacher
    (``aggregator``) turns the images of a camera pair into patch tokens, the trainable ``aligner``
    (``distill.CrossAttentionAlign``) maps the student's image feature of that pair onto the teacher's grid, a group-wise
    correlation volume is built from each, and ``loss_Smoothl1_KD`` / ``loss_cos_KD`` compare the two volumes.

    On top of ``OcRFDet4D``'s constructor keys:

    * ``aggregator``: the teacher, any ``nn.Module`` called as VGGT's ``Aggregator`` is: ``aggregator(images (B, 2, 3,
      h, w)) -> (list of token tensors, patch_start_idx)``, the last list entry (B, 2, patch_start_idx + (h // 14) *
      (w // 14), vit_dim).  VGGT itself is not part of this package.  It is registered as ``self.aggregator`` (so
      ``aggregator.*`` keys of a checkpoint line up), its parameters get ``requires_grad=False`` and it stays in
      ``eval()`` through ``train()``.  ``None``: the detector builds and tests, and a training forward raises.
    * ``aligner``: a dict for ``CrossAttentionAlign`` or the module.
    * ``distill``: ``max_disp`` and ``groups`` of the volumes, ``resize`` (h, w) of the teacher's images and its
      ``patch_size``.

    As in the reference, the student's pair feature is formed under ``no_grad``: the two losses train the aligner, not
    the image encoder.  ``fused_distill`` (class attribute, default ``distill.FUSED_DISTILL_DEFAULT``) selects the HIP
    kernels for the volumes and the losses; False takes the torch formulations."""

    fused_distill = None

    def __init__(self, *args, aggregator=None, aligner=None, distill=None, type=None, **kwargs):
        if type not in (None, 'OcRFDet4DVGGT'):
            raise NotImplementedError(f'type {type}: only OcRFDet4DVGGT')
        super().__init__(*args, **kwargs)
        from .distill import CrossAttentionAlign
        if aggregator is not None and not isinstance(aggregator, nn.Module):
            raise NotImplementedError('aggregator: pass the teacher as an nn.Module (VGGT is not part of this package)')
        self.aggregator = aggregator
        if aggregator is not None:
            aggregator.requires_grad_(False).eval()
        self.aligner = _build(dict(res_dim=512, vit_dim=2048, num_heads=8) if aligner is None else aligner,
                              'CrossAttentionAlign', CrossAttentionAlign)
        self.distill = dict(max_disp=4, groups=64, resize=(294, 518), patch_size=14)
        self.distill.update(distill or {})

    def train(self, mode=True):
        super().train(mode)
        if self.aggregator is not None:
            self.aggregator.eval()                   # the teacher is frozen: no batch statistics, no dropout
        return self

    def distill_volumes(self, img, x):
        """ocrfdet_vggt.py:243-268: ``[cost_volume_t, cost_volume_s]`` for a drawn camera pair, from the key frame's
        images ``img`` (B, N, 3, H, W) and image feature ``x`` (B, N, C, h, w)."""
        from . import distill as D
        if self.aggregator is None:
            raise RuntimeError('OcRFDet4DVGGT was built with aggregator=None: a training forward needs the teacher '
                               '(pass VGGT\'s Aggregator, or any module with its call, as `aggregator`)')
        cfg = self.distill
        i1, i2 = D.get_pair_indices()
        with torch.no_grad():
            x_s = torch.stack([x[:, i1], x[:, i2]], dim=1)
            # the reference resizes all six images and takes two; resizing works image by image
            x_t = D.resize_img(torch.stack([img[:, i1], img[:, i2]], dim=1).detach(), *cfg['resize'])
            B, _, _, H, W = x_t.shape
            tokens, patch_start_idx = self.aggregator(x_t)
            token_img = tokens[-1][:, :, patch_start_idx:]
            vit_dim = token_img.shape[-1]
            # channel-major in memory (the permuted tokens are a view): the volume and the aligner read (h, w) planes
            token_img = token_img.reshape(B * 2, -1, vit_dim).permute(0, 2, 1).reshape(
                B, 2, vit_dim, H // cfg['patch_size'], W // cfg['patch_size']).contiguous()
        aligned = self.aligner(x_s, token_img)
        return [D.build_cost_volume(f, max_disp=cfg['max_disp'], method='group_corr', groups=cfg['groups'],
                                    fused=self.fused_distill) for f in (token_img, aligned)]

    # ---------------------------------------------------------------- ocrfdet_vggt.py:232-295
    def prepare_bev_feat(self, img, rot, tran, sensor2keyego, ego2global, intrin, post_rot, post_tran, bda, mlp_input,
                         feat_prev_iv, k2s_sensor, extra_ref_frame, imgs_wo_norm, imgs_wo_aug, c2w, key_frame=False):
        """``OcRFDet4D.prepare_bev_feat`` with a sixth result: the two volumes for the key frame in training, else
        None."""
        if extra_ref_frame:
            return None, None, None, self.extract_stereo_ref_feat(img), None, None
        x, stereo_feat = self.image_encoder(img, stereo=True)
        F_ts = self.distill_volumes(img, x) if self.training and key_frame else None
        bev_feat, depth, bev_mask, extras = self.lift_to_bev(x, stereo_feat, img, rot, tran, intrin, post_rot, post_tran,
                                                             bda, mlp_input, feat_prev_iv, k2s_sensor, imgs_wo_norm,
                                                             imgs_wo_aug, c2w)
        return bev_feat, depth, bev_mask, stereo_feat, extras, F_ts

    # ---------------------------------------------------------------- ocrfdet_vggt.py:328-401, 436-498
    def frame_args(self, key_frame):
        """The key frame is marked for ``prepare_bev_feat``, whose sixth result, ``F_ts = [cost_volume_t,
        cost_volume_s]``, a training ``extract_img_feat`` therefore returns as its last element."""
        return (key_frame,)

    def losses_after_neck(self, F_ts):
        """``loss_Smoothl1_KD`` and ``loss_cos_KD``, where the reference puts them.  The reference calls
        ``smooth_l1_loss(F_ts[0], F_ts[1])``: both losses are symmetric in their operands, and the student's volume,
        ``F_ts[1]``, is the one a gradient flows into."""
        from .distill import kd_losses
        return dict(zip(LOSS_KEYS_KD, kd_losses(F_ts[1], F_ts[0], fused=self.fused_distill)))
