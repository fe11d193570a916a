"""``OcRFViewTransformerFull`` — the reference's neck (mmdet3d/models/necks/view_transformer_ocrf.py:
577-648 ctor, :1040-1201 ``view_transform_core``, :1319-1334 ``forward``) with the same constructor
keywords, sub-module attribute names and ``state_dict`` keys (the config addresses ``S_MLP``, ``R_MLP``,
``A_MLP``, ``C_MLP``, ``C_MLP_nerf``, ``D_MLP_nerf``, ``sigma``, ``img_feat_resize1/2`` by name,
configs/ocrfdet/ocrfdet.py:259-337), assembled MI355X-first:

  eval mode (inference): HIP kernels behind include/ocrf_hip.h (DESIGN.md section 1 has a row per stage) —
    ocrf_prefilter; ocrf_lss_prepare / ocrf_ht_prepare (rank vectors of both poolings, cached when ``accelerate=True``);
    ocrf_bev_pool_v2_nchw (LSS, HT); ocrf_pillar_sample_mean (voxel colours, alpha volume); ocrf_retain_valid_pixels
    (sparse ground-truth image, selected camera only); ocrf_gauss_heads (voxel lift + 4 heads, no (B,13,Y,X,80) tensor);
    the NeRF branch as 3 small MIOpen convolutions batched over all cameras, then ocrf_nerf_alpha / ocrf_nerf_render on
    composed maps (no (80,H,W) feature images); ocrf_rasterize_forward; ocrf_hoa1_forward, ocrf_hoa_v2b_forward,
    ocrf_hoa_opacity_mask_gate (HOA-1/2/3, geometry attention); ocrf_dual_feat_fusion; ProbNet's convolutions: MIOpen
  training mode: the reference's op sequence as differentiable torch ops around the differentiable HIP ops (bev_pool_v2,
    the rasteriser and the voxel heads have HIP backwards).
The building blocks live in ``neck_modules``, the calibration-only state and the camera staging in ``neck_geometry``, the
hipGraph wrapper in ``graphed_neck``; every name that used to be defined here is still importable from here.

``depth_net`` (view_transformer.py:463-630): an explicit ``depth_net=module`` is used as given.  Otherwise a
``depthnet_cfg`` without deformable convolution (``use_dcn=False``, the reference config's) builds the native
``depthnet.DepthNet`` (same ``state_dict``; its stereo cost volume is ocrf_stereo_cost_volume); any other cfg builds the
reference's ``DepthNet`` when its mmdet3d is importable, else none.  ``cv_frustum`` (LSSViewTransformerBEVStereo,
:783-789) is a non-persistent buffer, so the detector's ``cv_frustum.to(x)`` finds it on the device already.
"""
import functools
import random

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, bevpool, depthnet, hoa, index_prep, losses, neck_geometry, neck_ops
from .diff_gaussian_rasterization import rasterize_packed_autograd, rasterize_sets
from .graphed_neck import GraphedNeck
from .neck_geometry import Geometry as _Geometry, PinnedRing, calib_on_device
from .neck_modules import (  # noqa: F401
    MS_CAM, BEVGeomAttention, ChannelAttention, ColorFactorMLPGaussian, ColorFactorMLPNerf, DepthFactorMLPNerf, DiceLoss,
    DualFeatFusion, ImgFeatResize1, ImgFeatResize2, LearnedPositionalEncoding, LinearWeightedDepth, LinearWeightedImage,
    OpacityFactorMLP, ProbNet, ResCBAMBlock, ResizeNetwork, RotationFactorMLP, ScaleFactorMLP, SpatialAttention,
    VoxelFeatureExtractor, _Head, _LinearWeighted, _TallLinear, _ZEROS, _conv_bn, _drop_tensor_lists, _linear,
    _spatial_logits, _tensors_of, _zeros)

__all__ = ['OcRFViewTransformerFull', 'GraphedNeck', 'MS_CAM', 'ChannelAttention', 'SpatialAttention', 'ResCBAMBlock', 'ProbNet',
           'DualFeatFusion', 'BEVGeomAttention', 'ScaleFactorMLP', 'RotationFactorMLP', 'OpacityFactorMLP',
           'ColorFactorMLPGaussian', 'ColorFactorMLPNerf', 'DepthFactorMLPNerf', 'ImgFeatResize1', 'ImgFeatResize2',
           'VoxelFeatureExtractor', 'ResizeNetwork', 'LinearWeightedImage', 'LinearWeightedDepth',
           'LearnedPositionalEncoding', 'DiceLoss']
# the nine entries of the returned ``extras`` list (:1200), as keys of the two paths' tensor dicts
_EXTRAS = ('render_image', 'gt_images', 'render_image_G_all', 'render_N', 'opacity_alpha_view', 'cam_idx_list',
           'render_depth', 'render_depth_G_all', 'render_depth_N')


def _as_float32(a):
    if torch.is_tensor(a):
        return a.float() if a.dtype == torch.bfloat16 else a
    return [_as_float32(v) for v in a] if isinstance(a, list) else a


def _float32_under_autocast(fn):
    """The neck computes in float32 (its kernels, the calibration algebra and the layers between them): called under
    ``torch.autocast``, ``fn`` runs with autocast disabled and its bfloat16 tensor arguments, also those inside lists
    (``img_inputs``), arrive as float32 (autograd hands them bf16 gradients).  Outside autocast nothing changes."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        if not torch.is_autocast_enabled('cuda'):
            return fn(self, *args, **kwargs)
        with torch.autocast('cuda', enabled=False):
            return fn(self, *[_as_float32(a) for a in args], **{k: _as_float32(v) for k, v in kwargs.items()})
    return wrapper


class OcRFViewTransformerFull(nn.Module):
    # Two switches of the training path, class attributes (not in the state_dict), both off by default.  render_depth_grad:
    # the Gaussians render with depth_mode='mean', depth_grad=True, so render_depth_G_all is the differentiable mean depth
    # and loss_render_depth reaches them through LinearWeightedDepth and get_loss (the reference's depth has no gradient;
    # eval, the captured graph and the planned renders keep the median depth).  fused_hoa1_training: HOA-1 on the fused HIP
    # forward + backward (hoa._Hoa1Train: 2 + 6 launches); what the kernels do not take falls back to the ops.
    render_depth_grad = fused_hoa1_training = False

    def __init__(self, pc_range, bev_h=128, bev_w=128, num_height=13, collapse_z=True, loss_semantic_weight=25,
                 depth_threshold=1, semantic_threshold=0.25, depthnet_cfg=dict(), grid_config=None, input_size=None,
                 downsample=16, in_channels=512, out_channels=64, accelerate=False, loss_depth_weight=3.0,
                 depth_net=None):
        super().__init__()
        if grid_config is None or input_size is None:
            raise TypeError('grid_config and input_size are required (view_transformer.py:36-44)')
        # LSSViewTransformer (view_transformer.py:36-76)
        self.grid_config, self.downsample, self.input_size = grid_config, downsample, input_size
        self.grid_lower_bound, self.grid_interval, self.grid_size = index_prep.grid_infos(grid_config)
        self.frustum = index_prep.create_frustum(grid_config['depth'], input_size, downsample)
        self.D = self.frustum.shape[0]
        # LSSViewTransformerBEVStereo (:783-789): the stereo frustum at downsample 4, read by OcRFDet4D.prepare_bev_feat.  A
        # buffer follows .to(device) (the reference copies 16 MB per forward); not persistent: same state_dict keys
        self.register_buffer('cv_frustum', index_prep.create_frustum(grid_config['depth'], input_size, 4),
                             persistent=False)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.accelerate, self.initial_flag = accelerate, True
        self.loss_depth_weight = loss_depth_weight
        # :581-589
        self.loss_semantic_weight = loss_semantic_weight
        self.depth_threshold = depth_threshold / self.D
        self.semantic_threshold = semantic_threshold
        self.pc_range, self.bev_h, self.bev_w = pc_range, bev_h, bev_w
        self.num_height, self.collapse_z = num_height, collapse_z
        self.depth_net = depth_net if depth_net is not None else self._reference_depth_net(depthnet_cfg)
        self.fuser = DualFeatFusion(2 * out_channels, out_channels)
        self.geom_att = BEVGeomAttention()
        self.ObatinOpacityMask = hoa.ObatinOpacityMask()
        self.prob = ProbNet(in_channels=out_channels, with_centerness=True, bev_size=(bev_h, bev_w))
        self.positional_encoding = LearnedPositionalEncoding(out_channels // 2, bev_h, bev_w)
        self.positional_encoding1 = LearnedPositionalEncoding(8 // 4, bev_h, bev_w)
        # NeRF branch (:598-610)
        dim, hidden = 80, 4
        self.image_feat_resize = ResizeNetwork(dim)
        self.sigma = nn.Sequential(nn.Linear(dim, hidden), nn.Linear(hidden, 1), nn.Softplus())
        self.C_MLP_nerf = ColorFactorMLPNerf(dim, hidden, 3)
        self.D_MLP_nerf = DepthFactorMLPNerf(dim, hidden, 1)
        self.img_feat_resize1 = ImgFeatResize1(dim, hidden, 3)
        self.img_feat_resize2 = ImgFeatResize2(dim, hidden, 1)
        # Gaussian heads (:612-623)
        self.S_MLP = ScaleFactorMLP(dim, hidden, 3)
        self.R_MLP = RotationFactorMLP(dim, hidden, 4)
        self.A_MLP = OpacityFactorMLP(dim, hidden, 1)
        self.C_MLP = ColorFactorMLPGaussian(dim, hidden, 3)
        self.OpacityVoxelToBEV = hoa.OpacityVoxelToBEVConverter(input_channel=13)
        self.color_crit = nn.MSELoss(reduction='mean')
        self.zfar, self.znear, self.trans, self.scale = 999.9, 0.01, [0.0, 0.0, 0.0], 1.0
        self.ObtainVoxelFeature = VoxelFeatureExtractor()
        self.LinearWeightedImage, self.LinearWeightedDepth = LinearWeightedImage(), LinearWeightedDepth()
        self.defor_cross_attention = hoa.DeformableAttention2D(
            dim=13, dim_head=8, heads=1, dropout=0.1, downsample_factor=4, offset_scale=4, offset_groups=None,
            offset_kernel_size=6)
        self._geo, self._tmpl = None, None
        # cached geometry (accelerate=True): render through a static plan with an on-device guard (see _render_sets);
        # the plan's extent bound = margin x the largest Gaussian extent of the forward that builds it
        self.render_plan, self.render_plan_margin = True, 2.0
        # per-forward geometry, None (default) or True: the calibration algebra runs on the GPU whenever the calibration
        # tensors arrive there, in eval mode and under autograd (neck_geometry.choose_mode) — no read-back, but ~1 ulp off
        # the host formulation: a 1e-5 fraction of border points may change cell.  False: always the host formulation
        self.device_geometry = None
        # guard of the cached render plan (accelerate=True): 'device' — exact whatever the scale head emits, the per-call
        # pipeline armed behind every render (four near-empty launches, ~24 us at cfg2); 'host' — only a status bit is
        # raised, ``check_render()`` (one synchronising read) turns it into an exception: the caller decides when to pay
        self.render_guard = 'device'
        # training mode: the voxel lift + four Gaussian heads by the fused forward / backward kernels (csrc/neck_train.hip)
        # instead of torch layers on the (B,Zh,Y,X,C) voxel feature; False keeps the reference's layer formulation
        self.fused_heads_training = True
        # eval-mode strands on side HIP streams (_core_fused): a caller with its own stream discipline opts in
        self.parallel_branches, self._transient = False, hoa._LaunchCache()     # streams: not module state
        self.fork_c_after = 'pools'
        self.fork_ht_prep = True         # per-forward geometry: HT preparation + pooling beside the LSS pair (see _core_segments)
        self._rank_bufs = (index_prep._RankBuffers(), index_prep._RankBuffers())
        self._packs = {}
        # get_loss by the fused HIP kernels of csrc/losses.hip; False, the CPU, a gt that requires grad: torch formulation
        self.fused_losses = True
        # calls of get_loss so far: the box mask applies once it passes 3862 * 2 (:1375).  Per instance, where the
        # reference keeps a module-global counter; settable, not part of the state_dict
        self.loss_iteration = 0

    def _recording(self, *tensors):
        if not torch.is_grad_enabled():
            return False
        return (any(t is not None and t.requires_grad for t in tensors)
                or any(p.requires_grad for p in _tensors_of(self, 'all', (self,), buffers=False)))

    def _reference_depth_net(self, cfg):
        if depthnet.supports(cfg):
            return depthnet.DepthNet(self.in_channels, self.in_channels, self.out_channels, self.D + 2, **cfg)
        try:
            from mmdet3d.models.necks.view_transformer import DepthNet
        except Exception:
            return None           # forward() then raises; view_transform_core() does not need it
        return DepthNet(self.in_channels, self.in_channels, self.out_channels, self.D + 2, **cfg)

    # -------------------------------------------------------------------------------- geometry
    def pre_compute(self, input):
        """``accelerate=True``: the geometry of the first call is kept (:854-866; the reference's own version of this path
        does not survive ``get_ht_bev_feat``)."""
        if self.initial_flag or self._geo is None:
            self._geo = self._geometry(input)          # trimmed ranks: usable by both the fused and the autograd pooling
            self.initial_flag = False

    def _templates(self, dev):
        """Calibration-independent templates on the device (frustum :77-106, normalised pillar grid :651-673), built
        once."""
        if self._tmpl is None or self._tmpl[0].device != dev:
            ref = index_prep.get_reference_points_3d(self.bev_h, self.bev_w, bs=1, num_points_in_pillar=self.num_height,
                                                     device='cpu')[0]
            self._tmpl = (self.frustum.to(dev).contiguous(), ref.to(dev).contiguous())
        return self._tmpl

    def _geometry(self, input, mode=neck_geometry.CACHED):
        """-> ``Geometry``; ``mode`` says how its ranks are made and whether the persistent ``_rank_bufs`` may be written."""
        return neck_geometry.build_geometry(self, input, mode)

    _to_host = staticmethod(neck_geometry.to_host)

    def stage_cameras(self, geo, cam_idx_list, device, out=None):
        """Everything the device needs to know about the random camera choice (:1081): ``cam_sel`` (B) int32 and the
        rasteriser's packed camera rows (B,36).  The rows are cached per (sample, camera) for the lifetime of ``geo``;
        with ``out`` (a dict from an earlier call) the values are copied into its tensors in place — the static inputs of
        a captured graph."""
        return neck_geometry.stage_cameras(self, geo, cam_idx_list, device, out)

    def _small_h2d(self, host_tensor, device):
        """At most 64 host integers to a fresh device tensor without a hidden wait (the ring is not module state)."""
        ring = self._transient.get('pin_ring')
        if ring is None:
            ring = self._transient['pin_ring'] = PinnedRing(8, 64, torch.int32)
        return ring.put(host_tensor, device)

    # -------------------------------------------------------------------------------- packs
    def invalidate_packs(self):
        """Forget the cached tensor lists and weight packs (needed only after assigning a NEW Parameter object to a
        sub-module; value updates, ``load_state_dict``, ``.to()`` and ``train()`` are tracked)."""
        _drop_tensor_lists(self)
        self._packs.clear()

    def _apply(self, fn, *args, **kwargs):
        _drop_tensor_lists(self)
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        _drop_tensor_lists(self)
        return super().load_state_dict(*args, **kwargs)

    def train(self, mode=True):
        _drop_tensor_lists(self)
        return super().train(mode)

    def _pack(self, name, params, build):
        key = tuple((p._version, p.data_ptr()) for p in params)
        hit = self._packs.get(name)
        if hit is None or hit[0] != key:
            self._packs[name] = (key, build())
        return self._packs[name][1]

    def _head_params(self):
        mods = (self.ObtainVoxelFeature, self.S_MLP, self.R_MLP, self.A_MLP, self.C_MLP)
        return self._pack('heads', _tensors_of(self, 'heads', mods), lambda: neck_ops.pack_gauss_head_params(*mods))

    def _nerf_params(self):
        mods = (self.image_feat_resize, self.sigma, self.C_MLP_nerf, self.img_feat_resize1, self.img_feat_resize2)
        return self._pack('nerf', _tensors_of(self, 'nerf', mods, buffers=False),
                          lambda: neck_ops.compose_nerf_maps(*mods))

    def _pos(self, name, batch, like):
        """Eval-mode positional-encoding maps are constants of the weights: built once per (weights, batch) instead of
        arange + 2 embeddings + cat + an 80-channel strided ``repeat`` per forward."""
        enc = getattr(self, name)
        return self._pack((name, batch, like.dtype), _tensors_of(self, name, (enc,), buffers=False),
                          lambda: enc(_zeros((batch, self.bev_h, self.bev_w), like)).to(like.dtype).contiguous())

    # -------------------------------------------------------------------------------- pooling
    def _pool(self, ranks, depth, feat_cl, bev_shape, scratch_tag='bev_pool_nchw'):
        if len(ranks) == 2:                       # ((five capacity vectors), device counts)
            (rb, rd, rf, st, ln), counts = ranks
            if torch.is_grad_enabled() and (depth.requires_grad or feat_cl.requires_grad):
                return bevpool.bev_pool_v2_device_counts_autograd(depth, feat_cl, rd, rf, rb, bev_shape, st, ln, counts,
                                                                  scratch_tag=scratch_tag)
            return bevpool.bev_pool_v2_device_counts(depth, feat_cl, rd, rf, rb, bev_shape, st, ln, counts,
                                                     scratch_tag=scratch_tag)
        if ranks[0] is None:
            B, Z, Y, X, C = bev_shape
            return torch.zeros(B, Z * C, Y, X, device=depth.device)
        rb, rd, rf, st, ln = ranks
        return bevpool.bev_pool_v2_collapsed(depth, feat_cl, rd, rf, rb, bev_shape, st, ln)

    def _pool_cached(self, geo, which, ranks, depth, feat_cl, bev_shape, scratch_tag='bev_pool_nchw'):
        """Cached geometry + forward-only call: the rank-only half of the pooling is cached as well."""
        if (geo is self._geo and len(ranks) == 5 and ranks[0] is not None and not torch.is_grad_enabled()
                and bevpool._fusable(bev_shape[-1])):
            plan = geo.plans.get(which)
            if plan is None or plan.bev_shape != tuple(int(v) for v in bev_shape):
                plan = geo.plans[which] = bevpool.PoolPlan(*ranks, bev_shape)
            # HotPath's default back end through the same front end and plan arguments (the panel latency kernel, the tile
            # kernel where the channel count is no panel count); here each pooling runs its own weight pre-pass and HOA-3's
            # statistics stay a launch of their own
            return plan.pool(depth, feat_cl, 'panel', which)
        return self._pool(ranks, depth, feat_cl, bev_shape, scratch_tag)

    def get_lss_bev_feat(self, geo, depth, feat_cl):
        gx, gy, gz = (int(v) for v in self.grid_size.tolist())
        return self._pool_cached(geo, 'lss', geo.lss, depth, feat_cl, (depth.shape[0], gz, gy, gx, feat_cl.shape[-1]))

    def get_ht_bev_feat(self, geo, depth, feat_cl, scratch_tag='bev_pool_nchw'):
        """``scratch_tag``: the pooling's scratch is per tag; who pools HT beside LSS on a second stream names its own."""
        return self._pool_cached(geo, 'ht', geo.ht, depth, feat_cl,
                                 (depth.shape[0], 1, self.bev_h, self.bev_w, feat_cl.shape[-1]), scratch_tag)

    # -------------------------------------------------------------------------------- core
    @_float32_under_autocast
    def view_transform(self, input, depth, tran_feat, feat_channels_last=None, cameras=None):
        if self.accelerate:
            self.pre_compute(input)
        return self.view_transform_core(input, depth, tran_feat, feat_channels_last, cameras=cameras)

    @_float32_under_autocast
    def view_transform_core(self, input, depth, tran_feat, feat_channels_last=None, cam_idx_list=None, cameras=None):
        """Same inputs / outputs as the reference (:1040-1201).  ``feat_channels_last`` (B*N,H,W,C), when the caller
        already has it (``forward`` does), skips the permute of :875/:901; ``cam_idx_list`` overrides the random camera
        choice of :1081 (tests); ``cameras`` is a dict from ``stage_cameras`` (choice already made and staged on the
        device: nothing in the call then touches the host, so the whole call can be captured in a hipGraph)."""
        x = input[0]
        B, N, _, Hf, Wf = x.shape
        C = self.out_channels
        # fused HIP kernels are forward-only and fold the BatchNorm running statistics: eval mode with
        # nothing recorded by autograd; anything else takes the differentiable torch formulation
        fused = not self.training and not self._recording(depth, tran_feat, feat_channels_last)
        geo = self._geo if self.accelerate else None
        if geo is None:
            geo = self._geometry(input, neck_geometry.choose_mode(self.accelerate, fused, self.device_geometry,
                                                                  calib_on_device(input)))
        depth5 = depth.reshape(B, N, self.D, Hf, Wf).float()
        if feat_channels_last is None:
            feat_channels_last = tran_feat.reshape(B, N, C, Hf, Wf).permute(0, 1, 3, 4, 2)
        feat_cl = feat_channels_last.reshape(B, N, Hf, Wf, C).float().contiguous()
        if cameras is None:
            if cam_idx_list is None:
                cam_idx_list = [random.randint(0, 5) for _ in range(B)]
            cameras = self.stage_cameras(geo, cam_idx_list, x.device)
        if cameras.get('packed') is None:
            # only the choice was staged (a captured per-forward-geometry graph): the rasteriser's rows of the chosen
            # cameras are picked on the device from the rows ocrf_geometry_blocks made for every camera-frame
            cameras = dict(cameras, packed=geo.cam_rows_dev[torch.arange(B, device=x.device),
                                                            cameras['cam_sel'].long()].contiguous())
        voxel_coor = geo.voxel.reshape(B, self.num_height * self.bev_h * self.bev_w, 3)
        core = self._core_fused if fused else self._core_train
        return core(input, geo, depth, depth5, feat_cl, cameras, voxel_coor)

    def _weighted_images(self, T):
        T['render_image'] = self.LinearWeightedImage(T['render_image_G_all'], T['render_N'])
        T['render_depth'] = self.LinearWeightedDepth(T['render_depth_G_all'], T['render_depth_N'])

    @staticmethod
    def _gt_images(imgs_wo_norm, cam_sel):
        return imgs_wo_norm[torch.arange(len(cam_sel), device=cam_sel.device), cam_sel.long()] / 255.0

    def _core_train(self, input, geo, depth, depth5, feat_cl, cameras, voxel_coor):
        """``view_transform_core`` under autograd: the reference's op sequence (:1051-1201) as differentiable torch ops
        around the differentiable HIP ops.  Nothing here is cached across calls (no autograd graph outlives its iteration)."""
        x, imgs_wo_norm, dtype = input[0], input[9], input[0].dtype
        B, N, _, Hf, Wf = x.shape
        Zh, Y, X = self.num_height, self.bev_h, self.bev_w
        H, W = self.input_size
        cam_sel, T = cameras['cam_sel'], dict(cam_idx_list=cameras['cam_idx_list'])
        lss_feat = self.get_lss_bev_feat(geo, depth5, feat_cl)
        ht_feat = self.get_ht_bev_feat(geo, depth5, feat_cl)
        mask5 = geo.mask.unsqueeze(-1)

        def sample(imgs, h, w):
            c = imgs.shape[2]
            g = geo.pix.clone()
            g[..., 0] = (g[..., 0] / (w - 1)) * 2 - 1
            g[..., 1] = (g[..., 1] / (h - 1)) * 2 - 1
            v = F.grid_sample(imgs.reshape(B * N, c, h, w).float(), g.view(B * N, 1, Zh * Y * X, 2), align_corners=True)
            v = v.view(B, N, c, Zh, Y * X).permute(0, 1, 3, 4, 2) * mask5.float()
            cnt = mask5.sum(1).float().clamp(min=1)
            return v.sum(1) / cnt
        avg_rgb = sample(imgs_wo_norm, H, W)
        # retain_valid_pixels for the selected cameras, vectorised (:1004-1024)
        sel, ar = cam_sel.long(), torch.arange(B, device=x.device)
        pix_s, mask_s = geo.pix[ar, sel].reshape(B, -1, 2), geo.mask[ar, sel].reshape(B, -1)
        imgs_s = imgs_wo_norm[ar, sel].float()
        keep = torch.zeros(B, H * W, dtype=torch.bool, device=x.device)
        hi = max(W, H) - 1
        xi = pix_s[..., 0].long().clamp(0, min(hi, W - 1))
        yi = pix_s[..., 1].long().clamp(0, min(hi, H - 1))
        keep.scatter_(1, (yi * W + xi) * mask_s.long(), mask_s)          # masked-out points all hit pixel 0 with False
        keep[:, 0] = ((yi * W + xi == 0) & mask_s).any(1)
        sparse = torch.where(keep.view(B, 1, H, W), imgs_s, torch.full_like(imgs_s, 255.0))
        # alpha of EVERY camera image: ResizeNetwork is linear and sigma starts with two Linears, so sigma[:2](upsample3(
        # upsample2(z))) is one composed (32 -> 8x8 sub-positions) map of conv2's output z (neck_ops.compose_nerf_maps; here
        # with autograd through the composition).  The reference's formulation — a (B*N,80,H,W) feature image (692 MB at
        # 12 x 256 x 704), two transposed convolutions and an 80 -> 4 -> 1 MLP on 2.2 M rows — is kept only for the ONE
        # selected camera of each sample, whose features the four NeRF heads need.
        res, z = self.image_feat_resize, self.image_feat_resize.stem(x.reshape(B * N, -1, Hf, Wf).float())
        h2, w2 = z.shape[-2:]
        W2, b2, W3, b3 = (t.double() for t in (res.upsample2.weight, res.upsample2.bias, res.upsample3.weight,
                                               res.upsample3.bias))
        s0, s1 = self.sigma[0], self.sigma[1]
        ws = s1.weight.double() @ s0.weight.double()                                          # (1,80)
        cs = s1.weight.double() @ s0.bias.double() + s1.bias.double()
        t3 = torch.einsum('ofrs,kf->kors', W3, ws)                                             # (1,80,4,4)
        M = torch.einsum('iopq,kors->iprqs', W2, t3).reshape(W2.shape[0], 64)                 # y%8 = 4p + r, x%8 = 4q + s
        const = torch.einsum('o,kors->rs', b2, t3) + (ws @ b3 + cs)                           # (4,4)
        pre = (z.permute(0, 2, 3, 1) @ M.to(z.dtype)).view(B * N, h2, w2, 2, 4, 2, 4)
        pre = pre + const.to(z.dtype).view(1, 1, 1, 1, 4, 1, 4)
        pre = pre.permute(0, 1, 3, 4, 2, 5, 6).reshape(B * N, H, W, 1)
        alpha = 1. - torch.exp(-self.sigma[2](pre))                                           # (B*N,H,W,1)
        alpha_lidar = sample(alpha.reshape(B, N, 1, W, H), W, H).view(B, Zh, Y, X)
        fs = res.upsample3(res.upsample2(z.view(B, N, -1, h2, w2)[ar, sel])).permute(0, 2, 3, 1)   # (B,H,W,80)
        xin = torch.cat((fs, sparse.permute(0, 2, 3, 1) / 255.0), -1)
        radiance, radiance1 = self._nerf_heads_torch(xin)
        a_sel = alpha.view(B, N, H, W, 1)[ar, sel]
        T['render_N'] = (a_sel * radiance).permute(0, 3, 1, 2)
        T['render_depth_N'] = (a_sel * radiance1).permute(0, 3, 1, 2)
        if self.fused_heads_training and self._heads_fusable(ht_feat):
            # lift + four heads by ocrf_gauss_heads / ocrf_gauss_heads_backward: the (B,Zh,Y,X,C) voxel feature (333 MB at
            # cfg2, read or written by ~100 torch kernels of an iteration) exists in neither; the modules' parameters — and
            # ht_feat, also through the BatchNorm's batch statistics — get their gradients through the differentiable packing
            heads = (self.S_MLP, self.R_MLP, self.A_MLP, self.C_MLP)
            prm = neck_ops.pack_gauss_head_params_autograd(self.ObtainVoxelFeature, *heads, x=ht_feat)
            opacity, scaling, rotation, color = neck_ops.gauss_heads_train(ht_feat, avg_rgb.reshape(B, Zh, Y * X, 3), prm, Zh)
        else:
            voxel_feat = self.ObtainVoxelFeature(ht_feat.permute(0, 2, 3, 1).unsqueeze(1)).reshape(B, Zh * Y * X, -1)
            rgb01 = avg_rgb.reshape(B, Zh * Y * X, 3) / 255.0
            opacity, scaling, rotation, color = (self.A_MLP(voxel_feat), self.S_MLP(voxel_feat), self.R_MLP(voxel_feat),
                                                 self.C_MLP(torch.cat((voxel_feat, rgb01), -1)))
        # one differentiable render per sample (:1135-1153) from the rows stage_cameras put on the device once for the batch
        # (the reference's per-sample camera set-up — matrix uploads, focal arithmetic — is ~0.9 ms of host time each here)
        bg, render_G, render_depth_G = _zeros((3,), voxel_coor), [], []       # black background, as every render here
        for bs in range(B):
            img, dep, _, _ = rasterize_packed_autograd(voxel_coor[bs], color[bs], opacity[bs], scaling[bs], rotation[bs],
                                                       cameras['packed'][bs:bs + 1], H, W, bg,
                                                       **(dict(depth_mode='mean', depth_grad=True)
                                                          if self.render_depth_grad else {}))
            render_G.append(img), render_depth_G.append(dep)
        T['render_image_G_all'], T['render_depth_G_all'] = torch.cat(render_G), torch.cat(render_depth_G)
        self._weighted_images(T)
        T['gt_images'] = self._gt_images(imgs_wo_norm, cam_sel)
        # HOA-1 for the whole batch (the reference loops samples, :1159-1161)
        opacity_alpha = hoa.hoa1(self.defor_cross_attention, opacity.reshape(-1, 1), alpha_lidar, Zh, Y, X,
                                 fused_training=self.fused_hoa1_training)
        channel_feat = self.fuser(lss_feat, ht_feat)
        zeros = _zeros((B, Y, X), x)            # positional encodings only read its shape / device
        bev_mask_logit = self.prob(self.positional_encoding(zeros).to(dtype) + channel_feat)
        geom_feat = self.geom_att.gate(channel_feat, bev_mask_logit)
        T['opacity_alpha_view'] = self.OpacityVoxelToBEV(opacity_alpha, self.positional_encoding1(zeros).to(dtype))
        m = torch.sigmoid(_spatial_logits(geom_feat, self.ObatinOpacityMask.conv) + T['opacity_alpha_view'])
        return geom_feat * m, depth, bev_mask_logit, [T[k] for k in _EXTRAS]

    def _core_segments(self, input, geo, depth, depth5, feat_cl, cameras, voxel_coor, mark=lambda i: None):
        """The eval-mode step on the HIP kernels as its SEGMENTS: closures that read and write one dict of tensors, each
        running on whatever stream is current.  Who needs whom:
            b1 colours            <- inputs                       a1 poolings            <- inputs
            b2 NeRF branch, alpha <- inputs                       c  fusion, ProbNet, GA <- a1
            a2 Gaussian heads     <- a1, b1                       a3 render              <- a2
            a4 weighted images    <- a3, b2                       a5 HOA-1/2             <- a2, b2
            a6 HOA-3 gate (the module's main output)              <- c, a5
        ``_core_fused`` runs them on up to three streams in one pass (what the captured graph replays; the schedules
        that were measured against this one are in DESIGN 4.6).  -> (segments, the dict)."""
        x, imgs_wo_norm = input[0], input[9]
        dev = x.device
        B, N, _, Hf, Wf = x.shape
        Zh, Y, X = self.num_height, self.bev_h, self.bev_w
        H, W = self.input_size
        cam_sel = cameras['cam_sel']
        T = dict(cam_idx_list=cameras['cam_idx_list'])

        def b1():
            T['avg_rgb'] = neck_ops.pillar_sample_mean(imgs_wo_norm, geo.pix, geo.mask)             # (B,Zh,YX,3)
            mark(1)

        def b2():
            sparse = neck_ops.retain_valid_pixels(imgs_wo_norm, geo.pix, geo.mask, cam_sel)        # (B,3,H,W)
            w_s, c_s, nerf_block = self._nerf_params()
            z = self.image_feat_resize.stem(x.reshape(B * N, -1, Hf, Wf).float())
            alpha = neck_ops.nerf_alpha(z, w_s, c_s)                                                # (B*N,H,W)
            T['render_N'], T['render_depth_N'] = neck_ops.nerf_render(z, cam_sel, alpha, sparse, nerf_block, N)
            # the reference views the (6,H,W,1) stack as (1,6,1,W,H) before sampling it (:1123)
            alpha_lidar = neck_ops.pillar_sample_mean(alpha.view(B, N, 1, H, W), geo.pix, geo.mask, view_hw=(W, H))
            T['alpha_lidar'] = alpha_lidar.view(B, Zh, Y, X)
            T['gt_images'] = self._gt_images(imgs_wo_norm, cam_sel)
            mark(2)

        def a1():
            fork = geo.lss is None and self.parallel_branches and self.fork_ht_prep
            if fork:
                # per-forward geometry: each pooling right behind its own index preparation, the HT pair on a stream of
                # its own beside the LSS pair (the preparations' scratch is per stream, the poolings' per tag): in a row
                # the four are 89 + 62 + 54 + 50 us in front of everything that reads a pooled BEV
                cur = torch.cuda.current_stream(dev)
                s_ht = self._transient.get('stream_ht')
                if s_ht is None or s_ht.device != dev:
                    s_ht = self._transient['stream_ht'] = torch.cuda.Stream(dev)
                s_ht.wait_stream(cur)
                with torch.cuda.stream(s_ht):
                    geo.ht = geo.rank_vectors['ht']()
                    T['ht_feat'] = self.get_ht_bev_feat(geo, depth5, feat_cl, scratch_tag='bev_pool_nchw_b')
                geo.lss = geo.rank_vectors['lss']()
            elif geo.lss is None:
                # per-forward geometry: beside strand B (see build_geometry), both preparations on this stream
                geo.lss, geo.ht = geo.rank_vectors['lss'](), geo.rank_vectors['ht']()
            T['lss_feat'] = self.get_lss_bev_feat(geo, depth5, feat_cl)
            if fork:
                cur.wait_stream(s_ht)
            else:
                T['ht_feat'] = self.get_ht_bev_feat(geo, depth5, feat_cl)
            mark(3)

        def c():
            # the fused map and the map ProbNet reads (fused map + positional encoding) leave the fusion kernel together
            channel_feat, with_pos = self.fuser(T['lss_feat'], T['ht_feat'], addend=self._pos('positional_encoding', B, x))
            mark(4)
            T['bev_mask_logit'] = self.prob(with_pos)
            mark(5)
            T['geom_feat'] = self.geom_att.gate(channel_feat, T['bev_mask_logit'])
            mark(6)

        def a2():
            T['opacity'], T['scaling'], T['rotation'], T['color'] = neck_ops.gauss_heads(
                T['ht_feat'], T['avg_rgb'], self._head_params(), Zh)
            mark(7)

        def a3():
            # every sample is a Gaussian set with one camera: ONE rasteriser call for the batch, fed with the
            # staged camera rows (the reference loops samples, :1090-1153)
            o = self._render_sets(geo, voxel_coor, T['color'], T['opacity'], T['scaling'], T['rotation'], cameras, H, W)
            T['render_image_G_all'], T['render_depth_G_all'] = o['color'], o['depth']
            mark(8)

        def a4():
            self._weighted_images(T)
            mark(9)

        def a5():
            # HOA-1 for the whole batch (the reference loops samples, :1159-1161), HOA-2
            oa = hoa.hoa1(self.defor_cross_attention, T['opacity'].reshape(-1, 1), T['alpha_lidar'], Zh, Y, X)
            mark(10)
            T['opacity_alpha_view'] = self.OpacityVoxelToBEV(oa, self._pos('positional_encoding1', B, x))
            mark(11)

        def a6():
            T['bev_feat'] = self.ObatinOpacityMask.gate(T['geom_feat'], T['opacity_alpha_view'])[1]     # HOA-3
            mark(12)

        return dict(b1=b1, b2=b2, a1=a1, c=c, a2=a2, a3=a3, a4=a4, a5=a5, a6=a6), T

    def _core_fused(self, input, geo, depth, depth5, feat_cl, cameras, voxel_coor):
        """Eval-mode ``view_transform_core`` on the HIP kernels.  The step has three independent strands until HOA joins
        them — (A) poolings -> Gaussian heads -> render, (B) colour sampling + NeRF branch (needs only the images and the
        calibration), (C) BEV fusion -> ProbNet -> geometry attention (needs only the pooled BEVs).  With
        ``parallel_branches`` B and C run on two side HIP streams (captured as parallel branches of the graph): the many
        small kernels of C and the MIOpen convolutions of B fill the gaps of A instead of queueing behind it."""
        dev = input[0].device
        par = self.parallel_branches
        cur = torch.cuda.current_stream(dev)
        if par:
            streams = self._transient.get('streams')
            if streams is None or streams[0].device != dev:
                streams = self._transient['streams'] = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
            sB, sC = streams
            sB.wait_stream(cur)                    # inputs ready; last call's consumers of our buffers done
        stamps = self._transient.get('stamps')     # diagnostic timeline (tools/timeline_neck.py)
        mark = (lambda i: _lib.diag_stamp(stamps, i)) if stamps is not None else (lambda i: None)
        seg, T = self._core_segments(input, geo, depth, depth5, feat_cl, cameras, voxel_coor, mark)
        mark(0)
        # ---- strand B
        with torch.cuda.stream(sB if par else None):         # (None: a no-op context)
            seg['b1']()
            if par:
                rgb_ready = torch.cuda.Event()
                rgb_ready.record(sB)
            seg['b2']()
        # ---- strand A, first half.  The wait for B's colours sits in FRONT of the poolings although only the heads need
        # them: ROCm 7.2's graph executor serialises the two branches forked after a node (C, A) when one of them starts
        # with a second, cross-branch dependency (tools/diag_graph_parallel.py); ahead of the fork they overlap.
        if par:
            cur.wait_event(rgb_ready)
        seg['a1']()
        def strand_c():
            if par:
                sC.wait_stream(cur)
            with torch.cuda.stream(sC if par else None):
                seg['c']()
        # Where strand C is forked: it needs only the poolings, and the early fork replays fastest (0.70 ms against 0.74
        # behind the heads and 0.76 behind the render; these and the other schedules tried: DESIGN 4.6)
        fork_at = self.fork_c_after
        if fork_at == 'pools':
            strand_c()
        seg['a2']()
        if fork_at == 'heads':
            strand_c()
        # ---- strand A, second half (a second fork behind the heads costs more than it returns: DESIGN 4.6)
        seg['a3']()
        if fork_at == 'render':
            strand_c()
        if par:
            cur.wait_stream(sB)
        seg['a4']()
        seg['a5']()
        if par:
            cur.wait_stream(sC)
        seg['a6']()
        return T['bev_feat'], depth, T['bev_mask_logit'], [T[k] for k in _EXTRAS]

    def _render_sets(self, geo, voxel_coor, color, opacity, scaling, rotation, cameras, H, W):
        """One rendered view per sample.  With CACHED geometry (``accelerate=True``) the rasteriser's calibration-only
        front end is cached too: the Gaussian means are the voxel grid and every (sample, camera) pair a fixed view, so a
        static render plan over all of them (``raster_plan.RasterPlan``) leaves two launches per forward; the sample's
        random camera is a device-side index into the plan, and the plan's extent bound is guarded ON THE DEVICE (the
        per-call pipeline is armed behind it), so the result is exact whatever the scale head emits and the forward stays
        free of host reads (graph-capturable).  Otherwise: the per-call pipeline (``rasterize_sets``)."""
        B, N, bg = voxel_coor.shape[0], 6, _zeros((3,), voxel_coor)
        state = geo.raster_plan
        if (state is None and self.render_plan and self.accelerate and geo is self._geo and B * N <= 32
                and not torch.cuda.is_current_stream_capturing()):
            state = geo.raster_plan = self._build_raster_plan(geo, voxel_coor, scaling, rotation, B, N, H, W)
        if not state:            # not eligible (per-forward geometry, > 32 views, samples with different means)
            return rasterize_sets(voxel_coor, color, opacity, scaling, rotation, cameras['packed'], H, W, bg)
        plan, base = geo.raster_plan
        item_view = (base + cameras['cam_sel'].to(torch.int32)).contiguous()
        # (sample b renders one of ITS OWN N plan views: no view is named by two sets)
        return plan.render(color, opacity, scaling, rotation, bg, item_view=item_view,
                           guard=getattr(self, 'render_guard', 'device'), views_disjoint=True, want_radii=False)

    def check_render(self):
        """``render_guard='host'``: synchronising check of the cached render plan's status word — raises if a render since
        the last check had a Gaussian beyond the plan's extent bound (those images are not valid)."""
        state = self._geo.raster_plan if self._geo is not None else None
        if state:
            state[0].check()
        return True

    def _build_raster_plan(self, geo, voxel_coor, scaling, rotation, B, N, H, W):
        """-> (RasterPlan over the B*N (sample, camera) views, int32 view offsets b*N) or False when the samples do not
        share one set of means.  Runs once per cached geometry (host work + one synchronisation)."""
        from .raster_plan import RasterPlan
        dev = voxel_coor.device
        if any(not torch.equal(voxel_coor[b], voxel_coor[0]) for b in range(1, B)):
            return False
        if geo.cam_rows_dev is not None:
            rows = geo.cam_rows_dev.reshape(B * N, 36).contiguous()
        else:
            rows = torch.cat([geo.cam_row(bs, c, (H, W), self.znear, self.zfar)
                              for bs in range(B) for c in range(N)], 0).to(dev)
        plan = RasterPlan(voxel_coor[0], rows, H, W, scales=scaling, rotations=rotation, margin=self.render_plan_margin)
        return plan, torch.arange(B, device=dev, dtype=torch.int32) * N

    def _nerf_heads_torch(self, xin):
        """radiance = img_feat_resize1(xin) * softmax(C_MLP_nerf(xin)), radiance1 = img_feat_resize2(xin) *
        softmax(D_MLP_nerf(xin)) (:1113-1121).  The four heads read the same 83-column rows (360 448 of them at cfg2):
        their first layers run as ONE 83 -> 16 Linear and their second layers as one block-diagonal 16 -> 8 Linear — two
        split-K weight gradients instead of eight (each ~115 us of host time per backward), a third of the launches."""
        heads = (self.img_feat_resize1, self.C_MLP_nerf, self.img_feat_resize2, self.D_MLP_nerf)
        kinds = (ImgFeatResize1, ColorFactorMLPNerf, ImgFeatResize2, DepthFactorMLPNerf)
        if not (all(type(m) is k for m, k in zip(heads, kinds))
                and len({(m.fc1.in_features, m.fc1.out_features) for m in heads}) == 1
                and all(m.fc1.bias is not None and m.fc2.bias is not None for m in heads)):
            return (self.img_feat_resize1(xin) * F.softmax(self.C_MLP_nerf(xin), dim=-1),
                    self.img_feat_resize2(xin) * F.softmax(self.D_MLP_nerf(xin), dim=-1))
        w1, b1 = torch.cat([m.fc1.weight for m in heads]), torch.cat([m.fc1.bias for m in heads])
        w2, b2 = torch.block_diag(*[m.fc2.weight for m in heads]), torch.cat([m.fc2.bias for m in heads])
        rows = xin.numel() // xin.shape[-1]
        lin = _TallLinear.apply if (xin.is_cuda and rows >= 8 * _TallLinear.CHUNK) else F.linear
        out = lin(torch.relu(lin(xin, w1, b1)), w2, b2)
        n1, n2, n3 = (heads[0].fc2.out_features, heads[1].fc2.out_features, heads[2].fc2.out_features)
        feat, col, dfeat, dep = out.split((n1, n2, n3, out.shape[-1] - n1 - n2 - n3), dim=-1)
        return (torch.relu(feat) * F.softmax(torch.sigmoid(col), dim=-1),
                torch.relu(dfeat) * F.softmax(torch.relu(dep), dim=-1))

    def _heads_fusable(self, ht_feat):
        """The shapes csrc/neck_train.hip has register tiles for, and exactly the reference's layer types (a converted
        ``SyncBatchNorm`` needs cross-rank statistics and takes the layer path)."""
        vfe = self.ObtainVoxelFeature
        conv, bn = vfe.conv[0], vfe.conv[1]
        C = ht_feat.shape[1]
        heads = ((self.S_MLP, ScaleFactorMLP, C, 3), (self.R_MLP, RotationFactorMLP, C, 4),
                 (self.A_MLP, OpacityFactorMLP, C, 1), (self.C_MLP, ColorFactorMLPGaussian, C + 3, 3))
        return (ht_feat.is_cuda and ht_feat.dtype == torch.float32 and self.num_height in (1, 2, 4, 6, 8, 13)
                and type(conv) is nn.Conv3d and conv.in_channels == 1 and conv.kernel_size == (1, 1, 1)
                and conv.out_channels == self.num_height
                and type(bn) is nn.BatchNorm3d and bn.affine and bn.track_running_stats
                and all(type(m) is cls and m.fc1.in_features == cin and m.fc1.out_features == 4
                        and m.fc2.out_features == cout and m.fc1.bias is not None and m.fc2.bias is not None
                        for m, cls, cin, cout in heads))

    # -------------------------------------------------------------------------------- training losses
    def _fused_loss_inputs(self, *tensors):
        return self.fused_losses and all(t.is_cuda for t in tensors)

    def get_downsampled_gt_depth_and_semantic(self, gt_depths, gt_semantics):
        """:1203-1282 -> (depth_labels (B*N*h*w, D), semantic_labels (B*N*h*w, 2)).  The gt tensors are not written
        (the reference zeroes their out-of-range depths in place)."""
        if self._fused_loss_inputs(gt_depths, gt_semantics) and not (gt_depths.requires_grad or gt_semantics.requires_grad):
            return losses.depth_labels(gt_depths, gt_semantics, self.grid_config['depth'], self.D, self.downsample)
        return losses.depth_labels_torch(gt_depths, gt_semantics, self.grid_config['depth'], self.D, self.downsample)

    def get_depth_and_semantic_loss(self, depth_labels, depth_preds, semantic_labels, semantic_preds):
        """:1284-1314 -> (loss_depth_weight * depth BCE, loss_semantic_weight * focal BCE); no host read."""
        if (self._fused_loss_inputs(depth_labels, depth_preds, semantic_labels, semantic_preds)
                and not (depth_labels.requires_grad or semantic_labels.requires_grad)):
            return losses.depth_semantic_loss(depth_labels, depth_preds, semantic_labels, semantic_preds,
                                              self.loss_depth_weight, self.loss_semantic_weight)
        return losses.depth_semantic_loss_torch(depth_labels, depth_preds.float(), semantic_labels,
                                                semantic_preds.float(), self.loss_depth_weight, self.loss_semantic_weight)

    def depth_l1_loss(self, pred_depth, gt_depth):
        return F.l1_loss(pred_depth, gt_depth)

    def Box2dtoMask(self, gt_bboxes, new_width, new_height, device=None):
        """:1337-1352 -> (1,3,H,W) float mask on ``device`` (default: the boxes' device), without a host loop."""
        m = losses.box_mask(gt_bboxes, new_width, new_height, device)
        return m.view(1, 1, new_height, new_width).repeat(1, 3, 1, 1)

    @_float32_under_autocast
    def get_loss(self, depth, semantic, gt_depth, gt_semantic, gt_bboxes, cam_idx_list, render_imgs, gt_images,
                 render_image_G_all, render_image_N_all, render_depth, render_depth_G_all, render_depth_N_all):
        """:1354-1417 -> (loss_depth, loss_ce_semantic, color_loss, ssim_loss, render_depth_loss).  ``cam_idx_list``:
        the forward's camera of each sample (host ints); ``gt_bboxes[b][cam]`` the (n,4) 2D boxes of that camera.
        On the GPU the three parts run as the fused kernels of csrc/losses.hip: no host synchronisation.  Deviations
        (INTEGRATION.md): the debug ``visualize_images`` call is dropped, the gt tensors are not written, the iteration
        counter is ``self.loss_iteration``."""
        self.loss_iteration += 1
        use_mask = self.loss_iteration > losses.MASK_AFTER_ITERATION
        depth_labels, semantic_labels = self.get_downsampled_gt_depth_and_semantic(gt_depth, gt_semantic)
        loss_depth, loss_ce_semantic = self.get_depth_and_semantic_loss(depth_labels, depth, semantic_labels, semantic)
        B = render_imgs.shape[0]
        boxes = [gt_bboxes[b][cam_idx_list[b]] for b in range(B)]
        renders = (render_imgs, render_image_G_all, render_image_N_all)
        render_depths = (render_depth, render_depth_G_all, render_depth_N_all)
        depth_range = self.grid_config['depth'][:2]
        if (self._fused_loss_inputs(gt_images, gt_depth, *renders, *render_depths)
                and not (gt_images.requires_grad or gt_depth.requires_grad)):
            color_loss, ssim_loss, render_depth_loss = losses.render_losses(
                gt_images, renders, render_depths, gt_depth, cam_idx_list, boxes, use_mask, depth_range)
        else:
            H, W = gt_images.shape[2:]
            masks = [self.Box2dtoMask(bx, W, H, device=gt_images.device) if use_mask else None for bx in boxes]
            color_loss, ssim_loss, render_depth_loss = losses.render_losses_torch(
                gt_images, renders, render_depths, gt_depth, cam_idx_list, masks, depth_range)
        return loss_depth, loss_ce_semantic, color_loss, ssim_loss, render_depth_loss

    # -------------------------------------------------------------------------------- forward
    def forward(self, input, stereo_metas=None):
        """:1319-1334.  ``input``: the 12-entry ``img_inputs`` list."""
        if self.depth_net is None:
            raise RuntimeError('OcRFViewTransformerFull.forward needs a depth_net (pass depth_net=... or install '
                               'the reference mmdet3d); view_transform_core() runs without it')
        x, mlp_input = input[0], input[7]
        B, N, C, H, W = x.shape
        y = self.depth_net(x.view(B * N, C, H, W), mlp_input, stereo_metas)
        if y.dtype == torch.bfloat16:               # a DepthNet under bf16 autocast; from here on float32
            y = y.float()
        if y.is_cuda and not self.training and not self._recording(y):
            depth, filter_depth, semantic, feat_cl = neck_ops.prefilter(y, self.D, self.out_channels,
                                                                        self.depth_threshold, self.semantic_threshold)
            bev_feat, _, bev_mask, extras = self.view_transform(input, filter_depth, None, feat_cl)
        else:
            depth = y[:, :self.D].softmax(dim=1)
            semantic = y[:, self.D:self.D + 2].softmax(dim=1)
            tran_feat = y[:, self.D + 2:self.D + 2 + self.out_channels]
            filter_depth = torch.where(depth < self.depth_threshold, torch.zeros_like(depth), depth)
            filter_feat = (semantic[:, 1:2] >= self.semantic_threshold) * tran_feat
            bev_feat, _, bev_mask, extras = self.view_transform(input, filter_depth, filter_feat)
        return bev_feat, depth, (bev_mask, semantic), extras

    def get_mlp_input(self, rot, tran, intrin, post_rot, post_tran, bda):
        """27 camera-aware scalars per view for the DepthNet's SE layers (view_transformer.py:696-722)."""
        B, N = rot.shape[:2]
        bda = bda.view(B, 1, 3, 3).repeat(1, N, 1, 1)
        v = torch.stack([intrin[:, :, 0, 0], intrin[:, :, 1, 1], intrin[:, :, 0, 2], intrin[:, :, 1, 2],
                         post_rot[:, :, 0, 0], post_rot[:, :, 0, 1], post_tran[:, :, 0], post_rot[:, :, 1, 0],
                         post_rot[:, :, 1, 1], post_tran[:, :, 1], bda[:, :, 0, 0], bda[:, :, 0, 1], bda[:, :, 1, 0],
                         bda[:, :, 1, 1], bda[:, :, 2, 2]], dim=-1)
        s2e = torch.cat([rot, tran.reshape(B, N, 3, 1)], dim=-1).reshape(B, N, -1)
        return torch.cat([v, s2e], dim=-1)
