"""Geometry distillation of ``OcRFDet4DVGGT`` (mmdet3d/models/detectors/ocrfdet_vggt.py, bevdet_vggt.py:16-49) without
mmcv, mmdet or mmdet3d: what the detector's key-frame branch is made of.

* ``build_cost_volume``: the reference's signature (ocrfdet_vggt.py:175-230).  ``'group_corr'``, the one method the
  detector calls, is implemented: ``out[b, g, d, h, w] = sum_c L[b, g Cg + c, h, w] * R[b, g Cg + c, h, max(w - d, 0)]``
  for ``d = 0 .. max_disp``, with L, R = ``feats[:, 0]``, ``feats[:, 1]``.  ``group_corr_volume`` is the fused form: one
  HIP launch that reads each feature once (``ocrf_group_corr_forward``; the backward, two gathers, writes straight into
  the two halves of the gradient of ``feats``).  ``group_corr_volume_torch`` is the same sum as ``D`` shifted products,
  without the reference's (B, G, D, Cg, H, W) expansion, on any device and dtype.
* ``kd_losses``: ``(loss_Smoothl1_KD, loss_cos_KD)`` of two volumes (ocrfdet_vggt.py:476-480): the fused form
  accumulates in double in a fixed two-stage order (``ocrf_kd_losses_forward`` / ``_backward``); ``kd_losses_torch`` is the
  reference's three lines.  Only the first volume gets a gradient from the fused form.
* ``CrossAttentionAlign``, ``resize_img``, ``get_pair_indices``: the reference's, in torch.

Neither fused op reads anything back to the host.  Under ``torch.autocast`` both run in float32 on ``.float()``
operands, like the package's other fused ops.
"""
import random

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib

FUSED_DISTILL_DEFAULT = True
MAX_DISPARITIES = 16                  # include/ocrf_hip.h: 1 <= D <= 16
_HALVES = (torch.float16, torch.bfloat16)


# ------------------------------------------------------------------------------------------------ the volume
def _check_feats(feats, groups, max_disp):
    if feats.dim() != 5 or feats.shape[1] != 2:
        raise ValueError(f'feats must be (B, 2, C, H, W), got {tuple(feats.shape)}')
    if int(max_disp) < 0:
        raise ValueError(f'max_disp must be >= 0, got {max_disp}')
    if feats.shape[2] % int(groups):
        raise ValueError(f'{feats.shape[2]} channels are not {groups} groups')


def group_corr_volume_torch(feats, max_disp=8, groups=32):
    """The group-wise correlation volume (B, groups, max_disp + 1, H, W) in torch: for every disparity ``d`` the right
    view shifted by ``d`` columns (its column 0 repeated on the left: the reference's ``clamp(idx - d, min=0)``) times the
    left view, summed over the channels of a group.  Any device, any floating dtype, differentiable."""
    _check_feats(feats, groups, max_disp)
    B, _, C, H, W = feats.shape
    G, D = int(groups), int(max_disp) + 1
    left = feats[:, 0].reshape(B, G, C // G, H, W)
    right = feats[:, 1].reshape(B, G, C // G, H, W)
    planes = []
    for d in range(D):
        k = min(d, W)
        shifted = right if k == 0 else torch.cat([right[..., :1].expand(B, G, C // G, H, k), right[..., :W - k]], dim=-1)
        planes.append((left * shifted).sum(dim=2))
    return torch.stack(planes, dim=2)


def _batch_stride(view):
    """Floats between the samples of a (B, C, H, W) view with contiguous (C, H, W) blocks (B = 1: torch's stride of a
    dimension of size 1 means nothing)."""
    return view.stride(0) if view.shape[0] > 1 else view.shape[1] * view.shape[2] * view.shape[3]


def _is_view_pair(left, right):
    if left.dim() != 4:
        return False
    C, H, W = left.shape[1:]
    return (left.shape == right.shape and left.dtype == right.dtype == torch.float32
            and left.is_cuda and left.device == right.device and left.numel() > 0
            and left.stride()[1:] == right.stride()[1:] == (H * W, W, 1)
            and _batch_stride(left) == _batch_stride(right) >= C * H * W)


def corr_forward_views(left, right, groups, num_disp):
    """One forward launch on two (B, C, H, W) float32 CUDA views with contiguous (C, H, W) blocks and one batch stride,
    such as the halves of a (B, 2, C, H, W) tensor or two contiguous tensors: the volume (B, groups, num_disp, H, W).
    Records no gradient."""
    _lib.require_cuda(left, right)
    if not _is_view_pair(left, right):
        raise _lib.OcrfHipError('corr_forward_views takes two non-empty float32 (B, C, H, W) views of one shape and batch '
                                'stride on one GPU, with contiguous (C, H, W) blocks')
    B, C, H, W = left.shape
    out = torch.empty(B, int(groups), int(num_disp), H, W, dtype=torch.float32, device=left.device)
    _lib.launch('ocrf_group_corr_forward', left.device, B, C, H, W, int(groups), int(num_disp), left, right,
                _batch_stride(left), out)
    return out


class _GroupCorr(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, feats, groups, num_disp):
        out = corr_forward_views(feats[:, 0], feats[:, 1], groups, num_disp)
        ctx.save_for_backward(feats)
        ctx.groups, ctx.num_disp = groups, num_disp
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type='cuda')
    def backward(ctx, grad_out):
        feats, = ctx.saved_tensors
        B, _, C, H, W = feats.shape
        grad = torch.empty_like(feats)
        _lib.launch('ocrf_group_corr_backward', feats.device, B, C, H, W, ctx.groups, ctx.num_disp, grad_out.contiguous(),
                    feats[:, 0], feats[:, 1], 2 * C * H * W, grad[:, 0], grad[:, 1], 2 * C * H * W)
        return grad, None, None


def _float32_operand(t):
    """float32, or under CUDA autocast a float16 / bfloat16 tensor, which the fused ops compute in float32."""
    return t.dtype == torch.float32 or (t.dtype in _HALVES and torch.is_autocast_enabled('cuda'))


def corr_fusable(feats, max_disp=8):
    """The kernels take this: a non-empty contiguous float32 (B, 2, C, H, W) CUDA tensor (under autocast also a float16
    or bfloat16 one) and at most 16 disparities."""
    return (feats.dim() == 5 and feats.shape[1] == 2 and feats.is_cuda and _float32_operand(feats)
            and feats.is_contiguous() and feats.numel() > 0 and 0 <= int(max_disp) < MAX_DISPARITIES)


def group_corr_volume(feats, max_disp=8, groups=32):
    """``group_corr_volume_torch`` as one HIP launch, differentiable (the backward: two launches, both gathers, no
    atomics).  ``feats``: contiguous float32 on the GPU, ``max_disp`` at most 15; anything else raises.  The two views
    are read in place: no copy is made."""
    _check_feats(feats, groups, max_disp)
    _lib.require_cuda(feats)
    if not corr_fusable(feats, max_disp):
        raise _lib.OcrfHipError('group_corr_volume takes a non-empty contiguous float32 (B, 2, C, H, W) tensor on the GPU '
                                f'and max_disp < {MAX_DISPARITIES}; got {feats.dtype}, contiguous={feats.is_contiguous()}, '
                                f'max_disp={max_disp}')
    return _GroupCorr.apply(feats.float(), int(groups), int(max_disp) + 1)


def build_cost_volume(feats, max_disp=8, method='concat', groups=32, fused=None):
    """``OcRFDet4DVGGT.build_cost_volume`` (ocrfdet_vggt.py:175-230) for ``feats`` (B, 2, C, H, W).

    ``method='group_corr'``: (B, groups, max_disp + 1, H, W).  ``fused`` None (``FUSED_DISTILL_DEFAULT``): the HIP kernel
    where ``corr_fusable`` accepts the tensor, the torch formulation everywhere else; True: the kernel or an error;
    False: ``group_corr_volume_torch``.

    ``'concat'`` and ``'variance'`` raise ``NotImplementedError``: the reference's own code for them fails (``concat`` in
    its ``permute`` of a tensor indexed to six dimensions, ``variance`` in ``expand`` unless D == H), so there is no
    result to match."""
    if method in ('concat', 'variance'):
        raise NotImplementedError(f"build_cost_volume(method='{method}'): the reference's own code for it fails (concat "
                                  "in permute, variance in expand unless D == H); only 'group_corr' is implemented")
    if method != 'group_corr':
        raise ValueError('Unknown method')
    if fused is None:
        fused = FUSED_DISTILL_DEFAULT and corr_fusable(feats, max_disp)
    if fused:
        return group_corr_volume(feats, max_disp, groups)
    return group_corr_volume_torch(feats, max_disp, groups)


# ------------------------------------------------------------------------------------------------ the two losses
def kd_losses_torch(volume_s, volume_t):
    """``(loss_Smoothl1_KD, loss_cos_KD)`` as the reference computes them (ocrfdet_vggt.py:476-480)."""
    smooth = F.smooth_l1_loss(volume_s, volume_t, beta=1.0) * 0.1
    cos = 1 - F.cosine_similarity(volume_s.flatten(1), volume_t.flatten(1), dim=1).mean()
    return smooth, cos


class _KDLosses(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, s, t):
        B, n = s.shape
        dev = s.device
        smooth = torch.empty((), dtype=torch.float32, device=dev)
        cos = torch.empty((), dtype=torch.float32, device=dev)
        sums = torch.empty(B, 3, dtype=torch.float64, device=dev)
        nbytes = _lib.lib().ocrf_kd_losses_workspace_bytes(B, n)
        if nbytes == 0:
            raise _lib.OcrfHipError(f'kd_losses: ({B}, {n}) is beyond the kernels\' limits (B * n < 2^31)')
        ws = _lib.workspace.get(dev, nbytes, 'kd_losses')
        _lib.launch('ocrf_kd_losses_forward', dev, B, n, s, t, smooth, cos, sums, ws, nbytes)
        ctx.save_for_backward(s, t, sums)
        return smooth, cos

    @staticmethod
    @torch.amp.custom_bwd(device_type='cuda')
    def backward(ctx, grad_smooth, grad_cos):
        s, t, sums = ctx.saved_tensors
        B, n = s.shape
        grad_s = torch.empty_like(s)
        _lib.launch('ocrf_kd_losses_backward', s.device, B, n, s, t, sums, grad_smooth.float().contiguous(),
                    grad_cos.float().contiguous(), grad_s)
        return grad_s, None


def kd_fusable(volume_s, volume_t):
    """The kernels take these: two non-empty contiguous float32 CUDA tensors of one shape (B, ...) on one device."""
    return (volume_s.shape == volume_t.shape and volume_s.dim() >= 2 and volume_s.is_cuda
            and volume_s.device == volume_t.device and _float32_operand(volume_s) and _float32_operand(volume_t)
            and volume_s.is_contiguous() and volume_t.is_contiguous() and volume_s.numel() > 0)


def kd_losses(volume_s, volume_t, fused=None):
    """``(loss_Smoothl1_KD, loss_cos_KD)`` between two volumes (B, ...): ``0.1 * smooth_l1(s, t, beta=1)`` over all
    elements and ``1 - mean_b(cosine_similarity(s_b, t_b))`` over the flattened samples, each a 0-dim float32 tensor.

    ``fused`` None (``FUSED_DISTILL_DEFAULT``): the HIP kernels where ``kd_fusable`` accepts the operands (two launches
    forward, one backward, sums in double, no host read), ``kd_losses_torch`` everywhere else; True: the kernels or an
    error; False: ``kd_losses_torch``.  The kernels give ``volume_s`` its gradient and ``volume_t``, the teacher, none."""
    if fused is None:
        fused = FUSED_DISTILL_DEFAULT and kd_fusable(volume_s, volume_t)
    if not fused:
        return kd_losses_torch(volume_s, volume_t)
    _lib.require_cuda(volume_s, volume_t)
    if not kd_fusable(volume_s, volume_t):
        raise _lib.OcrfHipError('kd_losses takes two non-empty contiguous float32 tensors of one shape (B, ...) on one '
                                f'GPU; got {tuple(volume_s.shape)} {volume_s.dtype} and {tuple(volume_t.shape)} '
                                f'{volume_t.dtype}')
    return _KDLosses.apply(volume_s.float().flatten(1), volume_t.detach().float().flatten(1))


# ------------------------------------------------------------------------------------------------ the branch's modules
class CrossAttentionAlign(nn.Module):
    """``CrossAttentionAlign`` (bevdet_vggt.py:16-49) with the reference's parameter names, hence ``state_dict`` keys:
    the student's pixels (``res_feat`` (B, N, res_dim, h, w)) query the teacher's patch tokens (``vit_feat`` (B, N,
    vit_dim, H, W)) through one multi-head attention; the result is projected and resized bilinearly to the teacher's
    grid: (B, N, vit_dim, H, W)."""

    def __init__(self, res_dim=256, vit_dim=2048, num_heads=8):
        super().__init__()
        self.query_proj = nn.Linear(res_dim, vit_dim)
        self.key_proj = nn.Linear(vit_dim, vit_dim)
        self.value_proj = nn.Linear(vit_dim, vit_dim)
        self.attn = nn.MultiheadAttention(embed_dim=vit_dim, num_heads=num_heads, batch_first=True)
        self.output_proj = nn.Linear(vit_dim, vit_dim)

    def forward(self, res_feat, vit_feat):
        B, N, c_res, h, w = res_feat.shape
        c_vit, H, W = vit_feat.shape[2:]
        pixels = res_feat.reshape(B * N, c_res, h * w).transpose(1, 2)
        tokens = vit_feat.reshape(B * N, c_vit, H * W).transpose(1, 2)
        aligned, _ = self.attn(self.query_proj(pixels), self.key_proj(tokens), self.value_proj(tokens), need_weights=False)
        # NCHW in memory before the resize: interpolate keeps its input's layout, and the volume reads contiguous planes
        aligned = self.output_proj(aligned).transpose(1, 2).reshape(B * N, c_vit, h, w).contiguous()
        aligned = F.interpolate(aligned, size=(H, W), mode='bilinear', align_corners=False)
        return aligned.view(B, N, c_vit, H, W)


def resize_img(img, new_h=294, new_w=518):
    """``OcRFDet4DVGGT.resize_img``: (B, V, C, H, W) resized bilinearly (``align_corners=False``) to (B, V, C, new_h,
    new_w)."""
    B, V, C, H, W = img.shape
    out = F.interpolate(img.reshape(B * V, C, H, W), size=(new_h, new_w), mode='bilinear', align_corners=False)
    return out.view(B, V, C, new_h, new_w)


def get_pair_indices(rng=random):
    """``OcRFDet4DVGGT.get_pair_indices``: a camera ``i1 = rng.randint(0, 5)`` and its neighbour ``(i1 + 1) % 6``, with
    the neighbours 5 and 3 exchanged: (0, 1), (1, 2), (2, 5), (3, 4), (4, 3), (5, 0).  ``rng``: the ``random`` module
    (one draw, as the reference makes it, so that a seeded run draws its pairs) or a ``random.Random``."""
    i1 = rng.randint(0, 5)
    i2 = (i1 + 1) % 6
    return i1, {5: 3, 3: 5}.get(i2, i2)
