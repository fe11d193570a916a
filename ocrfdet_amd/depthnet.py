"""The stereo depth network of the neck: the reference's ``DepthNet`` (view_transformer.py:464-626) with its submodules
``Mlp``, ``SELayer``, ``ASPP`` / ``_ASPPModule`` (:316-462), written from their structure with the same constructor
arguments and the same ``state_dict`` keys and shapes, and mmdet 2.x's ``BasicBlock`` from ``blocks.py``.

The convolutions are stock PyTorch-ROCm layers (MIOpen).  The one operation that is not a convolution, the stereo cost
volume (``gen_grid`` + ``calculate_cost_volumn``, :538-596), has two formulations of the same arithmetic:

* the fused one, ``ocrf_stereo_cost_volume`` (csrc/stereo.hip): one launch writes the softmax over depth, reading each
  feature map about once; no warped (BN, 4, D*H, W) tensor per channel group, no host synchronisation;
* the torch one, ``stereo_cost_volume_torch``: the CPU path, and the GPU path when ``DepthNet.fused_cost_volume`` is
  False.  Its 3x3 inverses are closed-form as in the kernel, so it does not synchronise either.

bfloat16 features (an image encoder under bf16 autocast) are cast to float32 for the kernel by default.  Opt-in
(``DepthNet.fused_cost_volume_bf16``, ``stereo_cost_volume(..., keep_bf16=True)``) they stay bfloat16: two
``ocrf_stereo_pack_bf16`` launches put 8 channels of a pixel side by side and ``ocrf_stereo_cost_volume_bf16``
(csrc/stereo_bf16.hip) gathers them 16 bytes at a time; the float32 volume is bit for bit the default's.

Both run under ``no_grad`` as in the reference (:617): the cost volume has no backward.  ``use_dcn=True`` (the
reference's default, :515-526) is refused unless ``NATIVE_DCN`` is set: then ``deform_conv.DeformConv2dPack`` follows the
ASPP as in the reference.
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.utils.checkpoint import checkpoint

from . import _lib
from . import deform_conv
from .blocks import BasicBlock, kaiming_init, unfuse_tails

__all__ = ['BasicBlock', 'Mlp', 'SELayer', 'ASPP', '_ASPPModule', 'DepthNet', 'stereo_cost_volume',
           'stereo_cost_volume_torch', 'stereo_cost_volume_hip', 'stereo_cost_volume_hip_bf16', 'stereo_pack_bf16',
           'stereo_pack_bf16_torch', 'stereo_grid_torch', 'supports']

GROUP = 4                   # channels per group of the reference's loop (:580)
PLANE_BYTES_MAX = 2 ** 32 - 1   # one camera's prev in bytes: the kernel addresses it in unsigned 32-bit
PACK = 8                    # channels per pixel of a packed bfloat16 block: two groups, 16 bytes
PACKED_BYTES_MAX = 2 ** 32 - 1  # one camera's packed bfloat16 prev in bytes, addressed likewise
# use_dcn=True builds the native deformable convolution (deform_conv.DeformConv2dPack).  Off by default: while it is
# False, use_dcn=True is refused and ``supports({})`` is False, as before the native operator existed
NATIVE_DCN = False


# --------------------------------------------------------------------------------------------- building blocks
class _ASPPModule(nn.Module):
    """Atrous conv (no bias) + BN + ReLU."""

    def __init__(self, inplanes, planes, kernel_size, padding, dilation, BatchNorm=nn.BatchNorm2d):
        super().__init__()
        self.atrous_conv = nn.Conv2d(inplanes, planes, kernel_size, stride=1, padding=padding, dilation=dilation,
                                     bias=False)
        self.bn = BatchNorm(planes)
        self.relu = nn.ReLU()
        kaiming_init(self, mode='fan_in')

    def forward(self, x):
        return self.relu(self.bn(self.atrous_conv(x)))


class ASPP(nn.Module):
    """Four atrous branches (dilations 1, 6, 12, 18) and a global-pool branch, concatenated, 1x1 conv + BN + ReLU,
    dropout 0.5."""

    def __init__(self, inplanes, mid_channels=256, BatchNorm=nn.BatchNorm2d):
        super().__init__()
        for i, dil in enumerate((1, 6, 12, 18)):
            k, pad = (1, 0) if dil == 1 else (3, dil)
            setattr(self, f'aspp{i + 1}', _ASPPModule(inplanes, mid_channels, k, pad, dil, BatchNorm))
        self.global_avg_pool = nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)),
                                             nn.Conv2d(inplanes, mid_channels, 1, stride=1, bias=False),
                                             BatchNorm(mid_channels), nn.ReLU())
        self.conv1 = nn.Conv2d(5 * mid_channels, inplanes, 1, bias=False)
        self.bn1 = BatchNorm(inplanes)
        self.relu = nn.ReLU()
        self.dropout = nn.Dropout(0.5)
        kaiming_init(self, mode='fan_in')

    def forward(self, x):
        branches = [self.aspp1(x), self.aspp2(x), self.aspp3(x), self.aspp4(x)]
        pooled = self.global_avg_pool(x)
        branches.append(F.interpolate(pooled, size=branches[3].shape[2:], mode='bilinear', align_corners=True))
        return self.dropout(self.relu(self.bn1(self.conv1(torch.cat(branches, dim=1)))))


class Mlp(nn.Module):
    """fc1 -> act -> dropout -> fc2 -> dropout."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.ReLU, drop=0.0):
        super().__init__()
        hidden_features = hidden_features or in_features
        out_features = out_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.drop1 = nn.Dropout(drop)
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop2 = nn.Dropout(drop)

    def forward(self, x):
        return self.drop2(self.fc2(self.drop1(self.act(self.fc1(x)))))


class SELayer(nn.Module):
    """x * sigmoid(expand(relu(reduce(x_se)))), both 1x1 convolutions with bias."""

    def __init__(self, channels, act_layer=nn.ReLU, gate_layer=nn.Sigmoid):
        super().__init__()
        self.conv_reduce = nn.Conv2d(channels, channels, 1, bias=True)
        self.act1 = act_layer()
        self.conv_expand = nn.Conv2d(channels, channels, 1, bias=True)
        self.gate = gate_layer()

    def forward(self, x, x_se):
        return x * self.gate(self.conv_expand(self.act1(self.conv_reduce(x_se))))


# --------------------------------------------------------------------------------------------- cost volume
def _inv3(m):
    """Closed-form inverse of (..., 3, 3) matrices (adjugate / determinant): no LAPACK call, no ``info`` check, so no
    host synchronisation on the GPU.  The same formula as the kernel's."""
    a = [[m[..., i, j] for j in range(3)] for i in range(3)]
    c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1]
    c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2]
    c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0]
    inv_det = 1.0 / (a[0][0] * c00 + a[0][1] * c01 + a[0][2] * c02)
    rows = [[c00, a[0][2] * a[2][1] - a[0][1] * a[2][2], a[0][1] * a[1][2] - a[0][2] * a[1][1]],
            [c01, a[0][0] * a[2][2] - a[0][2] * a[2][0], a[0][2] * a[1][0] - a[0][0] * a[1][2]],
            [c02, a[0][1] * a[2][0] - a[0][0] * a[2][1], a[0][0] * a[1][1] - a[0][1] * a[1][0]]]
    return torch.stack([torch.stack([e * inv_det for e in r], -1) for r in rows], -2)


def _mv(m, x, y, z):
    """Rows of m (BN, 1, 1, 1, 3, 3) applied to (x, y, z), k ascending."""
    return tuple(m[..., i, 0] * x + m[..., i, 1] * y + m[..., i, 2] * z for i in range(3))


def stereo_grid_torch(metas, H, W):
    """Normalised sample grid (BN, D, H, W, 2) of ``gen_grid``: the image size is (4 H, 4 W), cells whose depth
    before the intrinsics is below 1e-3 get -2."""
    fr = metas['frustum']
    B, N, _ = metas['post_trans'].shape
    BN = B * N
    view = lambda t, *s: t.reshape(BN, 1, 1, 1, *s)          # noqa: E731
    pt = view(metas['post_trans'].float(), 3)
    pr = metas['post_rots'].float().reshape(BN, 3, 3)
    K = metas['intrins'].float().reshape(BN, 3, 3)
    S = metas['k2s_sensor'].float().reshape(BN, 4, 4)
    comb = view(S[:, :3, :3] @ _inv3(K), 3, 3)
    K, pri = view(K, 3, 3), view(_inv3(pr), 3, 3)
    t = view(S[:, :3, 3].contiguous(), 3)
    u, v, d = (fr[..., i].unsqueeze(0) for i in range(3))
    x, y, z = _mv(pri, u - pt[..., 0], v - pt[..., 1], d - pt[..., 2])
    x, y, z = _mv(comb, x * z, y * z, z)
    x, y, z = x + t[..., 0], y + t[..., 1], z + t[..., 2]
    neg = ~(z >= 1e-3)
    x, y, z = _mv(K, x, y, z)
    x, y = x / z, y / z
    p2 = view(pr[:, :2, :2].contiguous(), 2, 2)
    sx = p2[..., 0, 0] * x + p2[..., 0, 1] * y + pt[..., 0]
    sy = p2[..., 1, 0] * x + p2[..., 1, 1] * y + pt[..., 1]
    m2 = torch.full_like(sx, -2.0)
    px = torch.where(neg, m2, sx / (4.0 * W - 1.0) * 2.0 - 1.0)
    py = torch.where(neg, m2, sy / (4.0 * H - 1.0) * 2.0 - 1.0)
    return torch.stack([px, py], -1)


def _split(metas):
    prev, curr = metas['cv_feat_list']
    D, H, W, _ = metas['frustum'].shape
    B, N, _ = metas['post_trans'].shape
    prev, curr = prev.reshape(B * N, -1, H, W), curr.reshape(B * N, -1, H, W)
    return prev, curr, B * N, curr.shape[1], D, H, W


def stereo_cost_volume_torch(metas, bias, raw=False):
    """Torch formulation: per group of 4 channels one ``grid_sample`` (align_corners, zeros padding) of ``prev`` and
    the absolute difference to ``curr`` summed over the group, the group sums added; ``bias`` where the warp of
    channel 4 (C // 4 - 1) is exactly 0.  Returns softmax_D(raw), or raw = -(cost + bias [warp == 0])."""
    prev, curr, BN, C, D, H, W = _split(metas)
    G = C // GROUP
    if G < 1:
        raise ValueError(f'the stereo cost volume needs at least {GROUP} channels, got {C}')
    grid = stereo_grid_torch(metas, H, W).to(curr.dtype).reshape(BN, D * H, W, 2)
    cost = None
    for g in range(G):
        sl = slice(g * GROUP, (g + 1) * GROUP)
        warp = F.grid_sample(prev[:, sl], grid, mode='bilinear', padding_mode='zeros', align_corners=True)
        part = (curr[:, sl].unsqueeze(2) - warp.view(BN, GROUP, D, H, W)).abs().sum(1)
        cost = part if cost is None else cost + part
    if bias != 0:
        cost = cost + bias * (warp[:, 0].view(BN, D, H, W) == 0)
    raw_cost = -cost
    return raw_cost if raw else raw_cost.softmax(1)


def _checked_split(metas):
    """``_split`` for features that both kernels take: one channel count, a group or more."""
    prev, curr, BN, C, D, H, W = _split(metas)
    if C < GROUP or prev.shape[1] != C:
        raise ValueError(f'stereo features must have the same channel count >= {GROUP}: {prev.shape} vs {curr.shape}')
    return prev, curr, BN, C, D, H, W


def _launch_cost_volume(entry, metas, bias, raw, prev, curr, BN, C, D, H, W):
    """One launch of ``entry`` on the features as its kernel reads them.  The frustum axes are passed as strided views of
    ``metas['frustum']``; the small calibration tensors are moved to the features' device if they are elsewhere."""
    dev = curr.device
    cal = [metas[k].detach().to(dev, torch.float32).reshape(BN, -1).contiguous()
           for k in ('k2s_sensor', 'intrins', 'post_rots', 'post_trans')]
    fr = metas['frustum'].detach().to(dev, torch.float32)
    u, v, d = fr[0, 0, :, 0], fr[0, :, 0, 1], fr[:, 0, 0, 2]
    out = torch.empty(BN, D, H, W, device=dev)
    _lib.launch(entry, dev, BN, C, H, W, D, prev, curr, u, u.stride(0), v, v.stride(0), d, d.stride(0), *cal,
                float(bias), 1 if raw else 0, out)
    return out


def stereo_cost_volume_hip(metas, bias, raw=False):
    """``stereo_cost_volume_torch`` by ``ocrf_stereo_cost_volume``: one launch, forward only, deterministic, on the
    features cast to float32."""
    prev, curr, BN, C, D, H, W = _checked_split(metas)
    if C * H * W * 4 > PLANE_BYTES_MAX or D * H * W >= 2 ** 31:
        raise ValueError(f'stereo cost volume: C * H * W * 4 = {C * H * W * 4} bytes per camera must be at most '
                         f'2^32 - 1 (32-bit plane addressing) and D * H * W = {D * H * W} below 2^31')
    _lib.require_cuda(prev, curr)
    prev, curr = prev.detach().float().contiguous(), curr.detach().float().contiguous()
    return _launch_cost_volume('ocrf_stereo_cost_volume', metas, bias, raw, prev, curr, BN, C, D, H, W)


def packed_blocks(C):
    """Blocks of ``PACK`` channels that hold the C // 4 whole groups of C channels."""
    return (C // GROUP + 1) // 2


def stereo_pack_bf16_torch(x):
    """(BN, C, H, W) -> (BN, NB, H, W, 8), the layout ``ocrf_stereo_cost_volume_bf16`` reads, by torch ops on any
    device: ``out[n, b, y, x, k] = x[n, 8 b + k, y, x]`` for the channels of the C // 4 whole groups, +0 in the upper half
    of the last block when their number is odd; channels past the last whole group are dropped."""
    BN, C, H, W = x.shape
    G, NB = C // GROUP, packed_blocks(C)
    out = x.new_zeros(BN, NB * PACK, H, W)
    out[:, :GROUP * G] = x[:, :GROUP * G]
    return out.view(BN, NB, PACK, H, W).permute(0, 1, 3, 4, 2).contiguous()


def stereo_pack_bf16(x):
    """``stereo_pack_bf16_torch`` of a CUDA bfloat16 tensor by ``ocrf_stereo_pack_bf16``: one launch that writes every
    element of the result."""
    _lib.require_cuda(x)
    if x.dtype != torch.bfloat16 or x.dim() != 4:
        raise ValueError(f'stereo_pack_bf16 takes a (BN, C, H, W) bfloat16 tensor, got {tuple(x.shape)} {x.dtype}')
    BN, C, H, W = x.shape
    if C < GROUP or BN < 1 or H < 2 or W < 2:
        raise ValueError(f'stereo_pack_bf16 needs at least {GROUP} channels and a 2 x 2 map, got {tuple(x.shape)}')
    NB = packed_blocks(C)
    if NB * H * W * PACK * 2 > PACKED_BYTES_MAX:
        raise ValueError(f'stereo_pack_bf16: {NB * H * W * PACK * 2} packed bytes per camera, at most 2^32 - 1 '
                         '(32-bit block addressing)')
    x = x.detach().contiguous()
    out = torch.empty(BN, NB, H, W, PACK, device=x.device, dtype=torch.bfloat16)
    _lib.launch('ocrf_stereo_pack_bf16', x.device, BN, C, H, W, x, out)
    return out


def _checked_packed(entry, name, like, BN, C, H, W):
    """A ``cv_feat_packed`` entry for features ``like`` (BN, C, H, W): the layout ``stereo_pack_bf16`` writes."""
    shape = (BN, packed_blocks(C), H, W, PACK)
    if not (isinstance(entry, torch.Tensor) and tuple(entry.shape) == shape and entry.dtype == torch.bfloat16
            and entry.is_contiguous() and entry.device == like.device):
        got = (tuple(entry.shape), entry.dtype, entry.device) if isinstance(entry, torch.Tensor) else type(entry)
        raise ValueError(f'cv_feat_packed[{name}] must be a contiguous bfloat16 {shape} tensor on {like.device} '
                         f'(stereo_pack_bf16 of the feature), got {got}')
    return entry.detach()


def stereo_cost_volume_hip_bf16(metas, bias, raw=False):
    """``stereo_cost_volume_hip`` for bfloat16 features without the cast to float32: two ``ocrf_stereo_pack_bf16``
    launches and ``ocrf_stereo_cost_volume_bf16``.  The float32 result holds the bits ``stereo_cost_volume_hip`` gives on
    ``.float()`` of the same features.

    ``metas['cv_feat_packed'] = [prev_packed | None, curr_packed | None]`` (optional): features the caller has packed
    already (``stereo_pack_bf16``; a streaming step keeps the previous frame's).  An entry that is given is not packed
    again; one of another shape, dtype or device raises ``ValueError`` before anything is launched."""
    prev, curr, BN, C, D, H, W = _checked_split(metas)
    if prev.dtype != torch.bfloat16 or curr.dtype != torch.bfloat16:
        raise ValueError(f'stereo_cost_volume_hip_bf16 takes bfloat16 features, got {prev.dtype} and {curr.dtype}')
    packed = packed_blocks(C) * H * W * PACK * 2
    if packed > PACKED_BYTES_MAX:
        raise ValueError(f'stereo cost volume: {packed} packed bytes per camera must be at most 2^32 - 1 (32-bit '
                         'block addressing)')
    if D * H * W >= 2 ** 31:
        raise ValueError(f'stereo cost volume: D * H * W = {D * H * W} must be below 2^31')
    given = metas.get('cv_feat_packed') or (None, None)
    if len(given) != 2:
        raise ValueError(f'cv_feat_packed holds [prev_packed, curr_packed], got {len(given)} entries')
    given = [None if e is None else _checked_packed(e, name, x, BN, C, H, W)
             for e, name, x in zip(given, ('prev', 'curr'), (prev, curr))]
    _lib.require_cuda(prev, curr)
    prev, curr = (stereo_pack_bf16(x) if e is None else e for e, x in zip(given, (prev, curr)))
    return _launch_cost_volume('ocrf_stereo_cost_volume_bf16', metas, bias, raw, prev, curr, BN, C, D, H, W)


def stereo_cost_volume(metas, bias, fused=True, raw=False, keep_bf16=False):
    """The kernel for CUDA float32 features when ``fused``, else the torch formulation (also on the CPU).  bfloat16
    features (an image encoder under bf16 autocast) take the kernel too, after its cast to float32: the volume is then
    float32, where the reference computes it in the features' dtype.  ``keep_bf16``: a CUDA bfloat16 pair skips that
    cast and takes ``stereo_cost_volume_hip_bf16`` (the same float32 volume, bit for bit); anything else goes where it
    goes without the flag."""
    prev, curr = metas['cv_feat_list']
    dtypes = (torch.float32, torch.bfloat16)
    if fused and curr.is_cuda and prev.is_cuda and curr.dtype in dtypes and prev.dtype in dtypes:
        if keep_bf16 and curr.dtype == prev.dtype == torch.bfloat16:
            return stereo_cost_volume_hip_bf16(metas, bias, raw)
        return stereo_cost_volume_hip(metas, bias, raw)
    return stereo_cost_volume_torch(metas, bias, raw)


# --------------------------------------------------------------------------------------------- DepthNet
def supports(cfg):
    """Whether ``DepthNet(..., **cfg)`` can be built natively: without deformable convolution, or with it when
    ``NATIVE_DCN`` is set."""
    return NATIVE_DCN or not cfg.get('use_dcn', True)


class DepthNet(nn.Module):
    """view_transformer.py:464-626.  ``forward(x, mlp_input, stereo_metas=None)`` returns cat(depth logits
    (depth_channels), context (context_channels)) along channels."""

    # bfloat16 stereo features keep their dtype up to ocrf_stereo_cost_volume_bf16 (two packs + one launch) instead of
    # being cast to float32 for ocrf_stereo_cost_volume; the volume is the same, bit for bit.  Off by default
    fused_cost_volume_bf16 = False

    def __init__(self, in_channels, mid_channels, context_channels, depth_channels, use_dcn=True, use_aspp=True,
                 with_cp=False, stereo=False, bias=0.0, aspp_mid_channels=-1):
        super().__init__()
        if use_dcn and not NATIVE_DCN:
            raise NotImplementedError('DepthNet(use_dcn=True) needs mmcv\'s deformable convolution; the native one is '
                                      'opt-in: set depthnet.NATIVE_DCN = True (INTEGRATION.md 3c, 3m)')
        self.reduce_conv = nn.Sequential(nn.Conv2d(in_channels, mid_channels, 3, stride=1, padding=1),
                                         nn.BatchNorm2d(mid_channels), nn.ReLU(inplace=True))
        self.context_conv = nn.Conv2d(mid_channels, context_channels, 1, stride=1, padding=0)
        self.bn = nn.BatchNorm1d(27)
        self.depth_mlp = Mlp(27, mid_channels, mid_channels)
        self.depth_se = SELayer(mid_channels)
        self.context_mlp = Mlp(27, mid_channels, mid_channels)
        self.context_se = SELayer(mid_channels)
        # the stereo branch feeds depth_channels - 2 cost channels (the frustum's D) into the first block
        first_in, downsample = mid_channels, None
        if stereo:
            cv = depth_channels - 2
            first_in = mid_channels + cv
            downsample = nn.Conv2d(first_in, mid_channels, 1, 1, 0)
            self.cost_volumn_net = nn.Sequential(nn.Conv2d(cv, cv, 3, stride=2, padding=1), nn.BatchNorm2d(cv),
                                                 nn.Conv2d(cv, cv, 3, stride=2, padding=1), nn.BatchNorm2d(cv))
            self.bias = bias
        layers = [BasicBlock(first_in, mid_channels, downsample=downsample), BasicBlock(mid_channels, mid_channels),
                  BasicBlock(mid_channels, mid_channels)]
        if use_aspp:
            layers.append(ASPP(mid_channels, mid_channels if aspp_mid_channels < 0 else aspp_mid_channels))
        if use_dcn:
            layers.append(deform_conv.build_dcn(dict(type='DCN', in_channels=mid_channels, out_channels=mid_channels,
                                                     kernel_size=3, padding=1, groups=4, im2col_step=128)))
        layers.append(nn.Conv2d(mid_channels, depth_channels, 1, stride=1, padding=0))
        self.depth_conv = nn.Sequential(*layers)
        # off because the tail is unmeasured at these shapes; flipping it is a separate change with its own
        # tools/time_bev_encoder.py row
        unfuse_tails(self.depth_conv)
        self.with_cp = with_cp
        self.depth_channels = depth_channels
        # the stereo cost volume by ocrf_stereo_cost_volume for CUDA float32 features; False: its torch formulation
        self.fused_cost_volume = True

    def cost_volume(self, stereo_metas):
        return stereo_cost_volume(stereo_metas, self.bias, fused=self.fused_cost_volume,
                                  keep_bf16=self.fused_cost_volume_bf16)

    def forward(self, x, mlp_input, stereo_metas=None):
        mlp_input = self.bn(mlp_input.reshape(-1, mlp_input.shape[-1]))
        x = self.reduce_conv(x)
        context = self.context_conv(self.context_se(x, self.context_mlp(mlp_input)[..., None, None]))
        depth = self.depth_se(x, self.depth_mlp(mlp_input)[..., None, None])
        if stereo_metas is not None:
            if stereo_metas['cv_feat_list'][0] is None:
                BN, _, H, W = x.shape
                scale = float(stereo_metas['downsample']) / stereo_metas['cv_downsample']
                cv = x.new_zeros((BN, self.depth_channels - 2, int(H * scale), int(W * scale)))
            else:
                with torch.no_grad():
                    cv = self.cost_volume(stereo_metas)
            depth = torch.cat([depth, self.cost_volumn_net(cv)], dim=1)
        if self.with_cp:
            depth = checkpoint(self.depth_conv, depth, use_reentrant=False)
        else:
            depth = self.depth_conv(depth)
        return torch.cat([depth, context], dim=1)
