"""Deformable convolution, DCN v1: mmcv 1.x ``deform_conv2d`` / ``DeformConv2d`` / ``DeformConv2dPack`` (type ``'DCN'``)
with their arguments and ``state_dict`` keys, built without mmcv.  No bias and no modulation mask (that is DCNv2).

Semantics (include/ocrf_hip.h states them for the kernels).  ``x`` (n, C, H, W), ``weight`` (Cout, C / groups, kh, kw),
``offset`` (n, dg * 2 * kh * kw, Ho, Wo).  For tap ``k = i * kw + j`` of deformable group ``g`` (input channel ``c`` uses
``g = c // (C // dg)``), offset channel ``g * 2K + 2k`` is the ROW offset and ``2k + 1`` the COLUMN offset; the row
coordinate is ``ho * stride_h - pad_h + i * dil_h + off_h``.  The sample is 0 unless ``h > -1 and w > -1 and h < H and
w < W``; inside it is zero-padded bilinear.  ``col[n, c * K + k, ho * Wo + wo]`` is the sample and ``out = weight (*)
col``, grouped over ``groups``.

Two formulations of the same arithmetic:

* the fused one: ``ocrf_deform_im2col`` writes the columns in one launch and a ``bmm`` over the groups multiplies them
  image by image; the backward is a ``bmm`` per image for the column gradient, one ``ocrf_deform_col2im`` (grad_x by float
  atomics, grad_offset summed in registers), the columns recomputed and a ``bmm`` per image for grad_weight.  The column
  buffer holds at most ``COL_BYTES`` of images at a time; ``out``, ``grad_offset`` and ``grad_weight`` do not depend on
  the chunking, bit for bit: every GEMM is one image's (a batched GEMM over a chunk's images is not bit-identical across
  batch counts), and grad_weight adds the per-image products in ascending image order.  ``grad_x`` is accumulated atomically and is reproducible only to rounding.  No host synchronisation;
* the torch one, ``deform_conv2d_torch``: gathers and ``matmul``, differentiable by autograd, any device and dtype.  The
  CPU path, and the GPU path with ``fused=False`` or operands that are not contiguous float32.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from . import _lib

__all__ = ['deform_conv2d', 'deform_conv2d_torch', 'deform_im2col', 'deform_col2im', 'deform_taps', 'output_size',
           'DeformConv2d', 'DeformConv2dPack', 'build_dcn', 'COL_BYTES']

COL_BYTES = 256 * 2 ** 20       # the column buffer of the fused path holds at most this many bytes of images (>= 1 image)
TWO_GIB = 2 ** 31


def output_size(H, W, kernel, stride, padding, dilation):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel, stride, padding, dilation
    return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def _check(x, offset, weight, stride, padding, dilation, groups, deform_groups):
    """Shapes of one call -> (n, C, H, W, Cout, kh, kw, Ho, Wo)."""
    if x.dim() != 4 or offset.dim() != 4 or weight.dim() != 4:
        raise ValueError(f'deform_conv2d takes 4-d x, offset and weight, got {tuple(x.shape)}, {tuple(offset.shape)}, '
                         f'{tuple(weight.shape)}')
    n, C, H, W = x.shape
    Cout, Cg, kh, kw = weight.shape
    if groups < 1 or deform_groups < 1 or C % groups or Cout % groups or C % deform_groups or Cg != C // groups:
        raise ValueError(f'deform_conv2d: {C} -> {Cout} channels, weight {tuple(weight.shape)}, groups {groups}, '
                         f'deform_groups {deform_groups} do not fit')
    if min(stride) < 1 or min(dilation) < 1 or min(padding) < 0:
        raise ValueError(f'deform_conv2d: stride {stride}, padding {padding}, dilation {dilation}')
    if H + 2 * padding[0] < dilation[0] * (kh - 1) + 1 or W + 2 * padding[1] < dilation[1] * (kw - 1) + 1:
        raise NotImplementedError(f'deform_conv2d: a {H} x {W} input is smaller than the {kh} x {kw} kernel (mmcv pads '
                                  'such an input; this implementation does not)')
    Ho, Wo = output_size(H, W, (kh, kw), stride, padding, dilation)
    if tuple(offset.shape) != (n, deform_groups * 2 * kh * kw, Ho, Wo):
        raise ValueError(f'deform_conv2d: offset {tuple(offset.shape)}, expected '
                         f'{(n, deform_groups * 2 * kh * kw, Ho, Wo)}')
    return n, C, H, W, Cout, kh, kw, Ho, Wo


# --------------------------------------------------------------------------------------------- torch formulation
def deform_columns_torch(x, offset, kernel, stride, padding, dilation, deform_groups):
    """The columns (n, C * K, P) by torch gathers, differentiable in ``x`` and ``offset``."""
    n, C, H, W = x.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel, stride, padding, dilation
    dg, K = deform_groups, kh * kw
    Ho, Wo = offset.shape[2:]
    P = Ho * Wo
    dev, dt = x.device, x.dtype
    off = offset.reshape(n, dg, K, 2, Ho, Wo)
    i = torch.arange(kh, device=dev).repeat_interleave(kw)
    j = torch.arange(kw, device=dev).repeat(kh)
    base_h = (torch.arange(Ho, device=dev) * sh - ph).view(1, Ho, 1) + (i * dh).view(K, 1, 1)
    base_w = (torch.arange(Wo, device=dev) * sw - pw).view(1, 1, Wo) + (j * dw).view(K, 1, 1)
    h = base_h.to(dt) + off[:, :, :, 0]
    w = base_w.to(dt) + off[:, :, :, 1]                                   # (n, dg, K, Ho, Wo)
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)                       # a NaN fails
    h = torch.where(inside, h, torch.zeros_like(h))
    w = torch.where(inside, w, torch.zeros_like(w))
    hl, wl = h.detach().floor(), w.detach().floor()
    lh, lw = h - hl, w - wl
    xg = x.reshape(n, dg, C // dg, H * W)
    col = None
    for a in (0, 1):
        for b in (0, 1):
            r, c = hl + a, wl + b
            ok = inside & (r >= 0) & (r <= H - 1) & (c >= 0) & (c <= W - 1)
            idx = (r.clamp(0, H - 1) * W + c.clamp(0, W - 1)).long().reshape(n, dg, 1, K * P)
            wgt = ((lh if a else 1 - lh) * (lw if b else 1 - lw)) * ok.to(dt)
            v = xg.gather(3, idx.expand(-1, -1, C // dg, -1))             # (n, dg, C / dg, K * P)
            # a corner that is not read contributes 0 whatever lies at the clamped index
            v = torch.where(ok.reshape(n, dg, 1, K * P), v, torch.zeros_like(v))
            term = v * wgt.reshape(n, dg, 1, K * P)
            col = term if col is None else col + term
    return col.reshape(n, C * K, P)


def deform_conv2d_torch(x, offset, weight, stride=1, padding=0, dilation=1, groups=1, deform_groups=1):
    """The deformable convolution in torch ops (gathers + ``matmul``): any device and dtype, differentiable."""
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    n, C, H, W, Cout, kh, kw, Ho, Wo = _check(x, offset, weight, stride, padding, dilation, groups, deform_groups)
    col = deform_columns_torch(x, offset, (kh, kw), stride, padding, dilation, deform_groups)
    G, Kd = groups, (C // groups) * kh * kw
    out = torch.matmul(weight.reshape(G, Cout // G, Kd), col.reshape(n, G, Kd, Ho * Wo))
    return out.reshape(n, Cout, Ho, Wo)


# --------------------------------------------------------------------------------------------- kernels
def _operands(*tensors):
    _lib.require_cuda(*tensors)
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.OcrfHipError(f'the deformable convolution kernels take contiguous float32 tensors, got '
                                    f'{tuple(t.shape)} {t.dtype} with strides {t.stride()}')
        if t.numel() * 4 >= TWO_GIB:
            raise _lib.OcrfHipError(f'the deformable convolution kernels index with int: {tuple(t.shape)} is 2 GiB or more')


def _geometry(x, kernel, stride, padding, dilation, deform_groups):
    n, C, H, W = x.shape
    return (n, C, H, W, kernel[0], kernel[1], stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1],
            deform_groups)


def deform_im2col(x, offset, kernel, stride, padding, dilation, deform_groups, n0=0, n1=None, out=None):
    """``ocrf_deform_im2col``: the columns (n1 - n0, C * K, P) of the images ``n0 <= b < n1`` in one launch."""
    _operands(x, offset)
    n, C = x.shape[:2]
    n1 = n if n1 is None else n1
    K, P = kernel[0] * kernel[1], offset.shape[2] * offset.shape[3]
    if tuple(offset.shape[:2]) != (n, deform_groups * 2 * K) or not 0 <= n0 < n1 <= n:
        raise _lib.OcrfHipError(f'deform_im2col: offset {tuple(offset.shape)} for x {tuple(x.shape)}, images [{n0}, {n1})')
    if out is None:
        out = torch.empty(n1 - n0, C * K, P, device=x.device)
    _operands(out)
    if out.numel() != (n1 - n0) * C * K * P:
        raise _lib.OcrfHipError(f'deform_im2col: out {tuple(out.shape)} does not hold {(n1 - n0, C * K, P)}')
    _lib.launch('ocrf_deform_im2col', x.device, *_geometry(x, kernel, stride, padding, dilation, deform_groups), n0, n1,
                x, offset, out)
    return out


def deform_col2im(gcol, x, offset, kernel, stride, padding, dilation, deform_groups, grad_x, grad_offset, n0=0, n1=None):
    """``ocrf_deform_col2im``: ``gcol`` (n1 - n0, C * K, P) -> ``grad_x`` and ``grad_offset`` of the images
    ``n0 <= b < n1``, a memset and one launch."""
    _operands(gcol, x, offset, grad_x, grad_offset)
    n, C = x.shape[:2]
    n1 = n if n1 is None else n1
    K, P = kernel[0] * kernel[1], offset.shape[2] * offset.shape[3]
    if (tuple(offset.shape[:2]) != (n, deform_groups * 2 * K) or not 0 <= n0 < n1 <= n
            or gcol.numel() != (n1 - n0) * C * K * P or grad_x.shape != x.shape or grad_offset.shape != offset.shape):
        raise _lib.OcrfHipError(f'deform_col2im: gcol {tuple(gcol.shape)}, offset {tuple(offset.shape)}, x '
                                f'{tuple(x.shape)}, images [{n0}, {n1})')
    _lib.launch('ocrf_deform_col2im', x.device, *_geometry(x, kernel, stride, padding, dilation, deform_groups), n0, n1,
                gcol, x, offset, grad_x, grad_offset)


def deform_taps(H, W, base_h, base_w, off_h, off_w):
    """``ocrf_deform_taps`` (host only, no GPU): (weights[4], index[4], (lh, lw)) of one tap by the kernels' own function."""
    import ctypes
    wts, idx, frac = (ctypes.c_float * 4)(), (ctypes.c_int * 4)(), (ctypes.c_float * 2)()
    _lib.check(_lib.lib().ocrf_deform_taps(H, W, base_h, base_w, ctypes.c_float(off_h), ctypes.c_float(off_w), wts, idx,
                                           frac), 'ocrf_deform_taps')
    return list(wts), list(idx), tuple(frac)


def _chunks(n, image_bytes):
    """Image ranges [(n0, n1)] whose columns fit ``COL_BYTES`` (at least one image each): from the shapes alone."""
    per = max(1, min(n, int(COL_BYTES) // max(1, image_bytes)))
    return [(s, min(n, s + per)) for s in range(0, n, per)]


class _DeformConv2d(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, x, offset, weight, stride, padding, dilation, groups, deform_groups):
        n, C, H, W = x.shape
        Cout, _, kh, kw = weight.shape
        Ho, Wo = offset.shape[2:]
        x, offset, weight = x.detach(), offset.detach(), weight.detach()
        G, K, P = groups, kh * kw, Ho * Wo
        Kd = (C // G) * K
        ctx.geometry = ((kh, kw), stride, padding, dilation, deform_groups)
        ctx.groups = G
        ctx.save_for_backward(x, offset, weight)
        out = torch.empty(n, Cout, Ho, Wo, device=x.device)
        chunks = _chunks(n, C * K * P * 4)
        col = torch.empty(chunks[0][1] - chunks[0][0], C * K, P, device=x.device)
        w = weight.view(G, Cout // G, Kd)
        for n0, n1 in chunks:
            deform_im2col(x, offset, *ctx.geometry, n0=n0, n1=n1, out=col[:n1 - n0])
            # one product per image: the same GEMM whatever the chunking is (a batched GEMM over the images of a chunk
            # is not bit-identical across batch counts)
            for b in range(n0, n1):
                torch.bmm(w, col[b - n0].view(G, Kd, P), out=out[b].view(G, Cout // G, P))
        return out

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type='cuda')
    def backward(ctx, grad_out):
        x, offset, weight = ctx.saved_tensors
        n, C, H, W = x.shape
        Cout, _, kh, kw = weight.shape
        Ho, Wo = offset.shape[2:]
        G, K, P = ctx.groups, kh * kw, Ho * Wo
        Kd, M = (C // G) * K, Cout // G
        need_x, need_off, need_w = ctx.needs_input_grad[:3]
        grad_out = grad_out.contiguous().float()
        grad_x = grad_offset = grad_weight = None
        if need_x or need_off:
            grad_x, grad_offset = torch.empty_like(x), torch.empty_like(offset)
        # grad_weight: the per-image products grad_out x col^T added up in ascending image order, whatever the chunking
        gw = torch.empty(G, M, Kd, device=x.device) if need_w else None
        chunks = _chunks(n, C * K * P * 4)
        col = torch.empty(chunks[0][1] - chunks[0][0], C * K, P, device=x.device)
        w_t = weight.view(G, M, Kd).transpose(1, 2)
        for n0, n1 in chunks:
            nb = n1 - n0
            if need_x or need_off:
                for b in range(n0, n1):
                    torch.bmm(w_t, grad_out[b].view(G, M, P), out=col[b - n0].view(G, Kd, P))
                deform_col2im(col[:nb], x, offset, *ctx.geometry, grad_x, grad_offset, n0=n0, n1=n1)
            if need_w:
                deform_im2col(x, offset, *ctx.geometry, n0=n0, n1=n1, out=col[:nb])
                for b in range(n0, n1):
                    go, col_t = grad_out[b].view(G, M, P), col[b - n0].view(G, Kd, P).transpose(1, 2)
                    if b == 0:
                        torch.bmm(go, col_t, out=gw)
                    else:
                        torch.baddbmm(gw, go, col_t, out=gw)
        if need_w:
            grad_weight = gw.view_as(weight)
        return (grad_x if need_x else None, grad_offset if need_off else None, grad_weight, None, None, None, None, None)


def _fusable(*tensors):
    return all(t.is_cuda and t.is_contiguous() and t.numel() > 0
               and (t.dtype == torch.float32 or torch.is_autocast_enabled('cuda') and t.is_floating_point())
               for t in tensors)


def deform_conv2d(x, offset, weight, stride=1, padding=0, dilation=1, groups=1, deform_groups=1, fused=True):
    """mmcv's ``deform_conv2d`` without its ``bias`` and ``im2col_step``.  CUDA float32 contiguous operands take the HIP
    kernels when ``fused`` (under autocast the op runs in float32); everything else ``deform_conv2d_torch``."""
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    _check(x, offset, weight, stride, padding, dilation, groups, deform_groups)
    if fused and _fusable(x, offset, weight):
        return _DeformConv2d.apply(x, offset, weight, stride, padding, dilation, groups, deform_groups)
    return deform_conv2d_torch(x, offset, weight, stride, padding, dilation, groups, deform_groups)


# --------------------------------------------------------------------------------------------- modules
class DeformConv2d(nn.Module):
    """mmcv's ``DeformConv2d``: ``forward(x, offset)``, parameter ``weight`` (Cout, Cin / groups, kh, kw), no bias."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 deform_groups=1, bias=False, im2col_step=32):
        super().__init__()
        if bias:
            raise NotImplementedError('DeformConv2d(bias=True): mmcv does not support it either')
        if in_channels % groups or out_channels % groups:
            raise ValueError(f'in_channels {in_channels} and out_channels {out_channels} must be multiples of groups '
                             f'{groups}')
        if in_channels % deform_groups:
            raise ValueError(f'in_channels {in_channels} must be a multiple of deform_groups {deform_groups}')
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = _pair(kernel_size), _pair(stride), _pair(padding)
        self.dilation = _pair(dilation)
        self.groups, self.deform_groups = groups, deform_groups
        self.im2col_step = im2col_step          # accepted and ignored: the column buffer is sized by COL_BYTES
        self.transposed, self.output_padding = False, _pair(0)
        self.fused = True                       # the HIP kernels for CUDA float32 operands; False: the torch formulation
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *self.kernel_size))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, nonlinearity='relu')

    def forward(self, x, offset):
        return deform_conv2d(x, offset, self.weight, self.stride, self.padding, self.dilation, self.groups,
                             self.deform_groups, fused=self.fused)

    def extra_repr(self):
        return (f'{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, '
                f'padding={self.padding}, dilation={self.dilation}, groups={self.groups}, '
                f'deform_groups={self.deform_groups}')


class DeformConv2dPack(DeformConv2d):
    """mmcv's ``DeformConv2dPack`` (type ``'DCN'``): the offsets come from ``conv_offset``, a plain convolution with the
    same geometry whose weight and bias start at zero.  Keys: ``weight``, ``conv_offset.weight``, ``conv_offset.bias``."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        kh, kw = self.kernel_size
        self.conv_offset = nn.Conv2d(self.in_channels, self.deform_groups * 2 * kh * kw, kernel_size=self.kernel_size,
                                     stride=self.stride, padding=self.padding, dilation=self.dilation, bias=True)
        self.init_offset()

    def init_offset(self):
        self.conv_offset.weight.data.zero_()
        self.conv_offset.bias.data.zero_()

    def forward(self, x):
        return super().forward(x, self.conv_offset(x))


def build_dcn(cfg, *args, **kwargs):
    """mmcv's ``build_conv_layer`` for ``dict(type='DCN', ...)``."""
    cfg = dict(cfg)
    kind = cfg.pop('type', None)
    if kind != 'DCN':
        raise NotImplementedError(f'build_dcn: conv type {kind!r}; only DCN (deformable convolution v1) is implemented')
    return DeformConv2dPack(*args, **kwargs, **cfg)
