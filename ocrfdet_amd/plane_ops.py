"""The three fused passes over (B, C, H, W) planes between the encoders' convolutions, each with its torch formulation:

* ``add_relu(a, b)``: the residual tail ``relu(out + identity)`` of a block, one launch and three tensor passes
  instead of two launches and five; the backward is one launch whose result is the gradient of both addends;
* ``upsample_add(dst, src, size | scale_factor)``: ``CustomFPN``'s ``laterals[i - 1] += F.interpolate(laterals[i])`` in
  mode ``nearest``, one launch instead of two; the backward is one gather launch, and the gradient of ``dst`` is
  ``grad_out`` itself;
* ``upsample_cat(x2, x1, scale)``: ``FPN_LSS``'s ``cat([x2, up(x1)], 1)`` and ``up2[0]``, bilinear upsampling with
  ``align_corners=True`` by an integer factor written straight into its channels of the concatenation; the backward is
  one gather launch without atomics.

The first two (``csrc/resnet_fuse.hip``) are bit-equal to ``add_relu_torch`` / ``upsample_add_torch`` forward.  The
third (``csrc/upsample_cat.hip``) takes its interpolation weights from integer arithmetic with one rounding, torch from
a float product: the two differ in the last bits.

The first two also take bfloat16 tensors (the ``*_bf16`` entry points of the same file), which is what they see between
the convolutions under ``torch.autocast('cuda', dtype=torch.bfloat16)``: operands, result and gradients are all bf16,
the sum is one float32 addition rounded once to nearest even, as torch's bf16 ops, and forward and ``add_relu``'s
backward stay bit-equal to the ``*_torch`` formulations.

``upsample_cat`` takes bfloat16 tensors too (``ocrf_upsample_cat_forward_bf16`` / ``_backward_bf16``), which is what it
sees in a ``BEVEncoder`` with ``autocast_bf16=True`` under bf16 autocast: operands, result and gradients are all bf16,
and the result is, bit for bit, that of the float32 kernel on the widened operands rounded once to nearest even
(``upsample_cat(x2.float(), x1.float(), s).bfloat16()``; the backward alike).  A ``BEVEncoder`` as it is built keeps
float32 and never sees bf16 here.

The ops themselves never fall back: they raise on an input the kernels do not take.  The modules dispatch with the
``*_fusable`` predicates: CUDA contiguous tensors that are all float32 (or all bfloat16: ``upsample_cat_bf16_fusable``
for the third op) take the kernels, everything else (the CPU, float16 and float64, mixed dtypes, non-contiguous maps)
the ``*_torch`` formulation.
"""
import torch
import torch.nn.functional as F

from . import _lib

# Defaults of the image encoder's two dispatch flags, from the measurement in profiles/image_encoder_time.txt
# (tools/time_image_encoder.py; INTEGRATION 3f has the table): by device time each op is faster than its torch
# formulation at the reference shapes, forward and forward + backward, at 12 and at 48 images (tail 1.07x to 1.65x, merge
# 2.0x to 2.4x), and the whole encoder with both flags on is the fastest of the four flag pairs in eval and in training
# (1.02x to 1.09x of the unfused one).
FUSED_TAIL_DEFAULT = True
FUSED_MERGE_DEFAULT = True
# The same for bfloat16 operands (the modules' ``fused_tail_bf16`` / ``fused_merge_bf16``, which apply while
# ``fused_tail`` / ``fused_merge`` are on), from profiles/image_encoder_bf16_time.txt
# (tools/time_image_encoder.py --autocast bf16; INTEGRATION 3i has the table).
# By device time each op is faster than its torch formulation on bf16 tensors at the reference shapes, forward and
# forward + backward, at 12 and at 48 images (tail 1.11x to 1.90x, merge 1.61x to 2.48x), and the whole encoder under
# autocast with both flags on is the fastest of the four flag pairs in eval and in training (1.01x to 1.07x of the
# unfused one, which is what autocast ran before).  By wall time the ops alone lose at 12 images, where a launch costs
# the host more than the device (0.59x to 0.86x); the encoder in training at 12 images is host-bound either way (0.96x).
FUSED_TAIL_BF16_DEFAULT = True
FUSED_MERGE_BF16_DEFAULT = True
# Default of ``FPN_LSS.fused_upsample_bf16`` (bfloat16 operands of ``upsample_cat``, which applies while ``fused_upsample``
# is on; it only matters inside ``BEVEncoder``'s ``autocast_bf16`` opt-in), decided as the flags above, from
# profiles/bev_encoder_bf16_time.txt (tools/time_bev_encoder.py --autocast bf16; INTEGRATION 3i has the table).  By device
# time the bf16 kernels are faster than ``interpolate`` + ``cat`` on the same bf16 tensors at both reference shapes,
# forward and forward + backward (up + cat 38x / 17x, ``up2[0]`` 10x / 5.1x; wall times agree), and the whole encoder
# under autocast with the flag on is the fastest of the three arms: 3.32 against 6.65 ms eval forward and 10.0 against
# 14.0 ms forward + backward in training (float32 inside autocast: 9.08 and 27.6 ms).
FUSED_UPSAMPLE_BF16_DEFAULT = True

# what the kernels of add_relu / upsample_add exist for: the suffix of their entry points
_SUFFIX = {torch.float32: '', torch.bfloat16: '_bf16'}


def _plain(t, dtypes=(torch.float32,)):
    return t.is_cuda and t.dtype in dtypes and t.is_contiguous()


def _plain_pair(a, b):
    """Both CUDA contiguous on one device and both float32 or both bfloat16."""
    return _plain(a, _SUFFIX) and _plain(b, _SUFFIX) and a.dtype == b.dtype and a.device == b.device


def _check_grad(grad_out, dtype, op):
    """``grad_out`` must come in the dtype of the forward's tensors."""
    if grad_out.dtype != dtype:
        raise _lib.OcrfHipError(f'{op} backward: grad_out is {grad_out.dtype}, the forward ran in {dtype}')


# ------------------------------------------------------------------------------------------------ add + relu
def add_relu_torch(a, b):
    """``relu(a + b)``: the residual tail as eager torch runs it."""
    return torch.relu_(a + b)


def add_relu_fusable(a, b):
    return _plain_pair(a, b) and a.shape == b.shape and a.numel() > 0


class _AddRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        out = torch.empty_like(a)
        _lib.launch('ocrf_add_relu_forward' + _SUFFIX[a.dtype], a.device, a.numel(), a, b, out)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        out, = ctx.saved_tensors
        _check_grad(grad_out, out.dtype, 'add_relu')
        grad_out = grad_out.contiguous()
        grad = torch.empty_like(out)
        _lib.launch('ocrf_add_relu_backward' + _SUFFIX[out.dtype], out.device, out.numel(), grad_out, out, grad)
        return grad, grad


def add_relu(a, b):
    """``add_relu_torch`` as one HIP launch (``ocrf_add_relu_forward`` / ``_backward``, or their ``_bf16`` forms).  CUDA
    contiguous tensors of equal shape, both float32 or both bfloat16, only: anything else raises (the blocks
    dispatch)."""
    _lib.require_cuda(a, b)
    if not add_relu_fusable(a, b):
        raise _lib.OcrfHipError('add_relu takes two non-empty contiguous tensors of equal shape on one device, both '
                                'float32 or both bfloat16')
    return _AddRelu.apply(a, b)


# ------------------------------------------------------------------------------------------------ upsample + add
def upsample_add_torch(dst, src, size=None, scale_factor=None, mode='nearest', **kwargs):
    """``dst + F.interpolate(src, size=size | scale_factor=scale_factor, mode=mode)``."""
    if scale_factor is not None:
        return dst + F.interpolate(src, scale_factor=scale_factor, mode=mode, **kwargs)
    return dst + F.interpolate(src, size=size, mode=mode, **kwargs)


def _target(src, size, scale_factor):
    """(Hout, Wout) of ``F.interpolate(src, size | scale_factor)`` where the kernel's index rule is torch's: a ``size``,
    or an integer ``scale_factor`` (torch then scales by 1 / factor, which is in / out rounded once).  Else None."""
    if (size is None) == (scale_factor is None) or src.dim() != 4:
        return None
    if size is not None:
        size = (size, size) if isinstance(size, int) else tuple(size)
        return (int(size[0]), int(size[1])) if len(size) == 2 else None
    if isinstance(scale_factor, (tuple, list)):
        if len(scale_factor) != 2 or scale_factor[0] != scale_factor[1]:
            return None
        scale_factor = scale_factor[0]
    if not isinstance(scale_factor, (int, float)) or scale_factor != int(scale_factor) or scale_factor < 1:
        return None
    return src.shape[2] * int(scale_factor), src.shape[3] * int(scale_factor)


def upsample_add_fusable(dst, src, size, scale_factor):
    if not (_plain_pair(dst, src) and dst.dim() == 4 and src.dim() == 4):
        return False
    hw = _target(src, size, scale_factor)
    return (hw is not None and dst.numel() > 0 and src.numel() > 0 and dst.shape[:2] == src.shape[:2]
            and tuple(dst.shape[2:]) == hw and hw[0] >= src.shape[2] and hw[1] >= src.shape[3])


class _UpsampleAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dst, src):
        B, C, Hout, Wout = dst.shape
        Hin, Win = src.shape[2:]
        out = torch.empty_like(dst)
        _lib.launch('ocrf_upsample_add_forward' + _SUFFIX[dst.dtype], dst.device, B, C, Hin, Win, Hout, Wout, dst, src,
                    out)
        ctx.shape = (B, C, Hin, Win, Hout, Wout)
        ctx.dtype = dst.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        B, C, Hin, Win, Hout, Wout = ctx.shape
        grad_src = None
        _check_grad(grad_out, ctx.dtype, 'upsample_add')
        if ctx.needs_input_grad[1]:
            g = grad_out.contiguous()
            grad_src = torch.empty(B, C, Hin, Win, dtype=ctx.dtype, device=g.device)
            _lib.launch('ocrf_upsample_add_backward' + _SUFFIX[ctx.dtype], g.device, B, C, Hin, Win, Hout, Wout, g,
                        grad_src)
        return (grad_out if ctx.needs_input_grad[0] else None), grad_src


def upsample_add(dst, src, size=None, scale_factor=None):
    """``upsample_add_torch`` in mode ``nearest`` as one HIP launch (``ocrf_upsample_add_forward`` / ``_backward``):
    ``src`` (B, C, Hin, Win) upsampled to the size of ``dst`` (B, C, Hout, Wout) and added to it; ``size`` must be that
    of ``dst``, or ``scale_factor`` an integer with ``Hout = Hin * scale_factor``.  CUDA contiguous tensors, both
    float32 or both bfloat16, only: anything else raises (``CustomFPN`` dispatches)."""
    _lib.require_cuda(dst, src)
    if not upsample_add_fusable(dst, src, size, scale_factor):
        raise _lib.OcrfHipError('upsample_add takes contiguous NCHW tensors, both float32 or both bfloat16, with the '
                                'same B and C, dst of the target size and no smaller than src, and either size or an '
                                'integer scale_factor')
    return _UpsampleAdd.apply(dst, src)


# ------------------------------------------------------------------------------------------------ upsample + cat
def upsample_cat_torch(x2, x1, scale):
    """``cat([x2, interpolate(x1, scale_factor=scale, mode='bilinear', align_corners=True)], 1)``; ``x2`` None: the
    upsampling alone."""
    up = F.interpolate(x1, scale_factor=scale, mode='bilinear', align_corners=True)
    return up if x2 is None else torch.cat([x2, up], dim=1)


def _upsample_cat_takes(x2, x1, scale, dtype):
    if not isinstance(scale, (int, float)) or scale != int(scale) or scale < 1:
        return False
    for t in (x1, x2):
        if t is not None and not (_plain(t, (dtype,)) and t.dim() == 4):
            return False
    return x2 is None or (x2.shape[0] == x1.shape[0] and x2.shape[2] == x1.shape[2] * int(scale)
                          and x2.shape[3] == x1.shape[3] * int(scale))


def upsample_cat_fusable(x2, x1, scale):
    """The float32 kernels take these operands."""
    return _upsample_cat_takes(x2, x1, scale, torch.float32)


def upsample_cat_bf16_fusable(x2, x1, scale):
    """The bfloat16 kernels take these operands: ``x1`` and ``x2`` (where there is one) both bfloat16."""
    return _upsample_cat_takes(x2, x1, scale, torch.bfloat16)


class _UpsampleCat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, x1, scale):
        B, C1, Hin, Win = x1.shape
        C2 = 0 if x2 is None else x2.shape[1]
        out = torch.empty(B, C2 + C1, Hin * scale, Win * scale, dtype=x1.dtype, device=x1.device)
        _lib.launch('ocrf_upsample_cat_forward' + _SUFFIX[x1.dtype], x1.device, B, C2, C1, Hin, Win, scale, x2, x1, out)
        ctx.shape = (B, C2, C1, Hin, Win, scale)
        ctx.dtype = x1.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        B, C2, C1, Hin, Win, scale = ctx.shape
        _check_grad(grad_out, ctx.dtype, 'upsample_cat')
        grad_out = grad_out.contiguous()
        grad_x2 = grad_x1 = None
        if ctx.needs_input_grad[0] and C2:
            grad_x2 = grad_out[:, :C2]
        if ctx.needs_input_grad[1]:
            grad_x1 = torch.empty(B, C1, Hin, Win, dtype=ctx.dtype, device=grad_out.device)
            _lib.launch('ocrf_upsample_cat_backward' + _SUFFIX[ctx.dtype], grad_out.device, B, C2, C1, Hin, Win, scale,
                        grad_out, grad_x1)
        return grad_x2, grad_x1, None


def upsample_cat(x2, x1, scale):
    """``upsample_cat_torch`` as one HIP launch (``ocrf_upsample_cat_forward`` / ``_backward``, or their ``_bf16``
    forms): ``x1`` (B, C1, H, W) upsampled by the integer ``scale`` behind the channels of ``x2`` (B, C2, H*scale,
    W*scale), or alone with ``x2`` None.  CUDA contiguous tensors, both float32 or both bfloat16, only: anything else
    (a mixed pair too) raises (``FPN_LSS`` dispatches).  The result and the gradients have the dtype of the operands."""
    _lib.require_cuda(x1, x2)
    if not (upsample_cat_fusable(x2, x1, scale) or upsample_cat_bf16_fusable(x2, x1, scale)):
        raise _lib.OcrfHipError('upsample_cat takes contiguous NCHW tensors, both float32 or both '
                                'bfloat16, x2 scale times the size of x1, and an integer scale')
    return _UpsampleCat.apply(x2, x1, int(scale))
