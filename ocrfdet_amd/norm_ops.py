"""Batch norm fused with what follows it in the blocks of ``blocks.py``: ``relu(bn(x))`` and ``relu(bn(x) + residual)``.

* ``bn_act_torch(bn, x, residual=None, relu=True)``: the formulation the blocks run without the op, ``bn(x)``, then
  ``+ residual``, then ``relu``, on any device and dtype;
* ``bn_act(bn, x, residual=None, relu=True)``: the same through ``csrc/bn_act.hip``.  In training (and in eval for a norm
  without running statistics) three launches forward, ``ocrf_bn_stats`` -> ``ocrf_bn_finalize`` ->
  ``ocrf_bn_act_forward``, which read ``x`` twice and write ``out`` once, and two backward,
  ``ocrf_bn_act_backward_reduce`` -> ``ocrf_bn_act_backward``; in eval with running statistics ``ocrf_bn_finalize`` turns
  them into ``scale`` and ``shift`` and the apply pass is the only pass over the map.  The statistics, the parameters,
  their gradients and every accumulation are float32; ``x``, ``residual``, the result and their gradients are float32
  or, with the ``_bf16`` kernels, bfloat16, which is what the op sees between the convolutions under
  ``torch.autocast('cuda', dtype=torch.bfloat16)``.  Nothing reads the device back: with ``momentum=None`` the kernel
  itself reads ``num_batches_tracked``.

``bn_act`` never falls back: it raises ``OcrfHipError`` on an input the kernels do not take.  The blocks dispatch with
``bn_act_fusable``.  A double backward is not supported: the backward is not differentiable and says so.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib

_SUFFIX = {torch.float32: '', torch.bfloat16: '_bf16'}
_TAG = 'bn_act'                  # the partials of a reduction, consumed by the next launch on the same stream


def bn_act_torch(bn, x, residual=None, relu=True):
    """``relu(bn(x) + residual)`` as eager torch runs it; ``residual`` None: no addition, ``relu`` False: no ReLU."""
    out = bn(x)
    if residual is not None:
        out = out + residual
    return torch.relu_(out) if relu else out


def _batch_stats(bn):
    """The statistics come from the batch: in training, and in eval for a norm that keeps no running statistics."""
    return bn.training or bn.running_mean is None


def bn_act_fusable(bn, x, residual=None):
    """The kernels take these operands: a plain affine ``BatchNorm2d`` with float32 parameters on the device of ``x``, a
    CUDA contiguous (N, C, H, W) map, float32 or bfloat16, of fewer than 2^31 elements, a residual (if any) of the same
    shape, dtype and device, and more than one value per channel where the statistics come from the batch."""
    if type(bn) is not nn.BatchNorm2d or not bn.affine:
        return False
    if not (x.is_cuda and x.dim() == 4 and x.dtype in _SUFFIX and x.is_contiguous() and 0 < x.numel() < 2 ** 31):
        return False
    if residual is not None and not (residual.shape == x.shape and residual.dtype == x.dtype
                                     and residual.device == x.device and residual.is_contiguous()):
        return False
    vectors = [bn.weight, bn.bias] + ([] if bn.running_mean is None else [bn.running_mean, bn.running_var])
    if any(v.dtype != torch.float32 or v.device != x.device or v.shape != (x.shape[1],) or not v.is_contiguous()
           for v in vectors):
        return False
    return not _batch_stats(bn) or x.numel() // x.shape[1] > 1


def _partials(x, per_chunk):
    N, C, H, W = x.shape
    chunks = _lib.lib().ocrf_bn_chunks(N, C, H, W)
    if chunks <= 0:
        raise _lib.OcrfHipError(f'bn_act: the kernels do not take a map of shape {tuple(x.shape)}')
    return _lib.workspace.get(x.device, C * chunks * per_chunk * 4, tag=_TAG)


class _BnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, bn, relu):
        N, C, H, W = x.shape
        suffix = _SUFFIX[x.dtype]
        batch_stats = _batch_stats(bn)
        update = bn.training and bn.running_mean is not None
        mean, invstd, scale, shift = torch.empty(4, C, dtype=torch.float32, device=x.device).unbind(0)
        partials = None
        if batch_stats:
            partials = _partials(x, 4)
            _lib.launch('ocrf_bn_stats' + suffix, x.device, N, C, H, W, x, partials)
        momentum = -1.0 if bn.momentum is None else float(bn.momentum)
        tracked = bn.num_batches_tracked if update and bn.momentum is None else None
        _lib.launch('ocrf_bn_finalize', x.device, N, C, H, W, 0 if batch_stats else 1, partials, weight, bias,
                    bn.running_mean if update or not batch_stats else None,
                    bn.running_var if update or not batch_stats else None, tracked, momentum, float(bn.eps), mean,
                    invstd, scale, shift)
        out = torch.empty_like(x)
        _lib.launch('ocrf_bn_act_forward' + suffix, x.device, N, C, H, W, x, residual, scale, shift, int(relu), out)
        ctx.save_for_backward(x, out if relu else None, mean, invstd, weight)
        ctx.batch_stats, ctx.has_residual = batch_stats, residual is not None
        return out

    @staticmethod
    @once_differentiable                 # no double backward: differentiating the backward raises
    def backward(ctx, grad_out):
        x, out, mean, invstd, weight = ctx.saved_tensors
        if grad_out.dtype != x.dtype:
            raise _lib.OcrfHipError(f'bn_act backward: grad_out is {grad_out.dtype}, the forward ran in {x.dtype}')
        need_x, need_res, need_w, need_b = ctx.needs_input_grad[:4]
        need_res = need_res and ctx.has_residual
        if not (need_x or need_res or need_w or need_b):
            return None, None, None, None, None, None
        N, C, H, W = x.shape
        suffix = _SUFFIX[x.dtype]
        g = grad_out.contiguous()
        dx = torch.empty_like(x) if need_x else None
        # without a ReLU the residual's gradient is grad_out itself
        dres = torch.empty_like(x) if need_res and out is not None else None
        dw = torch.empty_like(weight) if need_w else None
        db = torch.empty_like(weight) if need_b else None
        partials = None
        if (need_x and ctx.batch_stats) or need_w or need_b:
            partials = _partials(x, 2)
            _lib.launch('ocrf_bn_act_backward_reduce' + suffix, x.device, N, C, H, W, g, x, out, mean, invstd, partials)
        if dx is not None or dres is not None or partials is not None:
            _lib.launch('ocrf_bn_act_backward' + suffix, x.device, N, C, H, W, g, x, out, mean, invstd, weight, partials,
                        int(ctx.batch_stats), dx, dres, dw, db)
        if need_res and out is None:
            dres = grad_out
        return dx, dres, dw, db, None, None


def bn_act(bn, x, residual=None, relu=True):
    """``bn_act_torch`` through the HIP kernels of ``csrc/bn_act.hip``, behind one ``autograd.Function``: the batch norm
    ``bn`` (its mode, statistics and parameters as they are; the running statistics and ``num_batches_tracked`` are
    updated where the module would), then ``+ residual`` and the ReLU where asked for.  Operands ``bn_act_fusable``
    refuses raise ``OcrfHipError`` (the blocks dispatch); a double backward is not supported."""
    _lib.require_cuda(x, residual)
    if not bn_act_fusable(bn, x, residual):
        raise _lib.OcrfHipError('bn_act takes an affine nn.BatchNorm2d with float32 parameters and a contiguous CUDA '
                                '(N, C, H, W) map, float32 or bfloat16, of fewer than 2^31 elements on the same device, '
                                'a residual of the same shape and dtype, and more than one value per channel where the '
                                'statistics come from the batch')
    if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return _BnAct.apply(x, residual, bn.weight, bn.bias, bn, bool(relu))
