"""GPU: ``norm_ops.bn_act`` (csrc/bn_act.hip) against a float64 evaluation on the CPU, and the blocks with ``fused_norm``.

Shapes: the smallest at which the kernels can go wrong.  (3, 5, 7, 9): planes of 63 elements, which start off a 16-byte
boundary for float32 and for bfloat16, so that heads, bodies and tails are all walked; (2, 8, 8, 16): everything
aligned; (2, 3, 1, 1): two values per channel, the minimum; (5, 3, 41, 43): a channel of 8815 values spans three chunks
of ``kChunk`` = 4096 (read from the kernel's source) with a ragged last one, and planes of 1763 elements make chunks
cross from one sample into the next; (2, 70, 3, 5): more channels than a wave has lanes.  The kernels have no number of
channels per workgroup row: a workgroup owns one (channel, chunk).

Tolerances.  Statistics: the error against the float64 oracle is at most twice the error ``torch.batch_norm_stats`` and
``nn.BatchNorm2d``'s running update show against the same oracle on the same input, with a floor of 4 * 2^-24 relative.
Relative means: ``invstd`` and ``running_var`` to themselves; a mean to its channel's root mean square
sqrt(mean^2 + var), because a mean near zero still carries the rounding of the values it was summed from.  Gradients:
at most twice the error of torch's own float32 GPU autograd of ``bn_act_torch``, floor 8 * 2^-24 of the gradient's
largest magnitude.  Every test prints the figures it compares.

A pre-activation within 1e-4 of zero would make the ReLU's mask a matter of rounding, for torch's float32 autograd as
much as for the kernels, and a flipped mask is an error of the size of the gradient itself; ``case()`` moves such
elements of ``x`` away (there are a handful at most) before anything is computed.
"""
import copy
import functools
import itertools
import os
import re

import pytest
import torch
from torch import nn

from ocrfdet_amd import _lib, blocks, norm_ops
from tests import resnet_oracle

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'csrc', 'bn_act.hip')) as _f:
    K_CHUNK = int(re.search(r'constexpr int kChunk = (\d+);', _f.read()).group(1))

SHAPES = [(3, 5, 7, 9), (2, 8, 8, 16), (2, 3, 1, 1), (5, 3, 41, 43), (2, 70, 3, 5)]
KINDS = ['normal', 'offset', 'constant', 'nonfinite']
# training, residual, relu, momentum, trainable
MODES = list(itertools.product((True, False), (True, False), (True, False), (0.1, None), (True, False)))
EPS = 2.0 ** -24
DEV = 'cuda'


def test_the_shapes_cover_what_the_docstring_says():
    assert K_CHUNK == 4096
    N, C, H, W = SHAPES[3]
    assert N * H * W > 2 * K_CHUNK and (N * H * W) % K_CHUNK and K_CHUNK % (H * W) and H * W < K_CHUNK
    assert (7 * 9 * 4) % 16 and (7 * 9 * 2) % 16 and (8 * 16 * 2) % 16 == 0 and SHAPES[4][1] > 64
    assert len(MODES) == 32


def make_bn(C, training, momentum, trainable, seed, track=True, dtype=torch.float32, device=DEV):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(C, momentum=momentum, track_running_stats=track)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g) * 0.5 + 1.0)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.5)
        if track:
            bn.running_mean.copy_(torch.randn(C, generator=g) * 0.3)
            bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
            bn.num_batches_tracked.fill_(3)
    for p in bn.parameters():
        p.requires_grad = trainable
    return bn.train(training).to(device=device, dtype=dtype)


def make_x(shape, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if kind == 'offset':
        x = 100.0 + 0.1 * x                        # E[x^2] - E[x]^2 would cancel here
    elif kind == 'constant':
        x[:, 1] = 0.1                              # variance 0: invstd = 1 / sqrt(eps)
    elif kind == 'nonfinite':
        x[0, 1, 0, 0], x[-1, 1, -1, -1] = float('nan'), float('inf')
        if shape[2] * shape[3] > 1:
            x[0, 1, -1, -1] = float('-inf')
    return x


def clean_channels(shape, kind):
    keep = torch.ones(shape[1], dtype=torch.bool)
    if kind == 'nonfinite':
        keep[1] = False
    return keep


@functools.lru_cache(maxsize=None)
def case(shape, kind, mode):
    """The operands of one case on the CPU (float32), with the float64 results and gradients of ``bn_act_torch``."""
    training, residual, relu, momentum, trainable = mode
    x = make_x(shape, kind, 1)
    g = torch.Generator().manual_seed(2)
    res = torch.randn(shape, generator=g) if residual else None
    go = torch.randn(shape, generator=g)

    def oracle():
        bn = make_bn(shape[1], training, momentum, True, 3, dtype=torch.float64, device='cpu')
        xd = x.double().requires_grad_()
        rd = None if res is None else res.double().requires_grad_()
        pre = norm_ops.bn_act_torch(bn, xd, rd, relu=False)
        return bn, xd, rd, pre

    if relu:                                       # see the module docstring
        for _ in range(4):
            near = oracle()[3].detach().abs() < 1e-4
            if not near.any():
                break
            assert near.sum() <= 8
            x = torch.where(near, x + 0.05, x)
        assert not (oracle()[3].detach().abs() < 1e-4).any()
    bn, xd, rd, pre = oracle()
    out = torch.relu(pre) if relu else pre
    out.backward(go.double())
    want = dict(out=out.detach(), dx=xd.grad, dres=None if rd is None else rd.grad, dw=bn.weight.grad, db=bn.bias.grad,
                running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
                tracked=int(bn.num_batches_tracked))
    return x, res, go, want


def run(fn, shape, kind, mode, dtype=torch.float32, widen=False, channels=None):
    """``fn`` (``bn_act`` or ``bn_act_torch``) forward and backward on the GPU on the operands of ``case``; with
    ``channels`` (a mask) on those channels of them alone, which is the same computation for each of them."""
    training, residual, relu, momentum, trainable = mode
    x, res, go, _ = case(shape, kind, mode)
    bn = make_bn(shape[1], training, momentum, trainable, 3)
    if channels is not None:
        x, res, go = (None if t is None else t[:, channels].contiguous() for t in (x, res, go))
        part = make_bn(int(channels.sum()), training, momentum, trainable, 3)
        with torch.no_grad():
            for mine, whole in zip(list(part.parameters()) + list(part.buffers()),
                                   list(bn.parameters()) + list(bn.buffers())):
                mine.copy_(whole[channels.to(DEV)] if whole.dim() else whole)
        bn = part
    cast = (lambda t: t.to(DEV, dtype).float()) if widen else (lambda t: t.to(DEV, dtype))
    xg = cast(x).requires_grad_()
    rg = None if res is None else cast(res).requires_grad_()
    out = fn(bn, xg, rg, relu=relu)
    out.backward(cast(go))
    return dict(out=out.detach(), dx=xg.grad, dres=None if rg is None else rg.grad, dw=bn.weight.grad, db=bn.bias.grad,
                running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
                tracked=int(bn.num_batches_tracked))


def only(t, keep):
    """The channels ``keep`` of a map or of a per-channel vector."""
    return t[:, keep] if t.dim() == 4 else t[keep]


def max_err(got, want):
    return float((got.double().cpu() - want).abs().max())


def same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    view = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


# ------------------------------------------------------------------------------------------------ statistics
def kernel_stats(x, bn):
    """mean, invstd, scale, shift as ``ocrf_bn_stats`` + ``ocrf_bn_finalize`` write them (no running update)."""
    N, C, H, W = x.shape
    chunks = _lib.lib().ocrf_bn_chunks(N, C, H, W)
    partials = torch.empty(C * chunks * 4, device=x.device)
    stat = torch.empty(4, C, device=x.device)
    _lib.launch('ocrf_bn_stats' + norm_ops._SUFFIX[x.dtype], x.device, N, C, H, W, x, partials)
    _lib.launch('ocrf_bn_finalize', x.device, N, C, H, W, 0, partials, bn.weight, bn.bias, None, None, None, 0.1,
                float(bn.eps), *stat.unbind(0))
    return stat.unbind(0)


def relative(got, want, scale, keep):
    return float(((got.double().cpu() - want).abs() / scale)[keep].max())


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_statistics_against_float64(shape, kind):
    x = make_x(shape, kind, 1)
    keep = clean_channels(shape, kind)
    xd = x.double()
    n = x.numel() // shape[1]
    mean64 = xd.mean((0, 2, 3))
    var64 = xd.var((0, 2, 3), unbiased=False)
    invstd64 = 1.0 / torch.sqrt(var64 + 1e-5)
    rms = torch.sqrt(mean64 ** 2 + var64).clamp_min(1e-30)
    xg = x.to(DEV)
    bn = make_bn(shape[1], True, 0.1, True, 3)
    mean, invstd, scale, shift = kernel_stats(xg, bn)
    t_mean, t_invstd = torch.batch_norm_stats(xg, 1e-5)
    figures = [('mean', relative(mean, mean64, rms, keep), relative(t_mean, mean64, rms, keep)),
               ('invstd', relative(invstd, invstd64, invstd64, keep), relative(t_invstd, invstd64, invstd64, keep))]
    for momentum in (0.1, None):
        ours, theirs = make_bn(shape[1], True, momentum, True, 3), make_bn(shape[1], True, momentum, True, 3)
        m = momentum if momentum is not None else 1.0 / (int(ours.num_batches_tracked) + 1)
        rm64 = (1 - m) * ours.running_mean.double().cpu() + m * mean64
        rv64 = (1 - m) * ours.running_var.double().cpu() + m * var64 * n / (n - 1)
        norm_ops.bn_act(ours, xg)
        theirs(xg)
        assert int(ours.num_batches_tracked) == int(theirs.num_batches_tracked) == 4
        rscale = torch.maximum(rm64.abs(), rms)
        figures += [(f'running_mean m={momentum}', relative(ours.running_mean, rm64, rscale, keep),
                     relative(theirs.running_mean, rm64, rscale, keep)),
                    (f'running_var m={momentum}', relative(ours.running_var, rv64, rv64, keep),
                     relative(theirs.running_var, rv64, rv64, keep))]
    for name, ours_err, torch_err in figures:
        print(f'{shape} {kind} {name}: kernel {ours_err / EPS:.3f} torch {torch_err / EPS:.3f} (units of 2^-24)')
    for name, ours_err, torch_err in figures:
        assert ours_err <= max(2 * torch_err, 4 * EPS), name
    # scale and shift are the rounded products of what was written
    assert same_bits(scale, bn.weight.detach() * invstd)
    assert same_bits(shift[keep], (bn.bias.detach() - mean * scale)[keep])
    if kind == 'constant':
        assert float(mean[1]) == pytest.approx(0.1, rel=1e-7) and abs(float(invstd[1]) * 1e-5 ** 0.5 - 1) <= 4 * EPS
    if kind == 'nonfinite':
        assert torch.isnan(invstd[1]) and torch.isnan(t_invstd[1]) and torch.isfinite(invstd[keep]).all()


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_apply_pass_rounds_each_value_once(shape, kind):
    """Given the scale and shift the kernel wrote, every output lies within 2^-24 (|x scale + shift| + |result|) of the
    float64 value: half an ulp for the fused multiply-add and half for the addition of the residual."""
    x = make_x(shape, kind, 1).to(DEV)
    res = torch.randn(shape, generator=torch.Generator().manual_seed(2)).to(DEV)
    keep = clean_channels(shape, kind)
    bn = make_bn(shape[1], True, 0.1, True, 3)
    _, _, scale, shift = kernel_stats(x, bn)
    N, C, H, W = shape
    for residual, relu in itertools.product((None, res), (0, 1)):
        out = torch.full_like(x, float('nan'))
        _lib.launch('ocrf_bn_act_forward', x.device, N, C, H, W, x, residual, scale, shift, relu, out)
        v = x.double() * scale.double()[:, None, None] + shift.double()[:, None, None]
        want = v if residual is None else v + residual.double()
        want = torch.relu(want) if relu else want
        slack = (EPS * (v.abs() + want.abs()) - (out.double() - want).abs())[:, keep]
        assert (slack >= 0).all(), (residual is not None, relu, float(slack.min()))


# ------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_forward_and_gradients_against_float64_in_every_mode(shape, kind):
    keep = clean_channels(shape, kind)
    worst = {}
    for mode in MODES:
        training, residual, relu, momentum, trainable = mode
        want = case(shape, kind, mode)[3]
        got, ref = run(norm_ops.bn_act, shape, kind, mode), run(norm_ops.bn_act_torch, shape, kind, mode)
        # torch's backward lets the NaN of one channel into the gradients of the others: its own error on the channels
        # that have none is taken from a run on those channels alone
        ref_clean = run(norm_ops.bn_act_torch, shape, kind, mode, channels=keep) if kind == 'nonfinite' else ref
        assert got['tracked'] == ref['tracked'] == want['tracked'] == (4 if training else 3)
        # NaN and +-inf stay where torch has them, and stay out of the other channels
        assert torch.equal(torch.isnan(got['out']), torch.isnan(ref['out'])), mode
        assert torch.equal(torch.isinf(got['out']), torch.isinf(ref['out'])), mode
        assert torch.isfinite(got['out'][:, keep.to(DEV)]).all(), mode
        if not trainable:
            assert got['dw'] is None and got['db'] is None
        if not training:
            assert same_bits(got['running_mean'], ref['running_mean']) and same_bits(got['running_var'],
                                                                                       ref['running_var'])
        names = ['out', 'dx'] + (['dres'] if residual else []) + (['dw', 'db'] if trainable else [])
        for name in names:
            clean = only(want[name], keep)
            floor = 8 * EPS * float(clean.abs().max())
            e = max_err(only(got[name], keep.to(DEV)), clean)
            t = max_err(ref_clean[name] if kind == 'nonfinite' else only(ref_clean[name], keep.to(DEV)), clean)
            assert e <= max(2 * t, floor), (mode, name, e, t, floor)
            w = worst.setdefault(name, [0.0, 0.0])
            w[0], w[1] = max(w[0], e / max(floor, 1e-300)), max(w[1], t / max(floor, 1e-300))
    for name, (e, t) in worst.items():
        print(f'{shape} {kind} {name}: worst error over the modes, in units of the floor: kernel {e:.3f} torch {t:.3f}')


def test_without_running_statistics_the_batch_is_used_in_eval_as_well():
    shape = SHAPES[0]
    x = make_x(shape, 'normal', 1).to(DEV)
    for training in (True, False):
        a, b = (make_bn(shape[1], training, 0.1, True, 3, track=False) for _ in range(2))
        xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
        out, ref = norm_ops.bn_act(a, xa), norm_ops.bn_act_torch(b, xb)
        out.square().sum().backward()
        ref.square().sum().backward()
        assert a.running_mean is None and a.num_batches_tracked is None
        torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(a.weight.grad, b.weight.grad, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize('shape', SHAPES)
def test_bf16_is_the_float32_kernel_on_the_widened_input_rounded_once(shape):
    for kind, mode in itertools.product(('normal', 'offset'), MODES):
        training, residual, relu, momentum, trainable = mode
        low = run(norm_ops.bn_act, shape, kind, mode, dtype=torch.bfloat16)
        wide = run(norm_ops.bn_act, shape, kind, mode, dtype=torch.bfloat16, widen=True)
        assert low['out'].dtype == torch.bfloat16 and low['dx'].dtype == torch.bfloat16
        for name in ['out', 'dx'] + (['dres'] if residual else []):
            assert same_bits(low[name], wide[name].bfloat16()), (kind, mode, name)
        for name in ['running_mean', 'running_var'] + (['dw', 'db'] if trainable else []):
            assert low[name].dtype == torch.float32 and same_bits(low[name], wide[name]), (kind, mode, name)
    x = make_x(shape, 'offset', 1).to(DEV).bfloat16()
    bn = make_bn(shape[1], True, 0.1, True, 3)
    for a, b in zip(kernel_stats(x, bn), kernel_stats(x.float(), bn)):
        assert same_bits(a, b)


def test_bf16_planes_off_a_16_byte_boundary_and_a_base_off_it():
    """H W = 63 bf16 elements: a plane starts at a multiple of 2 bytes.  A view whose base is off a 16-byte boundary
    takes the single-element kernels and gives the same bits."""
    shape = SHAPES[0]
    bn = make_bn(shape[1], True, 0.1, True, 3)
    for dtype in (torch.bfloat16, torch.float32):
        x = make_x(shape, 'normal', 1).to(DEV, dtype)
        buf = torch.empty(x.numel() + 1, device=DEV, dtype=dtype)
        view = buf[1:].view(shape)
        view.copy_(x)
        assert view.is_contiguous() and view.data_ptr() % 16 and x.data_ptr() % 16 == 0
        want, got = norm_ops.bn_act(copy.deepcopy(bn), x, x), norm_ops.bn_act(copy.deepcopy(bn), view, x)
        assert same_bits(want, got)


def test_two_runs_are_bit_identical():
    for shape, dtype in itertools.product((SHAPES[0], SHAPES[3]), (torch.float32, torch.bfloat16)):
        mode = (True, True, True, 0.1, True)
        a, b = run(norm_ops.bn_act, shape, 'normal', mode, dtype), run(norm_ops.bn_act, shape, 'normal', mode, dtype)
        for name in ('out', 'dx', 'dres', 'dw', 'db', 'running_mean', 'running_var'):
            assert same_bits(a[name], b[name]), name


def test_nothing_reads_the_device_back():
    shape = SHAPES[3]
    x, res, go, _ = case(shape, 'normal', (True, True, True, None, True))
    x, res, go = x.to(DEV), res.to(DEV), go.to(DEV)
    bns = [make_bn(shape[1], training, momentum, True, 3) for training in (True, False) for momentum in (0.1, None)]
    norm_ops.bn_act(copy.deepcopy(bns[0]), x, res).backward(go)       # the library and the workspace exist
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for bn in bns:
            xi, ri = x.clone().requires_grad_(), res.clone().requires_grad_()
            norm_ops.bn_act(bn, xi, ri).backward(go)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert [int(bn.num_batches_tracked) for bn in bns] == [4, 4, 3, 3]


def test_an_in_place_write_between_forward_and_backward_raises():
    shape = SHAPES[0]
    bn = make_bn(shape[1], True, 0.1, True, 3)
    x = make_x(shape, 'normal', 1).to(DEV).requires_grad_()
    out = norm_ops.bn_act(bn, x)
    out.add_(1.0)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        out.sum().backward()
    xi = make_x(shape, 'normal', 1).to(DEV)
    out = norm_ops.bn_act(bn, xi)
    xi.mul_(2.0)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        out.sum().backward()


def test_a_double_backward_is_refused():
    shape = SHAPES[0]
    bn = make_bn(shape[1], True, 0.1, True, 3)
    x = make_x(shape, 'normal', 1).to(DEV).requires_grad_()
    grad, = torch.autograd.grad(norm_ops.bn_act(bn, x).square().sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable'):
        grad.sum().backward()


def test_bn_act_raises_on_what_the_kernels_do_not_take():
    shape = SHAPES[0]
    bn = make_bn(shape[1], True, 0.1, True, 3)
    x = make_x(shape, 'normal', 1).to(DEV)
    for bad in (x.half(), x.permute(0, 1, 3, 2), x[:1, :, :1, :1].contiguous()):
        with pytest.raises(_lib.OcrfHipError):
            norm_ops.bn_act(bn, bad)
    with pytest.raises(_lib.OcrfHipError):
        norm_ops.bn_act(bn, x, residual=x.bfloat16())
    with pytest.raises(_lib.OcrfHipError):
        norm_ops.bn_act(nn.SyncBatchNorm(shape[1]).to(DEV), x)
    assert int(bn.num_batches_tracked) == 3


# ------------------------------------------------------------------------------------------------ the modules
class Net(nn.Module):
    """A stem and three blocks in torchvision's key layout (what ``resnet_oracle`` reads): a Bottleneck with a
    downsample, a Bottleneck, a BasicBlock."""

    def __init__(self, with_cp=False):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 8, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(8)
        down = nn.Sequential(nn.Conv2d(8, 16, 1, bias=False), nn.BatchNorm2d(16))
        self.layer1 = nn.Sequential(blocks.Bottleneck(8, 4, downsample=down, with_cp=with_cp),
                                    blocks.Bottleneck(16, 4, with_cp=with_cp))
        self.layer2 = nn.Sequential(blocks.BasicBlock(16, 16, with_cp=with_cp))

    def forward(self, x):
        x = nn.functional.max_pool2d(torch.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        return self.layer2(self.layer1(x))


def make_net(with_cp=False):
    torch.manual_seed(5)
    net = Net(with_cp)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5), m.bias.normal_(0, 0.3)
                m.running_mean.normal_(0, 0.3), m.running_var.uniform_(0.5, 1.5)
    return net


def image():
    return torch.randn(3, 3, 37, 45, generator=torch.Generator().manual_seed(6))


def count_calls(monkeypatch):
    calls = []
    real = norm_ops.bn_act
    monkeypatch.setattr(blocks, 'bn_act', lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    return calls


def test_blocks_in_eval_against_the_float64_oracle(monkeypatch):
    net, x = make_net().eval(), image()
    want = resnet_oracle.resnet_eval(net.state_dict(), x, strides=(1, 1))[-1]
    calls = count_calls(monkeypatch)
    errs = {}
    for flag in (False, True):
        m = copy.deepcopy(net).to(DEV)
        blocks.fuse_norms(m, flag)
        with torch.no_grad():
            errs[flag] = float((m(x.to(DEV)).double().cpu() - want).abs().max())
        assert len(calls) == (8 if flag else 0)
    print(f'eval output error against float64: fused {errs[True]:.3e} unfused {errs[False]:.3e}')
    assert errs[True] <= 2 * errs[False]


def test_blocks_in_training_against_float64(monkeypatch):
    """The oracle is eval only; in training the float64 evaluation is the unfused modules themselves in double."""
    net, x = make_net().train(), image()
    ref = copy.deepcopy(net).double()
    xd = x.double().requires_grad_()
    want = ref(xd)
    go = torch.randn(want.shape, generator=torch.Generator().manual_seed(7))
    want.backward(go.double())
    calls = count_calls(monkeypatch)
    errs = {}
    for flag in (False, True):
        m = copy.deepcopy(net).to(DEV)
        blocks.fuse_norms(m, flag)
        xi = x.to(DEV).requires_grad_()
        out = m(xi)
        out.backward(go.to(DEV))
        errs[flag] = (float((out.detach().double().cpu() - want.detach()).abs().max()), float((xi.grad.double().cpu() - xd.grad).abs().max()))
        assert len(calls) == (8 if flag else 0)
    print(f'training (output, input gradient) error against float64: fused {errs[True]} unfused {errs[False]}')
    assert errs[True][0] <= 2 * errs[False][0] and errs[True][1] <= 2 * errs[False][1]


def test_conv_module_with_and_without_a_relu(monkeypatch):
    calls = count_calls(monkeypatch)
    x = torch.randn(2, 6, 9, 7, generator=torch.Generator().manual_seed(8))
    for act_cfg in (dict(type='ReLU'), None, dict(type='LeakyReLU')):
        torch.manual_seed(9)
        mod = blocks.ConvModule(6, 10, 3, padding=1, norm_cfg=dict(type='BN'), act_cfg=act_cfg)
        ref = copy.deepcopy(mod).double()
        xd = x.double().requires_grad_()
        want = ref(xd)
        want.square().sum().backward()
        errs = {}
        for flag in (False, True):
            del calls[:]
            m = copy.deepcopy(mod).to(DEV)
            blocks.fuse_norms(m, flag)
            xi = x.to(DEV).requires_grad_()
            out = m(xi)
            out.square().sum().backward()
            errs[flag] = (float((out.detach().double().cpu() - want.detach()).abs().max()),
                          float((xi.grad.double().cpu() - xd.grad).abs().max()))
            fused = flag and (act_cfg is None or act_cfg['type'] == 'ReLU')
            assert [c.get('relu') for c in calls] == ([act_cfg is not None] if fused else [])
        print(f'ConvModule {act_cfg}: fused {errs[True]} unfused {errs[False]}')
        assert errs[True][0] <= 2 * errs[False][0] and errs[True][1] <= 2 * errs[False][1]


def test_checkpointed_blocks_update_the_running_statistics_twice_in_both_forms():
    x = image()
    ref = copy.deepcopy(make_net(with_cp=True)).double().train()
    ref(x.double().requires_grad_()).sum().backward()
    nets = {}
    for flag in (False, True):
        m = make_net(with_cp=True).to(DEV).train()
        blocks.fuse_norms(m, flag)
        m(x.to(DEV).requires_grad_()).sum().backward()
        nets[flag] = m
    for (name, want), fused, unfused in zip(ref.named_buffers(), nets[True].buffers(), nets[False].buffers()):
        if name.endswith('num_batches_tracked'):
            # a checkpointed block runs its forward again in the backward; the stem is outside the blocks
            assert int(fused) == int(unfused) == int(want) == (2 if name.startswith('layer') else 1), name
            continue
        scale = want.abs().clamp_min(float(want.abs().mean()))     # a mean near zero: relative to the vector's size
        e = float(((fused.double().cpu() - want).abs() / scale).max())
        t = float(((unfused.double().cpu() - want).abs() / scale).max())
        print(f'{name}: fused {e / EPS:.2f} unfused {t / EPS:.2f} (units of 2^-24)')
        assert e <= max(2 * t, 4 * EPS), name


def test_eval_autocast_and_deepcopy_of_a_fused_model(monkeypatch):
    calls = count_calls(monkeypatch)
    net = make_net().to(DEV)
    blocks.fuse_norms(net)
    twin = copy.deepcopy(net)                      # what the weight EMA does
    assert all(m.fused_norm for m in twin.modules() if isinstance(m, blocks._Block))
    x = image().to(DEV)
    with torch.no_grad():
        assert same_bits(net.eval()(x), twin.eval()(x))
    net.train()
    del calls[:]
    xi = x.clone().requires_grad_()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = net(xi)
    out.float().square().mean().backward()
    assert out.dtype == torch.bfloat16 and len(calls) == 8
    assert torch.isfinite(out).all() and torch.isfinite(xi.grad).all()
    for p in net.parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all()
    ref = copy.deepcopy(twin).train()
    blocks.fuse_norms(ref, False)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        want = ref(x)
    assert float((out.float() - want.float()).abs().max()) <= 0.05 * float(want.float().abs().max())
