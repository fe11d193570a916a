"""GPU: the fused deformable convolution (``ocrf_deform_im2col`` / ``ocrf_deform_col2im`` through
``ocrfdet_amd.deform_conv``) against the float64 oracle (tests/dcn_oracle.py) on the cases the host test runs.

Bounds.  The columns are held to ``4 eps32 (max(H, W) + 2) max|x|``: a coordinate below max(H, W) + 2 in magnitude is
rounded once (half an eps32 of it), two neighbouring taps differ by at most 2 max|x|, and the four products and three
sums of the value add a few eps32 of max|x|.  Taps the definition does not sample (the range test fails: exactly -1,
exactly the size, far outside, NaN, infinities, 1e30) are exactly 0.  ``out`` and the three gradients have no fixed
tolerance: each is compared with the error the torch formulation makes in float32 on the same GPU against the same
oracle, and the fused path may make at most 4 times that error (the order of summation differs; grad_x is accumulated
atomically), with a floor of 16 eps32 times the oracle's largest magnitude.  The measured figures, MI355X (``fused /
torch`` maximum error over the cases): see DESIGN 4.22.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib
from ocrfdet_amd import center_head as ch
from ocrfdet_amd import deform_conv as dc
from ocrfdet_amd import depthnet
from tests import dcn_oracle as do

pytestmark = pytest.mark.gpu

EPS32 = do.EPS32
NAMES = ('out', 'grad_x', 'grad_offset', 'grad_weight')
NOT_SAMPLED = ('minus_one', 'at_size', 'far_low', 'far_high', 'nan', 'plus_inf', 'minus_inf', 'plus_huge', 'minus_huge')


def run(cuda, name, fused, col_bytes=None):
    """(out, grad_x, grad_offset, grad_weight) float32 tensors on the GPU of one case."""
    x, offset, weight, grad_out, _, geo = do.problem(name)
    t = [torch.from_numpy(a.copy()).to(cuda).requires_grad_(True) for a in (x, offset, weight)]
    before = dc.COL_BYTES
    if col_bytes is not None:
        dc.COL_BYTES = col_bytes
    try:
        out = dc.deform_conv2d(*t, *geo, fused=fused)
        grads = torch.autograd.grad(out, t, torch.from_numpy(grad_out.copy()).to(cuda))
    finally:
        dc.COL_BYTES = before
    return (out.detach(),) + tuple(grads)


@functools.lru_cache(maxsize=None)
def errors(name):
    """{what: (fused error, torch error, bound)} of a case against the oracle, and the fused results; computed once."""
    cuda = torch.device('cuda:0')
    want = do.oracle(name)
    fused, plain = run(cuda, name, True), run(cuda, name, False)
    table = {}
    for what, f, p, w in zip(NAMES, fused, plain, want):
        e_f = float(np.abs(f.cpu().numpy().astype(np.float64) - w).max())
        e_t = float(np.abs(p.cpu().numpy().astype(np.float64) - w).max())
        table[what] = (e_f, e_t, max(4 * e_t, 16 * EPS32 * float(np.abs(w).max())))
    return table, fused


@pytest.mark.parametrize('name', list(do.CASES))
def test_columns_against_the_oracle(cuda, name):
    C, Cout, H, W, kernel, stride, padding, dilation, groups, dg = do.CASES[name]
    x, offset, _, _, classes, _ = do.problem(name)
    xt, ot = torch.from_numpy(x.copy()).to(cuda), torch.from_numpy(offset.copy()).to(cuda)
    got = dc.deform_im2col(xt, ot, kernel, stride, padding, dilation, dg).cpu().numpy()
    want = do.columns(x, offset, kernel, stride, padding, dilation, dg)
    assert got.shape == want.shape and got.dtype == np.float32
    err, bound = float(np.abs(got - want).max()), 4 * EPS32 * (max(H, W) + 2) * float(np.abs(x).max())
    print(f'{name}: columns {err:.3e} (bound {bound:.3e})')
    assert np.isfinite(got).all() and err <= bound
    # a tap that is not sampled is exactly 0 in every channel of its group
    n, K, P, cpg = x.shape[0], kernel[0] * kernel[1], got.shape[2], C // dg
    cols = got.reshape(n, dg, cpg, K, P)
    checked = 0
    for (cls, axis), where in classes.items():
        if cls in NOT_SAMPLED:
            b, g, k, p = np.unravel_index(where, (n, dg, K, P))
            assert not cols[b, g, :, k, p].any(), (cls, axis)
            checked += len(where)
    assert checked >= 2 * len(NOT_SAMPLED)
    # the image range: the second image alone, into a buffer of its own
    part = dc.deform_im2col(xt, ot, kernel, stride, padding, dilation, dg, n0=1, n1=2)
    assert np.array_equal(part.cpu().numpy(), got[1:2])


@pytest.mark.parametrize('name', list(do.CASES))
def test_output_and_gradients_against_the_oracle(cuda, name):
    table, fused = errors(name)
    fails = []
    for what, (e_f, e_t, bound) in table.items():
        print(f'{name}: {what} fused {e_f:.3e}, torch {e_t:.3e}, bound {bound:.3e}')
        if not e_f <= bound:
            fails.append(f'{what}: {e_f:.3e} > {bound:.3e}')
    assert all(torch.isfinite(t).all() for t in fused)
    assert not fails, fails


@pytest.mark.parametrize('name', ['groups 4 dg 2', 'stride 2', '3x1', 'plane 16x44'])
def test_reruns_and_chunkings(cuda, name):
    """out, grad_offset and grad_weight: bit-identical across reruns and with the column buffer capped at one image;
    grad_x (float atomics): within the bound of the oracle test each time."""
    table, first = errors(name)
    want_gx = do.oracle(name)[1]
    again = run(cuda, name, True)
    chunked = run(cuda, name, True, col_bytes=1)
    for other, tag in ((again, 'rerun'), (chunked, 'one image per chunk')):
        for k in (0, 2, 3):
            assert torch.equal(first[k], other[k]), (tag, NAMES[k])
        e = float(np.abs(other[1].cpu().numpy().astype(np.float64) - want_gx).max())
        print(f'{name} {tag}: grad_x {e:.3e} (bound {table["grad_x"][2]:.3e})')
        assert e <= table['grad_x'][2], tag


def test_launches_and_no_host_synchronisation(cuda, monkeypatch):
    name = 'groups 4 dg 2'
    run(cuda, name, True)                                  # warm-up: library, BLAS
    run(cuda, name, True, col_bytes=1)
    torch.cuda.synchronize()
    calls = []
    real = _lib.launch
    monkeypatch.setattr(dc._lib, 'launch', lambda fn, *a, **k: calls.append(fn) or real(fn, *a, **k))
    x, offset, weight, grad_out, _, geo = do.problem(name)
    t = [torch.from_numpy(a.copy()).to(cuda).requires_grad_(True) for a in (x, offset, weight)]
    g = torch.from_numpy(grad_out.copy()).to(cuda)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = dc.deform_conv2d(*t, *geo)
        assert calls == ['ocrf_deform_im2col']
        out.backward(g)
        assert calls == ['ocrf_deform_im2col', 'ocrf_deform_col2im', 'ocrf_deform_im2col']
        del calls[:]
        dc.deform_conv2d(t[0].detach(), t[1].detach(), t[2], *geo).backward(g)       # only the weight: no col2im
        assert calls == ['ocrf_deform_im2col', 'ocrf_deform_im2col']
        del calls[:]
        monkeypatch.setattr(dc, 'COL_BYTES', 1)                                       # one image per chunk, n = 2
        dc.deform_conv2d(*t, *geo).backward(g)
        assert calls == ['ocrf_deform_im2col'] * 2 + ['ocrf_deform_col2im', 'ocrf_deform_im2col'] * 2
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert all(torch.isfinite(p.grad).all() for p in t)


def test_dispatch_autocast_checkpoint_and_double_backward(cuda, monkeypatch):
    name = '3x3 pad 1'
    x, offset, weight, grad_out, _, geo = do.problem(name)
    t = [torch.from_numpy(a.copy()).to(cuda).requires_grad_(True) for a in (x, offset, weight)]
    calls = []
    real = _lib.launch
    monkeypatch.setattr(dc._lib, 'launch', lambda fn, *a, **k: calls.append(fn) or real(fn, *a, **k))
    want = dc.deform_conv2d(*t, *geo)
    assert len(calls) == 1 and 'DeformConv2d' in type(want.grad_fn).__name__
    # not contiguous, float64 or fused=False: the torch formulation
    strided = t[0].detach().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not strided.is_contiguous()
    for args, kw in (((strided, t[1], t[2]), {}), ((t[0].double(), t[1].double(), t[2].double()), {}),
                     (tuple(t), dict(fused=False))):
        got = dc.deform_conv2d(*args, *geo, **kw)
        assert len(calls) == 1 and float((got.float() - want).detach().abs().max()) <= 1e-3
    # under autocast the op runs in float32 on the bf16 operands widened
    with torch.autocast('cuda', dtype=torch.bfloat16):
        got = dc.deform_conv2d(t[0].bfloat16(), t[1], t[2], *geo)
    assert got.dtype == torch.float32 and len(calls) == 2
    assert torch.equal(got, dc.deform_conv2d(t[0].bfloat16().float(), t[1], t[2], *geo))
    # a non-reentrant checkpoint recomputes the forward and reaches the same gradients
    g = torch.from_numpy(grad_out.copy()).to(cuda)
    base = torch.autograd.grad(dc.deform_conv2d(*t, *geo), t, g)
    out = torch.utils.checkpoint.checkpoint(lambda a, b, c: dc.deform_conv2d(a, b, c, *geo), *t, use_reentrant=False)
    cp = torch.autograd.grad(out, t, g)
    assert torch.equal(cp[1], base[1]) and torch.equal(cp[2], base[2])
    assert float((cp[0] - base[0]).abs().max()) <= errors(name)[0]['grad_x'][2]
    # a double backward raises
    out = dc.deform_conv2d(*t, *geo)
    gx, = torch.autograd.grad(out, t[0], g, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def test_refusals_before_any_launch(cuda, monkeypatch):
    x, offset, weight, _, _, (stride, padding, dilation, groups, dg) = do.problem('3x3 pad 1')
    xt, ot = torch.from_numpy(x.copy()).to(cuda), torch.from_numpy(offset.copy()).to(cuda)
    launched = []
    monkeypatch.setattr(dc._lib, 'launch', lambda fn, *a, **k: launched.append(fn))
    geo = ((3, 3), stride, padding, dilation, dg)
    strided = xt.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    for bad_x, bad_o in ((strided, ot), (xt.cpu(), ot), (xt, ot.cpu()), (xt.double(), ot), (xt, ot[:, :-1]), (xt[:1], ot)):
        with pytest.raises(_lib.OcrfHipError):
            dc.deform_im2col(bad_x, bad_o, *geo)
    with pytest.raises(_lib.OcrfHipError):
        dc.deform_im2col(xt, ot, *geo, n0=1, n1=1)
    gcol = torch.zeros(2, 8 * 9, 35, device=cuda)
    with pytest.raises(_lib.OcrfHipError):
        dc.deform_col2im(gcol.cpu(), xt, ot, *geo, torch.empty_like(xt), torch.empty_like(ot))
    with pytest.raises(_lib.OcrfHipError):
        dc.deform_col2im(gcol, xt, ot, *geo, torch.empty_like(xt)[:, :4], torch.empty_like(ot))
    assert launched == []
    # operands of 2 GiB, and a geometry that does not fit, at the C boundary: refused on the arguments alone
    L = _lib.lib()
    p = ctypes.c_void_p(4096)                     # never dereferenced
    invalid = 1                                   # hipErrorInvalidValue
    ok = (2, 8, 5, 7, 3, 3, 1, 1, 1, 1, 1, 1, 1, 0, 2)
    for args in ((4, 1 << 17, 64, 64) + ok[4:13] + (0, 1),            # x: 4 * 2^17 * 2^12 floats = 2^33 bytes
                 (2, 64, 1024, 1024) + ok[4:13] + (0, 2),              # col: 2 * 64 * 9 * 2^20 floats
                 (2, 2, 4096, 4096, 3, 3, 1, 1, 1, 1, 1, 1, 1, 0, 2),  # offset: 2 * 18 * 2^24 floats
                 (2, 8, 5, 7, 7, 3, 1, 1, 0, 1, 1, 1, 1, 0, 2),        # the input is smaller than the kernel
                 (2, 8, 5, 7, 3, 3, 1, 1, 1, 1, 1, 1, 3, 0, 2),        # C is not a multiple of dg
                 (2, 8, 5, 7, 3, 3, 0, 1, 1, 1, 1, 1, 1, 0, 2), ok[:13] + (1, 1), ok[:13] + (0, 3)):
        assert L.ocrf_deform_im2col(*args, p, p, p, None) == invalid, args
        assert L.ocrf_deform_col2im(*args, p, p, p, p, p, None) == invalid, args
    assert L.ocrf_deform_im2col(*ok, None, p, p, None) == invalid


# --------------------------------------------------------------------------------------------- end to end
def _grads_against_float64(build, inputs, cuda):
    """A module built by ``build()`` (seeded), its float64 CPU form as the reference: for the output and every
    parameter's gradient the errors of the fused and the torch form in float32 on the GPU, and the bound."""
    torch.manual_seed(0)
    ref = build().double()
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    results = []
    for where, fused in (('cpu', False), ('gpu', True), ('gpu', False)):
        net = build()
        net.load_state_dict({k: v.float() for k, v in state.items()})
        if where == 'cpu':
            net = net.double()
            args = [a.double() for a in inputs]
        else:
            net = net.to(cuda)
            args = [a.to(cuda) for a in inputs]
        for m in net.modules():
            if isinstance(m, dc.DeformConv2d):
                m.fused = fused
        net.eval()
        out = net(*args)
        if isinstance(out, tuple):                   # CenterHead: every head of every task
            out = torch.cat([v.flatten(1) for task in out for v in task[0].values()], 1)
        torch.manual_seed(1)
        weights = torch.randn(out.shape, dtype=torch.float64).to(out)
        (out * weights).sum().backward()
        results.append([out.detach().double().cpu()] + [p.grad.double().cpu() for p in net.parameters()])
    want, fused, plain = results
    names = ['out'] + [k for k, _ in build().named_parameters()]
    fails = []
    for what, w, f, p in zip(names, want, fused, plain):
        e_f, e_t = float((f - w).abs().max()), float((p - w).abs().max())
        bound = max(4 * e_t, 16 * EPS32 * float(w.abs().max()))
        if 'conv_offset' in what or 'adapt' in what or what in ('out', 'depth_conv.4.weight'):
            print(f'{what}: fused {e_f:.3e}, torch {e_t:.3e}, bound {bound:.3e}')
        if not e_f <= bound:
            fails.append(f'{what}: {e_f:.3e} > {bound:.3e}')
    assert not fails, fails


def _move_the_offsets(net):
    for m in net.modules():
        if isinstance(m, dc.DeformConv2dPack):
            torch.nn.init.normal_(m.conv_offset.weight, std=0.05)
            torch.nn.init.uniform_(m.conv_offset.bias, -1.5, 1.5)
    return net


def test_depthnet_with_native_dcn_end_to_end(cuda):
    before = depthnet.NATIVE_DCN
    depthnet.NATIVE_DCN = True
    try:
        gen = torch.Generator().manual_seed(4)
        inputs = [torch.randn(2, 8, 6, 10, generator=gen), torch.randn(2, 27, generator=gen)]
        _grads_against_float64(lambda: _move_the_offsets(depthnet.DepthNet(8, 8, 4, 6)), inputs, cuda)
    finally:
        depthnet.NATIVE_DCN = before


def test_center_head_with_dcn_separate_head_end_to_end(cuda):
    tasks = [dict(num_class=1, class_names=['car']), dict(num_class=2, class_names=['truck', 'bus'])]
    common = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2))
    dcn = dict(type='DCN', in_channels=16, out_channels=16, kernel_size=3, padding=1, groups=4)

    def build():
        head = ch.CenterHead(in_channels=8, tasks=tasks, common_heads=common, share_conv_channel=16,
                             separate_head=dict(type='DCNSeparateHead', dcn_config=dcn, head_conv=16, final_kernel=3))
        return _move_the_offsets(head)
    inputs = [torch.randn(2, 8, 9, 13, generator=torch.Generator().manual_seed(6))]
    _grads_against_float64(lambda: _ListInput(build()), inputs, cuda)


class _ListInput(torch.nn.Module):
    """``CenterHead.forward`` takes a list of feature maps."""

    def __init__(self, head):
        super().__init__()
        self.head = head

    def forward(self, x):
        return self.head([x])
