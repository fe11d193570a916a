"""GPU: ``ocrf_bev_align_forward`` / ``_backward`` (csrc/bev_align.hip) through ``ocrfdet_amd.temporal`` against float64
``F.grid_sample`` autograd on the CPU at the true transform (tests/bev_align_oracle.py, where the bounds are derived).

Per shape the transforms are run in batches of n: the identity, an integer shift and a quarter turn with a flip (exact:
the forward is an indexing of x), the twelve realistic motions of the fixture (tests/golden/bev_align.npz: cases a, b,
c with ``bda_adj != bda``, d with flips), a shift that leaves 7 % of the plane covered, and scales 0.25 and 3 with a
rotation.  The oracle of a batch is computed once and shared.
"""
import functools
import os

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib
from ocrfdet_amd import temporal
from tests import bev_align_oracle as bo

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1, 13, 10), (3, 5, 16, 24), (2, 8, 9, 17), (2, 8, 128, 128)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bev_align.npz')


@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def transforms(h, w):
    """[(name, (2, 3) float64)]: the first three are exact.  The fixture's are float64 and not float32 numbers: the
    kernels round them, which the coordinate bound covers."""
    out = [('identity', bo.IDENTITY), ('shift', bo.integer_shift(3, -2)), ('turn', bo.rot90_flip(h, w))]
    for tag in 'abcd':
        out += [(f'fixture {tag}{b}', t) for b, t in enumerate(fixture()[f'{tag}.tf'][:, :2])]
    out += [('mostly outside', bo.affine(h, w, shift=(0.93 * w, 0.0))),
            ('scale 0.25', bo.affine(h, w, angle=0.3, scale=0.25, shift=(0.4, -0.7))),
            ('scale 3', bo.affine(h, w, angle=-0.3, scale=3.0, shift=(-0.6, 0.2)))]
    return [(name, np.asarray(t, np.float64)) for name, t in out]


@functools.lru_cache(maxsize=None)
def batches(shape):
    """[(names, tf (n, 3, 3) float64, x, g float32, oracle out, oracle grad_x)]; the last batch is filled up with the
    first transforms."""
    n, c, h, w = shape
    ts = transforms(h, w)
    rng = np.random.default_rng(sum(shape))
    out = []
    for s in range(0, len(ts), n):
        part = (ts[s:s + n] + ts[:n])[:n]
        tf = np.zeros((n, 3, 3))
        tf[:, 2, 2] = 1
        tf[:, :2] = np.stack([t for _, t in part])
        x = rng.standard_normal(shape).astype(np.float32)
        g = rng.standard_normal(shape).astype(np.float32)
        out.append(([name for name, _ in part], tf, x, g) + bo.oracle(x, tf, g))
    return out


def run(cuda, tf, x, g):
    xt = torch.from_numpy(x).to(cuda).requires_grad_(True)
    out = temporal.shift_feature(xt, torch.from_numpy(tf).to(cuda))
    out.backward(torch.from_numpy(g).to(cuda))
    return out.detach().cpu().numpy(), xt.grad.cpu().numpy()


@pytest.mark.parametrize('shape', SHAPES)
def test_forward_backward_and_adjoint_against_the_float64_oracle(cuda, shape):
    n, c, h, w = shape
    fails = []
    for names, tf, x, g, want, want_grad in batches(shape):
        got, got_grad = run(cuda, tf, x, g)
        assert got.shape == shape and got.dtype == np.float32 and got_grad.shape == shape
        absx = bo.sample(torch.from_numpy(np.abs(x).astype(np.float64)), tf).numpy()
        for b, name in enumerate(names):
            t = tf[b:b + 1]
            xmax, gmax = float(np.abs(x[b]).max()), float(np.abs(g[b]).max())
            e_f, b_f = float(np.abs(got[b] - want[b]).max()), bo.forward_bound(t, h, w, xmax)
            e_b, b_b = float(np.abs(got_grad[b] - want_grad[b]).max()), bo.backward_bound(t, h, w, gmax)
            lhs = float((got[b].astype(np.float64) * g[b]).sum())
            rhs = float((x[b].astype(np.float64) * got_grad[b]).sum())
            b_a = 16 * bo.EPS * float((absx[b] * np.abs(g[b])).sum())
            print(f'{shape} {name}: forward {e_f:.3e} (bound {b_f:.3e}), backward {e_b:.3e} (bound {b_b:.3e}), '
                  f'adjoint {abs(lhs - rhs):.3e} (bound {b_a:.3e})')
            if not e_f <= b_f:
                fails.append(f'{name}: forward {e_f:.3e} > {b_f:.3e}')
            if not e_b <= b_b:
                fails.append(f'{name}: backward {e_b:.3e} > {b_b:.3e}')
            if not abs(lhs - rhs) <= b_a:
                fails.append(f'{name}: adjoint {abs(lhs - rhs):.3e} > {b_a:.3e}')
    assert not fails, fails


@pytest.mark.parametrize('shape', SHAPES)
def test_exact_transforms_are_an_indexing_of_x(cuda, shape):
    n, c, h, w = shape
    done = set()
    for names, tf, x, g, _, _ in batches(shape):
        got, _ = run(cuda, tf, x, g)
        for b, name in enumerate(names):
            if name in ('identity', 'shift', 'turn'):
                assert np.array_equal(got[b], bo.index_sample(x[b], tf[b, :2])), name
                done.add(name)
    assert done == {'identity', 'shift', 'turn'}
    assert np.array_equal(bo.index_sample(batches(shape)[0][2][0], bo.IDENTITY), batches(shape)[0][2][0])


def test_singular_transform_reads_one_place_from_everywhere(cuda):
    """An all-zero 2 x 2 block at 8 x 8: the forward is constant per channel, the backward's box is the whole plane and
    four source pixels collect the whole gradient."""
    shape = (2, 3, 8, 8)
    rng = np.random.default_rng(8)
    tf = np.zeros((2, 3, 3))
    tf[:, 2, 2] = 1
    tf[0, :2, 2], tf[1, :2, 2] = (2.25, 4.5), (6.75, -0.5)
    x, g = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    want, want_grad = bo.oracle(x, tf, g)
    got, got_grad = run(cuda, tf, x, g)
    assert np.isfinite(got).all() and np.isfinite(got_grad).all()
    assert (got == got[:, :, :1, :1]).all()
    for b in range(2):
        t = tf[b:b + 1]
        assert int(bo.readers(tf[b, :2], 8, 8).max()) == 64
        assert np.abs(got[b] - want[b]).max() <= bo.forward_bound(t, 8, 8, float(np.abs(x[b]).max()))
        assert np.abs(got_grad[b] - want_grad[b]).max() <= bo.backward_bound(t, 8, 8, float(np.abs(g[b]).max()))
    assert np.count_nonzero(got_grad[0, 0]) == 4 and np.count_nonzero(got_grad[1, 0]) == 2


@pytest.mark.parametrize('shape', [(3, 5, 16, 24), (2, 8, 9, 17)])
def test_two_runs_are_bit_identical(cuda, shape):
    for names, tf, x, g, _, _ in batches(shape)[-2:]:
        a, b = run(cuda, tf, x, g), run(cuda, tf, x, g)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_out_writes_one_channel_slice_and_nothing_else(cuda):
    names, tf, x, g, _, _ = batches((3, 5, 16, 24))[1]
    xt, tft = torch.from_numpy(x).to(cuda), torch.from_numpy(tf).to(cuda)
    want = temporal.shift_feature(xt, tft)
    sentinel = -12345.5
    wide = torch.full((3, 15, 16, 24), sentinel, device=cuda)
    ret = temporal.shift_feature(xt, tft, out=wide[:, 5:10])
    assert ret.data_ptr() == wide[:, 5:10].data_ptr()
    assert torch.equal(wide[:, 5:10], want)
    assert (wide[:, :5] == sentinel).all() and (wide[:, 10:] == sentinel).all()
    # a destination 4 bytes off a 16-byte boundary takes the 4-byte stores: the same values, its neighbours untouched
    buf = torch.full((want.numel() + 2,), sentinel, device=cuda)
    off = buf[1:-1].view(want.shape)
    assert off.data_ptr() % 16 == 4
    temporal.shift_feature(xt, tft, out=off)
    assert torch.equal(off, want) and float(buf[0]) == sentinel and float(buf[-1]) == sentinel
    with pytest.raises(_lib.OcrfHipError):
        temporal.shift_feature(xt.clone().requires_grad_(True), tft, out=wide[:, 5:10])
    with pytest.raises(_lib.OcrfHipError):
        temporal.shift_feature(xt, tft, out=wide[:, 5:11])


def poses(cuda):
    """Per-frame poses of three frames (key, two adjacent ones) from the fixture's 16 x 24 cases, and the rest of
    ``align_and_cat``'s arguments."""
    f = fixture()
    t = lambda k: torch.from_numpy(f[k]).to(cuda)    # noqa: E731
    s2k = [t('b.curr'), t('b.adj'), t('c.adj')]
    return s2k, (t('b.bda'), torch.from_numpy(f['b.grid_interval']), torch.from_numpy(f['b.grid_lower_bound']))


def frames(cuda, grads=(True, True, True)):
    gen = torch.Generator().manual_seed(11)
    return [torch.randn(3, 5, 16, 24, generator=gen).to(cuda).requires_grad_(r) for r in grads]


@pytest.mark.parametrize('frame_ids', [[0, 1, 2], [2, 1, 0]])
def test_align_and_cat_against_the_torch_path(cuda, frame_ids):
    s2k, extra = poses(cuda)
    feats = frames(cuda)
    got = temporal.align_and_cat(feats, frame_ids, s2k, *extra, fused=True)
    want = temporal.align_and_cat(feats, frame_ids, s2k, *extra, fused=False)
    assert got.shape == want.shape == (3, 15, 16, 24) and got.is_contiguous()
    assert got.grad_fn is not None and 'AlignCat' in type(got.grad_fn).__name__
    key = frame_ids.index(0)
    assert torch.equal(got[:, 5 * key:5 * key + 5], feats[key])
    r = torch.randn(got.shape, generator=torch.Generator().manual_seed(5)).to(cuda)
    g_got, g_want = torch.autograd.grad(got, feats, r), torch.autograd.grad(want, feats, r)
    # the copied frame's gradient is a view of the incoming one
    assert g_got[key].data_ptr() == r[:, 5 * key:].data_ptr() and torch.equal(g_got[key], r[:, 5 * key:5 * key + 5])
    for k, fid in enumerate(frame_ids):
        if fid == 0:
            continue
        tf = temporal.feature_transform([s2k[0], s2k[fid]], *extra).cpu().numpy()
        b_f = 2 * bo.forward_bound(tf, 16, 24, float(feats[k].detach().abs().max()))
        b_b = 2 * bo.backward_bound(tf, 16, 24, float(r.abs().max()))
        e_f = float((got[:, 5 * k:5 * k + 5] - want[:, 5 * k:5 * k + 5]).abs().max())
        e_b = float((g_got[k] - g_want[k]).abs().max())
        print(f'{frame_ids} frame {fid}: fused - torch {e_f:.3e} (bound {b_f:.3e}), gradient {e_b:.3e} (bound {b_b:.3e})')
        assert e_f <= b_f and e_b <= b_b


def test_frames_without_a_gradient_launch_no_backward(cuda, monkeypatch):
    s2k, extra = poses(cuda)
    feats = frames(cuda, grads=(True, True, False))
    calls = []
    real = _lib.launch
    monkeypatch.setattr(temporal._lib, 'launch', lambda name, *a, **k: calls.append(name) or real(name, *a, **k))
    out = temporal.align_and_cat(feats, [0, 1, 2], s2k, *extra, fused=True)
    assert calls == ['ocrf_bev_align_forward'] * 2
    out.sum().backward()
    assert calls == ['ocrf_bev_align_forward'] * 2 + ['ocrf_bev_align_backward']
    assert feats[0].grad is not None and feats[1].grad is not None and feats[2].grad is None
    del calls[:]
    with torch.no_grad():
        temporal.align_and_cat(feats, [0, 1, 2], s2k, *extra)
    assert calls == (['ocrf_bev_align_forward'] * 2 if temporal.FUSED_ALIGN_DEFAULT else [])


def test_no_host_synchronisation(cuda):
    s2k, extra = poses(cuda)
    feats = frames(cuda, grads=(True, True, False))
    temporal.align_and_cat(feats, [0, 1, 2], s2k, *extra, fused=True).sum().backward()     # warm-up: library, BLAS
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for f in feats:
            f.grad = None
        out = temporal.align_and_cat(feats, [0, 1, 2], s2k, *extra, fused=True)
        out.backward(torch.ones_like(out))
        tf = temporal.feature_transform([s2k[0], s2k[1]], *extra)
        temporal.shift_feature(feats[2], tf)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.isfinite(feats[1].grad).all()


def test_sequential_form_through_the_method(cuda, monkeypatch):
    """``extract_img_feat_sequential`` (bevdet.py:401-406): the cached previous features as (num_frame - 1, C, H, W),
    poses repeated per frame, through ``shift_feature_method`` adopted on a detector-like object."""
    f = fixture()
    t = lambda k: torch.from_numpy(f[k]).to(cuda)    # noqa: E731
    det = type('Detector', (), dict(shift_feature=temporal.shift_feature_method, gen_grid=temporal.gen_grid))()
    det.img_view_transformer = type('VT', (), dict(grid_interval=torch.from_numpy(f['b.grid_interval']),
                                                   grid_lower_bound=torch.from_numpy(f['b.grid_lower_bound'])))()
    calls = []
    real = _lib.launch
    monkeypatch.setattr(temporal._lib, 'launch', lambda name, *a, **k: calls.append(name) or real(name, *a, **k))
    feat_prev = torch.randn(3, 5, 16, 24, generator=torch.Generator().manual_seed(2)).to(cuda)
    out = det.shift_feature(feat_prev, [t('b.curr'), t('b.adj')], t('b.bda'))
    assert calls == ['ocrf_bev_align_forward'] and out.shape == feat_prev.shape
    want, _ = bo.oracle(feat_prev.cpu().numpy(), f['b.tf'], np.zeros(feat_prev.shape))
    bound = bo.forward_bound(f['b.tf'], 16, 24, float(feat_prev.abs().max()))
    assert float(np.abs(out.cpu().numpy() - want).max()) <= bound
    assert out.view(1, 15, 16, 24).is_contiguous()
    det.fused_align = False
    assert float((det.shift_feature(feat_prev, [t('b.curr'), t('b.adj')], t('b.bda')) - out).abs().max()) <= 2 * bound
    assert calls == ['ocrf_bev_align_forward']
    grid = det.gen_grid(feat_prev, [t('b.curr'), t('b.adj')], t('b.bda'))
    assert grid.shape == (3, 16, 24, 2) and grid.is_cuda


def test_dispatch_and_refusals(cuda, monkeypatch):
    """float16 maps are computed in float32 (``@force_fp32``); float64, non-contiguous and CPU maps take the torch
    formulation in ``align_and_cat`` and are refused by ``shift_feature`` itself."""
    names, tf, x, g, _, _ = batches((3, 5, 16, 24))[1]
    xt, tft = torch.from_numpy(x).to(cuda), torch.from_numpy(tf).to(cuda)
    half = temporal.shift_feature(xt.half(), tft)
    assert half.dtype == torch.float32 and torch.equal(half, temporal.shift_feature(xt.half().float(), tft))
    strided = xt.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not strided.is_contiguous()
    for bad in (xt.double(), strided, xt.cpu(), xt[:0]):
        with pytest.raises(_lib.OcrfHipError):
            temporal.shift_feature(bad, tft)
    with pytest.raises(_lib.OcrfHipError):
        temporal.shift_feature(xt, tft[:2])
    s2k, extra = poses(cuda)
    feats = frames(cuda, grads=(False, False, False))
    calls = []
    real = _lib.launch
    monkeypatch.setattr(temporal._lib, 'launch', lambda name, *a, **k: calls.append(name) or real(name, *a, **k))
    want = temporal.align_and_cat(feats, [0, 1, 2], s2k, *extra, fused=True)
    assert len(calls) == 2
    other = [feats[0], strided_copy(feats[1]), feats[2]]
    got = temporal.align_and_cat(other, [0, 1, 2], s2k, *extra, fused=True)
    assert len(calls) == 2 and torch.allclose(got, want, rtol=0, atol=1e-3)
    got = temporal.align_and_cat([f.double() for f in feats], [0, 1, 2], s2k, *extra, fused=True)
    assert len(calls) == 2 and got.dtype == torch.float64
    # poses that require a gradient: the torch formulation, which is differentiable in them
    s2k_grad = [s2k[0], s2k[1].clone().requires_grad_(True), s2k[2]]
    got = temporal.align_and_cat(feats, [0, 1, 2], s2k_grad, *extra, fused=True)
    assert len(calls) == 2 and got.requires_grad
    halves = temporal.align_and_cat([f.half() for f in feats], [0, 1, 2], s2k, *extra, fused=True)
    assert len(calls) == 4 and halves.dtype == torch.float32


def strided_copy(t):
    out = t.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not out.is_contiguous() and torch.equal(out, t)
    return out


@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (1, 2, 4, 8)])
@pytest.mark.parametrize('half', [torch.float16, torch.bfloat16])
def test_half_maps_under_their_autocast_are_the_float32_call(cuda, monkeypatch, shape, half):
    """float16 maps under fp16 autocast, bfloat16 maps under bf16 autocast without ``keep_bf16``: ``shift_feature`` and
    ``align_and_cat`` (one warped, one copied frame) run the float32 kernels forward and backward and give, bit for
    bit, what they give outside autocast on the maps cast by hand; (2, 3, 5, 7) has an odd plane and takes the narrow
    path, (1, 2, 4, 8) the 16-byte one."""
    f = fixture()
    n, c, h, w = shape
    t = lambda k: torch.from_numpy(f[k][:n]).to(cuda)                                # noqa: E731
    s2k = [t('b.curr'), t('b.adj')]
    extra = (t('b.bda'), torch.from_numpy(f['b.grid_interval']), torch.from_numpy(f['b.grid_lower_bound']))
    tf = temporal.feature_transform(s2k, *extra)
    gen = torch.Generator().manual_seed(sum(shape))
    maps = [torch.randn(shape, generator=gen).to(cuda).to(half).requires_grad_(True) for _ in range(2)]
    wide = [m.detach().float().requires_grad_(True) for m in maps]
    r = torch.randn(n, 2 * c, h, w, generator=gen).to(cuda)
    want_cat = temporal.align_and_cat(wide, [1, 0], s2k, *extra, fused=True)
    want_one = temporal.shift_feature(wide[0], tf)
    (want_cat * r).sum().backward()
    want_grads = [m.grad.clone() for m in wide]
    wide[0].grad = None
    (want_one * r[:, :c]).sum().backward()
    calls = []
    real = _lib.launch
    monkeypatch.setattr(temporal._lib, 'launch', lambda name, *a, **k: calls.append(name) or real(name, *a, **k))
    with torch.autocast('cuda', dtype=half):
        got_cat = temporal.align_and_cat(maps, [1, 0], s2k, *extra, fused=True)
        got_one = temporal.shift_feature(maps[0], tf)
    assert calls == ['ocrf_bev_align_forward'] * 2
    assert got_cat.dtype == got_one.dtype == torch.float32
    assert torch.equal(got_cat, want_cat) and torch.equal(got_one, want_one)
    assert torch.equal(got_cat[:, c:], maps[1].detach().float())                     # the key frame: a copy
    (got_cat * r).sum().backward()
    assert calls[2:] == ['ocrf_bev_align_backward']                                  # the float32 gather
    # the float32 gradient, rounded once by the backward of the cast
    assert all(m.grad.dtype == half and torch.equal(m.grad, g.to(half)) for m, g in zip(maps, want_grads))
    maps[0].grad = None
    (got_one * r[:, :c]).sum().backward()
    assert calls[3:] == ['ocrf_bev_align_backward'] and torch.equal(maps[0].grad, wide[0].grad.to(half))
