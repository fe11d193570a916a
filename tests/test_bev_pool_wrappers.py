"""The Python layer around the pooling kernels (ocrfdet_amd/bevpool.py): one backward behind every autograd surface, one
``out=`` contract for the three planned wrappers, the 2 GiB refusal and the cached-pooling front end's backend table.
GPU tests are marked one by one; the others run on the host."""
import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib, bevpool, hotpath
from tests.test_pool_plan_host import _problem

SHAPE4 = (1, 2, 13, 21)                          # (B, Z, Y, X): ragged, the 8 x 8 tiles are cut by the border
N_PIX, N_DEPTH, N_PTS = 200, 1000, 9000         # feat (1,1,10,20,C), depth (1,1,5,10,20)
PAD_P, PAD_I = 517, 129


def _surface_problem(seed=3, n_pix=N_PIX):
    """Skewed voxel populations as ``test_pool_plan_host._problem``; a depth cell (d, h, w) belongs to ONE feature pixel
    (h, w) as in every real rank list, so the depth gradient has one writer per cell and is deterministic."""
    rb, rf, _, _, _ = _problem(seed, N_PTS, int(np.prod(SHAPE4)), n_pix)
    rng = np.random.default_rng(seed + 100)
    rd = (rng.integers(0, N_DEPTH // N_PIX, N_PTS) * N_PIX + rf % N_PIX).astype(np.int32)
    first = np.ones(N_PTS, bool)
    first[1:] = rb[1:] != rb[:-1]
    st = np.flatnonzero(first).astype(np.int32)
    ln = np.diff(np.append(st, N_PTS)).astype(np.int32)
    return rb, rd, rf, st, ln


def _junk(rng, n):
    return rng.integers(-2 ** 31, 2 ** 31 - 1, n, dtype=np.int64).astype(np.int32)


def _regroup(rf, rd, rb, n_pixels, n_live=None):
    """The backward's regroup by feature pixel as bevpool states it (stable sort, dense runs), on any device."""
    if n_live is not None:
        live = torch.arange(rf.numel(), dtype=torch.int32) < n_live
        rf = torch.where(live, rf, torch.full_like(rf, n_pixels))
    rf_sorted, perm = torch.sort(rf, stable=True)
    starts, lengths = bevpool.dense_runs(rf_sorted, n_pixels)
    return starts, lengths, rf_sorted, rd[perm], rb[perm]


def test_regroup_of_capacity_vectors_equals_that_of_exact_vectors():
    """Seed 3, 9000 points, 300 pixels, 517 junk entries: masking the tail past the count with a pixel index past the last
    one leaves starts, lengths, the sorted ranks and both permuted vectors of the live part unchanged."""
    rb, rd, rf, _, _ = _surface_problem(3, n_pix=300)
    rng = np.random.default_rng(3)
    exact = _regroup(*(torch.from_numpy(v) for v in (rf, rd, rb)), 300)
    cap = _regroup(*(torch.from_numpy(np.concatenate((v, _junk(rng, PAD_P)))) for v in (rf, rd, rb)), 300,
                   n_live=torch.tensor(N_PTS, dtype=torch.int32))
    assert torch.equal(cap[0], exact[0]) and torch.equal(cap[1], exact[1])
    for c, e in zip(cap[2:], exact[2:]):
        assert torch.equal(c[:N_PTS], e)
    assert int(exact[1].sum()) == N_PTS and int((exact[0] + exact[1]).max()) <= N_PTS     # no run reaches the tail


@pytest.fixture(scope='module')
def surface_case():
    """Ranks, operands and the oracle's results per channel count, computed once and left unchanged."""
    cache = {}

    def get(oracle_lib, c):
        if c not in cache:
            rb, rd, rf, st, ln = _surface_problem()
            rng = np.random.default_rng(17 + c)
            depth = rng.random((1, 1, 5, 10, 20)).astype(np.float32)
            feat = rng.standard_normal((1, 1, 10, 20, c)).astype(np.float32)
            shape = SHAPE4 + (c,)
            og = rng.standard_normal(shape).astype(np.float32)
            fwd = oracle_lib.bev_pool_v2(depth, feat, rd, rf, rb, shape, st, ln)          # (B,C,Z,Y,X)
            want_d, want_f = oracle_lib.bev_pool_v2_backward(og, depth, feat, rd, rf, rb)
            caps = [np.concatenate((v, _junk(rng, pad))) for v, pad in
                    ((rb, PAD_P), (rd, PAD_P), (rf, PAD_P), (st, PAD_I), (ln, PAD_I))]
            cache[c] = dict(ranks=(rb, rd, rf, st, ln), caps=caps, depth=depth, feat=feat, shape=shape, og=og, fwd=fwd,
                            want_d=want_d, want_f=want_f)
        return cache[c]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize('c', [12, 32, 80])
def test_one_backward_behind_every_autograd_surface(cuda, oracle_lib, surface_case, c):
    """C = 12 (not fusable: QuickCumsumCuda), 32 (fusable, no panel count), 80.  One upstream gradient, permuted into each
    surface's layout: the depth and feat gradients of QuickCumsumCuda, bev_pool_v2, bev_pool_v2_collapsed and
    bev_pool_v2_device_counts_autograd (layouts 0 and 1, capacity vectors with out-of-range junk behind the count) are
    ``torch.equal`` to each other and within test_backward_parity's tolerance of the C oracle; the forwards agree after the
    layout permutation."""
    p = surface_case(oracle_lib, c)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)              # noqa: E731
    B, Z, Y, X, C = p['shape']
    rb, rd, rf, st, ln = (dev(v) for v in p['ranks'])
    crb, crd, crf, cst, cln = (dev(v) for v in p['caps'])
    counts = dev(np.array([N_PTS, len(p['ranks'][3])], np.int32))
    og = dev(p['og'])                                                                # (B,Z,Y,X,C) rows
    og0 = og.permute(0, 4, 1, 2, 3).contiguous()                                     # (B,C,Z,Y,X)
    og1 = og.permute(0, 1, 4, 2, 3).reshape(B, Z * C, Y, X).contiguous()             # (B,Z*C,Y,X)
    rows0 = lambda o: o.permute(0, 2, 3, 4, 1)                                       # noqa: E731
    rows1 = lambda o: o.view(B, Z, C, Y, X).permute(0, 1, 3, 4, 2)                   # noqa: E731
    surfaces = [
        ('QuickCumsumCuda', lambda d, f: bevpool.QuickCumsumCuda.apply(d, f, rd, rf, rb, p['shape'], st, ln), og, lambda o: o),
        ('bev_pool_v2', lambda d, f: bevpool.bev_pool_v2(d, f, rd, rf, rb, p['shape'], st, ln), og0, rows0),
        ('collapsed', lambda d, f: bevpool.bev_pool_v2_collapsed(d, f, rd, rf, rb, p['shape'], st, ln), og1, rows1)]
    counted = [(f'counts{layout}', lambda d, f, layout=layout: bevpool.bev_pool_v2_device_counts_autograd(
        d, f, crd, crf, crb, p['shape'], cst, cln, counts, layout=layout), g, rows)
        for layout, g, rows in ((0, og0, rows0), (1, og1, rows1))]
    if bevpool._fusable(c):
        surfaces += counted
    else:
        for _, fn, _, _ in counted:
            with pytest.raises(_lib.OcrfHipError):
                fn(dev(p['depth']), dev(p['feat']))
    want_rows = torch.from_numpy(p['fwd']).permute(0, 2, 3, 4, 1)
    scale = float(np.abs(p['fwd']).max())
    results = []
    for name, fn, g, rows in surfaces:
        d, f = dev(p['depth']).requires_grad_(), dev(p['feat']).requires_grad_()
        out = fn(d, f)
        out.backward(g)
        err = float((rows(out.detach()).cpu() - want_rows).abs().max())
        print(f'C={c} {name}: forward max|err| {err:.3e} (scale {scale:.3e})')
        assert err <= 1e-4 * scale, name
        results.append((name, d.grad, f.grad))
    _, d0, f0 = results[0]
    np.testing.assert_allclose(d0.cpu().numpy(), p['want_d'], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(f0.cpu().numpy(), p['want_f'], rtol=1e-4, atol=1e-4)
    assert float(d0.abs().max()) > 0 and float(f0.abs().max()) > 0
    for name, dg, fg in results[1:]:
        assert torch.equal(dg, d0) and torch.equal(fg, f0), name


@pytest.mark.gpu
def test_out_contract_of_the_three_planned_wrappers(cuda):
    """planned / MFMA / panel on one (1,1,16,16,80) problem: a valid ``out`` comes back as the same object with the result
    of the call without ``out``; float64, a non-contiguous view, a ``numel`` off by one and a feat of 64 channels are
    refused before anything is launched."""
    rng = np.random.default_rng(5)
    shape = (1, 1, 16, 16, 80)
    n = 400
    rb = np.sort(rng.integers(0, 256, n)).astype(np.int32)
    rf = rng.integers(0, 64, n).astype(np.int32)
    rd = (rng.integers(0, 4, n) * 64 + rf).astype(np.int32)
    st = np.flatnonzero(np.r_[True, rb[1:] != rb[:-1]]).astype(np.int32)
    ln = np.diff(np.append(st, n)).astype(np.int32)
    rb, rf, rd, st, ln = (torch.from_numpy(v).to(cuda) for v in (rb, rf, rd, st, ln))
    depth = torch.from_numpy(rng.random((1, 1, 4, 8, 8)).astype(np.float32)).to(cuda)
    feat = torch.from_numpy(rng.standard_normal((1, 1, 8, 8, 80)).astype(np.float32)).to(cuda)
    tile = bevpool.DevicePoolPlan(rd, rf, rb, shape, st, ln)
    panel = bevpool.MfmaPoolPlan(rd, rf, rb, shape, group=8)
    numel = 80 * 16 * 16
    for fn, plan in ((bevpool.bev_pool_v2_planned, tile), (bevpool.bev_pool_v2_mfma, panel),
                     (bevpool.bev_pool_v2_panel, panel)):
        want = fn(depth, feat, plan)
        out = torch.full_like(want, float('nan'))
        assert fn(depth, feat, plan, out=out) is out and torch.equal(out, want), fn.__name__
        for bad in (torch.empty(want.shape, dtype=torch.float64, device=cuda),
                    torch.empty(1, 80, 16, 32, device=cuda)[..., ::2],
                    torch.empty(numel + 1, device=cuda)):
            with pytest.raises(_lib.OcrfHipError):
                fn(depth, feat, plan, out=bad)
        with pytest.raises(_lib.OcrfHipError):
            fn(depth, feat[..., :64].contiguous(), plan)
    torch.cuda.synchronize()


def test_size_check_refuses_two_gib_on_sizes_alone():
    bevpool._check_32bit_offsets(torch.empty(2 ** 29 - 1, device='meta'))
    with pytest.raises(_lib.OcrfHipError, match='2 GiB'):
        bevpool._check_32bit_offsets(torch.empty(2 ** 29, device='meta'))


@pytest.mark.parametrize('op', ['bev_pool_v2', 'bev_pool_v2_collapsed', 'bev_pool_v2_device_counts',
                                'bev_pool_v2_device_counts_autograd'])
def test_tile_kernel_wrappers_refuse_two_gib_before_any_device_call(op):
    """The tile kernel addresses ``feat`` through the same 32-bit buffer resource as the planned kernels: its wrappers
    refuse 2 GiB as well, on the sizes of meta tensors — before the device is asked for anything."""
    feat = torch.empty(1, 1, 2 ** 12, 2 ** 12, 32, device='meta')                   # 2^29 fp32 elements
    depth = torch.empty(1, 1, 2, 2 ** 12, 2 ** 12, device='meta')
    r = torch.empty(4, dtype=torch.int32, device='meta')
    args = (depth, feat, r, r, r, (1, 1, 8, 8, 32), r, r)
    if 'counts' in op:
        args += (torch.empty(2, dtype=torch.int32, device='meta'),)
    with pytest.raises(_lib.OcrfHipError, match='2 GiB'):
        getattr(bevpool, op)(*args)


def _ranks(n):
    return torch.zeros(n, dtype=torch.int32)


@pytest.mark.parametrize('backend,c,n,route', [('panel', 80, 5, 'panel'), ('mfma', 96, 5, 'mfma'), ('panel', 32, 5, 'tile'),
                                               ('mfma', 32, 5, 'tile'), ('tile', 80, 5, 'tile'), ('panel', 80, 0, 'unplanned'),
                                               ('tile', 32, 0, 'unplanned')])
def test_backend_table(backend, c, n, route):
    """The front end's pure decision: asked backend, channel count, point count -> kernel; statistics only from the panel
    kernel with Z == 1 in layout 0 or 1."""
    for z in (1, 2):
        plan = bevpool.PoolPlan(_ranks(n), _ranks(n), _ranks(n), _ranks(1), _ranks(1), (1, z, 13, 21, c))
        assert plan.route(backend) == route
        for layout in (0, 1, 2):
            assert plan.writes_stats(backend, layout) == (route == 'panel' and z == 1 and layout in (0, 1))
    assert hotpath.PoolPlan is bevpool.PoolPlan


@pytest.mark.parametrize('backend,c,n', [('panel', 80, 5), ('mfma', 96, 5), ('panel', 32, 5), ('tile', 80, 5), ('panel', 80, 0)])
def test_hotpath_pool_routes_and_plan_arguments(monkeypatch, backend, c, n):
    """``HotPath.pool`` with the kernels' wrappers and the plan builders replaced by recorders: which wrapper pools which of
    the path's plans, which plan is built (once) with which arguments, that a foreign plan object takes the tile kernel and
    that only the panel route accepts ``stats``."""
    calls = []
    for name in ('bev_pool_v2_planned', 'bev_pool_v2_mfma', 'bev_pool_v2_panel', 'bev_pool_v2_collapsed'):
        monkeypatch.setattr(bevpool, name, lambda *a, _n=name, **k: calls.append((_n, k)) or _n)
    for name in ('DevicePoolPlan', 'MfmaPoolPlan'):
        monkeypatch.setattr(bevpool, name, lambda *a, _n=name, **k: calls.append((_n, k)) or object())
    hp = object.__new__(hotpath.HotPath)
    hp.lss_pool_backend = hp.ht_pool_backend = backend
    hp.lss_mfma_group, hp.lss_panel_unit_cost = 3, 8.0
    mk = lambda z: hotpath.PoolPlan(_ranks(n), _ranks(n), _ranks(n), _ranks(1), _ranks(1), (1, z, 13, 21, c))   # noqa: E731
    hp.lss, hp.ht, other = mk(2), mk(1), mk(1)
    panel_route = n > 0 and c in (64, 80, 96, 128) and backend in ('panel', 'mfma')
    wrapper = 'bev_pool_v2_collapsed' if n == 0 else f'bev_pool_v2_{backend}' if panel_route else 'bev_pool_v2_planned'
    for plan, kw in ((hp.lss, dict(group=8, unit_cost=8.0) if backend == 'panel' else dict(group=3)), (hp.ht, dict(group=8))):
        for _ in range(2):
            assert hp.pool(plan, None, None) == wrapper
        built = [(k, a) for k, a in calls if k.endswith('Plan')]
        want = [] if n == 0 else [('MfmaPoolPlan', kw)] if panel_route else [('DevicePoolPlan', {})]
        assert built == want and [k for k, _ in calls if not k.endswith('Plan')] == [wrapper] * 2
        assert (plan.mfma_plan is not None) == (panel_route) and (plan.device_plan is not None) == (n > 0 and not panel_route)
        del calls[:]
    assert hp.pool(other, None, None) == ('bev_pool_v2_planned' if n else 'bev_pool_v2_collapsed')
    assert other.mfma_plan is None
    for plan in (hp.lss, hp.ht, other):
        if plan is hp.ht and panel_route and backend == 'panel':
            assert hp.pool(plan, None, None, stats='s') == wrapper and calls[-1][1]['stats'] == 's'
        elif plan is not hp.lss or not (panel_route and backend == 'panel'):
            with pytest.raises(_lib.OcrfHipError):
                hp.pool(plan, None, None, stats='s')
