"""The two plan-driven poolings (csrc/bev_pool_mfma.hip, csrc/bev_pool_panel.hip) and their plan (bevpool.MfmaPoolPlan)
at the plan's edges, against the float64 oracle and the derived bound of tests/panel_pool_oracle.py:
|got - want| <= gamma_(n_v + P_t) sum |d_p f_p|, element by element — no tolerance of this file's own.

Matrix: every scene x C in {64, 80, 96, 128} x (group, unit_cost) in {(1, -), (2, -), (8, -), (8, 8.0)}; every case is
the 480-voxel grid of the scenes.  Per case: the plan's records rebuilt on the host equal the scene's kept points; both
kernels in layouts 0, 1 and 2 inside the bound, writing nothing outside `out`; one plan serving several calls; and the
MFMA form against the panel form, bit for bit."""
import functools

import numpy as np
import pytest
import torch

from ocrfdet_amd import bevpool
from tests import panel_pool_oracle as ppo

pytestmark = pytest.mark.gpu

SETTINGS = {'g1': (1, None), 'g2': (2, None), 'g8': (8, None), 'g8_cost8': (8, 8.0)}
MATRIX = [(s, c, k) for s in ppo.SCENES for c in ppo.CHANNELS for k in SETTINGS]
KERNELS = {'mfma': bevpool.bev_pool_v2_mfma, 'panel': bevpool.bev_pool_v2_panel}
GUARD = 64                   # sentinel floats on each side of `out`: 256 bytes, the layout-2 stores stay 16-byte aligned
SENTINEL = 12345.0


def _t(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)                 # a copy: the shared references are read-only


@functools.lru_cache(maxsize=None)
def _scene(name):
    rd, rf, rb = ppo.SCENES[name]()
    return rd, rf, rb, ppo.structure(rd, rf, rb)


@functools.lru_cache(maxsize=None)
def _reference(name, c, seed):
    """Inputs, float64 sums, bound and point counts of a scene: computed once, shared, never written."""
    rd, rf, rb, _ = _scene(name)
    depth, feat = ppo.make_inputs(rd, rf, rb, c, seed)
    want, mag, n_v = ppo.oracle(depth, feat, rd, rf, rb, ppo.grid_shape(c))
    out = (depth, feat, want, ppo.bound(mag, n_v, rf, rb), n_v)
    for a in out:
        a.setflags(write=False)
    return out


def _plan(cuda, name, c, key):
    rd, rf, rb, _ = _scene(name)
    group, unit_cost = SETTINGS[key]
    return bevpool.MfmaPoolPlan(_t(rd, cuda), _t(rf, cuda), _t(rb, cuda), ppo.grid_shape(c), group=group, unit_cost=unit_cost)


def _guarded(cuda, n):
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device=cuda)
    buf[:GUARD] = SENTINEL
    buf[-GUARD:] = SENTINEL
    return buf, buf[GUARD:GUARD + n]


def _check_rows(got_rows, name, c, seed, what):
    """got (n_vox, C) float32 against the float64 sums -> largest err / bound."""
    rd, rf, rb, _ = _scene(name)
    depth, feat, want, bound, n_v = _reference(name, c, seed)
    assert np.isfinite(got_rows).all(), f'{what}: non-finite output'
    err = np.abs(got_rows.astype(np.float64) - want)
    live = n_v > 0
    ratio = float((err[live] / bound[live]).max())
    print(f'{what}: max err/bound {ratio:.4f}')
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (f'{what}: {bad.shape[0]} elements beyond the bound, first (voxel, channel) {bad[0].tolist()}: '
                           f'got {got_rows[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r} bound {bound[tuple(bad[0])]:.3e} '
                           f'n_v {n_v[bad[0][0]]}')
    assert np.all(got_rows[~live] == 0.0), f'{what}: a voxel without points is not exactly 0'
    krd, krf, krb = ppo.kept_points(rd, rf, rb)
    one = np.isin(krb, np.flatnonzero(n_v == 1))                   # krb is sorted: the voxels' order
    assert np.array_equal(got_rows[n_v == 1], depth[krd[one], None] * feat[krf[one]]), \
        f'{what}: a voxel of one point is not the rounded product'
    return ratio


# ----------------------------------------------------------------------------------------------------------------
# the plan
# ----------------------------------------------------------------------------------------------------------------
def _plan_records(plan):
    """The plan on the host -> per-panel tile, and per cell (panel, voxel slot, row slot, feature row, depth ranks)."""
    h = {k: getattr(plan, k).cpu().numpy() for k in ('units', 'unit_slab', 'panel_rows', 'panel_nrows', 'panel_cell_off',
                                                      'cells', 'rd_sorted', 'panel_voff', 'cell_code')}
    h['cells'] = h['cells'].view(np.uint32).astype(np.int64)
    h['cell_code'] = h['cell_code'].view(np.uint16).astype(np.int64)
    return h


@pytest.mark.parametrize('name,c,key', MATRIX)
def test_plan_is_the_scene_regrouped(cuda, name, c, key):
    rd, rf, rb, s = _scene(name)
    group, unit_cost = SETTINGS[key]
    plan = _plan(cuda, name, c, key)
    h = _plan_records(plan)
    KP, TV = ppo.KP, ppo.TV
    n_panels = s['n_panels']
    units = h['units'].astype(np.int64)
    u_tile, u_p0, u_p1, u_slice, u_n = units[:, 0], units[:, 1], units[:, 2], units[:, 3] & 0xFFFF, units[:, 3] >> 16
    assert plan.n_units == units.shape[0] and plan.n_tiles == ppo.N_TILES
    assert plan.n_panels == n_panels and plan.n_points == rb.size - 3

    # units: every tile's panels covered contiguously, slices 0 .. n-1, n in every unit, at most `group` panels each —
    # the very cuts the scene's numpy structure implies
    expect = ppo.expected_units(s, group, unit_cost)
    for t in range(ppo.N_TILES):
        m = np.flatnonzero(u_tile == t)
        order = m[np.argsort(u_slice[m])]
        assert u_slice[order].tolist() == list(range(order.size)) and np.all(u_n[m] == order.size)
        cuts = list(zip(u_p0[order].tolist(), u_p1[order].tolist()))
        assert cuts == expect[t]
        if s['panels_per_tile'][t]:
            assert cuts[0][0] == s['panel_off'][t] and cuts[-1][1] == s['panel_off'][t] + s['panels_per_tile'][t]
            assert all(a1 == b0 for (_, a1), (b0, _) in zip(cuts[:-1], cuts[1:]))
            assert all(1 <= b - a <= group for a, b in cuts)
        else:
            assert cuts == [(0, 0)]
        # slabs: one run of n slabs per tile of several units, the same first slab in each of its units
        if order.size > 1:
            assert np.all(h['unit_slab'][m] == h['unit_slab'][m[0]])
    multi = {int(t): (int(h['unit_slab'][i]), int(u_n[i])) for i, t in enumerate(u_tile) if u_n[i] > 1}
    spans = sorted(multi.values())
    assert all(a0 + an <= b0 for (a0, an), (b0, _) in zip(spans[:-1], spans[1:]))
    assert plan.n_slab_slices == sum(n for _, n in spans) and (not spans or (spans[0][0] >= 0 and sum(spans[-1]) <= plan.n_slab_slices))
    assert plan.slabs.numel() >= max(plan.n_slab_slices, 1) * TV * c * 4
    assert np.all(np.diff(u_p1 - u_p0) <= 0)                                   # heaviest first
    if name == 'units' and key == 'g1':
        assert {8, 9, 16, 17} <= set(u_n.tolist())                                # the kSB = 8 slab batches of the write-out
    if name == 'units' and key == 'g8':
        assert 8 in (u_p1 - u_p0)                                              # exactly kMaxUnitPanels
    if name == 'units' and key == 'g8_cost8':
        plain = ppo.expected_units(s, 8)
        assert all(cuts_c[0][1] - cuts_c[0][0] < cuts_p[0][1] - cuts_p[0][0]
                   for t, (cuts_c, cuts_p) in enumerate(zip(expect, plain)) if t in ppo.UNIT_TILE_ROWS)
        assert units.shape[0] > sum(len(e) for e in plain)

    # panels and cells -> (voxel, feature row, depth ranks in list order)
    pan_tile = np.repeat(np.arange(ppo.N_TILES), s['panels_per_tile'])
    assert h['panel_nrows'][:n_panels].sum() == s['rows_per_tile'].sum() == plan.unique_rows
    assert np.array_equal(h['panel_cell_off'][1:] - h['panel_cell_off'][:-1], s['cells_per_panel'])
    assert h['panel_cell_off'][0] == 0 and h['panel_cell_off'][-1] == plan.n_cells == plan.cw.numel() == h['cell_code'].size
    krd, krf, krb = ppo.kept_points(rd, rf, rb)
    scene_cells = {}
    for d, f, b in zip(krd.tolist(), krf.tolist(), krb.tolist()):
        scene_cells.setdefault((b, f), []).append(d)
    seen = set()
    for p in range(n_panels):
        nr = int(h['panel_nrows'][p])
        rows = h['panel_rows'][p * KP:p * KP + nr]
        assert np.all(np.diff(rows) > 0)                                       # unique, ascending
        c0, c1 = int(h['panel_cell_off'][p]), int(h['panel_cell_off'][p + 1])
        rec = h['cells'][c0:c1]
        v, r, npts = rec[:, 0] & 0xFF, (rec[:, 0] >> 8) & 0xFF, rec[:, 0] >> 16
        assert np.all(r < nr) and np.all(v < TV)
        assert np.all(np.diff(v * KP + r) > 0)                                 # voxel-major, rows ascending, no cell twice
        assert np.array_equal(h['cell_code'][c0:c1], r | (v << 8))            # the panel kernel's view of the same cells
        assert np.array_equal(h['panel_voff'][p * TV:(p + 1) * TV], np.searchsorted(v, np.arange(TV)))
        vox = ppo.voxel_of(np.full(v.size, pan_tile[p]), v)
        assert np.all(vox >= 0)
        for i in range(c1 - c0):
            if npts[i] <= 3:
                ranks = rec[i, 1:1 + npts[i]].tolist()
                assert npts[i] >= 1
            else:
                assert npts[i] == 0xFFFF and rec[i, 2] > 3
                ranks = h['rd_sorted'][rec[i, 1]:rec[i, 1] + rec[i, 2]].tolist()
            cell = (int(vox[i]), int(rows[r[i]]))
            assert cell not in seen
            seen.add(cell)
            assert scene_cells.get(cell) == ranks, f'cell {cell}: the plan holds other points than the scene'
    assert seen == set(scene_cells)                                            # no kept point left out


# ----------------------------------------------------------------------------------------------------------------
# the kernels
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,c,key', MATRIX)
def test_both_kernels_within_the_bound_in_every_layout(cuda, name, c, key):
    shape = ppo.grid_shape(c)
    depth, feat, want, bound, n_v = _reference(name, c, ppo.SEEDS[0])
    d, f = _t(depth, cuda), _t(feat, cuda)
    plan = _plan(cuda, name, c, key)
    rows, dev = {}, {}
    for layout in (0, 1, 2):
        for kname, pool in KERNELS.items():
            buf, out = _guarded(cuda, want.size)
            if kname == 'panel':
                plan.cw.fill_(float('nan'))                                    # the pre-pass writes every cell weight
            ret = pool(d, f, plan, layout=layout, out=out)
            assert ret.data_ptr() == out.data_ptr()
            host = buf.cpu().numpy()
            assert np.all(host[:GUARD] == SENTINEL) and np.all(host[-GUARD:] == SENTINEL), f'{kname}: wrote outside out'
            got = host[GUARD:-GUARD]
            assert not np.isnan(got).any(), f'{kname} layout {layout}: part of out was never written'
            rows[kname, layout], dev[kname] = ppo.from_layout(got, shape, layout), out
            _check_rows(rows[kname, layout], name, c, ppo.SEEDS[0], f'{name} C={c} {key} {kname} layout {layout}')
        diff = rows['mfma', layout] != rows['panel', layout]
        gap = float(np.abs(rows['mfma', layout].astype(np.float64) - rows['panel', layout]).max())
        print(f'{name} C={c} {key} layout {layout}: mfma vs panel {int(diff.sum())} elements differ, largest difference {gap:.3e}')
        assert torch.equal(dev['mfma'], dev['panel']), 'the MFMA and the panel form differ'
    assert int(plan.arrive.abs().max()) == 0
    for kname in KERNELS:                                                      # the layouts are one result, three ways out
        assert np.array_equal(rows[kname, 0], rows[kname, 1]) and np.array_equal(rows[kname, 0], rows[kname, 2])


@pytest.mark.parametrize('name,c,key', MATRIX)
def test_one_plan_serves_several_calls(cuda, name, c, key):
    """Inputs A, B, A again on one plan, nothing between the calls: the slabs and tickets of a call are the next one's."""
    ins = [tuple(_t(a, cuda) for a in _reference(name, c, seed)[:2]) for seed in ppo.SEEDS]
    plan = _plan(cuda, name, c, key)
    for kname, pool in KERNELS.items():
        outs = [pool(*ins[i], plan, layout=2) for i in (0, 1, 0)]
        a0, b, a1 = (o.cpu().numpy().reshape(-1, c) for o in outs)
        assert int(plan.arrive.abs().max()) == 0
        assert np.array_equal(a0, a1), f'{kname}: the same inputs, another result'
        _check_rows(a0, name, c, ppo.SEEDS[0], f'{name} C={c} {key} {kname} call A')
        _check_rows(b, name, c, ppo.SEEDS[1], f'{name} C={c} {key} {kname} call B')
