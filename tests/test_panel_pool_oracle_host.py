"""The scenes of tests/panel_pool_oracle.py hit the edges they name, and the derived bound is one a correct float32
pooling meets with room: the repository's C oracle (a chain of fmaf in point order) stays inside it on every scene, and
the smallest contribution of a single point stands a hundred times above the largest bound.  CPU only."""
import numpy as np
import pytest

from tests import panel_pool_oracle as ppo

C_HOST = 80


@pytest.fixture(scope='module')
def scenes():
    return {name: fn() for name, fn in ppo.SCENES.items()}


@pytest.fixture(scope='module')
def structures(scenes):
    return {name: ppo.structure(*pts) for name, pts in scenes.items()}


@pytest.mark.parametrize('name', list(ppo.SCENES))
def test_scene_frame(scenes, name):
    """What every scene promises: the grid, the three dropped points at the end, a stably sorted kept list that is not
    in construction order, row 0 / entry 0 unreferenced, and the same scene on every call."""
    rd, rf, rb = scenes[name]
    assert (ppo.B, ppo.Z, ppo.Y, ppo.X, ppo.N_VOX, ppo.TPP, ppo.N_TILES) == (1, 2, 12, 20, 480, 6, 12)
    assert rd.dtype == rf.dtype == rb.dtype == np.int32 and rd.shape == rf.shape == rb.shape
    assert rb[-3:].tolist() == [-1, ppo.N_VOX, ppo.N_VOX + 5]
    assert np.all(np.diff(rb[:-3]) >= 0) and rb[0] >= 0 and rb[-4] < ppo.N_VOX
    assert rf.min() > 0 and rd.min() > 0 and rf.max() < ppo.N_FEAT and rd.max() < ppo.N_DEPTH
    krd, krf, krb = ppo.kept_points(rd, rf, rb)
    assert krb.size == rb.size - 3
    assert not set(rf[-3:].tolist()) & set(krf.tolist()) and not set(rd[-3:].tolist()) & set(krd.tolist())
    again = ppo.SCENES[name]()
    assert all(np.array_equal(a, b) for a, b in zip(again, (rd, rf, rb)))
    depth, feat = ppo.make_inputs(rd, rf, rb, C_HOST, 1)
    assert np.isnan(depth[0]) and np.isnan(feat[0]).all()
    assert np.isnan(depth[rd[-3:]]).all() and np.isnan(feat[rf[-3:]]).all()
    assert np.isfinite(depth[krd]).all() and np.isfinite(feat[krf]).all()
    assert np.isnan(depth).sum() == ppo.N_DEPTH - np.unique(krd).size
    assert np.isnan(feat).all(1).sum() == ppo.N_FEAT - np.unique(krf).size
    live_d, live_f = depth[np.isfinite(depth)], np.abs(feat[np.isfinite(feat)])
    assert live_d.min() >= 0.25 and live_d.max() < 1.0 and live_f.min() >= 0.5 and live_f.max() < 2.0
    assert (feat[np.isfinite(feat)] < 0).any() and (feat[np.isfinite(feat)] > 0).any()


def test_cells_scene_hits_the_cell_sum_forks(scenes, structures):
    rd, rf, rb = scenes['cells']
    s = structures['cells']
    assert set(s['points_per_cell'].tolist()) == set(ppo.CELL_COUNTS)
    assert {3, 4, 8, 9, 16, 17} <= set(ppo.CELL_COUNTS)                  # inline | list, the batches of kPB = 8
    cells_of_voxel = np.bincount(s['cell_voxel'], minlength=ppo.N_VOX)
    one = int(ppo.voxel_of(*ppo.CELLS_ONE_VOXEL))
    assert cells_of_voxel[one] == len(ppo.CELL_COUNTS)
    assert sorted(s['points_per_cell'][s['cell_voxel'] == one].tolist()) == sorted(ppo.CELL_COUNTS)
    single = s['cell_voxel'][np.isin(s['cell_voxel'], np.flatnonzero(cells_of_voxel == 1))]
    lone = {int(v): int(n) for v, n in zip(s['cell_voxel'], s['points_per_cell']) if v in set(single.tolist())}
    lone.pop(ppo.N_VOX - 1)
    assert sorted(lone.values()) == sorted(ppo.CELL_COUNTS)              # the same counts, one cell per voxel
    last = rb == ppo.N_VOX - 1
    assert last.sum() == 1 and rf[last][0] == ppo.N_FEAT - 1
    assert ppo.tile_of(ppo.N_VOX - 1) == (ppo.N_TILES - 1, 3 * 8 + 3)      # (plane 1, y 11, x 19): the ragged corner tile
    assert np.all(np.diff(np.flatnonzero(rb == one)) == 1)
    krf = rf[rb == one]
    assert np.any(np.diff(krf) < 0)                                      # the list was permuted: a voxel's rows interleave


def test_rows_scene_hits_the_panel_borders(scenes, structures):
    rd, rf, rb = scenes['rows']
    s = structures['rows']
    assert s['rows_per_tile'].tolist() == list(ppo.ROWS_PER_TILE) == [1, 45, 47, 48, 49, 95, 96, 97, 0, 3, 50, 2]
    assert s['panels_per_tile'].tolist() == [1, 1, 1, 1, 2, 2, 2, 3, 0, 1, 2, 1]
    assert s['rows_in_last_panel'].tolist() == [1, 45, 47, 48, 1, 47, 48, 1, 0, 3, 2, 2]
    assert set(s['points_per_cell'].tolist()) == {1, 2}
    krd, krf, krb = ppo.kept_points(rd, rf, rb)
    tile, _ = ppo.tile_of(krb)
    pairs = np.unique(np.stack((tile, krf, krb), 1), axis=0)             # (tile, row, voxel) cells
    _, voxels_per_row = np.unique(pairs[:, :2], axis=0, return_counts=True)
    assert set(voxels_per_row.tolist()) == {1, 2, 3}


def test_units_scene_hits_the_unit_and_slab_borders(scenes, structures):
    s = structures['units']
    want_rows = np.zeros(ppo.N_TILES, np.int64)
    for t, n in ppo.UNIT_TILE_ROWS.items():
        want_rows[t] = n
    assert s['rows_per_tile'].tolist() == want_rows.tolist()
    assert sorted(want_rows[want_rows > 0].tolist()) == [384, 385, 768, 769, 816]
    assert sorted(s['panels_per_tile'][want_rows > 0].tolist()) == [8, 9, 16, 17, 17]
    for t in ppo.UNIT_TILE_ROWS:
        p0 = int(s['panel_off'][t])
        assert s['longest_run'][p0] == ppo.KP                            # one voxel owns the whole first panel
        assert s['longest_run'][p0 + 1:p0 + int(s['panels_per_tile'][t])].max() < 8
    n_units = {g: sorted(len(u) for t, u in enumerate(ppo.expected_units(s, g)) if want_rows[t]) for g in (1, 2, 8)}
    assert n_units[1] == [8, 9, 16, 17, 17] and n_units[2] == [4, 5, 8, 9, 9] and n_units[8] == [1, 2, 2, 3, 3]
    plain = ppo.expected_units(s, 8)
    cut = ppo.expected_units(s, 8, 8.0)
    assert any(b - a == 8 for u in plain for a, b in u)                  # a unit of exactly kMaxUnitPanels
    for t in ppo.UNIT_TILE_ROWS:
        assert cut[t][0][1] - cut[t][0][0] == 2                          # cost 7 + one ordinary panel fill unit_cost = 8
        assert len(cut[t]) > len(plain[t]) and max(b - a for a, b in cut[t]) <= 8
        assert [a for a, _ in cut[t][1:]] == [b for _, b in cut[t][:-1]]


def test_dense_scene_hits_the_cell_windows(scenes, structures):
    s = structures['dense']
    assert s['panels_per_tile'].tolist() == [1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0]
    assert s['rows_per_tile'][[0, 1, 6, 7]].tolist() == [8, 16, 9, 17]
    assert s['cells_per_panel'].tolist() == [512, 1024, 513, 1025]       # kCR * kBlock, kCellCap, each + 1
    assert set(s['points_per_cell'].tolist()) == {1}


def test_layouts_round_trip():
    shape = ppo.grid_shape(3)
    rows = np.arange(ppo.N_VOX * 3, dtype=np.float64).reshape(ppo.N_VOX, 3)
    l0, l1 = ppo.to_layout(rows, shape, 0), ppo.to_layout(rows, shape, 1)
    assert l0.shape == (1, 3, 2, 12, 20) and l1.shape == (1, 6, 12, 20)
    assert l0[0, 2, 1, 11, 19] == rows[-1, 2] and l1[0, 3 + 2, 11, 19] == rows[-1, 2] and l1[0, 1, 0, 1] == rows[1, 1]
    for layout in (0, 1, 2):
        assert np.array_equal(ppo.from_layout(ppo.to_layout(rows, shape, layout), shape, layout), rows)


@pytest.mark.parametrize('seed', ppo.SEEDS)
@pytest.mark.parametrize('c', ppo.CHANNELS)
@pytest.mark.parametrize('name', list(ppo.SCENES))
def test_float32_reference_within_the_bound_and_points_cannot_hide(oracle_lib, scenes, name, c, seed):
    """At every channel count and input seed the GPU test uses.  The C oracle knows no dropped points (it would write
    out of bounds): it gets the kept ones."""
    rd, rf, rb = scenes[name]
    shape = ppo.grid_shape(c)
    depth, feat = ppo.make_inputs(rd, rf, rb, c, seed)
    want, mag, n_v = ppo.oracle(depth, feat, rd, rf, rb, shape)
    bound = ppo.bound(mag, n_v, rf, rb)
    assert np.isfinite(want).all() and np.isfinite(bound).all()
    assert np.all(bound[n_v == 0] == 0) and np.all(want[n_v == 0] == 0) and np.all(bound[n_v > 0] > 0)
    assert np.all(mag[n_v > 0] >= ppo.MIN_TERM * n_v[n_v > 0, None])
    krd, krf, krb = (a.astype(np.int32) for a in ppo.kept_points(rd, rf, rb))
    st, ln = oracle_lib.intervals_from_sorted(krb)
    ref = ppo.from_layout(oracle_lib.bev_pool_v2(depth, feat, krd, krf, krb, shape, st, ln), shape, 0)
    err = np.abs(ref.astype(np.float64) - want)
    assert np.all(err <= bound)
    ratio = float((err[n_v > 0] / bound[n_v > 0]).max())
    print(f'{name} C={c} seed {seed}: float32 point-order sum reaches {ratio:.3f} of the bound; largest bound {bound.max():.3e}, '
          f'{ppo.MIN_TERM / bound.max():.0f}x below a single point')
    assert ppo.MIN_TERM / bound.max() >= 100
    one = n_v == 1                                                       # a voxel of one point: the rounded product
    assert one.any() or name in ('units', 'dense')
    assert np.array_equal(ref[one], (depth[krd, None] * feat[krf])[np.isin(krb, np.flatnonzero(one))])
