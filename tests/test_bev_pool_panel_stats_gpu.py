"""GPU: the panel pooling that also writes its output's channel statistics (``ocrf_bev_pool_v2_nchw_panel_stats``,
csrc/bev_pool_tile_out.h ``leave<C4, STATS>``).  The pooled BEV must not change by a bit, the statistics must be the
bits of ``hoa.channel_stats`` of that BEV (the kernel the epilogue replaces), every pixel of them written — tiles of
several units (statistics after the slab reduction, by the last arriver), tiles without panels, ragged grid edges, a
panel denser than the LDS cell window — and a ``HotPath`` step with the fused statistics must return what the step with
a statistics launch of its own returns."""
import numpy as np
import pytest
import torch

from ocrfdet_amd import bevpool, hoa, hotpath, synthetic
from tests import helpers
from tests.test_bev_pool_mfma_gpu import _t

pytestmark = pytest.mark.gpu


def _check(depth, feat, plan, layouts=(0, 1)):
    """out == the plain panel pooling, stats == channel_stats(out) on a NaN pre-fill, twice the same bits."""
    B, Z, Y, X, c = plan.shape
    for layout in layouts:
        want = bevpool.bev_pool_v2_panel(depth, feat, plan, layout=layout)
        want_stats = hoa.channel_stats(want.view(B, c, Y, X))
        runs = []
        for _ in range(2):
            stats = torch.full((B, 2, Y, X), float('nan'), device=depth.device)
            out = bevpool.bev_pool_v2_panel(depth, feat, plan, layout=layout, stats=stats)
            assert torch.equal(out, want)
            assert not torch.isnan(stats).any()                       # no pixel left unwritten
            assert torch.equal(stats, want_stats)
            runs.append((out, stats))
        assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
        assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))


@pytest.mark.parametrize('c', [64, 80, 96, 128])
@pytest.mark.parametrize('yx', [(8, 8), (13, 21)])
def test_random_problems_every_channel_count(cuda, c, yx):
    """Every instantiation, a grid of whole tiles and a ragged one.  Every tile collects ~ 900 feature rows: 19 panels in
    units of 2, so its statistics are taken by the last arriver after the slab reduction.  In the ragged case all points
    of batch 1's corner tile (ragged on both edges) are dropped: a unit without panels, whose statistics are zeros.  (On
    the 8 x 8 grid a tile is a whole plane of 30 000 points: a unit without panels exists only where one is built.)"""
    rng = np.random.default_rng(c + yx[0])
    Y, X = yx
    B, Z = 2, 1
    depth, feat, rd, rf, rb, _, _ = helpers.random_pool_problem(rng, 30000, B * Y * X, c, n_feat=900)
    ragged = (Y % 8 != 0) or (X % 8 != 0)
    if ragged:
        plane, y, x = rb // (Y * X), (rb % (Y * X)) // X, rb % X
        keep = ~((plane == 1) & (y // 8 == (Y - 1) // 8) & (x // 8 == (X - 1) // 8))
        assert keep.sum() < rb.size
        rd, rf, rb = rd[keep], rf[keep], rb[keep]
    plan = bevpool.MfmaPoolPlan(_t(rd, cuda), _t(rf, cuda), _t(rb, cuda), (B, Z, Y, X, c), group=2)
    units = plan.units.cpu().numpy()
    assert ((units[:, 3] >> 16) > 1).any()                            # a tile of several units
    if ragged:
        assert (units[:, 2] == units[:, 1]).any()                     # a unit without panels
    _check(_t(depth, cuda), _t(feat, cuda), plan)


def test_dense_panels(cuda):
    """The shape of test_bev_pool_panel_gpu.test_dense_panels_take_the_quarter_window_path: 3 072 cells per panel."""
    rng = np.random.default_rng(5)
    B, Z, Y, X, c = 1, 1, 8, 16, 80
    n_rows = 100
    v, r = np.meshgrid(np.arange(Y * X), np.arange(n_rows), indexing='ij')
    rb = np.repeat(v.ravel(), 2).astype(np.int32)                     # two points per cell
    rf = np.repeat(r.ravel(), 2).astype(np.int32)
    order = np.argsort(rb, kind='stable')
    rb, rf = rb[order], rf[order]
    rd = rng.integers(0, 5000, rb.size).astype(np.int32)
    depth = rng.random(5000, dtype=np.float32)
    feat = rng.standard_normal((n_rows, c)).astype(np.float32)
    plan = bevpool.MfmaPoolPlan(_t(rd, cuda), _t(rf, cuda), _t(rb, cuda), (B, Z, Y, X, c), group=8)
    assert int((plan.panel_cell_off[1:] - plan.panel_cell_off[:-1]).max()) == 64 * 48
    _check(_t(depth, cuda), _t(feat, cuda), plan, layouts=(1,))


def test_empty_plan_writes_zero_statistics(cuda):
    shape = (1, 1, 16, 16, 80)
    e = torch.zeros(0, dtype=torch.int32, device=cuda)
    plan = bevpool.MfmaPoolPlan(e, e, e, shape)
    stats = torch.full((1, 2, 16, 16), float('nan'), device=cuda)
    out = bevpool.bev_pool_v2_panel(torch.rand(100, device=cuda), torch.randn(10, 80, device=cuda), plan, layout=1,
                                    out=torch.full((1, 80, 16, 16), 7.0, device=cuda), stats=stats)
    assert float(out.abs().max()) == 0.0
    assert torch.equal(stats, torch.zeros_like(stats))


def test_wrapper_refuses_what_the_entry_point_refuses(cuda):
    e = torch.zeros(0, dtype=torch.int32, device=cuda)
    depth, feat = torch.rand(100, device=cuda), torch.randn(10, 80, device=cuda)
    from ocrfdet_amd import _lib
    plan = bevpool.MfmaPoolPlan(e, e, e, (1, 1, 16, 16, 80))
    for bad in (torch.zeros(1, 2, 16, 8, device=cuda), torch.zeros(1, 2, 16, 16, device=cuda, dtype=torch.float64),
                torch.zeros(1, 2, 16, 32, device=cuda)[..., ::2], torch.zeros(1, 2, 16, 16)):
        with pytest.raises(_lib.OcrfHipError):
            bevpool.bev_pool_v2_panel(depth, feat, plan, stats=bad)
    with pytest.raises(_lib.OcrfHipError):
        bevpool.bev_pool_v2_panel(depth, feat, plan, layout=2, stats=torch.zeros(1, 2, 16, 16, device=cuda))
    with pytest.raises(_lib.OcrfHipError):
        bevpool.bev_pool_v2_panel(depth, feat, bevpool.MfmaPoolPlan(e, e, e, (1, 2, 16, 16, 80)),
                                  stats=torch.zeros(1, 2, 16, 16, device=cuda))


@pytest.mark.parametrize('render', [False, True])
def test_hotpath_step_with_fused_statistics_equals_the_step_without(cuda, render):
    """The small HOA configuration of tests/test_sharded_hotpath_gpu.py; with ``render`` the two-stream step.  Three steps
    each way on the same inputs (issued call by call, recorded, replayed): every returned tensor equal, and the fused
    instance's recorded step holds the pooling with statistics and no statistics launch."""
    cfg = synthetic.PathConfig(**{**synthetic.CONFIGS['cfg0_1cam_128x352_bev64x64x4'].__dict__, 'name': 'small4cam_hoa',
                                  'n_cams': 4, 'n_frames': 2, 'render': render, 'hoa': True})
    fused, plain = (hotpath.HotPath(cfg, cuda, fuse_hoa_stats=f) for f in (True, False))
    assert fused._fused_stats() is not None and plain._fused_stats() is None
    depth, feat = fused.make_inputs(seed=3)
    for _ in range(3):
        a, b = fused.step(depth, feat), plain.step(depth, feat)
        torch.cuda.synchronize()
        ta, tb = list(hotpath.HotPath._flat_outputs(a)), list(hotpath.HotPath._flat_outputs(b))
        assert len(ta) == len(tb) >= 4
        assert all(torch.equal(x, y) for x, y in zip(ta, tb))
    for hp, with_stats, launches in ((fused, 1, 0), (plain, 0, 1)):
        assert hp.one_call_refused is None and len(hp._compiled) == 1
        names = next(iter(hp._compiled.values())).step.names
        assert names.count('ocrf_bev_pool_v2_nchw_panel_stats') == with_stats
        assert names.count('ocrf_bev_pool_v2_nchw_panel') == 2 - with_stats
        assert names.count('ocrf_hoa_channel_stats') == launches
    if render:
        fused.check_render_plans()
