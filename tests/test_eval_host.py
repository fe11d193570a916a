"""``detection_eval.evaluate_host`` (the arm of CPU tensors and ``fused=False``) against the sequential oracle of
tests/eval_oracle.py on every scene, the two hand-computed cases against literal numbers, the refusals and the
reference-keyed result dict.  No GPU.

The host arm matches per (sample, class) like the kernel and the oracle walks the whole set class by class, so their
agreement is also the check of that decomposition.  Integers, orderings and the per-match errors (the same float64
operations in the same order) must be equal; the curve results differ only by the order of sums of at most 90 addends
of magnitude <= max(1, max|err|) (numpy's pairwise ``mean`` in the oracle, a sequential sum in the host arm): 2 * 90 u
relative to that magnitude, u = 2^-53, plus one rounding per addend for mAP, mTP and NDS.
"""
import numpy as np
import pytest
import torch

from ocrfdet_amd import detection_eval as de
from tests import eval_oracle as eo

U = 2.0 ** -53


def to_tensors(batch):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)) for a in batch]


@pytest.mark.parametrize('name', list(eo.SCENES))
def test_evaluate_host_equals_the_oracle(name):
    scene, want = eo.SCENES[name], eo.result_of(name)
    cfg = eo.config_of(scene)
    got = de.evaluate_host(cfg, scene.batches())
    nc = cfg.n_classes
    evaluated = (got['info'] & de.EVALUATED) != 0
    assert np.array_equal(evaluated, want['evaluated'])
    assert np.array_equal(np.stack([(got['info'] >> (8 + t)) & 1 for t in range(4)], 1) * evaluated[:, None], want['tp'])
    assert np.array_equal(got['match'], want['match']) and np.array_equal(got['gt_count'], want['gt_count'])
    assert np.array_equal(got['err'], want['err'], equal_nan=True)
    for c in range(nc):
        lo, hi = np.searchsorted(got['sorted_cls'], c), np.searchsorted(got['sorted_cls'], c + 1)
        assert np.array_equal(got['order'][lo:hi], want['order'][c]), c
        for t in range(4):
            flag = (got['info'][got['order'][lo:hi]] >> (8 + t)) & 1
            tp = got['tp_excl'][t, lo:hi] - (got['tp_excl'][t, lo] if hi > lo else 0) + flag
            assert np.array_equal(tp, want['tp_cum'][c][t]), (c, t)
    res = got['result']
    ap, tpe = res[:4 * nc].reshape(nc, 4), res[4 * nc:9 * nc].reshape(nc, 5)
    mag = max(1.0, float(np.nanmax(np.abs(want['err']))) if np.isfinite(want['err']).any() else 1.0)
    bound = (2 * 90 + 4) * U * mag
    assert np.all(np.abs(ap - want['AP']) <= bound)
    assert np.array_equal(np.isnan(tpe), np.isnan(want['tp_errors']))
    assert np.all((np.abs(tpe - want['tp_errors']) <= bound) | np.isnan(tpe))
    assert abs(res[9 * nc] - want['mAP']) <= bound + 8 * nc * U
    assert np.array_equal(np.isnan(res[9 * nc + 1:9 * nc + 6]), np.isnan(want['mTP']))
    assert np.all((np.abs(res[9 * nc + 1:9 * nc + 6] - want['mTP']) <= bound + 2 * nc * U * mag) | np.isnan(want['mTP']))
    assert abs(res[9 * nc + 6] - want['NDS']) <= bound + 2 * nc * U * mag


def test_the_settings_equal_the_oracles_literal_tables():
    """``EvalConfig``'s defaults (ranges, predicted attributes, periods and exclusions, thresholds, first recall point)
    against the tables ``eval_oracle.Rules`` states literally."""
    cfg, rules = de.EvalConfig(eo.CLASSES), eo.Rules()
    assert cfg.class_names == rules.class_names == eo.CLASSES
    assert cfg.class_range == rules.class_range and cfg.class_tab == rules.class_tab
    assert cfg.dist_ths == rules.dist_ths and cfg.tp_index == rules.tp_index and cfg.first == 11
    assert (cfg.min_recall, cfg.min_precision) == (rules.min_recall, rules.min_precision)


def test_the_hand_computed_cases():
    """``perfect``: AP 1, errors 0, NDS 1.  ``half``: AP = ((36 + 2.25 (1/3 + 1/5 + ... + 1/19)) / 90) / 0.9 at every
    threshold (derived in ``eval_oracle.half``), errors 0 but the attribute error, 1, of a class without attributes."""
    cfg = de.EvalConfig(eo.CLASSES)
    res = de.evaluate_host(cfg, eo.SCENES['perfect'].batches())['result']
    assert np.allclose(res[:40], 1.0, rtol=0, atol=1e-12)
    assert np.nanmax(np.abs(res[40:90])) == 0.0 and np.isnan(res[40:90]).sum() == 5
    assert abs(res[90] - 1.0) < 1e-12 and np.all(res[91:96] == 0.0) and abs(res[96] - 1.0) < 1e-12
    res = de.evaluate_host(cfg, eo.SCENES['half'].batches())['result']
    assert abs(eo.HALF_AP - 0.47592376472665426) < 1e-15
    assert np.allclose(res[:4], 0.47592376472665426, rtol=0, atol=1e-9)
    assert list(res[40:45]) == [0.0, 0.0, 0.0, 0.0, 1.0]
    assert abs(res[90] - 0.047592376472665426) < 1e-9           # nine classes without a prediction: AP 0
    # mATE, mASE over ten classes (car 0, the others 1); mAOE over nine, mAVE and mAAE over eight (mAAE: all 1)
    assert np.allclose(res[91:96], [0.9, 0.9, 8 / 9, 7 / 8, 1.0], rtol=0, atol=1e-12)
    nds = (5 * 0.047592376472665426 + 0.1 + 0.1 + 1 / 9 + 1 / 8) / 10
    assert abs(res[96] - nds) < 1e-9


def test_the_evaluator_on_cpu_tensors_and_its_result_dict():
    scene = eo.SCENES['periods']
    cfg = eo.config_of(scene)
    ev = de.DetectionEval(cfg, eo.S, eo.M, eo.G, 'cpu')
    assert not ev.fused and ev.bytes_per_sample == 64 * eo.M + 4 * 10
    for batch in scene.batches():
        ev.update(*to_tensors(batch))
    out = ev.compute()
    want = de.evaluate_host(cfg, scene.batches())
    assert np.array_equal(out['result'].numpy(), want['result'], equal_nan=True)
    assert out['AP'].shape == (10, 4) and out['tp_errors'].shape == (10, 5) and out['tp_excl'].shape == (4, eo.S * eo.M)
    host = ev.results_to_host()
    res = want['result']
    p = 'pts_bbox_NuScenes'
    assert host[f'{p}/car_AP_dist_0.5'] == res[0] and host[f'{p}/car_AP_dist_4.0'] == res[3]
    assert host[f'{p}/barrier_AP_dist_2.0'] == res[4 * eo.BARRIER + 2]
    assert host[f'{p}/truck_orient_err'] == res[40 + 5 * eo.TRUCK + 2] and np.isnan(host[f'{p}/traffic_cone_attr_err'])
    assert [host[f'{p}/{k}'] for k in ('mATE', 'mASE', 'mAOE', 'mAVE', 'mAAE')] == list(res[91:96])
    assert host[f'{p}/mAP'] == res[90] and host[f'{p}/NDS'] == res[96]
    assert len(host) == 10 * 9 + 7 and all(type(v) is float for v in host.values())
    ev.reset()
    assert ev.n_samples == 0
    with pytest.raises(ValueError, match='nothing'):
        ev.compute()


def test_refusals():
    with pytest.raises(ValueError, match='dist_th_tp'):
        de.EvalConfig(eo.CLASSES, dist_th_tp=3.0)
    with pytest.raises(ValueError, match='class_names'):
        de.EvalConfig([f'c{k}' for k in range(17)], class_range={f'c{k}': 50.0 for k in range(17)})
    with pytest.raises(ValueError, match='no range'):
        de.EvalConfig(['car', 'tram'])
    with pytest.raises(ValueError, match='four'):
        de.EvalConfig(eo.CLASSES, dist_ths=(1.0, 2.0), dist_th_tp=2.0)
    cfg = de.EvalConfig(eo.CLASSES)
    with pytest.raises(TypeError, match='EvalConfig'):
        de.DetectionEval(dict(), 4, 8, 4, 'cpu')
    ev = de.DetectionEval(cfg, 4, 8, 4, 'cpu')
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype)      # noqa: E731
    i32 = torch.int32
    good = lambda B=1: [z(B, 8, 9), z(B, 8), z(B, 8, dtype=i32), z(B, dtype=i32), z(B, 4, 9), z(B, 4, dtype=i32),  # noqa: E731
                        z(B, dtype=i32)]
    ev.update(*good(3))
    with pytest.raises(ValueError, match='capacity'):
        ev.update(*good(2))
    ev.update(*good(1))
    assert ev.n_samples == 4
    ev.reset()
    for k, shape in ((0, (1, 9, 9)), (1, (1, 7)), (3, (2,)), (4, (1, 4, 7)), (5, (1, 5))):
        bad = good()
        bad[k] = z(*shape, dtype=bad[k].dtype)
        with pytest.raises(ValueError):
            ev.update(*bad)
    bad = good()
    bad[2] = z(1, 8, dtype=torch.int64)
    with pytest.raises(TypeError, match='labels'):
        ev.update(*bad)
    with pytest.raises(ValueError, match='gt_attrs'):
        ev.update(*good(), gt_attrs=z(1, 5, dtype=i32))
    with pytest.raises(TypeError, match='gt_valid'):
        ev.update(*good(), gt_valid=z(1, 4))
    assert ev.n_samples == 0


def test_score_keys_order_scores_descending():
    scores = np.array([0.5, -0.0, 0.0, -1.5, 1e-30, 3.0, -1e-30], np.float32)
    keys = de.score_keys(scores)
    assert list(np.argsort(keys, kind='stable')) == [5, 0, 4, 1, 2, 6, 3]       # -0 and +0 tie: by position
    back = de.key_scores(keys)
    assert np.array_equal(back, np.where(scores == 0, np.float32(0.0), scores)) and not np.signbit(back[1])
