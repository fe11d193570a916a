"""Host: the float64 decode oracle (tests/decode_oracle.py) pinned to the reference's values
(``tests/golden/center_head_decode.npz``), and the torch formulation of get_bboxes (``fused_decode = False``) held to the
oracle on the sweep of decode cases; the limits of the decode refused before anything runs."""
import json

import numpy as np
import pytest
import torch

from ocrfdet_amd import center_decode as cd

from . import decode_oracle as oracle
from .test_center_head_decode_host import check_padded, make_head, preds


@pytest.fixture(scope='module')
def g(golden):
    return golden('center_head_decode.npz')


def test_oracle_matches_reference(g):
    c = json.loads(str(g['cfg']))
    ncls = [t['num_class'] for t in c['tasks']]
    keys = ('heatmap', 'reg', 'height', 'dim', 'rot', 'vel')
    p = [{k: g[f't{t}.{k}'] for k in keys} for t in range(len(ncls))]
    want = oracle.decode(p, ncls, c['coder'], c['test_cfg'])
    check_padded(g, *(torch.from_numpy(x) for x in want))


def test_oracle_iou_matches_reference_pairs(g):
    """The reference's decided pairs (float64 polygon clipping) against mmcv's construction, and crafted geometry."""
    a, b, want = g['iou_a'], g['iou_b'], g['iou']
    got = np.array([oracle.iou_one_to_many(a[k], b[k:k + 1])[0] for k in range(len(a))])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
    sq = np.array([0.0, 0.0, 2.0, 2.0, 0.0])
    cases = [([0, 0, 2, 2, 0], 1.0), ([0, 0, 2, 2, np.pi / 2], 1.0), ([0, 0, 1, 1, 0], 0.25), ([2, 0, 2, 2, 0], 0.0),
             ([2, 2, 2, 2, 0], 0.0), ([5, 5, 2, 2, 0.3], 0.0), ([0, 0, 0, 2, 0], 0.0), ([1, 0, 2, 2, 0], 1 / 3),
             ([0, 0, 2, 2, np.pi / 4], (8 * (np.sqrt(2) - 1)) / (8 - 8 * (np.sqrt(2) - 1)))]
    got = oracle.iou_one_to_many(sq, np.array([c for c, _ in cases], np.float64))
    np.testing.assert_allclose(got, [w for _, w in cases], rtol=0, atol=1e-12)


def test_oracle_iou_matches_torch_clipping_on_random_pairs():
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.uniform(-1, 1, (400, 2)), rng.uniform(0.1, 3, (400, 2)), rng.uniform(-4, 4, (400, 1))], 1)
    b = np.concatenate([rng.uniform(-1, 1, (400, 2)), rng.uniform(0.1, 3, (400, 2)), rng.uniform(-4, 4, (400, 1))], 1)
    a, b = a.astype(np.float32), b.astype(np.float32)
    want = cd.iou_rotated_pairs(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    got = np.array([oracle.iou_one_to_many(a[k], b[k:k + 1])[0] for k in range(len(a))])
    assert (want > 0.05).sum() > 100
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)


@pytest.mark.parametrize('name', list(oracle.CASES))
def test_torch_formulation_matches_oracle(name):
    case = oracle.build(name)
    head = case.head()
    head.fused_decode = False
    oracle.assert_padded_close(head.get_bboxes_padded(case.torch_preds()), case.want)


def test_case_builder_reaches_its_branches():
    """The spill, tie, word and circle cases reach what they are named for (the builder asserts it; this records the
    kernel-side numbers)."""
    for name, K in (('spill_K705', 705), ('spill_K1024', 1024)):
        case = oracle.build(name)
        assert oracle.lds_rows(K, K) == {705: 682, 1024: 512}[K]
        assert all(s['n'] == K for s in case.stats.values())
    assert oracle.lds_rows(769, 769) == 630 and oracle.lds_rows(500, 500) == 500 and oracle.lds_rows(704, 704) == 704
    case = oracle.build('ties_saturated')
    assert all((s['key'][s['idx']] == 1.0).all() for s in case.stats.values())


def small_preds(B=1, ncls=(1,), H=4, W=4):
    return tuple([{'heatmap': torch.zeros(B, n, H, W), 'reg': torch.zeros(B, 2, H, W), 'height': torch.zeros(B, 1, H, W),
                   'dim': torch.zeros(B, 3, H, W), 'rot': torch.zeros(B, 2, H, W), 'vel': torch.zeros(B, 2, H, W)}]
                 for n in ncls)


def test_limits_refused_before_launch(g, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError('launched')
    monkeypatch.setattr(cd._lib, 'launch', no_launch)
    c = json.loads(str(g['cfg']))
    coder = cd.CenterPointBBoxCoder(**{k: v for k, v in c['coder'].items() if k != 'type'})
    test = dict(c['test_cfg'])
    coder.max_num = 1025
    with pytest.raises(ValueError, match='max_num'):
        cd.DecodeConfig(coder, test, [1] * 6)
    coder.max_num = 1024
    cd.DecodeConfig(coder, test, [1] * 6)
    with pytest.raises(ValueError, match='at most'):
        cd.DecodeConfig(coder, dict(test, nms_type='rotate', nms_thr=0.2, nms_rescale_factor=[1.0] * 9), [1] * 9)
    with pytest.raises(ValueError, match='at most'):
        cd.DecodeConfig(coder, test, [1, 9, 1, 1, 1, 1])
    coder.max_num = 17
    cfg = cd.DecodeConfig(coder, dict(test, nms_type='rotate', nms_thr=0.2, nms_rescale_factor=[1.0]), [1])
    with pytest.raises(ValueError, match='exceeds the map'):
        cd.decode_torch(small_preds(), cfg)
    with pytest.raises(ValueError, match='exceeds the map'):
        cd.decode_fused(small_preds(), cfg)
    # the head refuses at get_bboxes_padded, on either path
    head = make_head(g)
    head.bbox_coder.max_num = 1025
    for fused in (True, False):
        head.fused_decode = fused
        with pytest.raises(ValueError, match='max_num'):
            head.get_bboxes_padded(preds(g))
    head.bbox_coder.max_num = 24 * 32 + 1
    with pytest.raises(ValueError, match='exceeds the map'):
        head.get_bboxes_padded(preds(g))
