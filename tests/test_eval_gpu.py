"""The detection-metric kernels (csrc/det_eval.hip) against the sequential oracle of tests/eval_oracle.py on every scene.

What is an integer or an ordering (evaluated bits, TP bits, matched indices, per-class counts, the global order, the
cumulative tp / fp) must be equal.  The float64 results are held to bounds derived from the path, u = 2^-53 one rounding:

* a per-match error: the kernel keeps the oracle's operations and their order, and sqrt, the division and fmod are
  correctly rounded (fmod: exact) on both sides: equality;
* AP: precision, recall and the interpolation are the same operations on the same integers in both; the sum over the 90
  recall points is sequential in the kernel and pairwise in numpy, each within 90 u sum|x| of the exact sum, |x| <= 1:
  2 * 90 u, plus 4 u for the two divisions;
* a TP metric over K matches: each cumulative mean is within K u max|err| of exact in the kernel (a fixed-order chunked
  prefix) and in numpy (a sequential one), the interpolation passes at most three such differences on, and the mean over
  at most 90 points adds 2 * 90 u: (6 K + 200) u max(1, max|err|);
* mAP, mTP and NDS: the bound of what they average plus one rounding per addend.
"""
import copy

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib, detection_eval as de
from tests import eval_oracle as eo

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def tensors(batch, dev):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in batch]


def run(scene, dev, per_batch=eo.B):
    cfg = eo.config_of(scene)
    ev = de.DetectionEval(cfg, scene.boxes.shape[0], scene.M, scene.G, dev)
    for batch in scene.batches(per_batch):
        ev.update(*tensors(batch, dev))
    return cfg, ev


def bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def check_against_oracle(cfg, ev, scene, want):
    nc, n = cfg.n_classes, scene.boxes.shape[0] * scene.M
    out = {k: v.cpu().numpy() for k, v in ev.compute().items()}
    info, match = ev.rec_info[:n].cpu().numpy(), ev.rec_match[:n].cpu().numpy()
    err, gt_count = ev.rec_err[:n].cpu().numpy(), ev.gt_count.cpu().numpy()
    evaluated = (info & de.EVALUATED) != 0
    assert np.array_equal(evaluated, want['evaluated'])
    assert np.all(info[~evaluated] == de.NOT_EVALUATED)
    assert np.array_equal(np.stack([(info >> (8 + t)) & 1 for t in range(4)], 1) * evaluated[:, None], want['tp'])
    assert np.array_equal(match, want['match'])
    assert np.array_equal(gt_count, want['gt_count'])
    # the per-match errors: the same operations in the same order, so the same values (NaN where the oracle has NaN)
    for e in range(5):
        assert np.array_equal(err[:, e], want['err'][:, e], equal_nan=True), (scene.name, de.ERR_NAMES[e])
    # the order and the cumulative counts, class by class
    order, sorted_cls, tp_excl = out['order'], out['sorted_cls'], out['tp_excl']
    assert np.array_equal(np.sort(order), np.arange(n)) and np.all(np.diff(sorted_cls) >= 0)
    for c in range(nc):
        lo, hi = np.searchsorted(sorted_cls, c), np.searchsorted(sorted_cls, c + 1)
        assert np.array_equal(order[lo:hi], want['order'][c]), (scene.name, c)
        for t in range(4):
            flag = (info[order[lo:hi]] >> (8 + t)) & 1
            tp = tp_excl[t, lo:hi] - (tp_excl[t, lo] if hi > lo else 0) + flag
            assert np.array_equal(tp, want['tp_cum'][c][t]), (scene.name, c, t)
            assert np.array_equal(np.arange(1, hi - lo + 1) - tp, want['fp_cum'][c][t]), (scene.name, c, t)
    assert np.all(sorted_cls[np.searchsorted(sorted_cls, nc):] == de.REST_CLASS)
    # the curves' results
    ap_bound = (2 * 90 + 4) * U
    d_ap = np.abs(out['AP'] - want['AP'])
    print(scene.name, 'AP max |diff|', d_ap.max(), 'bound', ap_bound)
    assert np.all(d_ap <= ap_bound)
    assert np.array_equal(np.isnan(out['tp_errors']), np.isnan(want['tp_errors']))
    tp_bound = np.zeros((nc, 5))
    for c in range(nc):
        hits = want['order'][c][want['tp'][want['order'][c], cfg.tp_index] != 0]
        for e in range(5):
            vals = want['err'][hits, e]
            vals = vals[~np.isnan(vals)]
            tp_bound[c, e] = (6 * hits.size + 200) * U * max(1.0, np.abs(vals).max() if vals.size else 1.0)
    d_tp = np.abs(out['tp_errors'] - want['tp_errors'])
    print(scene.name, 'TP max |diff|', np.nanmax(d_tp), 'bound (largest)', tp_bound.max())
    assert np.all((d_tp <= tp_bound) | np.isnan(want['tp_errors']))
    assert abs(out['mAP'] - want['mAP']) <= ap_bound + 2 * 4 * nc * U
    mtp_bound = tp_bound.max(0) + 2 * nc * U * np.maximum(1.0, np.nan_to_num(np.abs(want['mTP'])))
    assert np.array_equal(np.isnan(out['mTP']), np.isnan(want['mTP']))
    assert np.all((np.abs(out['mTP'] - want['mTP']) <= mtp_bound) | np.isnan(want['mTP']))
    nds_bound = (5 * (ap_bound + 8 * nc * U) + mtp_bound.sum()) / 10 + 10 * U
    print(scene.name, 'NDS |diff|', abs(out['NDS'] - want['NDS']), 'bound', nds_bound)
    assert abs(out['NDS'] - want['NDS']) <= nds_bound
    return out


@pytest.mark.parametrize('name', [n for n in eo.SCENES if not n.startswith('classes_')])
def test_kernels_equal_the_oracle(cuda, name):
    scene = eo.SCENES[name]
    cfg, ev = run(scene, cuda)
    check_against_oracle(cfg, ev, scene, eo.result_of(name))


@pytest.mark.parametrize('n_classes', [1, 16])
def test_the_smallest_and_the_largest_workgroup(cuda, n_classes):
    scene = eo.SCENES[f'classes_{n_classes}']
    cfg, ev = run(scene, cuda)
    check_against_oracle(cfg, ev, scene, eo.result_of(scene.name))


@pytest.mark.parametrize('name', ['crowd', 'invalid', 'ties'])
def test_batching_does_not_change_a_bit_and_reruns_are_identical(cuda, name):
    """The 15 samples as one update, as five and as fifteen: the same records and the same result tensor, bit for bit;
    a second ``compute`` and a second evaluator give those bits again."""
    scene = eo.SCENES[name]
    outs = []
    for per_batch in (eo.S, eo.B, 1, eo.B):
        cfg, ev = run(scene, cuda, per_batch)
        first = {k: v.clone() for k, v in ev.compute().items()}
        again = ev.compute()
        for k, v in first.items():
            assert torch.equal(bits(v), bits(again[k])), (per_batch, k)
        first.update(key=ev.rec_key.clone(), info=ev.rec_info.clone(), match=ev.rec_match.clone(), err=ev.rec_err.clone(),
                     gt_count=ev.gt_count.clone())
        outs.append(first)
    for other in outs[1:]:
        for k, v in outs[0].items():
            assert torch.equal(bits(v), bits(other[k])), k


def test_one_launch_per_update_and_no_synchronisation(cuda, monkeypatch):
    """From the second ``update`` on a step is exactly one ``_lib.launch`` (``ocrf_det_eval_match``), and ``compute`` is
    one call of ``ocrf_det_eval_summary`` that only launches: both under torch's sync debug mode set to 'error'."""
    scene = eo.SCENES['invalid']
    cfg = eo.config_of(scene)
    batches = [tensors(b, cuda) for b in scene.batches()]
    calls = []
    real = _lib.launch
    monkeypatch.setattr(de._lib, 'launch', lambda name, *a, **k: calls.append(name) or real(name, *a, **k))
    ev = de.DetectionEval(cfg, eo.S, scene.M, scene.G, cuda)
    ev.update(*batches[0])
    ev.compute()                                      # the first call of each entry point loads its kernels
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for batch in batches[1:]:
            del calls[:]
            ev.update(*batch)
            assert calls == ['ocrf_det_eval_match'], calls
        del calls[:]
        out = ev.compute()
        assert calls == ['ocrf_det_eval_summary'], calls
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    want = eo.result_of('invalid')
    assert abs(float(out['NDS']) - want['NDS']) < 1e-12
    host = ev.results_to_host()
    assert host['pts_bbox_NuScenes/NDS'] == float(out['NDS']) and host['pts_bbox_NuScenes/mAP'] == float(out['mAP'])
    ev.reset()
    with pytest.raises(ValueError, match='nothing'):
        ev.compute()


def test_refusals_come_before_a_launch(cuda, monkeypatch):
    monkeypatch.setattr(de._lib, 'launch', lambda *a, **k: pytest.fail('a launch that should have been refused'))
    cfg = de.EvalConfig(eo.CLASSES)
    with pytest.raises(ValueError, match='LDS'):
        de.DetectionEval(cfg, 2, 1300, 24, cuda)      # 52 * 1300 bytes of LDS: above the limit
    ev = de.DetectionEval(cfg, 2, 8, 4, cuda)
    z = lambda *shape, dtype=torch.float32, dev=cuda: torch.zeros(*shape, dtype=dtype, device=dev)     # noqa: E731
    i32 = torch.int32
    good = lambda B=1, dev=cuda: [z(B, 8, 9, dev=dev), z(B, 8, dev=dev), z(B, 8, dtype=i32, dev=dev),      # noqa: E731
                                  z(B, dtype=i32, dev=dev), z(B, 4, 9, dev=dev), z(B, 4, dtype=i32, dev=dev),
                                  z(B, dtype=i32, dev=dev)]
    with pytest.raises(ValueError, match='capacity'):
        ev.update(*good(3))
    with pytest.raises(ValueError, match='cpu'):
        ev.update(*good(1, 'cpu'))
    bad = good()
    bad[4] = z(1, 5, 9)
    with pytest.raises(ValueError, match='gt_boxes'):
        ev.update(*bad)
    L = _lib.lib()
    assert L.ocrf_det_eval_match_lds_bytes(40, 24) == 52 * 40 + 28 * 24 + 128
    assert L.ocrf_det_eval_match_lds_bytes(0, 24) == 0 and L.ocrf_det_eval_summary_workspace_bytes(0) == 0


def test_the_entry_points_refuse_what_they_cannot_run(cuda):
    """``ocrf_det_eval_match`` and ``ocrf_det_eval_summary`` themselves return ``hipErrorInvalidValue`` (1) and launch
    nothing for an LDS size that does not fit, samples beyond the capacity, a threshold that is not finite, too many
    classes, another D, a NULL operand, a workspace that is too small: the buffers keep their sentinel."""
    L = _lib.lib()
    B, M, G, nc, cap = 2, 8, 4, 10, 4
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=cuda)     # noqa: E731
    i32 = torch.int32
    inputs = dict(boxes=z(B, 1300, 9), scores=z(B, 1300), labels=z(B, 1300, dtype=i32), counts=z(B, dtype=i32),
                  gt_boxes=z(B, G, 9), gt_labels=z(B, G, dtype=i32), gt_counts=z(B, dtype=i32))
    tables = de.EvalConfig(eo.CLASSES).tables_on(cuda)
    n = cap * 1300
    records = [torch.full((n,), -7, dtype=i32, device=cuda), torch.full((n,), -7, dtype=i32, device=cuda),
               torch.full((n, 4), -7, dtype=i32, device=cuda), torch.full((n, 5), -7.0, dtype=torch.float64, device=cuda),
               torch.full((cap, 16), -7, dtype=i32, device=cuda)]
    stream = _lib.stream_ptr(cuda)

    def match(B=B, M=M, D=9, G=G, nc=nc, index=0, cap=cap, th=(0.5, 1.0, 2.0, 4.0), tp=2, null=None):
        ptrs = [t.data_ptr() for t in inputs.values()] + [None, None] + [t.data_ptr() for t in tables]
        ptrs += [t.data_ptr() for t in records]
        if null is not None:
            ptrs[null] = None
        return L.ocrf_det_eval_match(B, M, D, G, nc, index, cap, *th, tp, *ptrs, stream)
    assert match(M=1300) == 1                         # 52 * 1300 bytes of LDS
    assert match(index=3) == 1 and match(index=-1) == 1 and match(B=0) == 1
    assert match(th=(0.5, float('nan'), 2.0, 4.0)) == 1 and match(th=(0.5, 1.0, 2.0, float('inf'))) == 1
    assert match(nc=17) == 1 and match(nc=0) == 1 and match(D=8) == 1 and match(tp=4) == 1
    assert match(null=0) == 1 and match(null=9) == 1 and match(null=15) == 1
    order, cls, excl = (torch.full((k * n,), -7, dtype=i32, device=cuda) for k in (1, 1, 4))
    result = torch.full((9 * nc + 7,), -7.0, dtype=torch.float64, device=cuda)
    ws = torch.empty(L.ocrf_det_eval_summary_workspace_bytes(cap * M), dtype=torch.uint8, device=cuda)

    def summary(samples=cap, M=M, nc=nc, tp=2, first=11, min_precision=0.1, ws_bytes=ws.numel(), result_ptr=result.data_ptr()):
        return L.ocrf_det_eval_summary(samples, M, nc, tp, first, min_precision, records[0].data_ptr(),
                                       records[1].data_ptr(), records[3].data_ptr(), records[4].data_ptr(),
                                       tables[1].data_ptr(), order.data_ptr(), cls.data_ptr(), excl.data_ptr(), result_ptr,
                                       ws.data_ptr(), ws_bytes, stream)
    assert summary(samples=0) == 1 and summary(nc=17) == 1 and summary(first=0) == 1 and summary(first=101) == 1
    assert summary(min_precision=1.0) == 1 and summary(ws_bytes=ws.numel() - 256) == 1 and summary(result_ptr=None) == 1
    assert summary(samples=2 ** 31 // M) == 1
    torch.cuda.synchronize()
    for t in records + [order, cls, excl]:
        assert bool((t == -7).all())
    assert bool((result == -7.0).all())
    assert match() == 0                               # and the same call with what fits runs
    torch.cuda.synchronize()
    assert not bool((records[1][:B * M] == -7).any()) and bool((records[1][B * M:] == -7).all())


def test_an_evaluator_on_a_device_without_an_index(cuda):
    """``DetectionEval(..., device='cuda')`` takes tensors of the current device, whose device carries its index."""
    scene = eo.SCENES['half']
    cfg = eo.config_of(scene)
    ev = de.DetectionEval(cfg, eo.S, scene.M, scene.G, 'cuda')
    assert ev.fused and ev.device == torch.device('cuda', torch.cuda.current_device())
    for batch in scene.batches():
        ev.update(*tensors(batch, cuda))
    assert abs(float(ev.compute()['AP'][eo.CAR, 2]) - eo.HALF_AP) < 1e-9


def test_evaluate_stream_on_the_detector(cuda):
    """``OcRFDet4D.evaluate_stream`` on ``tests.test_detector_host.MODEL``, B = 2, 3 frames, synthetic ground truth: no
    synchronisation from the second frame on, and the accumulated records and the result equal ``update`` on
    ``get_bboxes_padded`` of the head outputs of the same steps, bit for bit."""
    from ocrfdet_amd import detector as det_mod
    from tests import test_detector_host as model
    from tests.test_track_gpu import stream_frames
    B, FRAMES, G = 2, 3, 6
    torch.manual_seed(0)
    det = det_mod.OcRFDet4D(**copy.deepcopy(model.MODEL)).to(cuda).eval()
    frames = stream_frames(cuda, B, FRAMES)
    names = [n for task in det.pts_bbox_head.class_names for n in task]
    cfg = de.EvalConfig(names)
    gen = torch.Generator().manual_seed(5)
    gts = []
    for t in range(FRAMES):
        gt_boxes = torch.zeros(B, G, 9)
        gt_boxes[..., :2] = torch.rand(B, G, 2, generator=gen) * 40 - 20
        gt_boxes[..., 3:6] = torch.rand(B, G, 3, generator=gen) + 0.5
        gt_boxes[..., 6:] = torch.rand(B, G, 3, generator=gen) - 0.5
        gts.append(dict(gt_boxes=gt_boxes.to(cuda), gt_labels=torch.randint(0, len(names), (B, G), generator=gen,
                                                                            dtype=torch.int32).to(cuda),
                        gt_counts=torch.tensor([G, G - 2], dtype=torch.int32, device=cuda),
                        gt_attrs=torch.randint(-1, 8, (B, G), generator=gen, dtype=torch.int32).to(cuda)))
    head_outs = []
    hook = det.pts_bbox_head.register_forward_hook(lambda m, args, out: head_outs.append(out))
    try:
        with torch.no_grad():                         # a dry frame: the padded shape, and the library warms up
            (feats, _, _), _ = det.stream_step(frames[0])
            M = det.pts_bbox_head.get_bboxes_padded(det.pts_bbox_head(feats))[0].shape[1]
        del head_outs[:]
        ev = de.DetectionEval(cfg, B * FRAMES, M, G, cuda)

        def guarded():
            for t in range(FRAMES):
                if t == 1:                            # the first step allocates the stream state
                    torch.cuda.synchronize()
                    torch.cuda.set_sync_debug_mode('error')
                yield frames[t], gts[t]
        try:
            got, state = det.evaluate_stream(guarded(), ev)
            assert got is ev and state.steps == FRAMES             # the dry frame's state was not handed on
        finally:
            torch.cuda.set_sync_debug_mode('default')
    finally:
        hook.remove()
    torch.cuda.synchronize()
    assert len(head_outs) == FRAMES and ev.n_samples == B * FRAMES
    twin = de.DetectionEval(cfg, B * FRAMES, M, G, cuda)
    for outs, gt in zip(head_outs, gts):
        with torch.no_grad():
            twin.update(*det.pts_bbox_head.get_bboxes_padded(outs), gt['gt_boxes'], gt['gt_labels'], gt['gt_counts'],
                        gt_attrs=gt['gt_attrs'])
    for name in ('rec_key', 'rec_info', 'rec_match', 'rec_err', 'gt_count'):
        assert torch.equal(bits(getattr(ev, name)), bits(getattr(twin, name))), name
    assert torch.equal(bits(ev.compute()['result']), bits(twin.compute()['result']))
    host = ev.results_to_host()
    assert set(host) >= {f'pts_bbox_NuScenes/{names[0]}_AP_dist_0.5', 'pts_bbox_NuScenes/mATE', 'pts_bbox_NuScenes/NDS'}
