"""Generates ``tests/golden/center_head_decode.npz``: the reference's own ``CenterHead.get_bboxes`` /
``get_task_detections`` (mmdet3d/models/dense_heads/centerpoint_head.py), ``CenterPointBBoxCoder``
(core/bbox/coders/centerpoint_bbox_coders.py), ``circle_nms``, ``nms_bev`` (core/post_processing/box3d_nms.py) and
``xywhr2xyxyr``, run on the CPU.

    python tests/golden/make_golden_center_head_decode.py

Imports the reference as ``make_golden_center_head.py`` does, plus these stubs (neither mmcv, mmdet nor numba is part
of the reference tree): ``numba.jit`` as the identity, mmdet's ``BaseBBoxCoder`` and ``BBOX_CODERS`` as shells, and
mmcv's ``nms_rotated`` restated below in float64 numpy: boxes sorted by score (stable), greedy, a box suppressed by a
kept one when IoU > threshold, the IoU as mmcv's ``single_box_iou_rotated`` (0 when an area is below 1e-14, centres
shifted to their mean, intersection over area1 + area2 - inter) with the intersection by clipping one box's polygon
against the other's edges.  Rotation convention of this golden data: corners c + R(a) (+-w/2, +-h/2), R
counter-clockwise in x-right / y-up coordinates (unverified against mmcv).

Case: the reference config's six tasks, nms_type, nms_thr, nms_rescale_factor and min_radius on a 32 x 24 map (cell
0.5 m), B = 3, max_num 16, pre_max_size 10, post_max_size 6, coder score_threshold 0.1 and test score_threshold 0.2,
coder and test centre ranges that differ.  Background logits N(-6, 0.5), so every top 16 carries filtered cells.

* sample 0, crafted: identical boxes, a box inside another, a 90-degree-rotated square, boxes sharing an edge,
  boxes touching at a corner, disjoint boxes, a zero-area box (exp underflow), centres outside the coder's range and
  inside it but outside the test range (x, y and z), yaws in all four atan2 quadrants, multi-class tasks with
  per-class factors, circle pairs at 0.99 and 1.01 of the radius, more candidates than pre_max_size and kept boxes
  than post_max_size;
* sample 1: nothing above the coder's threshold;
* sample 2: random peaks in every task.

The generator asserts that no two top-K scores tie and that every IoU of a pair the NMS decides on lies at least 1e-4
from its threshold (and every circle pair's squared distance from its radius).  Stored: the head outputs, the configs,
the padded expected results, the crafted pairs' float64 IoUs, and the reference's nms_bev / circle_nms on a few inputs.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402
import make_golden_center_head as mgc  # noqa: E402

REF = _ref_import.REF
B, H, W = 3, 24, 32
TASKS = mgc.TASKS
NCLS = [t['num_class'] for t in TASKS]
COMMON = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2))
CODER = dict(type='CenterPointBBoxCoder', pc_range=[-8.0, -6.0], post_center_range=[-7.5, -5.5, -3.0, 7.5, 5.5, 3.0],
             max_num=16, score_threshold=0.1, out_size_factor=4, voxel_size=[0.125, 0.125], code_size=9)
TEST = dict(pc_range=[-8.0, -6.0], post_center_limit_range=[-7.0, -5.8, -2.5, 7.8, 5.0, 2.5], max_per_img=16,
            max_pool_nms=False, min_radius=[4, 12, 10, 1, 0.85, 0.175], score_threshold=0.2, out_size_factor=4,
            voxel_size=[0.125, 0.125], pre_max_size=10, post_max_size=6,
            nms_type=['rotate', 'rotate', 'rotate', 'circle', 'rotate', 'rotate'], nms_thr=[0.3, 0.1, 0.1, 0.1, 0.1, 0.5],
            nms_rescale_factor=[1.0, [0.7, 0.7], [0.4, 0.55], 1.1, [1.0, 1.0], [4.5, 9.0]])
MARGIN = 1e-4
NMS_LOG = []


# --------------------------------------------------------------------------------------------- mmcv restatement
def corners(x, y, w, h, a):
    c, s = np.cos(a), np.sin(a)
    local = [(-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2)]
    return [(x + c * u - s * v, y + s * u + c * v) for u, v in local]


def clip(poly, p, q):
    """The part of convex ``poly`` left of the directed line p -> q."""
    def side(r):
        return (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0])
    out = []
    for k in range(len(poly)):
        cur, prev = poly[k], poly[k - 1]
        sc, sp = side(cur), side(prev)
        if (sc >= 0) != (sp >= 0):
            t = sp / (sp - sc)
            out.append((prev[0] + t * (cur[0] - prev[0]), prev[1] + t * (cur[1] - prev[1])))
        if sc >= 0:
            out.append(cur)
    return out


def iou64(a, b):
    a = [float(v) for v in a]
    b = [float(v) for v in b]
    area_a, area_b = a[2] * a[3], b[2] * b[3]
    if area_a < 1e-14 or area_b < 1e-14:
        return 0.0
    sx, sy = (a[0] + b[0]) / 2, (a[1] + b[1]) / 2
    pa = corners(a[0] - sx, a[1] - sy, a[2], a[3], a[4])
    pb = corners(b[0] - sx, b[1] - sy, b[2], b[3], b[4])
    poly = pa
    for k in range(4):
        if not poly:
            break
        poly = clip(poly, pb[k], pb[(k + 1) % 4])
    inter = 0.0
    if len(poly) >= 3:
        inter = abs(sum(poly[k][0] * poly[(k + 1) % len(poly)][1] - poly[(k + 1) % len(poly)][0] * poly[k][1]
                        for k in range(len(poly))) / 2)
    return inter / (area_a + area_b - inter)


def nms_rotated(dets, scores, iou_threshold, labels=None):
    order = np.argsort(-scores.numpy(), kind='stable')
    d = dets.numpy().astype(np.float64)
    n = len(order)
    sup = np.zeros(n, bool)
    keep = []
    for ii in range(n):
        i = order[ii]
        if sup[i]:
            continue
        keep.append(i)
        for jj in range(ii + 1, n):
            j = order[jj]
            if sup[j]:
                continue
            v = iou64(d[i], d[j])
            assert abs(v - iou_threshold) >= MARGIN, f'IoU {v} within {MARGIN} of {iou_threshold}'
            NMS_LOG.append((d[i].copy(), d[j].copy(), v))
            if v > iou_threshold:
                sup[j] = True
    keep = torch.tensor(keep, dtype=torch.long)
    return torch.cat([dets[keep], scores[keep].reshape(-1, 1)], 1), keep


# --------------------------------------------------------------------------------------------- reference import
def import_reference():
    cph, Boxes = mgc.import_reference()
    _ref_import._mod('numba', jit=lambda *a, **k: (lambda f: f))
    ops = sys.modules['mmcv.ops']
    ops.nms_rotated = nms_rotated
    ops.nms = None

    class BaseBBoxCoder:
        def __init__(self, **kwargs):
            pass
    _ref_import._mod('mmdet.core.bbox', BaseBBoxCoder=BaseBBoxCoder)
    _ref_import._mod('mmdet.core.bbox.builder', BBOX_CODERS=_ref_import._Registry())
    nms = mgc._load('mmdet3d.core.post_processing.box3d_nms', REF + '/mmdet3d/core/post_processing/box3d_nms.py')
    coders = mgc._load('mmdet3d.core.bbox.coders.centerpoint_bbox_coders',
                       REF + '/mmdet3d/core/bbox/coders/centerpoint_bbox_coders.py')
    utils = mgc._load('mmdet3d.core.bbox.structures.utils', REF + '/mmdet3d/core/bbox/structures/utils.py')
    cph.circle_nms, cph.nms_bev, cph.xywhr2xyxyr = nms.circle_nms, nms.nms_bev, utils.xywhr2xyxyr
    cph.build_bbox_coder = lambda cfg: coders.CenterPointBBoxCoder(**{k: v for k, v in cfg.items() if k != 'type'})
    return cph, Boxes, nms, coders, utils


# --------------------------------------------------------------------------------------------- inputs
def make_preds(rng):
    P = {}
    for t, n in enumerate(NCLS):
        P[t] = dict(heatmap=rng.normal(-6.0, 0.5, (B, n, H, W)), reg=rng.uniform(0, 1, (B, 2, H, W)),
                    height=rng.uniform(-1, 1, (B, 1, H, W)), dim=rng.normal(0.3, 0.3, (B, 3, H, W)),
                    rot=rng.normal(0, 1, (B, 2, H, W)), vel=rng.normal(0, 1, (B, 2, H, W)))
    P[1]['heatmap'][1] = rng.normal(-5.0, 0.3, P[1]['heatmap'][1].shape)
    for t in range(len(NCLS)):                 # sample 1: nothing above the coder's threshold
        P[t]['heatmap'][1] = np.minimum(P[t]['heatmap'][1], -2.3)

    def peak(s, t, c, x, y, logit, cx, cy, dims, yaw, z=0.0):
        """A peak at cell (x, y) whose box centre is at (cx, cy) in cells, dims (w, l, h) in metres."""
        d = P[t]
        d['heatmap'][s, c, y, x] = logit
        d['reg'][s, :, y, x] = (cx - x, cy - y)
        d['height'][s, 0, y, x] = z
        d['dim'][s, :, y, x] = [np.log(v) if v > 0 else -200.0 for v in dims]
        r = rng.uniform(0.5, 2.0)
        d['rot'][s, :, y, x] = (r * np.sin(yaw), r * np.cos(yaw))

    s = 0
    # task 0 (thr 0.3, factor 1.0)
    peak(s, 0, 0, 10, 10, 3.0, 10.5, 10.5, (2.0, 2.0, 1.5), 0.0)           # A
    peak(s, 0, 0, 11, 10, 2.9, 10.5, 10.5, (2.0, 2.0, 1.5), 0.0)           # identical to A
    peak(s, 0, 0, 20, 5, 2.8, 20.5, 5.5, (4.0, 4.0, 1.0), 0.3)             # B
    peak(s, 0, 0, 21, 5, 2.7, 20.6, 5.4, (2.9, 2.9, 1.0), 0.3)             # inside B, IoU 0.53
    peak(s, 0, 0, 5, 18, 2.6, 5.5, 18.5, (1.6, 1.6, 1.0), 0.0)             # square
    peak(s, 0, 0, 6, 18, 2.5, 5.5, 18.5, (1.6, 1.6, 1.0), np.pi / 2)       # the square turned 90 degrees
    peak(s, 0, 0, 0, 12, 2.45, -1.5, 12.5, (2.0, 2.0, 1.0), 1.0)           # outside the coder's range (x)
    peak(s, 0, 0, 26, 18, 2.4, 26.5, 18.5, (1.0, 1.0, 1.0), 0.0)           # D
    peak(s, 0, 0, 28, 18, 2.3, 28.5, 18.5, (1.0, 1.0, 1.0), 0.0)           # shares an edge with D
    peak(s, 0, 0, 26, 12, 2.2, 26.5, 12.5, (1.0, 1.0, 1.0), 0.0)           # E
    peak(s, 0, 0, 28, 14, 2.1, 28.5, 14.5, (1.0, 1.0, 1.0), 0.0)           # touches E at a corner
    peak(s, 0, 0, 15, 20, 2.0, 15.5, 20.5, (0.0, 2.0, 1.0), -2.0)          # zero area (exp underflow)
    peak(s, 0, 0, 14, 22, 1.9, 14.5, 22.4, (1.0, 2.0, 1.0), -1.0)          # y in the coder's range, not the test's
    peak(s, 0, 0, 2, 2, 1.8, 2.5, 2.5, (1.0, 2.0, 1.0), 2.5, z=2.8)        # z likewise (after the pre cut)
    # task 1 (thr 0.1, factors 0.7 / 0.7): two classes overlapping
    peak(s, 1, 0, 8, 8, 2.0, 8.5, 8.5, (2.5, 7.0, 3.0), 0.4)
    peak(s, 1, 1, 9, 9, 1.9, 9.2, 9.0, (2.5, 6.0, 3.0), -2.7)              # overlaps the first after the factor
    peak(s, 1, 1, 20, 15, 1.5, 20.5, 15.5, (2.5, 6.0, 3.0), 1.9)
    peak(s, 1, 0, 31, 15, 1.4, 31.6, 15.5, (2.5, 6.0, 3.0), -0.9)          # x in the coder's range, not the test's
    # task 2 (thr 0.1, factors 0.4 / 0.55)
    peak(s, 2, 0, 16, 12, 2.5, 16.5, 12.5, (3.0, 11.0, 3.5), 0.2)
    peak(s, 2, 1, 17, 12, 2.4, 16.8, 12.5, (3.0, 12.0, 3.5), 2.0)
    peak(s, 2, 1, 4, 4, 2.3, 4.5, 4.5, (3.0, 12.0, 3.5), -1.2)
    # task 3 (circle, min_radius 1 m^2): pairs at 0.99 and 1.01 of it
    peak(s, 3, 0, 8, 16, 2.0, 8.5, 16.5, (2.5, 0.5, 1.0), 0.0)
    peak(s, 3, 0, 10, 16, 1.9, 8.5 + np.sqrt(0.99) / 0.5, 16.5, (2.5, 0.5, 1.0), 0.0)
    peak(s, 3, 0, 20, 20, 1.8, 20.5, 20.5, (2.5, 0.5, 1.0), 0.0)
    peak(s, 3, 0, 20, 18, 1.7, 20.5, 20.5 - np.sqrt(1.01) / 0.5, (2.5, 0.5, 1.0), 0.0)
    # task 4 (thr 0.1, factors 1 / 1): yaws in all four quadrants, both signs
    for k, yaw in enumerate((0.4, 2.2, -2.6, -0.8, 1.3, -1.9)):
        peak(s, 4, k % 2, 3 + 5 * k, 3 + 3 * k, 2.0 - 0.1 * k, 3.5 + 5 * k, 3.5 + 3 * k, (0.8, 2.1, 1.5), yaw)
    # task 5 (thr 0.5, factors 4.5 / 9.0): small boxes that overlap once rescaled
    peak(s, 5, 0, 12, 4, 2.0, 12.5, 4.5, (0.7, 0.7, 1.8), 0.0)
    peak(s, 5, 0, 12, 5, 1.9, 12.5, 5.3, (0.7, 0.7, 1.8), 0.1)             # suppressed (scaled IoU 0.6)
    peak(s, 5, 1, 24, 8, 1.8, 24.5, 8.5, (0.4, 0.4, 1.1), 0.0)
    peak(s, 5, 1, 25, 8, 1.7, 25.3, 8.5, (0.4, 0.4, 1.1), 0.0)             # kept (scaled IoU 0.38)
    # sample 2: random peaks
    s = 2
    for t, n in enumerate(NCLS):
        for k in range(rng.integers(4, 9)):
            x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
            peak(s, t, int(rng.integers(0, n)), x, y, rng.uniform(-1.5, 3.0), x + rng.uniform(-0.2, 1.2),
                 y + rng.uniform(-0.2, 1.2), tuple(rng.uniform(0.4, 4.0, 3)), rng.uniform(-3.1, 3.1),
                 z=rng.uniform(-2, 2))
    out = {}
    for t in range(len(NCLS)):
        for k, v in P[t].items():
            out[f't{t}.{k}'] = v.astype(np.float32)
    return out


def preds_of(arrs):
    return tuple([{k: torch.from_numpy(arrs[f't{t}.{k}'].copy()) for k in ('reg', 'height', 'dim', 'rot', 'vel',
                                                                             'heatmap')}] for t in range(len(NCLS)))


def main():
    cph, Boxes, nms, coders, utils = import_reference()
    for seed in range(20261015, 20261015 + 50):
        rng = np.random.default_rng(seed)
        arrs = make_preds(rng)
        # no ties among any task's top K
        ok = True
        for t in range(len(NCLS)):
            h = torch.from_numpy(arrs[f't{t}.heatmap']).sigmoid().reshape(B, -1)
            top = torch.topk(h, CODER['max_num'] + 1, dim=1)[0]
            ok &= bool((top[:, 1:] != top[:, :-1]).all())
        if not ok:
            continue
        NMS_LOG.clear()
        head = cph.CenterHead(in_channels=8, tasks=TASKS, common_heads=COMMON, share_conv_channel=8,
                              separate_head=dict(type='SeparateHead', init_bias=-2.19, final_kernel=3, head_conv=8),
                              bbox_coder=CODER, train_cfg=mgc.CFG, test_cfg=TEST, norm_bbox=True)
        metas = [dict(box_type_3d=Boxes) for _ in range(B)]
        try:
            res = head.get_bboxes(preds_of(arrs), metas)
            # circle pairs: no squared distance within the margin of its radius
            for t, typ in enumerate(TEST['nms_type']):
                if typ != 'circle':
                    continue
                dec = head.bbox_coder.decode(torch.from_numpy(arrs[f't{t}.heatmap']).sigmoid(),
                                             torch.from_numpy(arrs[f't{t}.rot'][:, 0:1]),
                                             torch.from_numpy(arrs[f't{t}.rot'][:, 1:2]),
                                             torch.from_numpy(arrs[f't{t}.height']),
                                             torch.from_numpy(np.exp(arrs[f't{t}.dim'])),
                                             torch.from_numpy(arrs[f't{t}.vel']), reg=torch.from_numpy(arrs[f't{t}.reg']))
                for d in dec:
                    c = d['bboxes'][:, :2].numpy()
                    d2 = ((c[:, None, 0] - c[None, :, 0]) ** 2 + (c[:, None, 1] - c[None, :, 1]) ** 2)
                    iu = np.triu_indices(len(c), 1)
                    assert (np.abs(d2[iu].astype(np.float64) - TEST['min_radius'][t]) >= MARGIN).all()
        except AssertionError as e:
            print('seed', seed, 'rejected:', e)
            continue
        break
    else:
        raise SystemExit('no seed satisfied the margins')
    print('seed', seed)
    M = len(NCLS) * TEST['post_max_size']
    gb = np.zeros((B, M, 9), np.float32)
    gs = np.zeros((B, M), np.float32)
    gl = np.zeros((B, M), np.int32)
    gc = np.zeros(B, np.int32)
    for i, (bx, sc, lab) in enumerate(res):
        assert isinstance(bx, Boxes) and lab.dtype == torch.int32
        n = bx.tensor.shape[0]
        gb[i, :n], gs[i, :n], gl[i, :n], gc[i] = bx.tensor.numpy(), sc.numpy(), lab.numpy(), n
    arrs.update(boxes=gb, scores=gs, labels=gl, counts=gc)
    arrs['iou_a'] = np.array([a for a, _, _ in NMS_LOG], np.float32).reshape(-1, 5)
    arrs['iou_b'] = np.array([b for _, b, _ in NMS_LOG], np.float32).reshape(-1, 5)
    arrs['iou'] = np.array([v for _, _, v in NMS_LOG], np.float64)
    # the drop-ins on their own: nms_bev on sample 0's task 0 boxes, circle_nms on random centres
    rng = np.random.default_rng(7)
    xywhr = torch.from_numpy(np.concatenate([rng.uniform(-4, 4, (40, 2)), rng.uniform(0.5, 3, (40, 2)),
                                             rng.uniform(-3, 3, (40, 1))], 1).astype(np.float32))
    sc = torch.from_numpy(rng.permutation(40).astype(np.float32) / 40 + 0.01)
    NMS_LOG.clear()
    for thr in (0.05, 0.3):
        keep = nms.nms_bev(utils.xywhr2xyxyr(xywhr), sc, thr, pre_max_size=30, post_max_size=12)
        arrs[f'nms_bev.keep{thr}'] = keep.numpy()
    arrs['nms_bev.boxes'], arrs['nms_bev.scores'] = xywhr.numpy(), sc.numpy()
    dets = np.concatenate([rng.uniform(-3, 3, (50, 2)), rng.permutation(50)[:, None] / 50 + 0.01], 1).astype(np.float32)
    for r in (0.3, 1.5):
        d2 = (dets[:, None, 0] - dets[None, :, 0]) ** 2 + (dets[:, None, 1] - dets[None, :, 1]) ** 2
        assert (np.abs(d2[np.triu_indices(50, 1)] - r) >= MARGIN).all()
        arrs[f'circle.keep{r}'] = np.array(nms.circle_nms(dets, r, post_max_size=20), np.int64)
    arrs['circle.dets'] = dets
    arrs['cfg'] = np.array(json.dumps(dict(coder=CODER, test_cfg=TEST, tasks=TASKS, common=COMMON, seed=seed)))
    ref_cfg = mgc.reference_config()
    arrs['ref_config'] = np.array(json.dumps(ref_cfg))
    path = os.path.join(HERE, 'center_head_decode.npz')
    np.savez_compressed(path, **arrs)
    print('wrote', path, os.path.getsize(path), 'bytes; counts', gc.tolist(), '; pairs', len(arrs['iou']))
    for i in range(B):
        print(i, gl[i, :gc[i]].tolist())


if __name__ == '__main__':
    main()
