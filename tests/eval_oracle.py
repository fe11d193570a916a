"""A sequential float64 restatement of the detection-metric rules of include/ocrf_hip.h (section "nuScenes detection
metrics"), in the benchmark's own loop order: one class at a time over the WHOLE accumulated set, the predictions sorted
by confidence, each taking the nearest unclaimed ground truth of its own sample, then ``np.cumsum`` and ``np.interp``.
It does not use the per-(sample, class) decomposition of the kernel and of ``evaluate_host``: that they agree with this
is the test of that decomposition.  Written from the benchmark's published procedure; nothing here has been compared
with the nuScenes devkit.

``SCENES`` holds the test scenes (B = 3, M = 40, G = 24, 10 classes, 5 batches unless a scene says otherwise); each
asserts the property it exists for on this oracle's own results (``check``), so a scene cannot silently stop exercising
its edge.
"""
import math

import numpy as np

CLASSES = ('car', 'truck', 'trailer', 'bus', 'construction_vehicle', 'bicycle', 'motorcycle', 'pedestrian',
           'traffic_cone', 'barrier')
CAR, TRUCK, TRAILER, BUS, CV, BICYCLE, MOTORCYCLE, PEDESTRIAN, CONE, BARRIER = range(10)
B, M, G, BATCHES = 3, 40, 24, 5
S = B * BATCHES


class Rules:
    """The oracle's own statement of the settings, literal and independent of ``detection_eval.EvalConfig``: per class the
    range in metres (detection_cvpr_2019), the attribute a moving and a still prediction gets (``AttrMapping`` numbers of
    ``_format_bbox``'s rule, -1 for none) and the flags (1: yaw period pi, 2: no orientation error, 4: no velocity error,
    8: no attribute error); the thresholds, the one that carries the errors, and the part of the curves that counts."""
    TEN = (('car', 50.0, 5, 6, 0), ('truck', 50.0, 5, 6, 0), ('trailer', 50.0, 5, 6, 0), ('bus', 50.0, 5, 7, 0),
           ('construction_vehicle', 50.0, 5, 6, 0), ('bicycle', 40.0, 0, 1, 0), ('motorcycle', 40.0, 0, 1, 0),
           ('pedestrian', 40.0, 2, 3, 0), ('traffic_cone', 30.0, -1, -1, 2 | 4 | 8), ('barrier', 30.0, -1, -1, 1 | 4 | 8))

    def __init__(self, n_classes=10):
        rows = self.TEN if n_classes == 10 else tuple((f'class_{k}', 50.0, -1, -1, 0) for k in range(n_classes))
        self.class_names = tuple(r[0] for r in rows)
        self.class_range = tuple(r[1] for r in rows)
        self.class_tab = tuple(r[2:] for r in rows)
        self.dist_ths, self.tp_index = (0.5, 1.0, 2.0, 4.0), 2
        self.min_recall, self.min_precision = 0.1, 0.1


# ------------------------------------------------------------------------------------------------ the oracle
def _finite(*v):
    return all(math.isfinite(float(x)) for x in v)


def _evaluated(cfg, box, label):
    if not 0 <= int(label) < len(cfg.class_names) or not _finite(box[0], box[1], box[2]):
        return False
    x, y, r = float(box[0]), float(box[1]), float(np.float32(cfg.class_range[int(label)]))
    return x * x + y * y < r * r


def _errors(cfg, D, cls, p, q, ga):
    p, q = [float(v) for v in p], [float(v) for v in q]
    dx, dy = p[0] - q[0], p[1] - q[1]
    trans = math.sqrt(dx * dx + dy * dy)
    inter = (min(p[3], q[3]) * min(p[4], q[4])) * min(p[5], q[5])
    scale = 1.0 - inter / (((p[3] * p[4]) * p[5] + (q[3] * q[4]) * q[5]) - inter)
    period = math.pi if cfg.class_tab[cls][2] & 1 else 2.0 * math.pi
    diff = ((q[6] - p[6]) + period / 2.0) % period - period / 2.0
    if diff > math.pi:
        diff = diff - 2.0 * math.pi
    orient = abs(diff)
    vel, moving = float('nan'), False
    if D == 9:
        dvx, dvy = p[7] - q[7], p[8] - q[8]
        vel = math.sqrt(dvx * dvx + dvy * dvy) if not (math.isnan(dvx) or math.isnan(dvy)) else float('nan')
        moving = p[7] * p[7] + p[8] * p[8] > 0.2 * 0.2
    attr = float('nan')
    if ga != -1:
        attr = 0.0 if cfg.class_tab[cls][0 if moving else 1] == ga else 1.0
    return [trans, scale, orient, vel, attr]


def evaluate(cfg, scene):
    """The oracle's results for ``scene`` (``Scene``) under ``cfg`` (``Rules``): per slot ``evaluated`` (bool), ``tp`` (n, 4) bits, ``match`` (n,
    4), ``err`` (n, 5); ``gt_count`` (S, C); per class ``order[c]`` (slots in the global order), ``tp_cum[c]`` /
    ``fp_cum[c]`` (4, n_c); ``AP`` (C, 4), ``tp_errors`` (C, 5), ``mAP``, ``mTP`` (5), ``NDS``."""
    nc, D, Ms, Gs = len(cfg.class_names), scene.D, scene.M, scene.G
    n_s = scene.boxes.shape[0]
    preds, gts = [], []                                # (sample, row, class, score) / (sample, index, class)
    evaluated = np.zeros(n_s * Ms, bool)
    gt_count = np.zeros((n_s, nc), np.int64)
    for s in range(n_s):
        for r in range(min(max(int(scene.counts[s]), 0), Ms)):
            if _finite(scene.scores[s, r]) and _evaluated(cfg, scene.boxes[s, r], scene.labels[s, r]):
                preds.append((s, r, int(scene.labels[s, r]), float(scene.scores[s, r])))
                evaluated[s * Ms + r] = True
        for g in range(min(max(int(scene.gt_counts[s]), 0), Gs)):
            if scene.gt_valid is not None and scene.gt_valid[s, g] == 0:
                continue
            if _evaluated(cfg, scene.gt_boxes[s, g], scene.gt_labels[s, g]):
                gts.append((s, g, int(scene.gt_labels[s, g])))
                gt_count[s, int(scene.gt_labels[s, g])] += 1
    tp = np.zeros((n_s * Ms, 4), np.int64)
    match = np.full((n_s * Ms, 4), -1, np.int64)
    err = np.full((n_s * Ms, 5), np.nan)
    order, tp_cum, fp_cum = {}, {}, {}
    AP, TPE = np.zeros((nc, 4)), np.ones((nc, 5))
    rec_interp = np.linspace(0, 1, 101)
    first = int(round(100 * cfg.min_recall)) + 1
    for c in range(nc):
        for e, bit in ((2, 2), (3, 4), (4, 8)):
            if cfg.class_tab[c][2] & bit:
                TPE[c, e] = np.nan
        mine = sorted((p for p in preds if p[2] == c), key=lambda p: (-p[3], p[0], p[1]))
        order[c] = np.array([s * Ms + r for s, r, _, _ in mine], np.int64)
        npos = sum(1 for g in gts if g[2] == c)
        flags = np.zeros((4, len(mine)), np.int64)
        for t, th in enumerate(cfg.dist_ths):
            taken = set()
            for i, (s, r, _, _) in enumerate(mine):
                min_d2, best = float('inf'), None
                px, py = float(scene.boxes[s, r, 0]), float(scene.boxes[s, r, 1])
                for gs, g, gc in gts:
                    if gs != s or gc != c or (gs, g) in taken:
                        continue
                    dx, dy = px - float(scene.gt_boxes[s, g, 0]), py - float(scene.gt_boxes[s, g, 1])
                    d2 = dx * dx + dy * dy
                    if d2 < min_d2:
                        min_d2, best = d2, g
                if best is not None and min_d2 < th * th:
                    taken.add((s, best))
                    flags[t, i] = 1
                    tp[s * Ms + r, t], match[s * Ms + r, t] = 1, best
                    if t == cfg.tp_index:
                        ga = -1 if scene.gt_attrs is None else int(scene.gt_attrs[s, best])
                        err[s * Ms + r] = _errors(cfg, D, c, scene.boxes[s, r], scene.gt_boxes[s, best], ga)
        tp_cum[c], fp_cum[c] = np.cumsum(flags, axis=1), np.cumsum(1 - flags, axis=1)
        if npos == 0 or not mine:
            continue
        conf = np.array([np.float64(np.float32(p[3])) for p in mine])
        conf_i = None
        for t in range(4):
            tpc, fpc = tp_cum[c][t].astype(float), fp_cum[c][t].astype(float)
            prec, rec = tpc / (tpc + fpc), tpc / float(npos)
            prec_i = np.interp(rec_interp, rec, prec, right=0)
            if t == cfg.tp_index:
                conf_i = np.interp(rec_interp, rec, conf, right=0)
            AP[c, t] = float(np.mean(np.maximum(prec_i[first:] - cfg.min_precision, 0.0))) / (1.0 - cfg.min_precision)
        hit = flags[cfg.tp_index] != 0
        nz = np.flatnonzero(conf_i)
        last = int(nz[-1]) if nz.size else 0
        if not hit.any() or last < first:
            continue
        for e in range(5):
            if np.isnan(TPE[c, e]):
                continue
            x = err[order[c], e][hit]
            if np.isnan(x).all():
                cm = np.ones(x.size)
            else:
                sums, cnts = np.nancumsum(x), np.cumsum(~np.isnan(x))
                cm = np.divide(sums, cnts, out=np.zeros_like(sums), where=cnts != 0)
            err_i = np.interp(conf_i[::-1], conf[hit][::-1], cm[::-1])[::-1]
            TPE[c, e] = float(np.mean(err_i[first:last + 1]))
    mAP = float(np.mean(np.mean(AP, axis=1)))
    mTP = np.array([np.nan if np.isnan(TPE[:, e]).all() else np.nanmean(TPE[:, e]) for e in range(5)])
    NDS = (5.0 * mAP + sum(1.0 - (1.0 if np.isnan(v) else min(1.0, v)) for v in mTP)) / 10.0
    return dict(evaluated=evaluated, tp=tp, match=match, err=err, gt_count=gt_count, order=order, tp_cum=tp_cum,
                fp_cum=fp_cum, AP=AP, tp_errors=TPE, mAP=mAP, mTP=mTP, NDS=NDS)


# ------------------------------------------------------------------------------------------------ the scenes
class Scene:
    """Padded arrays of S samples and the helpers that fill them; ``batches(k)`` cuts them into ``update`` arguments."""

    def __init__(self, name, n_samples=S, m=M, g=G, D=9, attrs=True, valid=False, n_classes=10):
        self.name, self.M, self.G, self.D, self.n_classes = name, m, g, D, n_classes
        self.boxes = np.zeros((n_samples, m, D), np.float32)
        self.boxes[..., 3:6] = 1.0
        self.scores = np.zeros((n_samples, m), np.float32)
        self.labels = np.zeros((n_samples, m), np.int32)
        self.counts = np.zeros(n_samples, np.int32)
        self.gt_boxes = np.zeros((n_samples, g, D), np.float32)
        self.gt_boxes[..., 3:6] = 1.0
        self.gt_labels = np.zeros((n_samples, g), np.int32)
        self.gt_counts = np.zeros(n_samples, np.int32)
        self.gt_attrs = np.full((n_samples, g), -1, np.int32) if attrs else None
        self.gt_valid = np.ones((n_samples, g), np.uint8) if valid else None
        self.check = lambda res: None

    def pred(self, s, cls, x, y, score, size=(1.0, 1.0, 1.0), yaw=0.0, vel=(0.0, 0.0), z=0.0):
        r = int(self.counts[s])
        self.boxes[s, r, :7] = (x, y, z, *size, yaw)
        if self.D == 9:
            self.boxes[s, r, 7:9] = vel
        self.scores[s, r], self.labels[s, r] = score, cls
        self.counts[s] = r + 1
        return s * self.M + r

    def gt(self, s, cls, x, y, size=(1.0, 1.0, 1.0), yaw=0.0, vel=(0.0, 0.0), attr=-1, valid=1, z=0.0):
        g = int(self.gt_counts[s])
        self.gt_boxes[s, g, :7] = (x, y, z, *size, yaw)
        if self.D == 9:
            self.gt_boxes[s, g, 7:9] = vel
        self.gt_labels[s, g] = cls
        if self.gt_attrs is not None:
            self.gt_attrs[s, g] = attr
        if self.gt_valid is not None:
            self.gt_valid[s, g] = valid
        self.gt_counts[s] = g + 1
        return g

    def arrays(self):
        return (self.boxes, self.scores, self.labels, self.counts, self.gt_boxes, self.gt_labels, self.gt_counts,
                self.gt_attrs, self.gt_valid)

    def batches(self, per_batch=B):
        n = self.boxes.shape[0]
        return [tuple(None if a is None else a[i:i + per_batch] for a in self.arrays()) for i in range(0, n, per_batch)]


def _class_names(n):
    return list(CLASSES) if n == 10 else [f'class_{k}' for k in range(n)]


def config_of(scene):
    from ocrfdet_amd.detection_eval import EvalConfig
    if scene.n_classes == 10:
        return EvalConfig(CLASSES)
    names = _class_names(scene.n_classes)
    return EvalConfig(names, class_range={n: 50.0 for n in names})


def perfect():
    """Predictions equal to the ground truth with distinct scores: AP 1, errors 0, NDS 1."""
    tab = Rules().class_tab
    sc = Scene('perfect')
    k = 0
    for s in range(S):
        for j in range(6):
            cls = (s + j) % 10
            x, y = 3.0 * j - 8.0, 1.5 * (s % 7) - 4.0 + 0.25 * j
            vel = (0.5 * (j % 3), 0.25 * (s % 2))
            moving = vel[0] * vel[0] + vel[1] * vel[1] > 0.04
            kw = dict(size=(1.0 + 0.5 * j, 2.0, 1.5), yaw=0.1 * k - 2.0, vel=vel)
            sc.gt(s, cls, x, y, attr=tab[cls][0 if moving else 1], **kw)
            sc.pred(s, cls, x, y, 0.99 - 0.005 * k, **kw)
            k += 1

    def check(res):
        assert np.allclose(res['AP'], 1.0, rtol=0, atol=1e-12)
        assert np.nanmax(np.abs(res['tp_errors'])) == 0.0
        assert abs(res['NDS'] - 1.0) < 1e-12 and abs(res['mAP'] - 1.0) < 1e-12
    sc.check = check
    return sc


HALF_AP = ((36.0 + 2.25 * sum(1.0 / (2 * k + 3) for k in range(9))) / 90.0) / 0.9


def half():
    """One class, ten ground truths, twenty predictions in descending score that alternate true and false positive.
    By hand: precision is 1/2 after every false positive and (k + 2) / (2 k + 3) at true positive k + 1, recall steps by
    1/10, so between recall (k + 1) / 10 and (k + 2) / 10 the interpolated precision rises linearly from 1/2 by
    1 / (2 (2 k + 3)); the recall points 11 .. 100 sum to 45 + 2.25 sum_k 1 / (2 k + 3) and
    AP = ((that - 9) / 90) / 0.9 = HALF_AP at every threshold.  Every match is exact: errors 0, but for the attribute error, which no ground truth here has: 1."""
    sc = Scene('half')
    for i in range(10):
        s = i % S
        sc.gt(s, CAR, 2.0 * i - 9.0, 3.0)
        sc.pred(s, CAR, 2.0 * i - 9.0, 3.0, 0.9 - 0.04 * i)
        sc.pred(s, CAR, 2.0 * i - 9.0, -30.0, 0.88 - 0.04 * i)

    def check(res):
        assert np.allclose(res['AP'][CAR], HALF_AP, rtol=0, atol=1e-9), (res['AP'][CAR], HALF_AP)
        assert np.all(res['tp_errors'][CAR, :4] == 0.0) and res['tp_errors'][CAR, 4] == 1.0      # no attribute: ones
        assert np.all(res['AP'][1:] == 0.0) and np.all(res['tp_errors'][1:8] == 1.0)
    sc.check = check
    return sc


def ties():
    """Equal scores across rows and across samples; two ground truths at equal d2 from one prediction."""
    sc = Scene('ties')
    for s in range(S):
        sc.gt(s, CAR, -1.0, 0.0)
        sc.gt(s, CAR, 1.0, 0.0)                        # both at d2 = 1 from the first prediction
        sc.gt(s, PEDESTRIAN, 5.0, 5.0)
        sc.pred(s, CAR, 0.0, 0.0, 0.5)
        sc.pred(s, CAR, 0.75, 0.0, 0.5)                # same score, next row: takes what the first left
        sc.pred(s, PEDESTRIAN, 5.0, 5.5, 0.5)
        sc.pred(s, PEDESTRIAN, 5.0, 4.5, 0.5)          # equal distance to the one box: the lower row wins
        sc.pred(s, CAR, 20.0, 20.0, 0.25 if s % 2 else 0.5)

    def check(res):
        m = res['match'].reshape(S, M, 4)
        assert np.all(m[:, 0, 2] == 0) and np.all(m[:, 1, 2] == 1)       # ties to the lowest index, then the rest
        assert np.all(m[:, 2, 2] == 2) and np.all(m[:, 3, 2] == -1)
        assert list(res['order'][CAR][:4]) == [0, 1, 4, M]                   # equal scores: by sample, then row
    sc.check = check
    return sc


def step_below(t):
    """float32 values (px, py, gy) for which d2 = px px + (py - gy) (py - gy), evaluated in float64 one operation at a
    time, is the float64 next below t t.  py - gy is exact in float64 (py near 2^-11, gy near 2^-41), which gives the
    difference far more digits than one float32 holds."""
    target = float(np.nextafter(np.float64(t * t), 0.0))
    px = float(np.nextafter(np.float32(t), np.float32(0.0)))
    want = math.sqrt(target - px * px)
    py = float(np.float32(want))
    for k in range(-64, 65):
        gy = float((np.array([np.float32(py - want)]).view(np.int32) + k).view(np.float32)[0])
        if px * px + (py - gy) * (py - gy) == target:
            return px, py, gy
    raise AssertionError(f'no float32 offsets one float64 step below {t} squared')


def thresholds():
    """Offsets of exactly 0.5, 1, 2 and 4 m (d2 == t t must not match), offsets whose d2 is one float64 step below t t
    (a hit; ``step_below``), the nearest float32 offset below along an axis (a hit), and predictions that claim different
    boxes at different thresholds."""
    sc = Scene('thresholds')
    for k, t in enumerate((0.5, 1.0, 2.0, 4.0)):
        sc.gt(k, CAR, 10.0, 0.0)
        sc.pred(k, CAR, 10.0 + t, 0.0, 0.9)            # exactly on the threshold
        sc.gt(k, TRUCK, -10.0, 0.0)
        below = np.nextafter(np.float32(t), np.float32(0.0))
        sc.pred(k, TRUCK, -10.0, float(below), 0.9)    # the nearest representable offset below it
        px, py, gy = step_below(t)
        sc.gt(k, TRAILER, 0.0, gy)
        sc.pred(k, TRAILER, px, py, 0.9)               # d2 is the float64 next below t t
    # sample 4: A takes the far box's neighbour at the small thresholds and B the rest
    sc.gt(4, BUS, 0.0, 0.0)
    sc.gt(4, BUS, 3.0, 0.0)
    sc.pred(4, BUS, 0.25, 0.0, 0.9)                    # 0.25 from box 0 at every threshold
    sc.pred(4, BUS, 0.75, 0.0, 0.8)                    # nearest unclaimed is box 1 at 2.25: TP at 4 only
    sc.gt(5, BICYCLE, 0.0, 0.0)
    sc.gt(5, BICYCLE, 1.5, 0.0)
    sc.pred(5, BICYCLE, 0.625, 0.0, 0.9)               # 0.625 from box 0: FP at 0.5 (box stays free), TP from 1 on
    sc.pred(5, BICYCLE, 0.25, 0.0, 0.8)                # box 0 at 0.5 m; box 1 (1.25) where the first took box 0

    def check(res):
        tp, m = res['tp'].reshape(S, M, 4), res['match'].reshape(S, M, 4)
        for k in range(4):
            assert list(tp[k, 0]) == [1 if j > k else 0 for j in range(4)], (k, tp[k, 0])      # equality is a miss
            assert list(tp[k, 1]) == [1 if j >= k else 0 for j in range(4)], (k, tp[k, 1])     # just below is a hit
            assert list(tp[k, 2]) == [1 if j >= k else 0 for j in range(4)], (k, tp[k, 2])     # one float64 step below
        assert list(tp[4, 1]) == [0, 0, 0, 1] and m[4, 1, 3] == 1
        assert list(m[5, 1]) == [0, -1, 1, 1] and list(tp[5, 1]) == [1, 0, 1, 1]
    sc.check = check
    return sc


def crowd(g=G, m=M):
    """One class with more than 64 predictions: over the samples at M = 40, in one sample's class list in the variant
    with M = 80; the variant with G = 80 puts more than 64 ground truths of the class into one sample."""
    sc = Scene('crowd' + ('' if g == G else f'_g{g}') + ('' if m == M else f'_m{m}'), g=g, m=m)
    rng = np.random.default_rng(7)
    for s in range(S):
        ng = g - 2 if s == 1 else 6
        for j in range(ng):
            sc.gt(s, PEDESTRIAN, float(j % 9) * 1.5 - 6.0, float(j // 9) * 1.5 - 6.0, vel=(0.5, 0.0), attr=2)
        for r in range(m - (s % 3)):
            j = r % ng
            jitter = rng.integers(-8, 9, 2) / 16.0
            sc.pred(s, PEDESTRIAN, float(j % 9) * 1.5 - 6.0 + jitter[0], float(j // 9) * 1.5 - 6.0 + jitter[1],
                    float(rng.integers(1, 200)) / 256.0, vel=(0.25, 0.25), yaw=float(rng.integers(-3, 4)))

    def check(res):
        assert res['order'][PEDESTRIAN].size > 64 * 8
        assert res['gt_count'][1, PEDESTRIAN] == g - 2 and (g == G or g - 2 > 64)
        assert 0.0 < res['AP'][PEDESTRIAN, 2] < 1.0
    sc.check = check
    return sc


def empty():
    """A class with ground truth and no predictions, one with predictions and no ground truth, a sample with count 0,
    counts outside [0, M] / [0, G]."""
    sc = Scene('empty')
    for s in range(S):
        if s == 2:
            continue                                   # nothing at all
        sc.gt(s, TRUCK, 4.0, 4.0)                      # never predicted
        sc.pred(s, BUS, -4.0, 4.0, 0.7)                # never annotated
        sc.gt(s, CAR, 1.0, 1.0)
        sc.pred(s, CAR, 1.25, 1.0, 0.6 + 0.01 * s)
    sc.counts[5], sc.gt_counts[6] = -3, -1             # clamped to 0
    sc.boxes[7, 2:, 0], sc.labels[7, 2:], sc.scores[7, 2:] = 45.0, CAR, 0.125
    sc.counts[7] = M + 100                             # clamped to M: the padding rows are far false positives
    sc.gt_boxes[8, 2:, 0], sc.gt_labels[8, 2:] = -45.0, CAR
    sc.gt_counts[8] = G + 100

    def check(res):
        assert np.all(res['AP'][TRUCK] == 0.0) and np.all(res['tp_errors'][TRUCK] == 1.0)
        assert np.all(res['AP'][BUS] == 0.0) and np.all(res['tp_errors'][BUS] == 1.0)
        assert res['evaluated'].reshape(S, M)[7].sum() == M and res['gt_count'][8, CAR] == G - 1
        assert not res['evaluated'].reshape(S, M)[5].any() and res['gt_count'][6].sum() == 0
        assert 0.0 < res['AP'][CAR, 2] < 1.0
    sc.check = check
    return sc


def ranges():
    """Boxes just inside, on and outside each class radius (30-40-50 and 18-24-30 triangles put a centre exactly on
    it)."""
    sc = Scene('range')
    on = {50.0: (30.0, 40.0), 40.0: (24.0, 32.0), 30.0: (18.0, 24.0)}
    for cls, name in enumerate(CLASSES):
        r = Rules().class_range[cls]
        x, y = on[r]
        s = cls
        inside = float(np.nextafter(np.float32(y), np.float32(0.0)))
        outside = float(np.nextafter(np.float32(y), np.float32(100.0)))
        for yy in (inside, y, outside):
            sc.gt(s, cls, x, yy)
            sc.pred(s, cls, x, yy, 0.5)
        sc.gt(s, cls, -r + 1.0, 0.0)
        sc.pred(s, cls, -r + 1.0, 0.5, 0.75)

    def check(res):
        ev = res['evaluated'].reshape(S, M)
        for cls in range(10):
            assert list(ev[cls, :4]) == [True, False, False, True], (cls, ev[cls, :4])
            assert res['gt_count'][cls, cls] == 2
    sc.check = check
    return sc


def invalid(D=9, attrs=True):
    """Labels -1 and >= C, NaN and infinite scores and centres, gt_valid zeros, NaN ground-truth velocity, D = 7,
    gt_attrs -1 and absent."""
    sc = Scene('invalid' + ('' if D == 9 else '_d7') + ('' if attrs else '_noattr'), D=D, attrs=attrs, valid=True)
    nan, inf = float('nan'), float('inf')
    for s in range(S):
        sc.gt(s, CAR, 0.0, 0.0, vel=(1.0, 0.0), attr=5)
        sc.gt(s, CAR, 5.0, 0.0, vel=(nan, 0.0) if s % 2 else (0.0, nan), attr=-1)
        sc.gt(s, CAR, 10.0, 0.0, valid=0)
        sc.gt(s, -1, 0.0, 5.0)
        sc.gt(s, 10, 0.0, 6.0)
        sc.gt(s, CAR, nan, 7.0)
        sc.gt(s, CAR, 1.0, -inf)
        sc.gt(s, PEDESTRIAN, -5.0, 0.0, vel=(nan, nan), attr=-1)
        sc.pred(s, CAR, 0.5, 0.0, 0.9 - 0.01 * s, vel=(1.0, 0.5))
        sc.pred(s, CAR, 5.0, 0.5, 0.8 - 0.01 * s, vel=(0.1, 0.0))
        sc.pred(s, CAR, 10.0, 0.0, 0.7)                # its box is not valid: a false positive
        sc.pred(s, -1, 0.0, 5.0, 0.9)
        sc.pred(s, 10, 0.0, 6.0, 0.9)
        sc.pred(s, CAR, 0.0, 0.0, nan)
        sc.pred(s, CAR, 0.0, 0.0, inf)
        sc.pred(s, CAR, inf, 0.0, 0.9)
        sc.pred(s, CAR, 0.0, 0.0, 0.9, z=nan)
        sc.pred(s, PEDESTRIAN, -5.0, 0.25, 0.6, vel=(0.0, 0.0))

    def check(res):
        ev = res['evaluated'].reshape(S, M)
        assert np.all(ev[:, :3]) and not ev[:, 3:9].any() and np.all(ev[:, 9])
        assert np.all(res['gt_count'][:, CAR] == 2) and np.all(res['gt_count'][:, PEDESTRIAN] == 1)
        e = res['err'].reshape(S, M, 5)
        assert np.isnan(e[:, 1, 3]).all() and np.isnan(e[:, 1, 4]).all()           # NaN velocity, attribute -1
        if D == 9:
            assert np.all(e[:, 0, 3] == 0.5)
        else:
            assert np.isnan(e[:, 0, 3]).all()
        assert (np.all(e[:, 0, 4] == (0.0 if D == 9 else 1.0)) if attrs else np.isnan(e[:, 0, 4]).all())
        # pedestrian: every velocity and attribute error is NaN, so the all-NaN series gives ones
        assert res['tp_errors'][PEDESTRIAN, 3] == 1.0 and res['tp_errors'][PEDESTRIAN, 4] == 1.0
        assert res['tp_errors'][PEDESTRIAN, 0] == 0.25
    sc.check = check
    return sc


def periods():
    """Barrier yaw differences near pi (period pi: nearly 0), other classes near 2 pi; cone and barrier have NaN where
    they have no error, and those drop from the means."""
    sc = Scene('periods')
    for s in range(S):
        d = 0.03125 * (s + 1)
        sc.gt(s, BARRIER, 3.0, 3.0, yaw=0.0)
        sc.pred(s, BARRIER, 3.0, 3.0, 0.9 - 0.01 * s, yaw=math.pi - d)
        sc.gt(s, CAR, -3.0, 3.0, yaw=-3.0)
        sc.pred(s, CAR, -3.0, 3.0, 0.9 - 0.01 * s, yaw=-3.0 + 2.0 * math.pi - d)
        sc.gt(s, TRUCK, -3.0, -3.0, yaw=0.0)
        sc.pred(s, TRUCK, -3.0, -3.0, 0.9 - 0.01 * s, yaw=math.pi - d)
        sc.gt(s, CONE, 3.0, -3.0, yaw=1.0)
        sc.pred(s, CONE, 3.0, -3.0, 0.9 - 0.01 * s, yaw=-1.0)

    def check(res):
        e = res['err'].reshape(S, M, 5)
        for s in range(S):
            d = 0.03125 * (s + 1)
            assert abs(e[s, 0, 2] - d) < 1e-6 and abs(e[s, 1, 2] - d) < 1e-6 and abs(e[s, 2, 2] - (math.pi - d)) < 1e-6
        t = res['tp_errors']
        assert np.isnan(t[CONE, 2:]).all() and np.isnan(t[BARRIER, 3:]).all() and not np.isnan(t[BARRIER, 2])
        assert not np.isnan(res['mTP']).any() and t[BARRIER, 2] < 0.6 and t[CAR, 2] < 0.6 and t[TRUCK, 2] > 2.5
    sc.check = check
    return sc


def low_recall():
    """A class whose recall never reaches 0.1: AP 0 and errors 1."""
    sc = Scene('low_recall')
    for s in range(S):
        for j in range(8):
            sc.gt(s, MOTORCYCLE, 2.0 * j - 8.0, 2.0)
    for s in range(5):
        sc.pred(s, MOTORCYCLE, -8.0, 2.25, 0.9)        # 5 of 120: recall 1/24
        sc.pred(s, MOTORCYCLE, 20.0, 20.0, 0.5)

    def check(res):
        assert res['tp_cum'][MOTORCYCLE][2][-1] == 5
        assert np.all(res['AP'][MOTORCYCLE] == 0.0) and np.all(res['tp_errors'][MOTORCYCLE] == 1.0)
    sc.check = check
    return sc


def many_classes(n):
    """The smallest and the largest workgroup: 1 class, 16 classes."""
    sc = Scene(f'classes_{n}', n_classes=n)
    rng = np.random.default_rng(n)
    for s in range(S):
        for j in range(12):
            cls = (s + j) % n
            x, y = float(rng.integers(-40, 41)) / 2.0, float(rng.integers(-40, 41)) / 2.0
            sc.gt(s, cls, x, y, vel=(0.5, 0.0))
            sc.pred(s, cls, x + float(rng.integers(-6, 7)) / 4.0, y, float(rng.integers(1, 250)) / 256.0, yaw=0.5)
            sc.pred(s, cls, x, y + float(rng.integers(-20, 21)) / 4.0, float(rng.integers(1, 250)) / 256.0)

    def check(res):
        assert res['AP'].shape == (n, 4) and 0.0 < res['mAP'] < 1.0
    sc.check = check
    return sc


SCENES = {sc.name: sc for sc in (perfect(), half(), ties(), thresholds(), crowd(), crowd(g=80), crowd(m=80), empty(), ranges(), invalid(),
                                 invalid(D=7), invalid(attrs=False), periods(), low_recall(), many_classes(1),
                                 many_classes(16))}
_RESULTS = {}


def result_of(name):
    """The oracle's result for scene ``name``, computed once and shared (do not modify it); the scene's own property is
    asserted on it."""
    if name not in _RESULTS:
        scene = SCENES[name]
        res = evaluate(Rules(scene.n_classes), scene)
        scene.check(res)
        _RESULTS[name] = res
    return _RESULTS[name]
