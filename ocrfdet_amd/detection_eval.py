"""nuScenes detection metrics on the device: AP over centre-distance thresholds, the five true-positive errors, mAP and
NDS (``detection_cvpr_2019``) from the padded output of the fused decode and padded ground truth, accumulated batch by
batch without a host read and read back once.

* ``EvalConfig``: the classes, their ranges, the thresholds and the attribute tables;
* ``DetectionEval``: ``update`` is ONE launch of ``ocrf_det_eval_match`` (csrc/det_eval.hip) per batch, ``compute``
  the launches of ``ocrf_det_eval_summary``, ``results_to_host`` the one read-back, keyed like the reference's
  ``NuScenesDataset.evaluate``; CPU tensors and ``fused=False`` take ``evaluate_host``, the same rules in numpy float64;
* ``evaluate_stream``: the body of ``OcRFDet4D.evaluate_stream``.

The rules are stated once, in include/ocrf_hip.h (section "nuScenes detection metrics").  They are written from the
benchmark's published procedure; the nuScenes devkit is not a dependency of this package and nothing here has been
compared with its output.  Everything is evaluated in the key frame's ego frame: centre distances, yaw and velocity
differences and speeds do not change under the rigid map to the global frame, so no pose is needed.
"""
import contextlib
import math

import numpy as np
import torch

from . import _lib
from .streaming import key_frame_inputs

MAX_CLASSES = _lib.OCRF_DET_EVAL_MAX_CLASSES
RECORD_BYTES = 4 + 4 + 16 + 40                      # key, info, four matched indices, five float64 errors
# detection_cvpr_2019's class ranges in metres; a setting, not a measurement
NUSCENES_CLASS_RANGE = dict(car=50.0, truck=50.0, bus=50.0, trailer=50.0, construction_vehicle=50.0, pedestrian=40.0,
                            motorcycle=40.0, bicycle=40.0, traffic_cone=30.0, barrier=30.0)
# NuScenesDataset.AttrMapping, DefaultAttribute and _format_bbox's rule: (moving, still) per class, '' = none
ATTR_MAPPING = {'cycle.with_rider': 0, 'cycle.without_rider': 1, 'pedestrian.moving': 2, 'pedestrian.standing': 3,
                'pedestrian.sitting_lying_down': 4, 'vehicle.moving': 5, 'vehicle.parked': 6, 'vehicle.stopped': 7}
PREDICTED_ATTRIBUTE = dict(
    car=('vehicle.moving', 'vehicle.parked'), truck=('vehicle.moving', 'vehicle.parked'),
    trailer=('vehicle.moving', 'vehicle.parked'), construction_vehicle=('vehicle.moving', 'vehicle.parked'),
    bus=('vehicle.moving', 'vehicle.stopped'), bicycle=('cycle.with_rider', 'cycle.without_rider'),
    motorcycle=('cycle.with_rider', 'cycle.without_rider'), pedestrian=('pedestrian.moving', 'pedestrian.standing'),
    traffic_cone=('', ''), barrier=('', ''))
ERR_NAMES = ('trans_err', 'scale_err', 'orient_err', 'vel_err', 'attr_err')
ERR_NAME_MAPPING = dict(trans_err='mATE', scale_err='mASE', orient_err='mAOE', vel_err='mAVE', attr_err='mAAE')
HALF_TURN, NO_ORIENT, NO_VEL, NO_ATTR = (_lib.OCRF_DET_EVAL_HALF_TURN, _lib.OCRF_DET_EVAL_NO_ORIENT,
                                         _lib.OCRF_DET_EVAL_NO_VEL, _lib.OCRF_DET_EVAL_NO_ATTR)
CLASS_FLAGS = dict(barrier=HALF_TURN | NO_VEL | NO_ATTR, traffic_cone=NO_ORIENT | NO_VEL | NO_ATTR)
EVALUATED, NOT_EVALUATED, REST_CLASS = _lib.OCRF_DET_EVAL_EVALUATED, 31, 16
_PI, _TWO_PI = math.pi, 2.0 * math.pi


class EvalConfig:
    """``class_names``: the names of the labels 0, 1, ... (at most 16); ``class_range``: a dict by class name of ranges
    in metres (default ``NUSCENES_CLASS_RANGE``; every class needs one); ``dist_ths``: the four centre-distance
    thresholds; ``dist_th_tp``: the one of them whose matches carry the true-positive errors; ``min_recall``,
    ``min_precision``: the part of the curves that counts."""

    def __init__(self, class_names, class_range=None, dist_ths=(0.5, 1.0, 2.0, 4.0), dist_th_tp=2.0, min_recall=0.1,
                 min_precision=0.1):
        names = list(class_names)
        if not names or len(names) > MAX_CLASSES or not all(isinstance(n, str) for n in names):
            raise ValueError(f'class_names: 1 to {MAX_CLASSES} strings, got {class_names!r}')
        if len(set(names)) != len(names):
            raise ValueError(f'class_names holds a name twice: {names}')
        table = NUSCENES_CLASS_RANGE if class_range is None else class_range
        if not isinstance(table, dict):
            raise TypeError(f'class_range is a dict by class name, got {type(class_range).__name__}')
        missing = [n for n in names if n not in table]
        if missing:
            raise ValueError(f'class_range has no range for {missing}')
        ranges = [float(table[n]) for n in names]
        if not all(math.isfinite(r) and r > 0.0 for r in ranges):
            raise ValueError(f'class_range: finite ranges > 0, got {ranges}')
        ths = tuple(float(t) for t in dist_ths)
        if len(ths) != 4 or not all(math.isfinite(t) and t > 0.0 for t in ths):
            raise ValueError(f'dist_ths: four finite thresholds > 0, got {dist_ths!r}')
        if float(dist_th_tp) not in ths:
            raise ValueError(f'dist_th_tp is one of dist_ths {ths}, got {dist_th_tp!r}')
        if not 0.0 <= float(min_recall) < 1.0 or not 0.0 <= float(min_precision) < 1.0:
            raise ValueError(f'min_recall and min_precision are in [0, 1), got {min_recall!r}, {min_precision!r}')
        self.class_names, self.class_range = tuple(names), tuple(ranges)
        self.dist_ths, self.dist_th_tp = ths, float(dist_th_tp)
        self.tp_index = ths.index(float(dist_th_tp))
        self.min_recall, self.min_precision = float(min_recall), float(min_precision)
        self.first = int(round(100 * self.min_recall)) + 1       # the first recall point that counts
        attr = lambda n, k: ATTR_MAPPING.get(PREDICTED_ATTRIBUTE.get(n, ('', ''))[k], -1)       # noqa: E731
        self.class_tab = tuple((attr(n, 0), attr(n, 1), CLASS_FLAGS.get(n, 0)) for n in names)
        self._on = {}

    @property
    def n_classes(self):
        return len(self.class_names)

    def tables_on(self, device):
        """``(class_range float32 (C), class_tab int32 (C, 3))`` on ``device``, uploaded once per device."""
        if device not in self._on:
            self._on[device] = (torch.tensor(self.class_range, dtype=torch.float32, device=device),
                                torch.tensor(self.class_tab, dtype=torch.int32, device=device))
        return self._on[device]


# ------------------------------------------------------------------------------------------------ the host arm
def score_keys(scores):
    """The sort key of float32 scores (uint32): ascending keys are descending scores, -0 counts as +0."""
    u = np.ascontiguousarray(scores, np.float32).view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    o = np.where(u >> np.uint32(31) != 0, ~u, u ^ np.uint32(0x80000000))
    return ~o


def key_scores(keys):
    o = ~np.ascontiguousarray(keys, np.uint32)
    return np.where(o & np.uint32(0x80000000) != 0, o ^ np.uint32(0x80000000), ~o).astype(np.uint32).view(np.float32)


def _evaluated(box, label, ranges, extra):
    """The class of each box that is evaluated, else ``NOT_EVALUATED``."""
    nc = len(ranges)
    lab = label.astype(np.int64)
    known = (lab >= 0) & (lab < nc) & extra & np.isfinite(box[:, :3]).all(1)
    r = ranges[np.clip(lab, 0, nc - 1)].astype(np.float64)
    x, y = box[:, 0].astype(np.float64), box[:, 1].astype(np.float64)
    with np.errstate(all='ignore'):
        inside = x * x + y * y < r * r
    return np.where(known & inside, lab, NOT_EVALUATED)


def _pair_errors(cfg, D, cls, p, q, ga):
    """The five errors of prediction ``p`` matched to ground truth ``q`` (rows of float32), ``ga`` its attribute."""
    p, q = p.astype(np.float64), q.astype(np.float64)
    dx, dy = p[0] - q[0], p[1] - q[1]
    with np.errstate(all='ignore'):
        trans = np.sqrt(dx * dx + dy * dy)
        inter = (min(p[3], q[3]) * min(p[4], q[4])) * min(p[5], q[5])
        scale = 1.0 - inter / (((p[3] * p[4]) * p[5] + (q[3] * q[4]) * q[5]) - inter)
        period = np.float64(_PI if cfg.class_tab[cls][2] & HALF_TURN else _TWO_PI)
        half = period / 2.0
        m = np.fmod((q[6] - p[6]) + half, period)
        if m < 0.0:
            m = m + period
        diff = m - half
        if diff > _PI:
            diff = diff - _TWO_PI
        orient = abs(diff)
        vel, moving = np.float64('nan'), False
        if D == 9:
            dvx, dvy = p[7] - q[7], p[8] - q[8]
            vel = np.sqrt(dvx * dvx + dvy * dvy)
            moving = bool(p[7] * p[7] + p[8] * p[8] > 0.2 * 0.2)
    attr = np.float64('nan')
    if ga != -1:
        attr = np.float64(0.0 if cfg.class_tab[cls][0 if moving else 1] == ga else 1.0)
    return trans, scale, orient, vel, attr


def match_sample_host(cfg, boxes, scores, labels, count, gt_boxes, gt_labels, gt_count, gt_attrs=None, gt_valid=None):
    """One sample's records by the header's rules: ``(key (M) uint32, info (M) int32, match (M, 4) int32, err (M, 5)
    float64, gt_count (C) int32)`` from numpy arrays."""
    M, D = boxes.shape
    G = gt_boxes.shape[0]
    nc = cfg.n_classes
    ranges = np.asarray(cfg.class_range, np.float32)
    n, ng = min(max(int(count), 0), M), min(max(int(gt_count), 0), G)
    key = np.full(M, 0xFFFFFFFF, np.uint32)
    info = np.full(M, NOT_EVALUATED, np.int32)
    match = np.full((M, 4), -1, np.int32)
    err = np.full((M, 5), np.nan, np.float64)
    cls_p = np.full(M, NOT_EVALUATED, np.int64)
    cls_p[:n] = _evaluated(boxes[:n], labels[:n], ranges, np.isfinite(scores[:n]))
    valid = np.ones(ng, bool) if gt_valid is None else gt_valid[:ng] != 0
    cls_g = _evaluated(gt_boxes[:ng], gt_labels[:ng], ranges, valid)
    keys = score_keys(scores)
    tp = np.zeros(M, np.int32)
    gtc = np.zeros(nc, np.int32)
    px, py = boxes[:, 0].astype(np.float64), boxes[:, 1].astype(np.float64)
    gx, gy = gt_boxes[:ng, 0].astype(np.float64), gt_boxes[:ng, 1].astype(np.float64)
    for c in range(nc):
        rows, gts = np.flatnonzero(cls_p == c), np.flatnonzero(cls_g == c)
        gtc[c] = gts.size
        if rows.size == 0 or gts.size == 0:
            continue
        rows = rows[np.argsort(keys[rows], kind='stable')]
        for t, th in enumerate(cfg.dist_ths):
            free = np.ones(gts.size, bool)
            for r in rows:
                dx, dy = px[r] - gx[gts], py[r] - gy[gts]
                with np.errstate(all='ignore'):
                    d2 = np.where(free, dx * dx + dy * dy, np.inf)
                k = int(np.argmin(d2))                               # the first of the smallest: lowest index
                if d2[k] < np.float64(th) * np.float64(th):
                    free[k] = False
                    tp[r] |= 1 << t
                    match[r, t] = gts[k]
    for r in np.flatnonzero(cls_p != NOT_EVALUATED):
        c = int(cls_p[r])
        key[r] = keys[r]
        info[r] = c | EVALUATED | (int(tp[r]) << 8)
        g = match[r, cfg.tp_index]
        if g >= 0:
            err[r] = _pair_errors(cfg, D, c, boxes[r], gt_boxes[g], -1 if gt_attrs is None else int(gt_attrs[g]))
    return key, info, match, err, gtc


def summarise_host(cfg, key, info, err, gt_count):
    """The summary of accumulated records by the header's rules: a dict of numpy arrays named like ``compute()``'s."""
    nc, n = cfg.n_classes, key.shape[0]
    cls = np.where(info & EVALUATED != 0, info & 31, REST_CLASS)
    by_key = np.argsort(key, kind='stable')
    order = by_key[np.argsort(cls[by_key], kind='stable')].astype(np.int32)
    sorted_cls = cls[order].astype(np.int32)
    flags = np.stack([(info[order] >> (8 + t)) & 1 for t in range(4)]).astype(np.int32)
    tp_excl = (np.cumsum(flags, axis=1) - flags).astype(np.int32)
    ap = np.zeros((nc, 4))
    tpe = np.ones((nc, 5))
    rec_interp = np.linspace(0, 1, 101)
    first = cfg.first
    npos_all = gt_count.reshape(-1, nc).sum(0)
    for c in range(nc):
        lo, hi = np.searchsorted(sorted_cls, c), np.searchsorted(sorted_cls, c + 1)
        npos = int(npos_all[c])
        for e, bit in enumerate((NO_ORIENT, NO_VEL, NO_ATTR), 2):
            if cfg.class_tab[c][2] & bit:
                tpe[c, e] = np.nan
        if npos == 0 or hi == lo:
            continue
        conf = key_scores(key[order[lo:hi]]).astype(np.float64)
        conf_i = None
        for t in range(4):
            f = flags[t, lo:hi]
            tp = np.cumsum(f).astype(np.float64)
            fp = np.cumsum(1 - f).astype(np.float64)
            prec, rec = tp / (tp + fp), tp / float(npos)
            prec_i = np.interp(rec_interp, rec, prec, right=0)
            if t == cfg.tp_index:
                conf_i = np.interp(rec_interp, rec, conf, right=0)
            part = np.maximum(prec_i[first:] - cfg.min_precision, 0.0)
            total = 0.0
            for v in part:
                total += v
            ap[c, t] = total / float(part.size) / (1.0 - cfg.min_precision)
        hit = flags[cfg.tp_index, lo:hi] != 0
        if not hit.any():
            continue
        nz = np.flatnonzero(conf_i)
        last = int(nz[-1]) if nz.size else 0
        if last < first:
            continue
        conf_m = conf[hit]
        for e in range(5):
            if np.isnan(tpe[c, e]):
                continue
            x = err[order[lo:hi], e][hit]
            if np.isnan(x).all():
                cm = np.ones(x.size)
            else:
                sums, cnts = np.nancumsum(x), np.cumsum(~np.isnan(x))
                cm = np.divide(sums, cnts, out=np.zeros_like(sums), where=cnts != 0)
            err_i = np.interp(conf_i[::-1], conf_m[::-1], cm[::-1])[::-1]
            total = 0.0
            for v in err_i[first:last + 1]:
                total += v
            tpe[c, e] = total / float(last - first + 1)
    result = np.empty(9 * nc + 7)
    result[:4 * nc], result[4 * nc:9 * nc] = ap.ravel(), tpe.ravel()
    m_ap = 0.0
    for c in range(nc):
        m_ap += (((ap[c, 0] + ap[c, 1]) + ap[c, 2]) + ap[c, 3]) / 4.0
    m_ap /= float(nc)
    nds = 5.0 * m_ap
    result[9 * nc] = m_ap
    for e in range(5):
        vals = [v for v in tpe[:, e] if not np.isnan(v)]
        total = 0.0
        for v in vals:
            total += v
        mean = total / float(len(vals)) if vals else float('nan')
        result[9 * nc + 1 + e] = mean
        nds += 1.0 - (1.0 if np.isnan(mean) else min(1.0, mean))
    result[9 * nc + 6] = nds / 10.0
    return dict(result=result, order=order, sorted_cls=sorted_cls, tp_excl=tp_excl)


def evaluate_host(cfg, batches):
    """The rules in numpy float64 on the host.  ``batches``: an iterable of ``update``'s argument tuples ``(boxes, scores,
    labels, counts, gt_boxes, gt_labels, gt_counts[, gt_attrs[, gt_valid]])`` as tensors or arrays.  Returns a dict of
    numpy arrays: ``result`` (9 C + 7) float64 = AP (C, 4), errors (C, 5), mAP, the five mTP, NDS; the records ``key``,
    ``info``, ``match``, ``err``, ``gt_count``; ``order``, ``sorted_cls``, ``tp_excl`` as ``ocrf_det_eval_summary``
    leaves them."""
    host = lambda t: None if t is None else (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))  # noqa: E731
    records = []
    for batch in batches:
        arrays = [host(t) for t in batch] + [None] * (9 - len(batch))
        boxes, scores, labels, counts, gt_boxes, gt_labels, gt_counts, gt_attrs, gt_valid = arrays
        for b in range(boxes.shape[0]):
            records.append(match_sample_host(cfg, boxes[b], scores[b], labels[b], counts[b], gt_boxes[b], gt_labels[b],
                                             gt_counts[b], None if gt_attrs is None else gt_attrs[b],
                                             None if gt_valid is None else gt_valid[b]))
    if not records:
        raise ValueError('nothing to evaluate: no sample was given')
    key, info, match, err, gt_count = (np.concatenate([r[k] for r in records]) for k in range(5))
    out = summarise_host(cfg, key, info, err, gt_count)
    out.update(key=key, info=info, match=match, err=err, gt_count=gt_count.reshape(-1, cfg.n_classes))
    return out


# ------------------------------------------------------------------------------------------------ the evaluator
def _checked(M, G, tensors, device):
    """(B, D) of ``update``'s arguments when they fit together and the evaluator; anything else raises."""
    boxes, scores, labels, counts, gt_boxes, gt_labels, gt_counts, gt_attrs, gt_valid = tensors
    named = dict(boxes=(boxes, torch.float32), scores=(scores, torch.float32), labels=(labels, torch.int32),
                 counts=(counts, torch.int32), gt_boxes=(gt_boxes, torch.float32), gt_labels=(gt_labels, torch.int32),
                 gt_counts=(gt_counts, torch.int32), gt_attrs=(gt_attrs, torch.int32), gt_valid=(gt_valid, None))
    for name, (t, dtype) in named.items():
        if t is None and name in ('gt_attrs', 'gt_valid'):
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'{name} is a tensor, got {type(t).__name__}')
        if name == 'gt_valid':
            if t.dtype not in (torch.uint8, torch.bool):
                raise TypeError(f'gt_valid is uint8 or bool, got {t.dtype}')
        elif t.dtype != dtype:
            raise TypeError(f'{name} is {dtype}, got {t.dtype}')
        if t.device != device:
            raise ValueError(f'{name} is on {t.device}, the evaluator on {device}')
    if boxes.dim() != 3 or boxes.shape[2] not in (7, 9) or boxes.shape[0] < 1 or boxes.shape[1] != M:
        raise ValueError(f'boxes is (B, {M}, 9 | 7) with B >= 1, got {tuple(boxes.shape)}')
    B, _, D = boxes.shape
    shapes = dict(scores=(B, M), labels=(B, M), counts=(B,), gt_boxes=(B, G, D), gt_labels=(B, G), gt_counts=(B,),
                  gt_attrs=(B, G), gt_valid=(B, G))
    for name, shape in shapes.items():
        t = named[name][0]
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f'{name} is {shape} for boxes {tuple(boxes.shape)} and G = {G}, got {tuple(t.shape)}')
    return B, D


class DetectionEval:
    """Accumulates the detection metrics of up to ``capacity`` samples of ``M`` padded predictions and ``G`` padded
    ground-truth boxes on ``device``.  The buffers (``RECORD_BYTES`` = 64 bytes per prediction slot, 4 per sample and
    class) and the summary's workspace are allocated here, once: ``update`` and ``compute`` only launch."""

    def __init__(self, cfg, capacity, M, G, device, fused=True):
        if not isinstance(cfg, EvalConfig):
            raise TypeError(f'cfg is an EvalConfig, got {type(cfg).__name__}')
        capacity, M, G = int(capacity), int(M), int(G)
        if capacity < 1 or M < 1 or G < 1 or capacity * M >= 2 ** 31:
            raise ValueError(f'capacity, M, G >= 1 and capacity * M < 2^31, got {capacity}, {M}, {G}')
        self.cfg, self.capacity, self.M, self.G = cfg, capacity, M, G
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:     # a tensor's device always carries its index
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.fused = bool(fused) and self.device.type == 'cuda'
        self.n_samples = 0
        self._batches = []
        if not self.fused:
            return
        L = _lib.lib()
        if L.ocrf_det_eval_match_lds_bytes(M, G) > _lib.OCRF_DET_EVAL_MAX_LDS:
            raise ValueError(f'ocrf_det_eval_match keeps a sample\'s rows and boxes in LDS: 52 * M + 28 * G + 128 <= '
                             f'{_lib.OCRF_DET_EVAL_MAX_LDS} bytes, got M = {M}, G = {G}; evaluate_host has no such limit')
        n, nc, dev = capacity * M, cfg.n_classes, self.device
        self.rec_key = torch.empty(n, dtype=torch.int32, device=dev)          # the uint32 keys' bits
        self.rec_info = torch.empty(n, dtype=torch.int32, device=dev)
        self.rec_match = torch.empty((n, 4), dtype=torch.int32, device=dev)
        self.rec_err = torch.empty((n, 5), dtype=torch.float64, device=dev)
        self.gt_count = torch.empty((capacity, nc), dtype=torch.int32, device=dev)
        self._order = torch.empty(n, dtype=torch.int32, device=dev)
        self._sorted_cls = torch.empty(n, dtype=torch.int32, device=dev)
        self._tp_excl = torch.empty(4 * n, dtype=torch.int32, device=dev)
        self._result = torch.empty(9 * nc + 7, dtype=torch.float64, device=dev)
        self._workspace = torch.empty(L.ocrf_det_eval_summary_workspace_bytes(n), dtype=torch.uint8, device=dev)
        self._tables = cfg.tables_on(dev)

    @property
    def bytes_per_sample(self):
        """What one accumulated sample takes in the record buffers."""
        return self.M * RECORD_BYTES + 4 * self.cfg.n_classes

    def reset(self):
        """Forget the accumulated samples; the buffers stay."""
        self.n_samples = 0
        self._batches = []

    def update(self, boxes, scores, labels, counts, gt_boxes, gt_labels, gt_counts, gt_attrs=None, gt_valid=None):
        """One batch: the padded decode output (``CenterHead.get_bboxes_padded``) and padded ground truth in the same
        column convention and frame, all on the evaluator's device.  On the device this is ONE launch and no read-back;
        samples beyond ``capacity``, or shapes, dtypes or devices that disagree, raise before it."""
        tensors = (boxes, scores, labels, counts, gt_boxes, gt_labels, gt_counts, gt_attrs, gt_valid)
        B, D = _checked(self.M, self.G, tensors, self.device)
        if self.n_samples + B > self.capacity:
            raise ValueError(f'{self.n_samples} + {B} samples exceed the capacity of {self.capacity}')
        if not self.fused:
            self._batches.append(tuple(None if t is None else t.detach().cpu().numpy().copy() for t in tensors))
            self.n_samples += B
            return
        if B > 65535:
            raise ValueError(f'at most 65535 samples per update, got {B}')
        cfg = self.cfg
        valid = None if gt_valid is None else gt_valid.contiguous().view(torch.uint8)
        _lib.launch('ocrf_det_eval_match', self.device, B, self.M, D, self.G, cfg.n_classes, self.n_samples,
                    self.capacity, *cfg.dist_ths, cfg.tp_index, boxes.contiguous(), scores.contiguous(),
                    labels.contiguous(), counts.contiguous(), gt_boxes.contiguous(), gt_labels.contiguous(),
                    gt_counts.contiguous(), None if gt_attrs is None else gt_attrs.contiguous(), valid, *self._tables,
                    self.rec_key, self.rec_info, self.rec_match, self.rec_err, self.gt_count)
        self.n_samples += B

    def compute(self):
        """The metrics of what was accumulated, as a dict of tensors on the evaluator's device: ``result`` (9 C + 7)
        float64 and its views ``AP`` (C, 4), ``tp_errors`` (C, 5), ``mAP``, ``mTP`` (5), ``NDS``; ``order``,
        ``sorted_cls`` (n) and ``tp_excl`` (4, n) int32 over the n = samples * M slots, as the header states them.  On
        the device it only launches; the tensors are the evaluator's own and are overwritten by the next call."""
        if self.n_samples < 1:
            raise ValueError('nothing to evaluate: no update since the last reset')
        nc, n = self.cfg.n_classes, self.n_samples * self.M
        if self.fused:
            cfg = self.cfg
            _lib.launch('ocrf_det_eval_summary', self.device, self.n_samples, self.M, nc, cfg.tp_index, cfg.first,
                        cfg.min_precision, self.rec_key, self.rec_info, self.rec_err, self.gt_count, self._tables[1],
                        self._order, self._sorted_cls, self._tp_excl, self._result, self._workspace,
                        self._workspace.numel())
            result, order, sorted_cls = self._result, self._order[:n], self._sorted_cls[:n]
            tp_excl = self._tp_excl[:4 * n].view(4, n)
        else:
            host = evaluate_host(self.cfg, self._batches)
            result, order, sorted_cls, tp_excl = (torch.from_numpy(np.ascontiguousarray(host[k])).to(self.device)
                                                  for k in ('result', 'order', 'sorted_cls', 'tp_excl'))
        return dict(result=result, AP=result[:4 * nc].view(nc, 4), tp_errors=result[4 * nc:9 * nc].view(nc, 5),
                    mAP=result[9 * nc], mTP=result[9 * nc + 1:9 * nc + 6], NDS=result[9 * nc + 6], order=order,
                    sorted_cls=sorted_cls, tp_excl=tp_excl)

    def results_to_host(self, prefix='pts_bbox_NuScenes'):
        """The one read-back: a plain dict of floats keyed like ``NuScenesDataset.evaluate``'s (``<prefix>/car_AP_dist_0.5``,
        ``<prefix>/car_trans_err``, ``<prefix>/mATE``, ``<prefix>/NDS``, ``<prefix>/mAP``), unrounded."""
        return result_dict(self.cfg, self.compute()['result'].cpu().numpy(), prefix)


def result_dict(cfg, result, prefix='pts_bbox_NuScenes'):
    """``results_to_host``'s dict from a ``result`` vector on the host."""
    nc = cfg.n_classes
    detail = {}
    for c, name in enumerate(cfg.class_names):
        for t, th in enumerate(cfg.dist_ths):
            detail[f'{prefix}/{name}_AP_dist_{th}'] = float(result[4 * c + t])
        for e, err in enumerate(ERR_NAMES):
            detail[f'{prefix}/{name}_{err}'] = float(result[4 * nc + 5 * c + e])
    for e, err in enumerate(ERR_NAMES):
        detail[f'{prefix}/{ERR_NAME_MAPPING[err]}'] = float(result[9 * nc + 1 + e])
    detail[f'{prefix}/NDS'] = float(result[9 * nc + 6])
    detail[f'{prefix}/mAP'] = float(result[9 * nc])
    return detail


def evaluate_stream(det, frames_with_gt, evaluator, state=None, multi_frame=False, bf16=False):
    """The body of ``OcRFDet4D.evaluate_stream``: per element ``(img_inputs, gt)`` of ``frames_with_gt`` one
    ``stream_step``, the head, ``get_bboxes_padded`` and ``evaluator.update`` with ``gt`` = ``dict(gt_boxes, gt_labels,
    gt_counts[, gt_attrs][, gt_valid][, new_sequence])``.  Returns ``(evaluator, state)``, ``state`` the stream state to
    hand to the next call; from the second frame on nothing synchronises with the host, and
    ``evaluator.results_to_host()`` is the one read-back.

    Precondition: the BEV augmentation ``bda`` is the identity, as at test time, so that the decoded boxes and the ground
    truth are both in the key frame's ego."""
    if not det.with_pts_bbox:
        raise RuntimeError('evaluate_stream needs a detection head (pts_bbox_head)')
    if not isinstance(evaluator, DetectionEval):
        raise TypeError(f'evaluator is a DetectionEval, got {type(evaluator).__name__}')
    head = det.pts_bbox_head
    for img_inputs, gt in frames_with_gt:
        if multi_frame:
            img_inputs = key_frame_inputs(img_inputs, det.num_frame)
        (img_feats, _, _), state = det.stream_step(img_inputs, state=state, new_sequence=gt.get('new_sequence'), bf16=bf16)
        with torch.no_grad(), (det.bf16_inference() if bf16 else contextlib.nullcontext()):
            boxes, scores, labels, counts = head.get_bboxes_padded(head(img_feats))
        evaluator.update(boxes, scores, labels, counts, gt['gt_boxes'], gt['gt_labels'], gt['gt_counts'],
                         gt_attrs=gt.get('gt_attrs'), gt_valid=gt.get('gt_valid'))
    return evaluator, state
