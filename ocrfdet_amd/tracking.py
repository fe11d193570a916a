"""Streaming object tracking: the detections of ``OcRFDet4D.stream_step`` get identities that last across frames, by
greedy closest-centre association (the scheme of CenterPoint's nuScenes tracker) on the head's ``vel`` output.

* ``TrackConfig``: the classes, their matching radii, ``max_age`` and ``min_score``;
* ``TrackState``: the tracks of B parallel sequences, double-buffered on the detections' device;
* ``track_step``: one step on the padded decode output, ONE launch of ``ocrf_track_step`` (csrc/track_assoc.hip) and no
  device -> host read; ``track_step_host``: the same rules in numpy float64, for CPU tensors and ``fused=False``;
* ``track_stream``: the body of ``OcRFDet4D.track_stream``; ``results_to_host``: the one read-back.

The rules are stated once, in include/ocrf_hip.h (section "Streaming object tracking"): a detection is moved back by its
velocity over ``time_lag`` in the global frame and takes the nearest unclaimed track of its label within the class's
``max_dist``, in row order; what matches keeps its id, what does not gets a new one, and a track that goes unmatched for
``max_age`` frames in a row is dropped.  Positions are float64 in the global frame: an ego pose lies thousands of metres
from the map's origin, a pedestrian's radius is one metre.
"""
import contextlib
import math
import numbers

import numpy as np
import torch

from . import _lib
from .streaming import _flags, _upload, key_frame_inputs

MAX_CLASSES = _lib.OCRF_TRACK_MAX_CLASSES
# CenterPoint's nuScenes table, metres per frame gap; a setting, not a measurement.  Any other class: 0, not tracked.
NUSCENES_MAX_DIST = dict(car=4.0, truck=4.0, bus=5.5, trailer=3.0, pedestrian=1.0, motorcycle=13.0, bicycle=3.0)
_STATE = (('pos', torch.float64, (2,)), ('vel', torch.float64, (2,)), ('label', torch.int32, ()), ('id', torch.int32, ()),
          ('misses', torch.int32, ()), ('hits', torch.int32, ()))


class TrackConfig:
    """``class_names``: the names of the labels 0, 1, ... (at most 16); ``max_dist``: a dict by class name of matching
    radii in metres (default ``NUSCENES_MAX_DIST``; a class that is not named gets 0: not tracked); ``max_age``: a track
    is dropped when it goes unmatched for this many frames in a row; ``min_score``: detections below it are not tracked."""

    def __init__(self, class_names, max_dist=None, max_age=3, min_score=0.0):
        names = list(class_names)
        if not names or len(names) > MAX_CLASSES or not all(isinstance(n, str) for n in names):
            raise ValueError(f'class_names: 1 to {MAX_CLASSES} strings, got {class_names!r}')
        table = NUSCENES_MAX_DIST if max_dist is None else max_dist
        if not isinstance(table, dict):
            raise TypeError(f'max_dist is a dict by class name, got {type(max_dist).__name__}')
        if max_dist is not None and set(table) - set(names):
            raise ValueError(f'max_dist names classes that are not in class_names: {sorted(set(table) - set(names))}')
        radii = [float(table.get(n, 0.0)) for n in names]
        if not all(math.isfinite(r) and r >= 0.0 for r in radii):
            raise ValueError(f'max_dist: finite radii >= 0, got {radii}')
        if isinstance(max_age, bool) or not isinstance(max_age, numbers.Integral) or max_age < 1:
            raise ValueError(f'max_age is an integer >= 1, got {max_age!r}')
        if not math.isfinite(float(min_score)):
            raise ValueError(f'min_score is finite, got {min_score!r}')
        self.class_names, self.max_dist = tuple(names), tuple(radii)
        self.max_age, self.min_score = int(max_age), float(min_score)
        self._on = {}

    @property
    def n_classes(self):
        return len(self.class_names)

    def max_dist_on(self, device):
        """The radii as a float32 tensor on ``device``, uploaded once per device."""
        if device not in self._on:
            self._on[device] = torch.tensor(self.max_dist, dtype=torch.float32, device=device)
        return self._on[device]


def default_config(det):
    """``TrackConfig`` over the classes of ``det.pts_bbox_head`` in label order, with the defaults; kept on ``det``."""
    cfg = getattr(det, '_track_cfg', None)
    if cfg is None:
        cfg = det._track_cfg = TrackConfig([n for names in det.pts_bbox_head.class_names for n in names])
    return cfg


class TrackState:
    """The tracks of B parallel sequences, allocated by the first step.  Per track (B, cap, ...), cap = max_age * M:
    ``pos`` (2) and ``vel`` (2) float64 in the global frame, ``label``, ``id``, ``misses``, ``hits`` int32; per sample
    ``count`` (B) int32, the live slots, and ``next_id`` (B) int32.  Slots past ``count`` are zero.  Every array exists
    twice: a step reads one set and writes the other, then they swap."""

    def __init__(self):
        self.shape = None                      # (B, M, D, max_age)
        self._sets, self._cur = None, 0
        self.steps = 0

    def allocate(self, B, M, D, max_age, device):
        cap = max_age * M
        self.shape, self._cur, self.steps = (B, M, D, max_age), 0, 0
        self._sets = []
        for _ in range(2):
            arrays = {name: torch.zeros((B, cap) + tail, dtype=dtype, device=device) for name, dtype, tail in _STATE}
            arrays['count'] = torch.zeros(B, dtype=torch.int32, device=device)
            arrays['next_id'] = torch.zeros(B, dtype=torch.int32, device=device)
            self._sets.append(arrays)

    def matches(self, B, M, D, max_age, device):
        return self._sets is not None and self.shape == (B, M, D, max_age) and self.count.device == device

    @property
    def cap(self):
        return self.shape[3] * self.shape[1]

    @property
    def current(self):
        """The arrays the next step reads, by name."""
        return self._sets[self._cur]

    @property
    def other(self):
        """The arrays the next step writes."""
        return self._sets[1 - self._cur]

    def swap(self):
        self._cur = 1 - self._cur
        self.steps += 1

    def __getattr__(self, name):
        if name in ('pos', 'vel', 'label', 'id', 'misses', 'hits', 'count', 'next_id'):
            sets = self.__dict__.get('_sets')
            if sets is None:
                raise AttributeError(f'{name}: the state is allocated by its first step')
            return sets[self._cur][name]
        raise AttributeError(name)

    def clone(self):
        """A copy that shares nothing with this state."""
        twin = TrackState()
        twin.shape, twin._cur, twin.steps = self.shape, self._cur, self.steps
        if self._sets is not None:
            twin._sets = [{k: v.clone() for k, v in arrays.items()} for arrays in self._sets]
        return twin


def _checked(boxes, scores, labels, counts, ego2global, cfg):
    """(B, M, D) of arguments that fit together; anything else raises before a launch."""
    if not isinstance(cfg, TrackConfig):
        raise TypeError(f'cfg is a TrackConfig, got {type(cfg).__name__}')
    named = dict(boxes=(boxes, torch.float32), scores=(scores, torch.float32), labels=(labels, torch.int32),
                 counts=(counts, torch.int32), ego2global=(ego2global, torch.float32))
    for name, (t, dtype) in named.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'{name} is a tensor, got {type(t).__name__}')
        if t.dtype != dtype:
            raise TypeError(f'{name} is {dtype}, got {t.dtype}')
        if t.device != boxes.device:
            raise ValueError(f'{name} is on {t.device}, boxes on {boxes.device}')
    if boxes.dim() != 3 or boxes.shape[2] not in (7, 9) or boxes.shape[0] < 1 or boxes.shape[1] < 1:
        raise ValueError(f'boxes is (B, M, 9 | 7) with B, M >= 1, got {tuple(boxes.shape)}')
    B, M, D = boxes.shape
    for name, t, shape in (('scores', scores, (B, M)), ('labels', labels, (B, M)), ('counts', counts, (B,)),
                           ('ego2global', ego2global, (B, 4, 4))):
        if tuple(t.shape) != shape:
            raise ValueError(f'{name} is {shape} for boxes {tuple(boxes.shape)}, got {tuple(t.shape)}')
    return B, M, D


def _time_lags(time_lag, B, device):
    """``time_lag`` as (B) float32 on ``device``: a device tensor as it is, host values from pinned memory,
    asynchronously."""
    if isinstance(time_lag, torch.Tensor):
        if time_lag.dtype != torch.float32:
            raise TypeError(f'time_lag is float32, got {time_lag.dtype}')
        if tuple(time_lag.shape) != (B,) or time_lag.device != device:
            raise ValueError(f'time_lag is ({B},) on {device}, got {tuple(time_lag.shape)} on {time_lag.device}')
        return time_lag.contiguous()
    if isinstance(time_lag, numbers.Real):
        values = [float(time_lag)] * B
    else:
        try:
            values = [float(v) for v in time_lag]
        except TypeError:
            raise TypeError(f'time_lag is a float, {B} floats or a device tensor, got {type(time_lag).__name__}') from None
        if len(values) != B:
            raise ValueError(f'time_lag has {len(values)} entries for {B} samples')
    if not all(math.isfinite(v) for v in values):
        raise ValueError(f'time_lag is finite, got {values}')
    host = torch.tensor(values, dtype=torch.float32)
    if device.type != 'cuda':
        return host.to(device)
    return host.pin_memory().to(device, non_blocking=True)


def _prepared(boxes, scores, labels, counts, ego2global, time_lag, state, new_sequence, cfg):
    """What both arms share: the checks, the state (a fresh one for another B, M, D, ``max_age`` or device) and the
    flags as a list of B bools, or None when no sample restarts."""
    B, M, D = _checked(boxes, scores, labels, counts, ego2global, cfg)
    if state is not None and not isinstance(state, TrackState):
        raise TypeError(f'state is a TrackState, got {type(state).__name__}')
    fresh = state is None or not state.matches(B, M, D, cfg.max_age, boxes.device)
    flags = _flags(new_sequence, B, False)
    lags = _time_lags(time_lag, B, boxes.device)
    if fresh:
        state = TrackState()
    return B, M, D, state, fresh, (flags if any(flags) and not fresh else None), lags


def track_step(boxes, scores, labels, counts, ego2global, time_lag, state=None, new_sequence=None, cfg=None, fused=True):
    """One tracking step for B samples on the padded decode output (``CenterHead.get_bboxes_padded``): boxes (B, M, 9 | 7)
    float32 with bottom-centre z, scores (B, M) float32, labels (B, M) int32, counts (B,) int32, ``ego2global`` (B, 4, 4)
    float32 (key ego -> global), all on one device.  ``time_lag``: seconds since each sample's previous frame, a float, B
    floats or a (B,) float32 tensor on that device.  ``new_sequence``: a host sequence of B bools, the samples whose tracks
    start over (their ids go on counting); ``state=None`` or a state of another B, M, D, ``max_age`` or device starts all.

    Returns ``(ids, hits, state)``: (B, M) int32 each, -1 and 0 for rows past the count and rows that are not tracked.
    On CUDA tensors with ``fused=True`` the step is one ``ocrf_track_step`` launch and reads nothing back; the host
    values (``time_lag``, mixed flags) go up from pinned memory, asynchronously.  CPU tensors and ``fused=False`` take
    ``track_step_host``.  Bad arguments raise ``ValueError`` / ``TypeError`` before any launch."""
    if not (fused and isinstance(boxes, torch.Tensor) and boxes.is_cuda):
        return track_step_host(boxes, scores, labels, counts, ego2global, time_lag, state=state,
                               new_sequence=new_sequence, cfg=cfg)
    B, M, D, state, fresh, flags, lags = _prepared(boxes, scores, labels, counts, ego2global, time_lag, state,
                                                   new_sequence, cfg)
    cap = cfg.max_age * M
    L = _lib.lib()
    if B > 65535 or L.ocrf_track_step_lds_bytes(M, cap) > _lib.OCRF_TRACK_MAX_LDS:
        raise ValueError(f'ocrf_track_step keeps a sample\'s rows and tracks in LDS: 32 * M + 24 * max_age * M <= '
                         f'{_lib.OCRF_TRACK_MAX_LDS} bytes and B <= 65535, got B = {B}, M = {M}, max_age = {cfg.max_age}; '
                         f'track_step_host has no such limit')
    device = boxes.device
    if fresh:
        state.allocate(B, M, D, cfg.max_age, device)
    restart = None if flags is None else _upload(flags, device)
    ids = torch.empty((B, M), dtype=torch.int32, device=device)
    hits = torch.empty((B, M), dtype=torch.int32, device=device)
    src, dst = state.current, state.other
    order = ('pos', 'vel', 'label', 'id', 'misses', 'hits', 'count', 'next_id')
    _lib.launch('ocrf_track_step', device, B, M, D, cfg.n_classes, cfg.max_age, cfg.min_score, cap, boxes.contiguous(),
                scores.contiguous(), labels.contiguous(), counts.contiguous(), ego2global.contiguous(), lags, restart,
                cfg.max_dist_on(device), *[src[k] for k in order], *[dst[k] for k in order], ids, hits)
    state.swap()
    return ids, hits, state


def track_step_host(boxes, scores, labels, counts, ego2global, time_lag, state=None, new_sequence=None, cfg=None):
    """``track_step`` by the same rules in numpy float64 on the host, bit for bit: the arm of CPU tensors and of
    ``fused=False``.  The results and the state's arrays are tensors on the detections' device.  On CUDA tensors it
    copies the detections and the state to the host and the results back, and so SYNCHRONISES with the device."""
    B, M, D, state, fresh, flags, lags = _prepared(boxes, scores, labels, counts, ego2global, time_lag, state,
                                                   new_sequence, cfg)
    if fresh:
        state.allocate(B, M, D, cfg.max_age, boxes.device)
    cap, nc = cfg.max_age * M, cfg.n_classes
    host = lambda t: t.detach().cpu().numpy()                    # noqa: E731
    boxes_h, scores_h, labels_h, counts_h, e2g, dt_h = (host(t) for t in (boxes, scores, labels, counts, ego2global, lags))
    src = {k: host(v) for k, v in state.current.items()}
    dst = {k: np.zeros_like(v) for k, v in src.items()}
    radii = np.asarray(cfg.max_dist, np.float32)
    ids = np.full((B, M), -1, np.int32)
    hits = np.zeros((B, M), np.int32)
    for b in range(B):
        n = min(max(int(counts_h[b]), 0), M)
        C = 0 if flags is not None and flags[b] else min(max(int(src['count'][b]), 0), cap)
        box, label = boxes_h[b, :n], labels_h[b, :n].astype(np.int64)
        known = (label >= 0) & (label < nc)
        radius = np.where(known, radii[np.clip(label, 0, nc - 1)], np.float32(0.0))
        tracked = known & (radius > 0) & ~(scores_h[b, :n] < np.float32(cfg.min_score)) & np.isfinite(box[:, :3]).all(1)
        if D == 9:
            tracked &= np.isfinite(box[:, 7:9]).all(1)
        E, dt = e2g[b].astype(np.float64), np.float64(dt_h[b])
        x, y, z = (box[:, k].astype(np.float64) for k in range(3))
        vx, vy = (box[:, k].astype(np.float64) for k in (7, 8)) if D == 9 else (np.zeros(n), np.zeros(n))
        with np.errstate(all='ignore'):                          # rows that are not tracked may hold anything
            gx = ((E[0, 0] * x + E[0, 1] * y) + E[0, 2] * z) + E[0, 3]
            gy = ((E[1, 0] * x + E[1, 1] * y) + E[1, 2] * z) + E[1, 3]
            vgx, vgy = E[0, 0] * vx + E[0, 1] * vy, E[1, 0] * vx + E[1, 1] * vy
            px, py = gx - vgx * dt, gy - vgy * dt
        old_label, old_pos = src['label'][b, :C], src['pos'][b, :C]
        taken = np.full(n, -1, np.int64)                         # the old slot a row claimed
        claimed = np.zeros(C, bool)
        for c in np.unique(label[tracked]):
            slots = np.flatnonzero(old_label == c)
            if slots.size == 0:
                continue
            tx, ty = old_pos[slots, 0], old_pos[slots, 1]
            free = np.ones(slots.size, bool)
            r2 = np.float64(radii[c]) * np.float64(radii[c])
            for r in np.flatnonzero(tracked & (label == c)):
                with np.errstate(all='ignore'):
                    d2 = (tx - px[r]) * (tx - px[r]) + (ty - py[r]) * (ty - py[r])
                    candidate = free & (d2 <= r2)
                if candidate.any():
                    k = int(np.argmin(np.where(candidate, d2, np.inf)))          # the first of the smallest: lowest slot
                    free[k] = False
                    taken[r], claimed[slots[k]] = slots[k], True
        rows = np.flatnonzero(tracked)
        matched = taken[rows] >= 0
        new_rank = np.cumsum(~matched) - 1
        with np.errstate(over='ignore'):
            row_id = np.where(matched, src['id'][b, np.maximum(taken[rows], 0)],
                              src['next_id'][b] + new_rank.astype(np.int32)).astype(np.int32)
            row_hits = np.where(matched, src['hits'][b, np.maximum(taken[rows], 0)] + np.int32(1),
                                np.int32(1)).astype(np.int32)
            dst['next_id'][b] = src['next_id'][b] + np.int32((~matched).sum())
        ids[b, rows], hits[b, rows] = row_id, row_hits
        stays = np.flatnonzero(~claimed & (src['misses'][b, :C] < cfg.max_age - 1))
        t, k = rows.size, stays.size
        room = max(min(cap - t, k), 0)                           # a state these rules wrote always fits
        stays = stays[:room]
        dst['pos'][b, :t, 0], dst['pos'][b, :t, 1] = gx[rows], gy[rows]
        dst['vel'][b, :t, 0], dst['vel'][b, :t, 1] = vgx[rows], vgy[rows]
        dst['label'][b, :t], dst['id'][b, :t], dst['hits'][b, :t] = label[rows], row_id, row_hits
        with np.errstate(all='ignore'):
            dst['pos'][b, t:t + room] = src['pos'][b, stays] + src['vel'][b, stays] * dt
        dst['vel'][b, t:t + room] = src['vel'][b, stays]
        dst['label'][b, t:t + room], dst['id'][b, t:t + room] = src['label'][b, stays], src['id'][b, stays]
        dst['misses'][b, t:t + room] = src['misses'][b, stays] + 1
        dst['count'][b] = t + room
    for name, array in dst.items():
        state.other[name].copy_(torch.from_numpy(array))
    state.swap()
    return torch.from_numpy(ids).to(boxes.device), torch.from_numpy(hits).to(boxes.device), state


def track_stream(det, img_inputs, state=None, tracks=None, time_lag=0.5, new_sequence=None, multi_frame=False, bf16=False,
                 track_cfg=None):
    """The body of ``OcRFDet4D.track_stream``: ``stream_step`` on one frame, the head, ``get_bboxes_padded`` and
    ``track_step`` with camera 0's ``ego2global`` of that frame.  Returns ``(dict(boxes, scores, labels, counts, ids,
    hits), state, tracks)``, the dict's tensors padded and on the device (``results_to_host`` reads them back).  From the
    second step on nothing synchronises with the host.  ``new_sequence`` resets the stream state and the tracks of the
    same samples.  ``track_cfg``: a ``TrackConfig``; default: the head's classes with ``NUSCENES_MAX_DIST``.

    Precondition: the BEV augmentation ``bda`` is the identity, as at test time, so that the decoded boxes are in the
    key frame's ego and ``ego2global`` takes them to the global frame."""
    if not det.with_pts_bbox:
        raise RuntimeError('track_stream needs a detection head (pts_bbox_head)')
    cfg = default_config(det) if track_cfg is None else track_cfg
    if not isinstance(cfg, TrackConfig):
        raise TypeError(f'track_cfg is a TrackConfig, got {type(track_cfg).__name__}')
    if tracks is not None and not isinstance(tracks, TrackState):
        raise TypeError(f'tracks is a TrackState, got {type(tracks).__name__}')
    if multi_frame:
        img_inputs = key_frame_inputs(img_inputs, det.num_frame)
    (img_feats, _, _), state = det.stream_step(img_inputs, state=state, new_sequence=new_sequence, bf16=bf16)
    head = det.pts_bbox_head
    with torch.no_grad(), (det.bf16_inference() if bf16 else contextlib.nullcontext()):
        boxes, scores, labels, counts = head.get_bboxes_padded(head(img_feats))
    ids, hits, tracks = track_step(boxes, scores, labels, counts, img_inputs[8][:, 0], time_lag, state=tracks,
                                   new_sequence=new_sequence, cfg=cfg)
    return dict(boxes=boxes, scores=scores, labels=labels, counts=counts, ids=ids, hits=hits), state, tracks


def results_to_host(result):
    """The one read-back of a ``track_stream`` result: per sample ``dict(boxes_3d, scores_3d, labels_3d, track_ids,
    track_hits)`` on the host, trimmed to the sample's count."""
    names = dict(boxes_3d='boxes', scores_3d='scores', labels_3d='labels', track_ids='ids', track_hits='hits')
    host = {k: result[k].cpu() for k in ('counts', *names.values())}
    M = host['boxes'].shape[1]
    return [{out: host[k][b, :min(max(int(n), 0), M)] for out, k in names.items()}
            for b, n in enumerate(host['counts'].tolist())]
