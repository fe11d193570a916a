"""The float64 oracle of the streaming tracker (include/ocrf_hip.h, "Streaming object tracking") and the scenes its tests
share.  The oracle is sequential plain Python, one detection at a time in row order over ALL classes, on Python floats
(IEEE float64, one operation per expression node, no contraction); it shares no code with ``ocrfdet_amd/tracking.py``.

``Oracle.step`` takes numpy arrays of one frame and returns ``(ids, hits)``; ``Oracle.arrays`` is the state as the
package lays it out (zeros past a sample's count), for bit comparison.
"""
import math

import numpy as np

CLASSES = ('car', 'truck', 'construction_vehicle', 'bus', 'trailer', 'barrier', 'motorcycle', 'bicycle', 'pedestrian',
           'traffic_cone')
# the default table over CLASSES, written out (not imported): classes 2, 5 and 9 are not tracked
MAX_DIST = (4.0, 4.0, 0.0, 5.5, 3.0, 0.0, 13.0, 3.0, 1.0, 0.0)
TRACKED = (0, 1, 3, 4, 6, 7, 8)
B, M, MAX_AGE, FRAMES = 3, 40, 3, 7


class Oracle:
    def __init__(self, B, M, max_dist=MAX_DIST, max_age=MAX_AGE, min_score=0.0):
        self.B, self.M, self.max_age = B, M, max_age
        self.radius = [float(np.float32(r)) for r in max_dist]
        self.min_score = np.float32(min_score)
        self.tracks = [[] for _ in range(B)]         # per sample: dicts in slot order
        self.next_id = [0] * B

    def step(self, boxes, scores, labels, counts, ego2global, time_lag, new_sequence=None):
        B, M, D = boxes.shape
        assert (B, M) == (self.B, self.M) and D in (7, 9)
        ids, hits = np.full((B, M), -1, np.int32), np.zeros((B, M), np.int32)
        for b in range(B):
            E = [[float(ego2global[b, i, j]) for j in range(4)] for i in range(2)]
            dt = float(np.float32(time_lag[b]))
            old = [] if new_sequence is not None and new_sequence[b] else self.tracks[b]
            claimed = [False] * len(old)
            new, fresh = [], 0
            for r in range(min(max(int(counts[b]), 0), M)):
                label = int(labels[b, r])
                if not 0 <= label < len(self.radius) or self.radius[label] <= 0.0 or scores[b, r] < self.min_score:
                    continue
                used = list(boxes[b, r, :3]) + (list(boxes[b, r, 7:9]) if D == 9 else [])
                if not all(math.isfinite(float(v)) for v in used):
                    continue
                x, y, z = (float(v) for v in boxes[b, r, :3])
                vx, vy = (float(boxes[b, r, 7]), float(boxes[b, r, 8])) if D == 9 else (0.0, 0.0)
                gx = ((E[0][0] * x + E[0][1] * y) + E[0][2] * z) + E[0][3]
                gy = ((E[1][0] * x + E[1][1] * y) + E[1][2] * z) + E[1][3]
                vgx = E[0][0] * vx + E[0][1] * vy
                vgy = E[1][0] * vx + E[1][1] * vy
                px = gx - vgx * dt
                py = gy - vgy * dt
                radius = self.radius[label]
                best, best_d2 = None, None
                for s, t in enumerate(old):
                    if t['label'] != label or claimed[s]:
                        continue
                    d2 = (t['x'] - px) * (t['x'] - px) + (t['y'] - py) * (t['y'] - py)
                    if d2 <= radius * radius and (best is None or d2 < best_d2):
                        best, best_d2 = s, d2
                if best is None:
                    track_id, track_hits = self.next_id[b] + fresh, 1
                    fresh += 1
                else:
                    claimed[best] = True
                    track_id, track_hits = old[best]['id'], old[best]['hits'] + 1
                ids[b, r], hits[b, r] = track_id, track_hits
                new.append(dict(x=gx, y=gy, vx=vgx, vy=vgy, label=label, id=track_id, misses=0, hits=track_hits))
            for s, t in enumerate(old):
                if not claimed[s] and t['misses'] + 1 < self.max_age:
                    new.append(dict(x=t['x'] + t['vx'] * dt, y=t['y'] + t['vy'] * dt, vx=t['vx'], vy=t['vy'],
                                    label=t['label'], id=t['id'], misses=t['misses'] + 1, hits=0))
            assert len(new) <= self.max_age * M
            self.tracks[b], self.next_id[b] = new, self.next_id[b] + fresh
        return ids, hits

    def arrays(self):
        cap = self.max_age * self.M
        out = dict(pos=np.zeros((self.B, cap, 2)), vel=np.zeros((self.B, cap, 2)),
                   **{k: np.zeros((self.B, cap), np.int32) for k in ('label', 'id', 'misses', 'hits')},
                   count=np.array([len(t) for t in self.tracks], np.int32), next_id=np.array(self.next_id, np.int32))
        for b, tracks in enumerate(self.tracks):
            for s, t in enumerate(tracks):
                out['pos'][b, s], out['vel'][b, s] = (t['x'], t['y']), (t['vx'], t['vy'])
                for k in ('label', 'id', 'misses', 'hits'):
                    out[k][b, s] = t[k]
        return out


def same_bits(got, want):
    """``got`` equals ``want`` bit for bit (numpy arrays of one dtype and shape)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    as_int = {1: np.uint8, 4: np.int32, 8: np.int64}[got.dtype.itemsize]
    return bool(np.array_equal(got.view(as_int), want.view(as_int)))


# ---------------------------------------------------------------------------------------------------------------- scenes
def ego_pose(t, b):
    """ego -> global of sample ``b`` at frame ``t`` as float32 (4, 4): a yaw that turns and a translation that moves
    around (2000, 1000) m, nuScenes-like."""
    yaw = 0.4 + 0.7 * b + 0.11 * t
    E = np.eye(4)
    E[:2, :2] = [[math.cos(yaw), -math.sin(yaw)], [math.sin(yaw), math.cos(yaw)]]
    E[:3, 3] = [2000.0 + 40.0 * b + 3.5 * t, 1000.0 - 25.0 * b + 1.25 * t * t, 1.5]
    return E.astype(np.float32)


def in_ego(E32, xy, z, vxy):
    """Global centres (K, 2), heights (K) and velocities (K, 2) seen from the ego of the float32 pose ``E32``: float32."""
    E = E32.astype(np.float64)
    R, t = E[:2, :2], E[:2, 3]
    p = (xy - t) @ R                                   # R^T (g - t), row-wise
    v = vxy @ R
    return p.astype(np.float32), (z - E[2, 3]).astype(np.float32), v.astype(np.float32)


def rows(E32, xy, z, vxy, labels, scores, M, D, order):
    """One sample's padded rows from global objects, in the row order ``order`` (indices into the objects)."""
    p, zz, v = in_ego(E32, xy[order], z[order], vxy[order])
    n = len(order)
    boxes = np.zeros((M, D), np.float32)
    boxes[:n, :2], boxes[:n, 2] = p, zz
    boxes[:n, 3:6], boxes[:n, 6] = (1.9, 4.5, 1.6), 0.3
    if D == 9:
        boxes[:n, 7:9] = v
    lab, sc = np.zeros(M, np.int32), np.zeros(M, np.float32)
    lab[:n], sc[:n] = labels[order], scores[order]
    return boxes, sc, lab, n


def sequence(seed, per_sample, D=9, frames=FRAMES, time_lag=(0.5, 0.25, 1.0), B=B, M=M):
    """``frames`` frames of B samples.  ``per_sample(b, rng)`` gives a sample's world: ``dict(xy (K, 2) offsets from the
    first ego position, vxy (K, 2), labels (K), seen)``, ``seen(t, rng)`` the indices of the objects detected at frame t
    in row order (at most M).  Objects move with their velocity; centres get 0.05 m of detection noise."""
    rng = np.random.default_rng(seed)
    worlds = [per_sample(b, rng) for b in range(B)]
    out = []
    for t in range(frames):
        frame = dict(boxes=np.zeros((B, M, D), np.float32), scores=np.zeros((B, M), np.float32),
                     labels=np.zeros((B, M), np.int32), counts=np.zeros(B, np.int32),
                     ego2global=np.stack([ego_pose(t, b) for b in range(B)]),
                     time_lag=np.asarray(time_lag, np.float32), new_sequence=None)
        for b, w in enumerate(worlds):
            order = np.asarray(w['seen'](t, rng), np.int64)
            assert len(order) <= M
            K = len(w['labels'])
            origin = ego_pose(0, b)[:2, 3].astype(np.float64)
            now = origin + w['xy'] + w['vxy'] * (float(time_lag[b]) * t) + rng.normal(0.0, 0.05, (K, 2))
            scores = rng.uniform(0.3, 0.9, K).astype(np.float32)
            frame['boxes'][b], frame['scores'][b], frame['labels'][b], frame['counts'][b] = rows(
                frame['ego2global'][b], now, rng.uniform(0.0, 2.0, K), w['vxy'], w['labels'], scores, M, D, order)
        out.append(frame)
    return out


def crowd(b, rng, pool=440, cars=400):
    """``pool`` objects on a jittered 3 m grid (closer than a car's 4 m radius: neighbours contend), moving slowly; 30 of
    a frame's 40 rows are cars drawn from ``cars`` of them (so the live cars pass 64), the rest from the other tracked
    classes."""
    side = int(math.ceil(math.sqrt(pool)))
    grid = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:pool] * 3.0 - 1.5 * side
    labels = np.array([0] * cars + [TRACKED[1 + k % 6] for k in range(pool - cars)], np.int32)
    world = dict(xy=grid + rng.normal(0.0, 0.4, (pool, 2)), vxy=rng.normal(0.0, 1.0, (pool, 2)), labels=labels)
    world['seen'] = lambda t, rng: rng.permutation(np.concatenate([rng.choice(cars, 30, replace=False),
                                                                    cars + rng.choice(pool - cars, 10, replace=False)]))
    return world


def run(frames, B=B, M=M, max_age=MAX_AGE, min_score=0.0):
    """The oracle over ``frames``: per frame ``(ids, hits, arrays)``."""
    oracle = Oracle(B, M, max_age=max_age, min_score=min_score)
    out = []
    for f in frames:
        ids, hits = oracle.step(f['boxes'], f['scores'], f['labels'], f['counts'], f['ego2global'], f['time_lag'],
                                f['new_sequence'])
        out.append((ids, hits, oracle.arrays()))
    return out


def apart(b, rng, count, seen, spacing=30.0):
    """``count`` static objects ``spacing`` metres apart on a line (beyond twice the largest radius), labels cycling
    through the tracked classes; ``seen(t)``: the objects detected at frame t.  The row orders are kept in ``orders``."""
    world = dict(xy=np.stack([spacing * np.arange(count) - 60.0, 7.0 * np.ones(count)], 1), vxy=np.zeros((count, 2)),
                 labels=np.array([TRACKED[k % len(TRACKED)] for k in range(count)], np.int32), orders=[])

    def detected(t, rng):
        order = rng.permutation(np.asarray(seen(t), np.int64))
        world['orders'].append(order)
        return order
    world['seen'] = detected
    return world


def scene_crowd():
    return dict(frames=sequence(1, crowd))


def scene_counts():
    """Sample 0 holds nothing, sample 1 is full, sample 2 partly filled; the rows past a count hold detections that must
    not be read, and a count below 0 or above M is clamped."""
    frames = sequence(2, crowd)
    for t, f in enumerate(frames):
        f['counts'][:] = (0, M, 17)
    frames[1]['counts'][0], frames[2]['counts'][1] = -3, M + 7
    return dict(frames=frames)


def scene_static():
    worlds = []

    def world(b, rng):
        worlds.append(apart(b, rng, 12, lambda t: range(12)))
        return worlds[-1]
    return dict(frames=sequence(3, world), worlds=worlds)


def scene_all_new():
    return dict(frames=sequence(4, lambda b, rng: apart(b, rng, M * FRAMES, lambda t: range(M * t, M * (t + 1)))))


def scene_missed():
    """Object 0 is missed at frames 1 and 2 (max_age - 1 frames) and found again at 3; object 1 is missed at frames 1 to
    3 (max_age frames) and comes back at 4; objects 2 to 5 are always seen."""
    worlds = []
    shown = lambda t: [k for k in range(6) if not (k == 0 and t in (1, 2)) and not (k == 1 and t in (1, 2, 3))]  # noqa: E731

    def world(b, rng):
        worlds.append(apart(b, rng, 6, shown))
        return worlds[-1]
    return dict(frames=sequence(5, world), worlds=worlds)


UNTRACKED_ROWS = range(1, 12)


def scene_untracked():
    """The crowd with ``min_score = 0.4`` (a third of its scores lie below) and eleven rows per frame that are not
    tracked, each for one reason."""
    frames = sequence(6, crowd)
    for f in frames:
        f['labels'][:, 1], f['labels'][:, 2], f['labels'][:, 3] = -1, 10, 2
        f['boxes'][:, 4, 0], f['boxes'][:, 5, 1], f['boxes'][:, 6, 2] = np.nan, np.inf, -np.inf
        f['boxes'][:, 7, 7], f['boxes'][:, 8, 8] = np.nan, np.inf
        f['scores'][:, 9] = 0.1
        f['labels'][:, 10], f['labels'][:, 11] = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    return dict(frames=frames, min_score=0.4)


def scene_restart():
    frames = sequence(7, crowd)
    frames[3]['new_sequence'] = [False, True, False]
    return dict(frames=frames)


def scene_d7():
    return dict(frames=sequence(8, crowd, D=7))


SCENES = dict(crowd=scene_crowd, counts=scene_counts, static=scene_static, all_new=scene_all_new, missed=scene_missed,
              untracked=scene_untracked, restart=scene_restart, d7=scene_d7)
_CACHE = {}


def scene(name):
    """The scene ``name`` with the oracle's per-frame results under ``want``: built once, shared, not to be changed."""
    if name not in _CACHE:
        s = SCENES[name]()
        s.setdefault('min_score', 0.0)
        s['want'] = run(s['frames'], min_score=s['min_score'])
        _CACHE[name] = s
    return _CACHE[name]


def check_scene(name):
    """What a scene is there to show, asserted on the oracle's own results (the tests compare the package to them)."""
    s = scene(name)
    frames, want = s['frames'], s['want']
    if name == 'crowd':
        cars = max(int((arrays['label'][b, :arrays['count'][b]] == 0).sum()) for _, _, arrays in want for b in range(B))
        assert cars > 64, cars                                    # a lane walks more than one track of the class
    elif name == 'counts':
        for ids, hits, arrays in want:
            assert (ids[0] == -1).all() and arrays['count'][0] == 0 and arrays['next_id'][0] == 0
            assert (ids[1] >= 0).all() and (ids[2, 17:] == -1).all() and (ids[2, :17] >= 0).all()
    elif name in ('static', 'missed'):
        for b, w in enumerate(s['worlds']):
            by_object = [dict(zip(order.tolist(), zip(ids[b].tolist(), hits[b].tolist())))
                         for order, (ids, hits, _) in zip(w['orders'], want)]
            if name == 'static':
                for k in range(12):                               # the ego moves, the object keeps its id
                    assert [f[k] for f in by_object] == [(by_object[0][k][0], t + 1) for t in range(FRAMES)], (b, k)
            else:
                first = by_object[0]
                assert by_object[3][0] == (first[0][0], 1)        # found again after max_age - 1 misses: same id, hits 1
                assert by_object[4][1][0] not in [i for i, _ in first.values()] and by_object[4][1][1] == 1
                assert by_object[4][1][0] == want[3][2]['next_id'][b]
                assert all(by_object[t][5] == (first[5][0], t + 1) for t in range(FRAMES))
    elif name == 'all_new':
        for t, (ids, hits, arrays) in enumerate(want):
            assert arrays['count'].tolist() == [min(t + 1, MAX_AGE) * M] * B
            assert (hits == 1).all() and (ids == np.arange(M * t, M * (t + 1))).all()
    elif name == 'untracked':
        for (ids, hits, _), f in zip(want, frames):
            for r in UNTRACKED_ROWS:
                assert (ids[:, r] == -1).all() and (hits[:, r] == 0).all(), r
            low = f['scores'] < np.float32(0.4)
            assert low[:, 12:].any() and (ids[low] == -1).all() and (ids[:, 12:][~low[:, 12:]] >= 0).all()
    elif name == 'restart':
        before, (ids, hits, arrays) = want[2][2], want[3]
        assert (ids[1] >= before['next_id'][1]).all() and (hits[1] == 1).all()
        assert arrays['count'][1] == M and arrays['next_id'][1] == before['next_id'][1] + M
        assert (hits[0] > 1).any() and (hits[2] > 1).any()
    elif name == 'd7':
        assert frames[0]['boxes'].shape[2] == 7 and (want[-1][1] > 1).any()
        assert all((arrays['vel'] == 0).all() for _, _, arrays in want)
