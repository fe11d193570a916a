"""Timing of streaming object tracking (``tracking.track_step``, ``OcRFDet4D.track_stream``).

Step, at the reference shape (M = 498 rows: six tasks of 83; the ten nuScenes classes; ``max_age`` 3) with B = 1 and
B = 8: a cycle of 8 frames of resting objects under a moving ego, 90 detections per frame drawn from 360 objects per
sample (three in ten of a class that is not tracked), which keeps about 150 tracks alive.  ``track_step`` (one launch
of ``ocrf_track_step``) alternates block by block with ``track_step_host`` on the same device tensors, whose figure
includes its copies to the host and back.

Whole detector: ``OcRFDet4D`` of the reference config (``tools/time_detector.reference_model``) at B = 1 in ``eval()`` on
a sequence of 6 frames; ``track_stream`` (everything stays on the device) alternates with ``simple_test_stream`` (the
boxes of every frame read back to the host, no identities).

Per arm: device time and launch count from the torch profiler, wall time per call from a host clock around synchronised
blocks, and the synchronising torch calls per call, counted with ``torch.cuda.set_sync_debug_mode('warn')``.  Reported
only: no ratio is fixed in advance; the acceptance conditions are structural (one launch, no synchronisation, bit
equality with the float64 oracle) and checked by the tests.

    python tools/time_track.py [--iters N] [--out profiles/track_time.txt]

Every case runs in a child process of its own under a time limit (``--limit`` seconds); the first case that fails or
runs out of time ends the run.
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = ['step', 'detector']
CLASSES = ('car', 'truck', 'construction_vehicle', 'bus', 'trailer', 'barrier', 'motorcycle', 'bicycle', 'pedestrian',
           'traffic_cone')
M, CYCLE, POOL, SEEN = 498, 8, 360, 90


def step_frames(B, dev, seed=0):
    """``CYCLE`` frames of (boxes, scores, labels, counts, ego2global) on ``dev``: POOL resting objects per sample 6 m
    apart on a grid around the ego, SEEN of them detected per frame with 0.1 m of noise, from an ego that yaws and moves
    around a nuScenes-like global position."""
    import math

    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    side = int(math.ceil(math.sqrt(POOL)))
    grid = (np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:POOL] - side / 2) * 6.0
    labels = rng.integers(0, len(CLASSES), (B, POOL)).astype(np.int32)
    frames = []
    for t in range(CYCLE):
        boxes, scores = np.zeros((B, M, 9), np.float32), np.zeros((B, M), np.float32)
        lab, counts, e2g = np.zeros((B, M), np.int32), np.full(B, SEEN, np.int32), np.zeros((B, 4, 4), np.float32)
        for b in range(B):
            yaw = 0.3 + 0.2 * b + 0.05 * math.sin(t)
            E = np.eye(4)
            E[:2, :2] = [[math.cos(yaw), -math.sin(yaw)], [math.sin(yaw), math.cos(yaw)]]
            E[:3, 3] = [612.5 + 50.0 * b + 2.0 * math.sin(0.8 * t), -1104.25 + 2.0 * math.cos(0.8 * t), 1.5]
            e2g[b] = E
            seen = rng.choice(POOL, SEEN, replace=False)
            world = E[:2, 3] + grid[seen] + rng.normal(0.0, 0.1, (SEEN, 2))
            boxes[b, :SEEN, :2] = (world - E[:2, 3]) @ E[:2, :2]
            boxes[b, :SEEN, 3:6] = (1.9, 4.5, 1.6)
            scores[b, :SEEN], lab[b, :SEEN] = rng.uniform(0.2, 0.9, SEEN), labels[b, seen]
        frames.append([torch.from_numpy(a).to(dev) for a in (boxes, scores, lab, counts, e2g)])
    return frames


def _arm(label, fn, wall, reps):
    from time_detector import _profile, _syncs
    launches, dev_ms, names = _profile(fn, reps=reps)
    return (f'{label} {dev_ms * 1e3:.1f} us device, {launches:.1f} launches, wall best {wall[0] * 1e3:.1f} / median '
            f'{wall[1] * 1e3:.1f} us, {_syncs(fn)} synchronisations'), dev_ms, names


def run_step(iters):
    import torch
    from time_bev_encoder import _wall
    from ocrfdet_amd import tracking
    dev = torch.device('cuda:0')
    cfg = tracking.TrackConfig(CLASSES)
    for B in (1, 8):
        frames = step_frames(B, dev)
        lag = torch.full((B,), 0.5, device=dev)
        clock = dict(fused=0, host=0, fused_state=None, host_state=None)

        def arm(key, step):
            def fn():
                t = clock[key] % CYCLE
                clock[key] += 1
                ids, hits, clock[key + '_state'] = step(*frames[t], lag, state=clock[key + '_state'], cfg=cfg)
                return ids
            return fn
        fused, host = arm('fused', tracking.track_step), arm('host', tracking.track_step_host)
        same = True
        for _ in range(2 * CYCLE):
            same = same and bool(torch.equal(fused(), host()))
        torch.cuda.synchronize()
        live = clock['fused_state'].count.tolist()
        walls = _wall([fused, host], iters)
        texts = [_arm(label, fn, wall, CYCLE) for label, fn, wall in zip(('track_step', 'track_step_host'), (fused, host),
                                                                         walls)]
        print(f'track step, B = {B}, M = {M}, {len(CLASSES)} classes, {SEEN} detections per frame, live tracks {live}: '
              + ' | '.join(t[0] for t in texts) + f' | host / fused wall median {walls[1][1] / walls[0][1]:.1f}x | same ids '
              f'over {2 * CYCLE} frames: {same}')


def run_detector(iters):
    import random

    import torch
    from time_bev_encoder import _wall
    from time_detector import INPUT_SIZE, N_CAMS, _profile, _syncs, reference_model
    from time_stream import SEQUENCE, frames_of
    from ocrfdet_amd import detector
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    det = detector.OcRFDet4D(**reference_model()).to(dev).eval()
    frames = frames_of(SEQUENCE, 1, N_CAMS, INPUT_SIZE, dev)
    clock = dict(track=0, plain=0, track_state=(None, None), plain_state=None)

    def track():
        random.seed(0)
        t = clock['track'] % SEQUENCE
        clock['track'] += 1
        state, tracks = clock['track_state']
        result, state, tracks = det.track_stream(frames[t], state=state, tracks=tracks, time_lag=0.5)
        clock['track_state'] = (state, tracks)
        return result

    def plain():
        random.seed(0)
        t = clock['plain'] % SEQUENCE
        clock['plain'] += 1
        results, clock['plain_state'] = det.simple_test_stream(frames[t], state=clock['plain_state'])
        return results
    for fn in (track, plain):
        for _ in range(SEQUENCE):
            fn()
    (tb, tm), (pb, pm) = _wall([track, plain], iters, blocks=3)
    tl, td, _ = _profile(track, reps=SEQUENCE)
    pl, pd, _ = _profile(plain, reps=SEQUENCE)
    result = track()
    torch.cuda.synchronize()
    print(f'OcRFDet4D, reference config, B = 1, a sequence of {SEQUENCE} frames, {int(result["counts"][0])} boxes in the '
          f'last: track_stream {td:.2f} ms device, {tl:.0f} launches, wall best {tb:.2f} / median {tm:.2f} ms, '
          f'{_syncs(track)} synchronisations | simple_test_stream {pd:.2f} ms device, {pl:.0f} launches, wall best {pb:.2f} '
          f'/ median {pm:.2f} ms, {_syncs(plain)} synchronisations | track_stream / simple_test_stream wall median '
          f'{tm / pm:.3f}x')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--limit', type=int, default=300, help='seconds per case')
    ap.add_argument('--case', type=int, default=None, help='(internal) run this one case in this process')
    a = ap.parse_args()
    if a.case is not None:
        import torch
        assert torch.cuda.is_available(), 'timing needs the GPU: there is no CPU fallback for a measurement'
        if a.case == 0:
            run_step(a.iters * 10)
        else:
            from time_stream import SEQUENCE
            run_detector(SEQUENCE * max(a.iters // 10, 1))
        return 0
    lines = []
    for k in range(len(CASES)):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', str(k), '--iters', str(a.iters)],
                               stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f'case {CASES[k]} ran out of its {a.limit} s: stopping', file=sys.stderr)
            return 124
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f'case {CASES[k]} ended with status {p.returncode}: stopping', file=sys.stderr)
            return p.returncode or 1
        lines.append(p.stdout)
    if a.out:
        import torch
        with open(a.out, 'w') as f:
            f.write(f'torch {torch.__version__}; one MI355X; the arms alternating block by block; device time and launches '
                    'from the torch profiler; synchronisations: warnings of torch.cuda.set_sync_debug_mode\n'
                    + ''.join(lines))
    return 0


if __name__ == '__main__':
    sys.exit(main())
