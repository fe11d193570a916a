"""Timing of the on-device nuScenes detection metrics (``detection_eval.DetectionEval``, ``OcRFDet4D.evaluate_stream``).

Update, at the reference shape (M = 498 rows: six tasks of 83; the ten nuScenes classes; G = 64 padded ground-truth
boxes) with B = 1 and B = 8: about 90 detections and 35 ground-truth boxes per sample, two in three detections within
2 m of a box of their class.  ``update`` (one launch of ``ocrf_det_eval_match``) alternates block by block with the host
arm on the same device tensors: the copies to the host and ``match_sample_host`` per sample, which is what
``evaluate_host`` does per batch.

Compute, at 600 and at 6 019 accumulated samples (the validation split's size): ``compute()`` (one call of
``ocrf_det_eval_summary``) alternates with ``summarise_host`` on the records copied from the device, measured at both
sizes, nothing scaled.

Whole detector: ``OcRFDet4D`` of the reference config (``tools/time_detector.reference_model``) at B = 1 in ``eval()`` on
a sequence of 6 frames; ``evaluate_stream`` (one frame per call, everything stays on the device) alternates with
``simple_test_stream`` (the boxes of every frame read back to the host, no metrics).

Per arm: device time and launch count from the torch profiler, wall time per call from a host clock around synchronised
blocks, and the synchronising torch calls per call, counted with ``torch.cuda.set_sync_debug_mode('warn')``.  Reported
only: no ratio is fixed in advance; the acceptance conditions are structural and checked by the tests.

    python tools/time_eval.py [--iters N] [--out profiles/eval_time.txt]

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

CASES = ['update', 'compute', 'detector']
CLASSES = ('car', 'truck', 'construction_vehicle', 'bus', 'trailer', 'barrier', 'motorcycle', 'bicycle', 'pedestrian',
           'traffic_cone')
M, G, SEEN, TRUTH, CYCLE = 498, 64, 90, 35, 8


def batches_of(B, dev, n_classes=len(CLASSES), m=M, seed=0):
    """``CYCLE`` batches of ``update`` arguments on ``dev``: TRUTH boxes per sample within 28 m, SEEN detections, two in
    three of them a box's class and centre with 0.5 m of noise, the others anywhere."""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(CYCLE):
        boxes, scores = np.zeros((B, m, 9), np.float32), np.zeros((B, m), np.float32)
        labels, counts = np.zeros((B, m), np.int32), np.full(B, SEEN, np.int32)
        gt_boxes, gt_labels = np.zeros((B, G, 9), np.float32), np.zeros((B, G), np.int32)
        gt_counts, gt_attrs = np.full(B, TRUTH, np.int32), np.full((B, G), -1, np.int32)
        for b in range(B):
            gt_boxes[b, :TRUTH, :2] = rng.uniform(-20.0, 20.0, (TRUTH, 2))
            gt_boxes[b, :TRUTH, 3:6] = rng.uniform(0.5, 4.5, (TRUTH, 3))
            gt_boxes[b, :TRUTH, 6:9] = rng.uniform(-1.0, 1.0, (TRUTH, 3))
            gt_labels[b, :TRUTH] = rng.integers(0, n_classes, TRUTH)
            gt_attrs[b, :TRUTH] = rng.integers(-1, 8, TRUTH)
            near = rng.integers(0, TRUTH, SEEN)
            hit = rng.uniform(size=SEEN) < 2.0 / 3.0
            boxes[b, :SEEN] = gt_boxes[b, near]
            boxes[b, :SEEN, :2] += rng.normal(0.0, 0.5, (SEEN, 2))
            boxes[b, :SEEN, :2] = np.where(hit[:, None], boxes[b, :SEEN, :2], rng.uniform(-25.0, 25.0, (SEEN, 2)))
            labels[b, :SEEN] = np.where(hit, gt_labels[b, near], rng.integers(0, n_classes, SEEN))
            scores[b, :SEEN] = np.sort(rng.uniform(0.1, 0.9, SEEN))[::-1]
        arrays = (boxes, scores, labels, counts, gt_boxes, gt_labels, gt_counts, gt_attrs)
        out.append([torch.from_numpy(a).to(dev) for a in arrays])
    return out


def _arm(label, fn, wall, reps, unit=1e3, name='us'):
    from time_detector import _profile, _syncs
    launches, dev_ms, _ = _profile(fn, reps=reps)
    return (f'{label} {dev_ms * unit:.1f} {name} device, {launches:.1f} launches, wall best {wall[0] * unit:.1f} / median '
            f'{wall[1] * unit:.1f} {name}, {_syncs(fn)} synchronisations')


def run_update(iters):
    import torch
    from time_bev_encoder import _wall
    from ocrfdet_amd import detection_eval as de
    dev = torch.device('cuda:0')
    cfg = de.EvalConfig(CLASSES)
    for B in (1, 8):
        batches = batches_of(B, dev)
        ev = de.DetectionEval(cfg, 4096, M, G, dev)
        clock = dict(fused=0, host=0)

        def fused():
            if ev.n_samples + B > ev.capacity:
                ev.reset()                            # a host counter: nothing is cleared on the device
            ev.update(*batches[clock['fused'] % CYCLE])
            clock['fused'] += 1

        def host():
            arrays = [t.cpu().numpy() for t in batches[clock['host'] % CYCLE]]
            clock['host'] += 1
            return [de.match_sample_host(cfg, *(a[b] for a in arrays)) for b in range(B)]
        for _ in range(CYCLE):
            fused()
        host()
        walls = _wall([fused, host], iters, blocks=3)
        texts = [_arm('update', fused, walls[0], CYCLE), _arm('host arm (copies + match_sample_host)', host, walls[1], 2)]
        print(f'update, B = {B}, M = {M}, G = {G}, {len(CLASSES)} classes, {SEEN} detections and {TRUTH} boxes per sample, '
              f'{ev.bytes_per_sample} buffer bytes per sample: ' + ' | '.join(texts)
              + f' | host / update wall median {walls[1][1] / walls[0][1]:.0f}x')


def run_compute(iters):
    import numpy as np
    import torch
    from time_bev_encoder import _wall
    from ocrfdet_amd import detection_eval as de
    dev = torch.device('cuda:0')
    cfg = de.EvalConfig(CLASSES)
    for n_samples in (600, 6019):
        ev = de.DetectionEval(cfg, n_samples, M, G, dev)
        batches, ones = batches_of(8, dev), batches_of(1, dev, seed=1)
        k = 0
        while ev.n_samples + 8 <= n_samples:
            ev.update(*batches[k % CYCLE])
            k += 1
        while ev.n_samples < n_samples:
            ev.update(*ones[k % CYCLE])
            k += 1
        n = n_samples * M

        def fused():
            return ev.compute()['result']

        def host():
            key = ev.rec_key[:n].cpu().numpy().view(np.uint32)
            return de.summarise_host(cfg, key, ev.rec_info[:n].cpu().numpy(), ev.rec_err[:n].cpu().numpy(),
                                     ev.gt_count.cpu().numpy())['result']
        got, want = fused().cpu().numpy(), host()
        worst = float(np.nanmax(np.abs(got - want)))
        walls = _wall([fused, host], iters, blocks=3)
        texts = [_arm('compute', fused, walls[0], 3, 1.0, 'ms'), _arm('summarise_host (copies included)', host, walls[1], 1,
                                                                       1.0, 'ms')]
        total = sum(t.numel() * t.element_size() for t in (ev.rec_key, ev.rec_info, ev.rec_match, ev.rec_err, ev.gt_count))
        print(f'compute, {n_samples} samples of M = {M} ({n} slots, {total / 2 ** 20:.0f} MiB of records, '
              f'{ev._workspace.numel() / 2 ** 20:.0f} MiB of workspace): ' + ' | '.join(texts)
              + f' | host / compute wall median {walls[1][1] / walls[0][1]:.1f}x | NDS {got[-1]:.4f}, largest difference '
              f'between the arms over the result vector {worst:.1e}')


def run_detector(iters):
    import random

    import torch
    from time_bev_encoder import _wall
    from time_detector import INPUT_SIZE, N_CAMS, _profile, _syncs, reference_model
    from time_stream import SEQUENCE, frames_of
    from ocrfdet_amd import detection_eval as de, detector
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    det = detector.OcRFDet4D(**reference_model()).to(dev).eval()
    frames = frames_of(SEQUENCE, 1, N_CAMS, INPUT_SIZE, dev)
    names = [n for task in det.pts_bbox_head.class_names for n in task]
    cfg = de.EvalConfig(names)
    with torch.no_grad():
        (feats, _, _), _ = det.stream_step(frames[0])
        m = det.pts_bbox_head.get_bboxes_padded(det.pts_bbox_head(feats))[0].shape[1]
    ev = de.DetectionEval(cfg, 1024, m, G, dev)
    keys = ('gt_boxes', 'gt_labels', 'gt_counts', 'gt_attrs')
    gts = [dict(zip(keys, batch[4:])) for batch in batches_of(1, dev, n_classes=len(names), m=m)]
    clock = dict(evaluate=0, plain=0, evaluate_state=None, plain_state=None)

    def evaluate():
        random.seed(0)
        t = clock['evaluate'] % SEQUENCE
        clock['evaluate'] += 1
        if ev.n_samples + 1 > ev.capacity:
            ev.reset()
        _, clock['evaluate_state'] = det.evaluate_stream([(frames[t], gts[t % CYCLE])], ev, state=clock['evaluate_state'])

    def plain():
        random.seed(0)
        t = clock['plain'] % SEQUENCE
        clock['plain'] += 1
        results, clock['plain_state'] = det.simple_test_stream(frames[t], state=clock['plain_state'])
        return results
    for fn in (evaluate, plain):
        for _ in range(SEQUENCE):
            fn()
    (eb, em), (pb, pm) = _wall([evaluate, plain], iters, blocks=3)
    el, ed, _ = _profile(evaluate, reps=SEQUENCE)
    pl, pd, _ = _profile(plain, reps=SEQUENCE)
    torch.cuda.synchronize()
    print(f'OcRFDet4D, reference config, B = 1, a sequence of {SEQUENCE} frames, M = {m}: evaluate_stream {ed:.2f} ms '
          f'device, {el:.0f} launches, wall best {eb:.2f} / median {em:.2f} ms, {_syncs(evaluate)} synchronisations | '
          f'simple_test_stream {pd:.2f} ms device, {pl:.0f} launches, wall best {pb:.2f} / median {pm:.2f} ms, '
          f'{_syncs(plain)} synchronisations | evaluate_stream / simple_test_stream wall median {em / pm:.3f}x')


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
            run_update(a.iters)
        elif a.case == 1:
            run_compute(max(a.iters // 10, 1))
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
