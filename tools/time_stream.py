"""Timing of streaming inference (``OcRFDet4D.stream_step``, ``temporal.stream_align``).

Align, at (1, 80, 128, 128) maps with K = 1 and K = 7 adjacent frames: ``stream_align`` on a ring of the K + 1 maps (one
launch of ``ocrf_bev_stream_align``, the transforms evaluated inside) against ``align_and_cat`` on the same maps and the
``sensor2keyegos`` of the same poses (one ``feature_transform`` and one warp launch per adjacent frame, a copy of the key
frame): the transforms are included in both.

Whole detector: ``OcRFDet4D`` of the reference config (``tools/time_detector.reference_model``: ResNet-50, 6 cameras of
256 x 704, a 128 x 128 BEV, ``num_adj`` 1) at B = 1 in ``eval()``, on a sequence of 6 frames (one rig, the ego moving as
``synthetic.ego_motion``).  The streaming step (one frame per call, the state carried along, the sequence repeated)
alternates block by block with the batch forward of the parent formulation (``extract_img_feat`` on the frames
(t, t - 1, t - 2) per call).

Per arm: device time and launch count from the torch profiler, wall time per call from a host clock around synchronised
blocks, and the synchronising torch calls per call, counted with ``torch.cuda.set_sync_debug_mode('warn')``.  Reported
only; the acceptance conditions are structural (one launch for the alignment, one encoder pass and no synchronisation per
step) and checked by the tests.

    python tools/time_stream.py [--iters N] [--out profiles/stream_time.txt]
    python tools/time_stream.py --bf16 [--iters N] [--out profiles/stream_bf16_time.txt]

``--bf16`` times bfloat16 streaming instead, in the same way.  Align, on the same maps rounded to bfloat16:
``stream_align(keep_bf16=True)`` (one launch of ``ocrf_bev_stream_align_bf16``) against the float32 kernel on the float32
ring and against ``stream_align_torch`` on the bfloat16 ring, which is where a bfloat16 ring goes without the keyword.
Whole detector, three arms alternating, each with a state of its own: (a) ``stream_step(bf16=True)``, (b) the float32
``stream_step``, (c) ``stream_step`` under plain ``torch.autocast('cuda', torch.bfloat16)`` with every switch at its
default.  Decode: ``CenterHead.get_bboxes_padded`` at B = 1 on the bfloat16 head outputs of a bf16 step, with and
without ``fused_decode_bf16``.

Every case runs in a child process of its own under a time limit (``--limit`` seconds); the first case that fails or
runs out of time ends the run.
"""
import argparse
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = ['align', 'detector']
CASES_BF16 = ['align_bf16', 'detector_bf16']
SEQUENCE = 6


def global_pose():
    import numpy as np
    yaw = math.radians(35.0)
    G = np.eye(4)
    G[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]]
    G[:3, 3] = [612.5, -1104.25, 2.5]
    return G


def frames_of(count, B, n_cams, input_size, dev, seed=0):
    """``count`` single-frame 12-entry lists, oldest first: the synthetic rig in every frame, frame t taken
    ``count - 1 - t`` steps of ``synthetic.ego_motion`` behind the last one."""
    import numpy as np
    import torch
    from ocrfdet_amd import synthetic
    H, W = input_size
    gen = torch.Generator().manual_seed(seed)
    rig = synthetic.rig(n_cams, input_size, B)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))      # noqa: E731
    G = global_pose()
    frames = []
    for t in range(count):
        e2g = t32(G @ synthetic.ego_motion(count - 1 - t)).view(1, 1, 4, 4).expand(B, n_cams, 4, 4).contiguous()
        raw = torch.rand(B, n_cams, 3, H, W, generator=gen) * 255
        frame = [(raw - 120.0) / 58.0] + [t32(rig[k]) for k in ('rots', 'trans', 'intrins', 'post_rots', 'post_trans')]
        frame += [t32(rig['bda']), t32(rig['c2w']), e2g, raw, raw.clone(), t32(rig['c2w'])]
        frames.append([e.to(dev) for e in frame])
    return frames


def batch_inputs(frames, ids):
    """The multi-frame ``img_inputs`` of the frames ``ids`` (key frame first): images camera-major, poses frame-major."""
    import torch
    B = frames[0][0].shape[0]
    out = []
    for k in range(12):
        if k == 6:
            out.append(frames[ids[0]][6])
        else:
            e = torch.stack([frames[i][k] for i in ids], 2 if k in (0, 9, 10) else 1)
            out.append(e.reshape(B, -1, *e.shape[3:]).contiguous())
    return out


def run_align(iters):
    import numpy as np
    import torch
    from time_bev_encoder import _wall
    from time_detector import _profile, _syncs
    from ocrfdet_amd import detector, synthetic, temporal
    dev = torch.device('cuda:0')
    B, C, H, W = 1, 80, 128, 128
    interval, lower = (0.8, 0.8, 8.0), (-51.2, -51.2, -5.0)
    for K in (1, 7):
        S = K + 1
        gen = torch.Generator().manual_seed(K)
        ring = torch.randn(S, B, C, H, W, generator=gen).to(dev)
        rig = synthetic.rig(1, (256, 704), B)
        s2e = torch.from_numpy(np.ascontiguousarray(rig['c2w'], np.float32))[:, 0].to(dev)            # (B, 4, 4)
        G = global_pose()
        # slot s was taken K - s steps behind slot K, the head
        e2g = torch.from_numpy(np.stack([G @ synthetic.ego_motion(K - s) for s in range(S)]).astype(np.float32))
        e2g = e2g.view(S, 1, 4, 4).expand(S, B, 4, 4).contiguous().to(dev)
        s2e_slots = s2e.expand(S, B, 4, 4).contiguous()
        bda = torch.eye(3, device=dev).expand(S, B, 3, 3).contiguous()
        valid = torch.full((B,), K, dtype=torch.int32, device=dev)
        head = K
        # the batch formulation's operands: frame f = age f, sensor2keyegos from the same poses
        order = [head - f for f in range(S)]
        pose = lambda t: torch.stack([t[s] for s in order], 1)[:, :, None].contiguous()       # noqa: E731  (B, F, 1, 4, 4)
        z33, z3 = torch.zeros(B, S, 1, 3, 3, device=dev), torch.zeros(B, S, 1, 3, device=dev)
        s2k, _, _ = detector.frame_poses(pose(s2e_slots), pose(e2g), z33, z3, z33, z33, z3, bda[0], 0)
        s2k = list(s2k.unbind(1))
        feats = [ring[head - (K - g)] for g in range(K)] + [ring[head]]                        # oldest first, key last
        frame_ids = [K - g for g in range(K)] + [0]

        def stream():
            return temporal.stream_align(ring, head, valid, s2e_slots, e2g, bda, interval, lower)[0]

        def batch():
            with torch.no_grad():
                return temporal.align_and_cat(feats, frame_ids, s2k, bda[0], interval, lower, fused=True)
        a, b = stream(), batch()
        torch.cuda.synchronize()
        diff = float((a - b).abs().max())
        for fn in (stream, batch):
            for _ in range(5):
                fn()
        (sb, sm), (bb, bm) = _wall([stream, batch], iters)
        sl, sd, names = _profile(stream)
        bl, bd, _ = _profile(batch)
        print(f'align, K = {K}, maps ({B}, {C}, {H}, {W}): stream_align {sd * 1e3:.1f} us device, {sl:.0f} launches, wall '
              f'best {sb * 1e3:.1f} / median {sm * 1e3:.1f} us, {_syncs(stream)} synchronisations | align_and_cat '
              f'{bd * 1e3:.1f} us device, {bl:.0f} launches, wall best {bb * 1e3:.1f} / median {bm * 1e3:.1f} us, '
              f'{_syncs(batch)} synchronisations | max |difference| {diff:.2e}')
        print(f'    kernels of stream_align: {dict(names)}')


def run_detector(iters):
    import random

    import torch
    from time_bev_encoder import _wall
    from time_detector import INPUT_SIZE, N_CAMS, _profile, _syncs, reference_model
    from ocrfdet_amd import detector
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    det = detector.OcRFDet4D(**reference_model()).to(dev).eval()
    frames = frames_of(SEQUENCE, 1, N_CAMS, INPUT_SIZE, dev)
    batches = [batch_inputs(frames, [t, max(t - 1, 0), max(t - 2, 0)]) for t in range(SEQUENCE)]
    clock = dict(stream=0, batch=0, state=None)

    def stream():
        random.seed(0)
        t = clock['stream'] % SEQUENCE
        clock['stream'] += 1
        out, clock['state'] = det.stream_step(frames[t], clock['state'])
        return out

    def batch():
        random.seed(0)
        t = clock['batch'] % SEQUENCE
        clock['batch'] += 1
        with torch.no_grad():
            return det.extract_img_feat(batches[t], None)
    for fn in (stream, batch):
        for _ in range(SEQUENCE):
            fn()
    (sb, sm), (bb, bm) = _wall([stream, batch], iters, blocks=3)
    sl, sd, _ = _profile(stream, reps=SEQUENCE)
    bl, bd, _ = _profile(batch, reps=SEQUENCE)
    print(f'OcRFDet4D, reference config, B = 1, a sequence of {SEQUENCE} frames: stream_step {sd:.2f} ms device, {sl:.0f} '
          f'launches, wall best {sb:.2f} / median {sm:.2f} ms, {_syncs(stream)} synchronisations | batch forward '
          f'(extract_img_feat on 3 frames) {bd:.2f} ms device, {bl:.0f} launches, wall best {bb:.2f} / median {bm:.2f} ms, '
          f'{_syncs(batch)} synchronisations | batch / stream device {bd / sd:.2f}x, wall median {bm / sm:.2f}x')


def _arm(label, fn, wall, reps=5):
    """One arm's figures as a phrase: device ms and launches per call (torch profiler), wall best / median, syncs."""
    from time_detector import _profile, _syncs
    launches, dev_ms, names = _profile(fn, reps=reps)
    return (f'{label} {dev_ms:.3f} ms device, {launches:.0f} launches, wall best {wall[0]:.3f} / median {wall[1]:.3f} ms, '
            f'{_syncs(fn)} synchronisations'), dev_ms, names


def run_align_bf16(iters):
    import numpy as np
    import torch
    from time_bev_encoder import _wall
    from ocrfdet_amd import synthetic, temporal
    dev = torch.device('cuda:0')
    B, C, H, W = 1, 80, 128, 128
    interval, lower = (0.8, 0.8, 8.0), (-51.2, -51.2, -5.0)
    for K in (1, 7):
        S = K + 1
        gen = torch.Generator().manual_seed(K)
        ring16 = torch.randn(S, B, C, H, W, generator=gen).to(dev).to(torch.bfloat16)
        ring32 = ring16.float()
        rig = synthetic.rig(1, (256, 704), B)
        s2e = torch.from_numpy(np.ascontiguousarray(rig['c2w'], np.float32))[:, 0].to(dev)
        G = global_pose()
        e2g = torch.from_numpy(np.stack([G @ synthetic.ego_motion(K - s) for s in range(S)]).astype(np.float32))
        e2g = e2g.view(S, 1, 4, 4).expand(S, B, 4, 4).contiguous().to(dev)
        s2e_slots = s2e.expand(S, B, 4, 4).contiguous()
        bda = torch.eye(3, device=dev).expand(S, B, 3, 3).contiguous()
        valid = torch.full((B,), K, dtype=torch.int32, device=dev)
        ops = (K, valid, s2e_slots, e2g, bda, interval, lower)

        def bf16():
            return temporal.stream_align(ring16, *ops, keep_bf16=True)[0]

        def f32():
            return temporal.stream_align(ring32, *ops)[0]

        def torch16():
            return temporal.stream_align(ring16, *ops)[0]           # no keyword: stream_align_torch on the bf16 ring
        a, b, c = bf16(), f32(), torch16()
        torch.cuda.synchronize()
        exact = bool(torch.equal(a, b.bfloat16()))
        diff = float((a.float() - c.float()).abs().max())
        fns = [bf16, f32, torch16]
        for fn in fns:
            for _ in range(5):
                fn()
        walls = _wall(fns, iters)
        texts = [_arm(label, fn, wall) for label, fn, wall in zip(
            ('stream_align(keep_bf16=True)', 'float32 stream_align', 'stream_align_torch on bf16'), fns, walls)]
        print(f'align, K = {K}, maps ({B}, {C}, {H}, {W}) bf16: ' + ' | '.join(t[0] for t in texts)
              + f' | float32 / bf16 kernel device {texts[1][1] / texts[0][1]:.2f}x, torch / bf16 kernel device '
                f'{texts[2][1] / texts[0][1]:.1f}x | bf16 == float32 kernel rounded once: {exact}; max |bf16 kernel - '
                f'torch on bf16| {diff:.2e}')
        print(f'    kernels of stream_align(keep_bf16=True): {dict(texts[0][2])}')


def run_detector_bf16(iters):
    import random

    import torch
    from time_bev_encoder import _wall
    from time_detector import INPUT_SIZE, N_CAMS, reference_model
    from ocrfdet_amd import detector
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    det = detector.OcRFDet4D(**reference_model()).to(dev).eval()
    frames = frames_of(SEQUENCE, 1, N_CAMS, INPUT_SIZE, dev)
    clock = dict(a=0, b=0, c=0, sa=None, sb=None, sc=None)

    def arm(key, **kw):
        def step():
            random.seed(0)
            t = clock[key] % SEQUENCE
            clock[key] += 1
            out, clock['s' + key] = det.stream_step(frames[t], clock['s' + key], **kw)
            return out
        return step
    a, b, plain = arm('a', bf16=True), arm('b'), arm('c')

    def c():
        with torch.autocast('cuda', dtype=torch.bfloat16):          # every switch at its default
            return plain()
    fns = [a, b, c]
    for fn in fns:
        for _ in range(SEQUENCE):
            fn()
    walls = _wall(fns, iters, blocks=3)
    texts = [_arm(label, fn, wall, reps=SEQUENCE) for label, fn, wall in zip(
        ('(a) stream_step(bf16=True)', '(b) float32 stream_step', '(c) stream_step under plain autocast'), fns, walls)]
    print(f'OcRFDet4D, reference config, B = 1, a sequence of {SEQUENCE} frames: ' + ' | '.join(t[0] for t in texts)
          + f' | (b) / (a) device {texts[1][1] / texts[0][1]:.2f}x, wall median {walls[1][1] / walls[0][1]:.2f}x | '
            f'(c) / (a) device {texts[2][1] / texts[0][1]:.2f}x, wall median {walls[2][1] / walls[0][1]:.2f}x')
    own = {k.split('(anonymous namespace)::', 1)[1].split('(')[0]: v for k, v in texts[0][2].items()
           if 'anonymous namespace' in k}
    print(f'    library kernels of {SEQUENCE} steps of (a): {own}')
    # decode: the bfloat16 head outputs of a bf16 step, with and without the in-place read
    head = det.pts_bbox_head
    x, _, _ = a()
    with torch.no_grad(), det.bf16_inference():
        preds = head(x)
    assert all(v.dtype == torch.bfloat16 for p in preds for v in p[0].values())

    def decode(flag):
        def fn():
            head.fused_decode_bf16 = flag
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                return head.get_bboxes_padded(preds)
        return fn
    on, off = decode(True), decode(False)
    got, want = on(), off()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(p, q)) for p, q in zip(got, want))
    for fn in (on, off):
        for _ in range(5):
            fn()
    walls = _wall([on, off], iters * 5)
    texts = [_arm(label, fn, wall) for label, fn, wall in zip(
        ('fused_decode_bf16 on', 'fused_decode_bf16 off (36 casts)'), (on, off), walls)]
    del head.fused_decode_bf16
    print(f'get_bboxes_padded, B = 1, {len(preds)} tasks on bf16 heads: ' + ' | '.join(t[0] for t in texts)
          + f' | off / on device {texts[1][1] / texts[0][1]:.2f}x, wall median {walls[1][1] / walls[0][1]:.2f}x | '
            f'same results: {same}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--bf16', action='store_true', help='time bfloat16 streaming (see the module docstring)')
    ap.add_argument('--limit', type=int, default=300, help='seconds per case')
    ap.add_argument('--case', type=int, default=None, help='(internal) run this one case in this process')
    a = ap.parse_args()
    if a.case is not None:
        import torch
        assert torch.cuda.is_available(), 'timing needs the GPU: there is no CPU fallback for a measurement'
        if a.case == 0:
            (run_align_bf16 if a.bf16 else run_align)(a.iters * 10)
        else:
            (run_detector_bf16 if a.bf16 else run_detector)(SEQUENCE * max(a.iters // 10, 1))   # whole sequences per block
        return 0
    lines = []
    cases = CASES_BF16 if a.bf16 else CASES
    for k in range(len(cases)):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', str(k), '--iters', str(a.iters)]
                               + (['--bf16'] if a.bf16 else []), stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f'case {cases[k]} ran out of its {a.limit} s: stopping', file=sys.stderr)
            return 124
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f'case {cases[k]} ended with status {p.returncode}: stopping', file=sys.stderr)
            return p.returncode or 1
        lines.append(p.stdout)
    if a.out:
        import torch
        with open(a.out, 'w') as f:
            f.write(f'torch {torch.__version__}; the arms alternating block by block; device time and launches from the '
                    'torch profiler; synchronisations: warnings of torch.cuda.set_sync_debug_mode\n' + ''.join(lines))
    return 0


if __name__ == '__main__':
    sys.exit(main())
