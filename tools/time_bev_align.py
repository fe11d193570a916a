"""Timing of the temporal BEV alignment at the reference shape: ``temporal.align_and_cat`` with the HIP kernels
(``ocrf_bev_align_forward`` / ``_backward``, one launch per warped frame into its channels of the result) against its
torch formulation (``feature_transform`` + ``shift_feature_torch`` + ``torch.cat``) in the same process, alternating —
device time and launch count from the torch profiler, wall time per call from a host clock around synchronised blocks —
for (8, 80, 128, 128) maps, the key frame plus 1 and plus 8 warped frames, forward (``no_grad``) and forward + backward
(every map requires a gradient, so that every warped frame runs its gather).  Both arms compute the transforms.

    python tools/time_bev_align.py [--iters N] [--out profiles/bev_align_time.txt]

``--dtype bf16``: the same rows for bfloat16 maps kept bfloat16 (``keep_bf16=True``): ``ocrf_bev_align_forward_bf16`` /
``_backward_bf16`` against the torch formulation on the bf16 maps (``grid_sample`` + ``cat``).

    python tools/time_bev_align.py --dtype bf16 [--iters N] [--out profiles/bev_align_bf16_time.txt]

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

SHAPE = (8, 80, 128, 128)
CASES = [(frames, mode) for frames in (1, 8) for mode in ('forward', 'forward+backward')]
HBM_TBS = 6.29                               # MI355X_MICROARCH: measured float4 copy rate


def poses(n_frames, B, dev):
    """Per-frame (B, 6, 4, 4) sensor-to-key-ego poses: frame k has moved 0.9 k m and turned 1.5 k degrees."""
    import torch
    out = []
    for k in range(n_frames):
        yaw = math.radians(1.5 * k)
        m = torch.eye(4)
        m[0, 0], m[0, 1], m[1, 0], m[1, 1] = math.cos(yaw), -math.sin(yaw), math.sin(yaw), math.cos(yaw)
        m[0, 3], m[1, 3] = 0.9 * k, -0.3 * k
        out.append(m.repeat(B, 6, 1, 1).to(dev))
    return out


def _profile(fn, reps=5):
    """(launches per call, device ms per call, device ms per call of the library's two kernels) from the torch profiler."""
    import collections

    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as p:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    count, dev_us, own = 0, 0.0, collections.Counter()
    for e in p.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and e.name:
            us = e.device_time_total if hasattr(e, 'device_time_total') else e.cuda_time_total
            count += 1
            dev_us += us
            if 'bev_align' in e.name:
                own['backward' if 'backward' in e.name else 'forward'] += us
    return count / reps, dev_us / 1e3 / reps, {k: v / 1e3 / reps for k, v in own.items()}


def run_case(frames, mode, iters, dtype=None):
    import torch
    from time_bev_encoder import _wall
    from ocrfdet_amd import temporal
    assert torch.cuda.is_available(), 'timing needs the GPU: there is no CPU fallback for a measurement'
    dev = torch.device('cuda:0')
    B, C, H, W = SHAPE
    train = mode != 'forward'
    keep = dtype == 'bf16'
    kw = dict(keep_bf16=True) if keep else {}
    feats = [torch.randn(SHAPE, device=dev, requires_grad=train) for _ in range(frames + 1)]
    if keep:
        feats = [f.detach().bfloat16().requires_grad_(train) for f in feats]
    s2k = poses(frames + 1, B, dev)
    bda = torch.eye(3, device=dev).repeat(B, 1, 1)
    interval, lower = torch.tensor([0.8, 0.8, 8.0]), torch.tensor([-51.2, -51.2, -5.0])
    ids = list(range(frames + 1))
    g = torch.randn(B, (frames + 1) * C, H, W, device=dev) if train else None
    if keep and train:
        g = g.bfloat16()

    def arm(fused):
        def run():
            if not train:
                with torch.no_grad():
                    return temporal.align_and_cat(feats, ids, s2k, bda, interval, lower, fused=fused, **kw)
            for f in feats:
                f.grad = None
            temporal.align_and_cat(feats, ids, s2k, bda, interval, lower, fused=fused, **kw).backward(g)
        return run
    fused, torch_ = arm(True), arm(False)
    for fn in (fused, torch_):
        for _ in range(3):
            fn()
    (fb, fm), (tb, tm) = _wall([fused, torch_], iters)
    fl, fd, own = _profile(fused)
    tl, td, _ = _profile(torch_)
    print(f'{frames} warped frame(s) of {SHAPE}{" bf16" if keep else ""}, {mode}: fused {fd:.4f} ms device, {fl:.0f} launches, wall best {fb:.4f} '
          f'/ median {fm:.4f} ms | torch {td:.4f} ms device, {tl:.0f} launches, wall best {tb:.4f} / median {tm:.4f} ms '
          f'| torch / fused device {td / fd:.2f}x, wall median {tm / fm:.2f}x')
    # a map read once, its channels of the result written once
    nbytes = (2 if keep else 4) * 2 * B * C * H * W
    for which, ms in sorted(own.items()):
        ms /= frames
        print(f'    {which} kernel {ms:.4f} ms per warped frame: {nbytes / 1e6:.1f} MB -> {nbytes / ms / 1e9:.2f} TB/s, '
              f'{nbytes / ms / 1e9 / HBM_TBS:.0%} of the {HBM_TBS} TB/s copy rate')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--limit', type=int, default=240, help='seconds per case')
    ap.add_argument('--case', type=int, default=None, help='(internal) run this one case in this process')
    ap.add_argument('--dtype', choices=['bf16'], default=None, help='bfloat16 maps kept bfloat16 (keep_bf16=True)')
    a = ap.parse_args()
    extra = ['--dtype', a.dtype] if a.dtype else []
    if a.case is not None:
        run_case(*CASES[a.case], a.iters, a.dtype)
        return 0
    lines = []
    for k in range(len(CASES)):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', str(k), '--iters', str(a.iters)] + extra,
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
            f.write(f'torch {torch.__version__}; iters {a.iters} x 5 blocks, alternating; device time from the torch '
                    'profiler\n' + ''.join(lines))
    return 0


if __name__ == '__main__':
    sys.exit(main())
