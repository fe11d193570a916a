"""Timing of the distillation tail of ``OcRFDet4DVGGT``: the two group-wise correlation volumes (teacher tokens and
aligned student feature) and the two losses between them, at the reference config's shape -- features (B, 2, 2048, 21,
37), 64 groups, 5 disparities -- for B = 4 (``samples_per_gpu``) and B = 1, forward (``no_grad``) and forward + backward
(the student feature requires a gradient).  Three arms in one process, alternating:

* ``fused``: ``distill.build_cost_volume(fused=True)`` and ``distill.kd_losses(fused=True)``, the HIP kernels;
* ``reference``: the reference's formulation (ocrfdet_vggt.py:205-216, :476-480) -- both operands expanded to (B, G, D,
  Cg, H, W), a gather along the last axis, product, sum -- with ``kd_losses_torch``;
* ``shifted``: ``distill.group_corr_volume_torch`` (D shifted products) with ``kd_losses_torch``, the package's path
  for tensors the kernels do not take.

Per arm: launches and device time from the torch profiler, host synchronisations from torch's sync debug mode, wall time
per call from a host clock around synchronised blocks, and the peak of allocated memory above the operands.

    python tools/time_distill.py [--iters N] [--out profiles/distill_time.txt]

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

C, H, W, G, MAX_DISP = 2048, 21, 37, 64, 4
CASES = [(B, mode) for B in (4, 1) for mode in ('forward', 'forward+backward')]


def expanded_volume(feats, max_disp, groups):
    """The reference's formulation of the volume: six-dimensional expansions of both views and a gather."""
    import torch
    B, _, c, h, w = feats.shape
    D, cg = max_disp + 1, c // groups
    left = feats[:, 0].view(B, groups, 1, cg, h, w).expand(B, groups, D, cg, h, w)
    right = feats[:, 1].view(B, groups, 1, cg, h, w).expand(B, groups, D, cg, h, w)
    cols = torch.arange(w, device=feats.device).view(1, w) - torch.arange(D, device=feats.device).view(D, 1)
    index = cols.clamp(min=0).view(1, 1, D, 1, 1, w).expand(B, groups, D, cg, h, w)
    return (left * torch.gather(right, 5, index)).sum(dim=3)


def _profile(fn, reps=5):
    """(launches per call, device ms per call, {own kernel: device ms per call}) from the torch profiler."""
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
            for key in ('group_corr_forward', 'group_corr_grad_left', 'group_corr_grad_right', 'kd_partial', 'kd_final',
                        'kd_backward'):
                if key in e.name:
                    own[key] += us
    return count / reps, dev_us / 1e3 / reps, {k: v / 1e3 / reps for k, v in own.items()}


def _peak_mib(fn):
    """Peak of allocated device memory during one call, above what was allocated before it."""
    import torch
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 2 ** 20


def run_case(B, mode, iters):
    import torch
    from ocrfdet_amd import distill
    from time_bev_encoder import _wall
    from time_dcn import _syncs
    dev = torch.device('cuda:0')
    train = mode != 'forward'
    gen = torch.Generator().manual_seed(0)
    teacher = torch.randn(B, 2, C, H, W, generator=gen).to(dev)
    student = (teacher.cpu() + 0.5 * torch.randn(B, 2, C, H, W, generator=gen)).to(dev).requires_grad_(train)

    def tail(volume, losses):
        def forward():
            return losses(volume(student), volume(teacher))

        def run():
            if not train:
                with torch.no_grad():
                    return forward()
            student.grad = None
            smooth, cos = forward()
            (smooth + cos).backward()
        return run
    arms = {
        'fused': tail(lambda f: distill.build_cost_volume(f, MAX_DISP, 'group_corr', G, fused=True),
                      lambda s, t: distill.kd_losses(s, t, fused=True)),
        'reference': tail(lambda f: expanded_volume(f, MAX_DISP, G), distill.kd_losses_torch),
        'shifted': tail(lambda f: distill.group_corr_volume_torch(f, MAX_DISP, G), distill.kd_losses_torch),
    }
    with torch.no_grad():
        a = distill.build_cost_volume(student, MAX_DISP, 'group_corr', G, fused=True)
        diff = float((a - expanded_volume(student, MAX_DISP, G)).abs().max())
    for fn in arms.values():
        for _ in range(3):
            fn()
    walls = _wall(list(arms.values()), iters)
    print(f'B = {B}, (B, 2, {C}, {H}, {W}), {G} groups, {MAX_DISP + 1} disparities, {mode} '
          f'(max |fused - reference| of a volume {diff:.2e}):')
    device = {}
    for (name, fn), (best, median) in zip(arms.items(), walls):
        launches, dev_ms, own = _profile(fn)
        device[name] = dev_ms
        print(f'    {name:9s} {dev_ms:8.4f} ms device, {launches:3.0f} launches, {_syncs(fn)} synchronisations, wall best '
              f'{best:.4f} / median {median:.4f} ms, peak memory {_peak_mib(fn):.1f} MiB')
        for which, ms in sorted(own.items()):
            print(f'        {which} {ms:.4f} ms per call')
    print(f'    reference / fused device {device["reference"] / device["fused"]:.2f}x, shifted / fused device '
          f'{device["shifted"] / device["fused"]:.2f}x')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--limit', type=int, default=240, help='seconds per case')
    ap.add_argument('--case', type=int, default=None, help='(internal) run this one case in this process')
    a = ap.parse_args()
    if a.case is not None:
        import torch
        assert torch.cuda.is_available(), 'timing needs the GPU: there is no CPU fallback for a measurement'
        run_case(*CASES[a.case], a.iters)
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
            f.write(f'torch {torch.__version__}; iters {a.iters} x 5 blocks, alternating; device time and launches from '
                    'the torch profiler, synchronisations from torch.cuda.set_sync_debug_mode, peak memory from '
                    'torch.cuda.max_memory_allocated above the operands\n' + ''.join(lines))
    return 0


if __name__ == '__main__':
    sys.exit(main())
