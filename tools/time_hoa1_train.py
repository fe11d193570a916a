"""Diagnostic: forward + backward of ``hoa.hoa1`` with B = 2 at 128 x 128 and 200 x 200, the fused HIP path
(``fused_training=True``: csrc/hoa1_train.hip) against the torch sequence, arms alternating.  Kernel count and device
time from the torch profiler, wall time from a host clock around synchronised blocks, synchronisations counted with
torch's sync debug mode (warnings).  The module is in train() with dropout 0.1: the fused arm draws its keep-mask.

    python tools/time_hoa1_train.py [--iters N] [--blocks N]
"""
import argparse
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ocrfdet_amd import hoa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=7)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    m = hoa.DeformableAttention2D(dim=13, dim_head=8, heads=1, dropout=0.1, downsample_factor=4, offset_scale=4,
                                  offset_groups=None, offset_kernel_size=6).to(dev).train()
    params = hoa._hoa1_params(m)
    for size in (128, 200):
        op = torch.rand(2, 13, size, size, device=dev)
        al = torch.rand(2, 13, size, size, device=dev)
        go = torch.randn(2, 13, size, size, device=dev)

        def step(fused):
            o, al_ = op.clone().requires_grad_(True), al.clone().requires_grad_(True)
            out = hoa.hoa1(m, o.reshape(-1, 1), al_, 13, size, size, fused_training=fused)
            return torch.autograd.grad(out, [o, al_] + params, go)

        for fused in (True, False):
            for _ in range(3):
                step(fused)
        wall = {True: [], False: []}
        for _ in range(a.blocks):
            for fused in (True, False):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    step(fused)
                torch.cuda.synchronize()
                wall[fused].append(1e3 * (time.perf_counter() - t0) / a.iters)
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        for fused in (True, False):
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as p:
                for _ in range(3):
                    step(fused)
                torch.cuda.synchronize()
            kern = [e for e in p.key_averages() if e.device_type == DeviceType.CUDA]
            n, dev_ms = sum(e.count for e in kern) // 3, sum(e.self_device_time_total for e in kern) / 3e3
            torch.cuda.set_sync_debug_mode('warn')
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter('always')
                step(fused)
            torch.cuda.set_sync_debug_mode('default')
            syncs = sum('synchroniz' in str(w.message).lower() and 'prototype' not in str(w.message) for w in caught)
            b = sorted(wall[fused])
            print(f'hoa1 B=2 {size}x{size} {"fused HIP     " if fused else "torch sequence"}: {n:4d} kernels, '
                  f'{dev_ms:7.3f} ms device, wall {b[0]:.3f} ms best / {b[len(b) // 2]:.3f} median / {b[-1]:.3f} worst of '
                  f'{a.blocks} alternating blocks of {a.iters}, {syncs} synchronisations')
            if fused:
                for e in sorted(kern, key=lambda e: -e.self_device_time_total):
                    print(f'    {e.self_device_time_total / 3e3:8.4f} ms  n={e.count // 3:2d}  {e.key[:100]}')


if __name__ == '__main__':
    main()
