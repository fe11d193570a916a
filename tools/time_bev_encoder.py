"""Timing of the BEV encoder's fused upsample-concat at the reference shapes: ``bev_encoder.upsample_cat``
(``ocrf_upsample_cat_forward`` / ``_backward``) against ``upsample_cat_torch`` in the same run — device time and launch
count from the torch profiler, wall time per call from a host clock around synchronised blocks, the two alternating —
forward and forward + backward, at

* ``up`` + cat: B = 8, x2 (160, 64, 64), x1 (640, 16, 16), scale 4;
* ``up2[0]``:   B = 8, x1 (512, 64, 64), scale 2;

with the kernel's algorithmic bytes against the MI355X's measured HBM copy rate, and the whole ``BEVEncoder`` of the
reference config on (8, 160, 128, 128), fused against unfused.

    python tools/time_bev_encoder.py [--iters N] [--out profiles/bev_encoder_time.txt]
"""
import argparse
import collections
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ocrfdet_amd import bev_encoder as be  # noqa: E402

HBM_TBS = 6.29                               # MI355X_MICROARCH: measured float4 copy rate


def _wall(fns, iters, blocks=5):
    """Best and median wall ms per call of each fn, the fns alternating block by block."""
    out = [[] for _ in fns]
    for _ in range(blocks):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            out[k].append(1e3 * (time.perf_counter() - t0) / iters)
    return [(min(v), sorted(v)[len(v) // 2]) for v in out]


def _profile(fn, reps=5):
    """(launches per call, device ms per call) from the torch profiler."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as p:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    names, dev_us = collections.Counter(), 0.0
    for e in p.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and e.name:
            names[e.name] += 1
            dev_us += e.device_time_total if hasattr(e, 'device_time_total') else e.cuda_time_total
    return sum(names.values()) / reps, dev_us / 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'timing needs the GPU: there is no CPU fallback for a measurement'
    dev = torch.device('cuda:0')
    lines = [f'device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; iters {a.iters} x 5 blocks, alternating']

    def report(name, fused, torch_):
        for fn in (fused, torch_):
            for _ in range(3):
                fn()
        (fb, fm), (tb, tm) = _wall([fused, torch_], a.iters)
        fl, fd = _profile(fused)
        tl, td = _profile(torch_)
        lines.append(f'{name}: fused {fd:.4f} ms device, {fl:.0f} launches, wall best {fb:.4f} / median {fm:.4f} ms | '
                     f'torch {td:.4f} ms device, {tl:.0f} launches, wall best {tb:.4f} / median {tm:.4f} ms | '
                     f'torch / fused device {td / fd:.2f}x, wall median {tm / fm:.2f}x')
        return fd

    shapes = [('up+cat  B=8 x2 (160,64,64) x1 (640,16,16) x4', (8, 160, 64, 64), (8, 640, 16, 16), 4),
              ('up2[0]  B=8 x1 (512,64,64) x2', None, (8, 512, 64, 64), 2)]
    for name, s2, s1, scale in shapes:
        x2 = torch.randn(*s2, device=dev) if s2 else None
        x1 = torch.randn(*s1, device=dev, requires_grad=True)
        g = torch.randn(s1[0], (s2[1] if s2 else 0) + s1[1], s1[2] * scale, s1[3] * scale, device=dev)
        with torch.no_grad():
            fd = report(name + ' forward', lambda: be.upsample_cat(x2, x1, scale),
                        lambda: be.upsample_cat_torch(x2, x1, scale))
        nbytes = 4 * (g.numel() + x1.numel() + (x2.numel() if s2 else 0))
        lines.append(f'    forward bytes {nbytes / 1e6:.1f} MB -> {nbytes / fd / 1e9:.2f} TB/s, '
                     f'{nbytes / fd / 1e9 / HBM_TBS:.0%} of the {HBM_TBS} TB/s copy rate')

        def fb(op):
            def run():
                x1.grad = None
                op(x2, x1, scale).backward(g)
            return run
        report(name + ' forward + backward', fb(be.upsample_cat), fb(be.upsample_cat_torch))

    enc = be.BEVEncoder(dict(type='CustomResNet', numC_input=160, num_channels=[160, 320, 640]),
                        dict(type='FPN_LSS', in_channels=800, out_channels=256)).to(dev)
    x = torch.randn(8, 160, 128, 128, device=dev)

    def set_fused(flag):
        enc.img_bev_encoder_neck.fused_upsample = flag

    def fwd(flag):
        def run():
            set_fused(flag)
            with torch.no_grad():
                enc(x)
        return run

    def fwd_bwd(flag):
        def run():
            set_fused(flag)
            enc.zero_grad(set_to_none=True)
            enc(x).square().mean().backward()
        return run
    enc.eval()
    report('BEVEncoder (8,160,128,128) forward, eval', fwd(True), fwd(False))
    enc.train()
    report('BEVEncoder (8,160,128,128) forward + backward, train', fwd_bwd(True), fwd_bwd(False))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
