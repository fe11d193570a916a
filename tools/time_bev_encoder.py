"""Timing of the BEV encoder's fused upsample-concat at the reference shapes: ``bev_encoder.upsample_cat``
(``ocrf_upsample_cat_forward`` / ``_backward``) against ``upsample_cat_torch`` in the same run — device time and launch
count from the torch profiler, wall time per call from a host clock around synchronised blocks, the two alternating —
forward and forward + backward, at

* ``up`` + cat: B = 8, x2 (160, 64, 64), x1 (640, 16, 16), scale 4;
* ``up2[0]``:   B = 8, x1 (512, 64, 64), scale 2;

with the kernel's algorithmic bytes against the MI355X's measured HBM copy rate, and the whole ``BEVEncoder`` of the
reference config on (8, 160, 128, 128), fused against unfused.

    python tools/time_bev_encoder.py [--iters N] [--out profiles/bev_encoder_time.txt]

``--autocast bf16``: the same rows for the bfloat16 form instead.  The ops on bf16 tensors
(``ocrf_upsample_cat_forward_bf16`` / ``_backward_bf16`` against ``upsample_cat_torch`` on the same tensors), each
kernel's bytes against the copy rate, and the encoder under ``torch.autocast('cuda', dtype=torch.bfloat16)`` in three
arms alternating in one process: ``autocast_bf16=True`` with the kernels, ``autocast_bf16=True`` with the torch
formulation, and ``autocast_bf16=False`` (float32 inside autocast, the default), with the RMS error of the two bf16 arms
against the float32 one on the same input.

    python tools/time_bev_encoder.py --autocast bf16 [--iters N] [--out profiles/bev_encoder_bf16_time.txt]
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


def _kernel_ms(fn, part, reps=5):
    """Device ms per call of the kernels whose name contains ``part``, from the torch profiler."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as p:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    us = sum(e.device_time_total if hasattr(e, 'device_time_total') else e.cuda_time_total for e in p.events()
             if e.device_type == torch.autograd.DeviceType.CUDA and e.name and part in e.name)
    return us / 1e3 / reps


def _rate(nbytes, ms):
    return (f'{nbytes / 1e6:.1f} MB in {ms:.4f} ms -> {nbytes / ms / 1e9:.2f} TB/s, '
            f'{nbytes / ms / 1e9 / HBM_TBS:.0%} of the {HBM_TBS} TB/s copy rate')


def bf16_rows(a, dev, lines):
    """The rows of ``main`` for bfloat16: the ops on bf16 tensors, then the encoder under bf16 autocast in three arms."""
    bf16 = torch.bfloat16

    def arms(name, fns):
        """``fns``: [(label, fn)], the first the fused arm; wall times alternate, device times from the profiler."""
        for _, fn in fns:
            for _ in range(3):
                fn()
        walls = _wall([fn for _, fn in fns], a.iters)
        devs = [_profile(fn) for _, fn in fns]
        parts = [f'{label} {d:.4f} ms device, {n:.0f} launches, wall best {wb:.4f} / median {wm:.4f} ms'
                 for (label, _), (n, d), (wb, wm) in zip(fns, devs, walls)]
        ratios = [f'{label} / {fns[0][0]} device {d / devs[0][1]:.2f}x, wall median {wm / walls[0][1]:.2f}x'
                  for (label, _), (_, d), (_, wm) in list(zip(fns, devs, walls))[1:]]
        lines.append(f'{name}: ' + ' | '.join(parts + ratios))

    shapes = [('up+cat  B=8 x2 (160,64,64) x1 (640,16,16) x4', (8, 160, 64, 64), (8, 640, 16, 16), 4),
              ('up2[0]  B=8 x1 (512,64,64) x2', None, (8, 512, 64, 64), 2)]
    for name, s2, s1, scale in shapes:
        x2 = torch.randn(*s2, device=dev).to(bf16) if s2 else None
        x1 = torch.randn(*s1, device=dev).to(bf16).requires_grad_(True)
        g = torch.randn(s1[0], (s2[1] if s2 else 0) + s1[1], s1[2] * scale, s1[3] * scale, device=dev).to(bf16)
        with torch.no_grad():
            arms(name + ' bf16 forward', [('fused', lambda: be.upsample_cat(x2, x1, scale)),
                                          ('torch', lambda: be.upsample_cat_torch(x2, x1, scale))])
            fwd_ms = _kernel_ms(lambda: be.upsample_cat(x2, x1, scale), 'upsample_cat_kernel')

        def fb(op):
            def run():
                x1.grad = None
                op(x2, x1, scale).backward(g)
            return run
        arms(name + ' bf16 forward + backward', [('fused', fb(be.upsample_cat)), ('torch', fb(be.upsample_cat_torch))])
        bwd_ms = _kernel_ms(fb(be.upsample_cat), 'upsample_cat_backward_kernel')
        # forward: x2 and x1 read, the result written; backward: the upsampled channels of grad_out read, grad_x1 written
        lines.append('    forward kernel ' + _rate(2 * (g.numel() + x1.numel() + (x2.numel() if s2 else 0)), fwd_ms))
        lines.append('    backward kernel ' + _rate(2 * (g.numel() - (x2.numel() if s2 else 0) + x1.numel()), bwd_ms))

    enc = be.BEVEncoder(dict(type='CustomResNet', numC_input=160, num_channels=[160, 320, 640]),
                        dict(type='FPN_LSS', in_channels=800, out_channels=256)).to(dev)
    neck = enc.img_bev_encoder_neck
    neck.fused_upsample = True
    x = torch.randn(8, 160, 128, 128, device=dev)
    x16 = x.to(bf16)

    def setup(keep, fused):
        enc.autocast_bf16, neck.fused_upsample_bf16 = keep, fused

    def fwd(keep, fused):
        def run():
            setup(keep, fused)
            with torch.no_grad(), torch.autocast('cuda', dtype=bf16):
                return enc(x16)
        return run

    def fwd_bwd(keep, fused):
        def run():
            setup(keep, fused)
            enc.zero_grad(set_to_none=True)
            with torch.autocast('cuda', dtype=bf16):
                out = enc(x16)
            out.float().square().mean().backward()
        return run
    labels = [('bf16 fused', (True, True)), ('bf16 torch', (True, False)), ('float32 (autocast_bf16=False)', (False, True))]
    enc.eval()
    arms('BEVEncoder (8,160,128,128) under bf16 autocast, forward, eval', [(label, fwd(*k)) for label, k in labels])
    want, fused, unfused = fwd(False, True)().double(), fwd(True, True)().double(), fwd(True, False)().double()
    e_fused, e_torch = ((t - want).square().mean().sqrt().item() for t in (fused, unfused))
    lines.append(f'    RMS error against the float32 arm (RMS of its output {want.square().mean().sqrt().item():.4e}): '
                 f'bf16 fused {e_fused:.4e}, bf16 torch {e_torch:.4e}, fused / torch {e_fused / e_torch:.3f}')
    enc.train()
    arms('BEVEncoder (8,160,128,128) under bf16 autocast, forward + backward, train',
         [(label, fwd_bwd(*k)) for label, k in labels])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--autocast', choices=['bf16'], default=None, help='the rows of the bfloat16 form instead')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'timing needs the GPU: there is no CPU fallback for a measurement'
    dev = torch.device('cuda:0')
    lines = [f'device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; iters {a.iters} x 5 blocks, alternating']
    if a.autocast:
        bf16_rows(a, dev, lines)
        text = '\n'.join(lines)
        print(text)
        if a.out:
            with open(a.out, 'w') as f:
                f.write(text + '\n')
        return

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
