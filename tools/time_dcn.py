"""Timing of the deformable convolution: ``deform_conv.deform_conv2d`` with the HIP kernels (``ocrf_deform_im2col`` /
``ocrf_deform_col2im`` + batched matmuls) against its torch formulation ``deform_conv2d_torch`` (gathers + matmul) in
the same process, alternating -- device time and launch count from the torch profiler, wall time per call from a host
clock around synchronised blocks, host synchronisations counted with torch's sync debug mode -- forward (``no_grad``)
and forward + backward (x, offset and weight require a gradient), at

* the ``DepthNet`` shape: n = 12, 256 -> 256 channels, 16 x 44, 3 x 3, pad 1, groups 4, dg 1;
* the CenterPoint head shape: n = 8, 64 -> 64 channels, 128 x 128, 3 x 3, pad 1, groups 4, dg 1;

with smooth offsets of about a pixel, as a trained ``conv_offset`` produces.  The last case is ``DepthNet`` itself
(256, 256, 80, 120, aspp_mid_channels=96; 12 cameras, 16 x 44) in eval mode, forward: ``NATIVE_DCN`` on against
``use_dcn=False``.

    python tools/time_dcn.py [--iters N] [--out profiles/dcn_time.txt]

Every case runs in a child process of its own under a time limit (``--limit`` seconds); the first case that fails or
runs out of time ends the run.
"""
import argparse
import os
import subprocess
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPES = {'DepthNet': (12, 256, 256, 16, 44), 'CenterPoint head': (8, 64, 64, 128, 128)}
CASES = [(shape, mode) for shape in SHAPES for mode in ('forward', 'forward+backward')] + [('DepthNet module', 'forward')]


def _profile(fn, reps=5):
    """(launches per call, device ms per call, device ms per call of the library's own kernels) from the torch profiler."""
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
            if 'deform_' in e.name:
                own['col2im' if 'col2im' in e.name else 'im2col'] += us
    return count / reps, dev_us / 1e3 / reps, {k: v / 1e3 / reps for k, v in own.items()}


def _syncs(fn):
    """Host synchronisations of one call, as torch's sync debug mode reports them."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    return sum('synchroniz' in str(w.message).lower() for w in seen)


def _compare(label, fused, torch_, iters, names=('fused', 'torch')):
    from time_bev_encoder import _wall
    for fn in (fused, torch_):
        for _ in range(3):
            fn()
    (fb, fm), (tb, tm) = _wall([fused, torch_], iters)
    fl, fd, own = _profile(fused)
    tl, td, _ = _profile(torch_)
    print(f'{label}: {names[0]} {fd:.4f} ms device, {fl:.0f} launches, {_syncs(fused)} synchronisations, wall best '
          f'{fb:.4f} / median {fm:.4f} ms | {names[1]} {td:.4f} ms device, {tl:.0f} launches, {_syncs(torch_)} '
          f'synchronisations, wall best {tb:.4f} / median {tm:.4f} ms | {names[1]} / {names[0]} device {td / fd:.2f}x, '
          f'wall median {tm / fm:.2f}x')
    for which, ms in sorted(own.items()):
        print(f'    {which} kernel(s) {ms:.4f} ms per call')


def run_op(shape, mode, iters):
    import torch
    from ocrfdet_amd import deform_conv as dc
    dev = torch.device('cuda:0')
    n, C, Cout, H, W = SHAPES[shape]
    train = mode != 'forward'
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(n, C, H, W, generator=gen).to(dev).requires_grad_(train)
    weight = (0.05 * torch.randn(Cout, C // 4, 3, 3, generator=gen)).to(dev).requires_grad_(train)
    # smooth offsets of about a pixel: a coarse random field upsampled
    coarse = torch.randn(n, 18, max(2, H // 8), max(2, W // 8), generator=gen)
    offset = torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=True)
    offset = offset.to(dev).contiguous().requires_grad_(train)
    g = torch.randn(n, Cout, H, W, generator=gen).to(dev) if train else None

    def arm(fused):
        def run():
            if not train:
                with torch.no_grad():
                    return dc.deform_conv2d(x, offset, weight, 1, 1, 1, 4, 1, fused=fused)
            x.grad = offset.grad = weight.grad = None
            dc.deform_conv2d(x, offset, weight, 1, 1, 1, 4, 1, fused=fused).backward(g)
        return run
    with torch.no_grad():
        a = dc.deform_conv2d(x, offset, weight, 1, 1, 1, 4, 1, fused=True)
        b = dc.deform_conv2d(x, offset, weight, 1, 1, 1, 4, 1, fused=False)
    diff = float((a - b).abs().max())
    _compare(f'{shape} {n} x {C}->{Cout} x {H} x {W}, {mode} (max |fused - torch| {diff:.2e})', arm(True), arm(False), iters)


def run_module(iters):
    import torch
    from ocrfdet_amd import depthnet
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    depthnet.NATIVE_DCN = True
    with_dcn = depthnet.DepthNet(256, 256, 80, 120, aspp_mid_channels=96).to(dev).eval()
    torch.nn.init.normal_(with_dcn.depth_conv[4].conv_offset.weight, std=0.01)
    without = depthnet.DepthNet(256, 256, 80, 120, use_dcn=False, aspp_mid_channels=96).to(dev).eval()
    x, mlp = torch.randn(12, 256, 16, 44, device=dev), torch.randn(12, 27, device=dev)

    def arm(net):
        def run():
            with torch.no_grad():
                return net(x, mlp)
        return run
    _compare('DepthNet(256, 256, 80, 120) eval forward, 12 x 16 x 44', arm(with_dcn), arm(without), iters,
             names=('NATIVE_DCN', 'use_dcn=False'))


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
        shape, mode = CASES[a.case]
        if shape == 'DepthNet module':
            run_module(a.iters)
        else:
            run_op(shape, mode, a.iters)
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
                    'the torch profiler, synchronisations from torch.cuda.set_sync_debug_mode\n' + ''.join(lines))
    return 0


if __name__ == '__main__':
    sys.exit(main())
