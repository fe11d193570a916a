"""Timing of the image encoder's two fused passes against their torch formulations in the same run, the variants
alternating block by block — device time and launch count from the torch profiler, wall time per call from a host clock
around synchronised blocks — at 12 and at 48 images of 3 x 256 x 704 (B = 2 and B = 8 key frames of the reference config,
6 cameras):

* the residual tail ``add_relu`` against ``add_relu_torch`` at ``layer1``'s shape (256, 64, 176) and ``layer4``'s
  (2048, 8, 22), forward and forward + backward;
* the top-down merge ``upsample_add`` against ``upsample_add_torch`` at the reference's shape, (256, 8, 22) ->
  (256, 16, 44), forward and forward + backward;
* the reference config's whole ``ImageEncoder`` (ResNet-50 with ``with_cp=True`` and ``CustomFPN``, ``stereo=True``):
  forward in ``eval()`` and forward + backward in ``train()``, with each pair of ``fused_tail`` / ``fused_merge``;

with the kernels' algorithmic bytes against the MI355X's measured HBM copy rate.  The defaults of the two flags in
``ocrfdet_amd/plane_ops.py`` follow from this file's output.

``--autocast bf16`` runs the same arms as training under ``torch.autocast('cuda', dtype=torch.bfloat16)`` sees them: the
two ops on bfloat16 tensors, the encoder inside the autocast region with ``fused_tail_bf16`` / ``fused_merge_bf16``
following the arm's flags (the unfused arm is what the encoder ran before the ops took bfloat16), and each encoder row
against its float32 time in ``profiles/image_encoder_time.txt``.  The defaults ``FUSED_TAIL_BF16_DEFAULT`` /
``FUSED_MERGE_BF16_DEFAULT`` follow from that output, ``profiles/image_encoder_bf16_time.txt``.

    python tools/time_image_encoder.py [--iters N] [--enc-iters N] [--images 12 48] [--autocast bf16]
                                       [--out profiles/image_encoder_time.txt]
"""
import argparse
import collections
import contextlib
import os
import re
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ocrfdet_amd import image_encoder as ie  # noqa: E402

HBM_TBS = 6.29                               # MI355X_MICROARCH: measured float4 copy rate


def emit(lines, text):
    """Keep a line of the report, and show it as soon as it is there."""
    lines.append(text)
    print(text, flush=True)


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


def _profile(fn, reps):
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


def measure(lines, name, variants, iters, reps=5):
    """``variants``: [(label, fn)], the last one the torch formulation every other one is compared with.  Returns the
    device ms of each."""
    for _, fn in variants:
        for _ in range(2):
            fn()
    walls = _wall([fn for _, fn in variants], iters)
    profs = [_profile(fn, reps) for _, fn in variants]
    base_dev, base_wall = profs[-1][1], walls[-1][1]
    for (label, _), (best, med), (launches, dev) in zip(variants, walls, profs):
        emit(lines, f'{name} | {label}: {dev:.4f} ms device, {launches:.0f} launches, wall best {best:.4f} / median '
                     f'{med:.4f} ms | torch / this: device {base_dev / dev:.2f}x, wall median {base_wall / med:.2f}x')
    return [dev for _, dev in profs]


def traffic(lines, what, nbytes, ms):
    emit(lines, f'    {what}: {nbytes / 1e6:.1f} MB -> {nbytes / ms / 1e9:.2f} TB/s, '
                 f'{nbytes / ms / 1e9 / HBM_TBS:.0%} of the {HBM_TBS} TB/s copy rate')


def float32_rows(path=os.path.join(ROOT, 'profiles', 'image_encoder_time.txt')):
    """{row name | label: device ms} of the float32 run's encoder rows."""
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        return {m.group(1): float(m.group(2)) for m in re.finditer(r'^(ImageEncoder [^\n]*?): ([\d.]+) ms device', f.read(),
                                                                   re.M)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--enc-iters', type=int, default=3)
    ap.add_argument('--images', type=int, nargs='+', default=[12, 48])
    ap.add_argument('--autocast', choices=['none', 'bf16'], default='none')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    bf16 = a.autocast == 'bf16'
    dtype, width = (torch.bfloat16, 2) if bf16 else (torch.float32, 4)
    region = (lambda: torch.autocast('cuda', dtype=torch.bfloat16)) if bf16 else contextlib.nullcontext
    f32 = float32_rows() if bf16 else {}
    assert torch.cuda.is_available(), 'timing needs the GPU: there is no CPU fallback for a measurement'
    dev = torch.device('cuda:0')
    lines = []
    emit(lines, f'device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; ops {a.iters} and encoder '
             f'{a.enc_iters} iters x 5 blocks, alternating; device ms from the torch profiler'
             + ('; bfloat16 operands, the encoder under torch.autocast(bf16)' if bf16 else ''))

    for n_img in a.images:
        for layer, shape in (('layer1', (n_img, 256, 64, 176)), ('layer4', (n_img, 2048, 8, 22))):
            x = torch.randn(*shape, device=dev).to(dtype).requires_grad_(True)
            y = torch.randn(*shape, device=dev).to(dtype).requires_grad_(True)
            g = torch.randn(*shape, device=dev).to(dtype)
            name = f'tail {layer} {shape}'
            with torch.no_grad():
                fd, _ = measure(lines, name + ' forward', [('add_relu', lambda: ie.add_relu(x, y)),
                                                             ('torch', lambda: ie.add_relu_torch(x, y))], a.iters)
            nbytes = 3 * width * x.numel()
            traffic(lines, 'forward bytes (a, b, out)', nbytes, fd)

            def fb(op):
                def run():
                    x.grad = y.grad = None
                    op(x, y).backward(g)
                return run
            measure(lines, name + ' forward + backward', [('add_relu', fb(ie.add_relu)),
                                                           ('torch', fb(ie.add_relu_torch))], a.iters)
            del x, y, g

        dst = torch.randn(n_img, 256, 16, 44, device=dev).to(dtype).requires_grad_(True)
        src = torch.randn(n_img, 256, 8, 22, device=dev).to(dtype).requires_grad_(True)
        g = torch.randn(n_img, 256, 16, 44, device=dev).to(dtype)
        name = f'merge ({n_img}, 256, 8, 22) -> (16, 44)'
        with torch.no_grad():
            fd, _ = measure(lines, name + ' forward',
                            [('upsample_add', lambda: ie.upsample_add(dst, src, size=(16, 44))),
                             ('torch', lambda: ie.upsample_add_torch(dst, src, size=(16, 44)))], a.iters)
        traffic(lines, 'forward bytes (dst, src, out)', width * (2 * dst.numel() + src.numel()), fd)

        def fbm(op):
            def run():
                dst.grad = src.grad = None
                op(dst, src, size=(16, 44)).backward(g)
            return run
        measure(lines, name + ' forward + backward', [('upsample_add', fbm(ie.upsample_add)),
                                                       ('torch', fbm(ie.upsample_add_torch))], a.iters)
        del dst, src, g

        enc = ie.ImageEncoder(
            dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 2, 3), frozen_stages=-1,
                 norm_cfg=dict(type='BN', requires_grad=True), norm_eval=False, with_cp=True, style='pytorch'),
            dict(type='CustomFPN', in_channels=[1024, 2048], out_channels=256, num_outs=1, start_level=0,
                 out_ids=[0])).to(dev)
        enc.img_backbone.init_weights()
        img = torch.randn(n_img // 6, 6, 3, 256, 704, device=dev)

        def set_flags(tail, merge):
            enc.img_backbone.fused_tail = enc.img_backbone.fused_tail_bf16 = tail
            enc.img_neck.fused_merge = enc.img_neck.fused_merge_bf16 = merge

        def fwd(tail, merge):
            def run():
                set_flags(tail, merge)
                with torch.no_grad(), region():
                    enc(img, stereo=True)
            return run

        def fwd_bwd(tail, merge):
            def run():
                set_flags(tail, merge)
                enc.zero_grad(set_to_none=True)
                with region():
                    x, stereo = enc(img, stereo=True)
                (x.float().square().mean() + stereo.float().square().mean()).backward()
            return run
        pairs = [(True, True), (True, False), (False, True), (False, False)]
        label = lambda t, m: f'fused_tail={t}, fused_merge={m}' + (' (torch)' if not (t or m) else '')  # noqa: E731
        def encoder_rows(name, make):
            devs = measure(lines, name, [(label(t, m), make(t, m)) for t, m in pairs], a.enc_iters, reps=3)
            for (t, m), ms in zip(pairs, devs):
                ref = f32.get(f'{name} | {label(t, m)}')
                if ref is not None:
                    emit(lines, f'    {label(t, m)}: float32 {ref:.4f} ms device (profiles/image_encoder_time.txt) / '
                                 f'bf16 autocast {ms:.4f} = {ref / ms:.2f}x')
        enc.eval()
        encoder_rows(f'ImageEncoder {n_img} x (3, 256, 704) forward, eval', fwd)
        enc.train()
        encoder_rows(f'ImageEncoder {n_img} x (3, 256, 704) forward + backward, train, with_cp', fwd_bwd)
        del enc, img
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
