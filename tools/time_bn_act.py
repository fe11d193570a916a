"""Timing of the fused batch-norm passes (``norm_ops.bn_act``, csrc/bn_act.hip) against the torch formulation in the same
run, the two alternating block by block (``time_image_encoder.measure``: device time and launch count from the torch
profiler, wall time per call from a host clock around synchronised blocks):

* the op alone against ``bn_act_torch`` (``bn`` + ``relu_``, + ``add`` with a residual) on the same tensors, in training
  mode, at 48 x (64, 64, 176) and 48 x (256, 64, 176), with and without a residual, float32 and bfloat16, forward and
  forward + backward, with the kernels' algorithmic bytes against the MI355X's measured HBM copy rate;
* the reference config's whole ``ImageEncoder`` at 12 and 48 images and the ``BEVEncoder`` at (8, 160, 128, 128),
  ``fuse_norms`` on against off (off is the code path the modules ran before the flag existed), forward in ``eval()``
  and forward + backward in ``train()``, in float32 and under ``torch.autocast('cuda', dtype=torch.bfloat16)`` (the BEV
  encoder with ``autocast_bf16=True`` there: without it it runs float32 inside autocast).

The flag's default stays off whatever this prints.

    python tools/time_bn_act.py [--iters N] [--enc-iters N] [--images 12 48] [--out profiles/bn_act_time.txt]
"""
import argparse
import contextlib
import os
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from ocrfdet_amd import bev_encoder as be, blocks, image_encoder as ie, norm_ops  # noqa: E402
from time_image_encoder import emit, measure, traffic  # noqa: E402

WIDTH = {torch.float32: 4, torch.bfloat16: 2}


def op_rows(lines, dev, shape, dtype, residual, iters):
    C = shape[1]
    bn = nn.BatchNorm2d(C).to(dev).train()
    x = torch.randn(*shape, device=dev).to(dtype).requires_grad_(True)
    res = torch.randn(*shape, device=dev).to(dtype).requires_grad_(True) if residual else None
    g = torch.randn(*shape, device=dev).to(dtype)
    name = f'bn_act {shape} {str(dtype)[6:]}' + (' + residual' if residual else '')
    with torch.no_grad():
        fd, _ = measure(lines, name + ' forward', [('bn_act', lambda: norm_ops.bn_act(bn, x, res)),
                                                   ('torch', lambda: norm_ops.bn_act_torch(bn, x, res))], iters)
    n, w = x.numel(), WIDTH[dtype]
    traffic(lines, 'forward bytes (x twice' + (', residual' if residual else '') + ', out)',
            (3 + bool(residual)) * w * n, fd)

    def fb(op):
        def run():
            x.grad = bn.weight.grad = bn.bias.grad = None
            if res is not None:
                res.grad = None
            op(bn, x, res).backward(g)
        return run
    bd, _ = measure(lines, name + ' forward + backward', [('bn_act', fb(norm_ops.bn_act)),
                                                          ('torch', fb(norm_ops.bn_act_torch))], iters)
    # backward: grad_out, x, out read by the reduction and again by the apply pass; dx (and dresidual) written
    traffic(lines, 'forward + backward bytes', ((3 + bool(residual)) + 6 + 1 + bool(residual)) * w * n, bd)


def encoder_rows(lines, name, model, call, loss, region, iters):
    def fwd(flag):
        def run():
            blocks.fuse_norms(model, flag)
            with torch.no_grad(), region():
                call()
        return run

    def fwd_bwd(flag):
        def run():
            blocks.fuse_norms(model, flag)
            model.zero_grad(set_to_none=True)
            with region():
                out = call()
            loss(out).backward()
        return run
    arms = [('fuse_norms on', True), ('fuse_norms off (torch)', False)]
    model.eval()
    measure(lines, name + ' forward, eval', [(label, fwd(flag)) for label, flag in arms], iters, reps=3)
    model.train()
    measure(lines, name + ' forward + backward, train', [(label, fwd_bwd(flag)) for label, flag in arms], iters, reps=3)
    blocks.fuse_norms(model, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--enc-iters', type=int, default=3)
    ap.add_argument('--images', type=int, nargs='+', default=[12, 48])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'timing needs the GPU: there is no CPU fallback for a measurement'
    dev = torch.device('cuda:0')
    lines = []
    emit(lines, f'device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; ops {a.iters} and encoders '
                f'{a.enc_iters} iters x 5 blocks, alternating; device ms from the torch profiler')
    for shape in ((48, 64, 64, 176), (48, 256, 64, 176)):
        for dtype in (torch.float32, torch.bfloat16):
            for residual in (False, True):
                op_rows(lines, dev, shape, dtype, residual, a.iters)
                torch.cuda.empty_cache()

    autocast = lambda: torch.autocast('cuda', dtype=torch.bfloat16)  # noqa: E731
    for n_img in a.images:
        enc = ie.ImageEncoder(
            dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 2, 3), frozen_stages=-1,
                 norm_cfg=dict(type='BN', requires_grad=True), norm_eval=False, with_cp=True, style='pytorch'),
            dict(type='CustomFPN', in_channels=[1024, 2048], out_channels=256, num_outs=1, start_level=0,
                 out_ids=[0])).to(dev)
        enc.img_backbone.init_weights()
        img = torch.randn(n_img // 6, 6, 3, 256, 704, device=dev)
        loss = lambda out: out[0].float().square().mean() + out[1].float().square().mean()  # noqa: E731
        for label, region in (('float32', contextlib.nullcontext), ('bf16 autocast', autocast)):
            encoder_rows(lines, f'ImageEncoder {n_img} x (3, 256, 704) {label}', enc, lambda: enc(img, stereo=True), loss,
                         region, a.enc_iters)
        del enc, img
        torch.cuda.empty_cache()

    bev = be.BEVEncoder(dict(type='CustomResNet', numC_input=160, num_channels=[160, 320, 640]),
                        dict(type='FPN_LSS', in_channels=800, out_channels=256)).to(dev)
    x = torch.randn(8, 160, 128, 128, device=dev, requires_grad=True)
    for label, region, keep in (('float32', contextlib.nullcontext, False), ('bf16 autocast', autocast, True)):
        bev.autocast_bf16 = keep
        encoder_rows(lines, f'BEVEncoder (8, 160, 128, 128) {label}', bev, lambda: bev(x),
                     lambda out: out.float().square().mean(), region, a.enc_iters)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
