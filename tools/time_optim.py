"""Timing of the training step's tail (clip + AdamW + weight EMA) over the parameters of the reference config's native
modules instantiated together: ``ImageEncoder``, ``OcRFViewTransformerFull`` with its ``DepthNet``,
``build_pre_process``, ``BEVEncoder`` and ``CenterHead`` (configs/ocrfdet/ocrfdet.py:44-121), one param group per
parameter with the config's ``lr_mult`` keys (``optim.paramwise_groups``), random gradients.  Three arms in one
process, alternating:

  1. the reference's formulation: ``clip_grad_norm_`` + ``float(grad_norm)`` (mmcv's read-back) + ``AdamW`` at its
     defaults + the per-entry EMA loop of mmdet3d/core/hook/ema.py:57-60;
  2. torch at its best: foreach ``clip_grad_norm_`` without the read-back + ``AdamW(fused=True)`` + a
     ``torch._foreach_`` EMA over the floating entries;
  3. ``optim.FusedAdamW(max_grad_norm=5)`` with an attached ``optim.ModelEMA``.

Each arm owns a copy of the model, so the arms do not see each other's updates.  Reported per arm: wall ms per step
(host clock around synchronised blocks), device ms per step and launches per step (torch profiler); for arm 3 the
achieved fraction of the 6.29 TB/s copy rate over 40 bytes per parameter element (36 in the update pass, 4 in the norm
pass).

    python tools/time_optim.py [--iters N] [--out profiles/optim_time.txt]

Every case runs in a child process of its own under a time limit (``--limit`` seconds); the first case that fails or
runs out of time ends the run.
"""
import argparse
import copy
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = ['reference modules']
HBM_TBS = 6.29                               # MI355X_MICROARCH: measured float4 copy rate
MAX_NORM, LR, WD, EMA_DECAY, EMA_UPDATES = 5.0, 2e-4, 1e-2, 0.9990, 10560
CUSTOM_KEYS = {k: dict(lr_mult=2) for k in (
    'img_view_transformer.S_MLP', 'img_view_transformer.R_MLP', 'img_view_transformer.A_MLP',
    'img_view_transformer.C_MLP', 'img_view_transformer.C_MLP_nerf', 'img_view_transformer.D_MLP_nerf',
    'img_view_transformer.sigma', 'img_feat_resize1', 'img_feat_resize2')}


def reference_modules():
    """The native modules of configs/ocrfdet/ocrfdet.py:44-121 under the detector's attribute names."""
    from torch import nn

    from ocrfdet_amd import bev_encoder as be
    from ocrfdet_amd import center_head as ch
    from ocrfdet_amd import image_encoder as ie
    from ocrfdet_amd import view_transformer_ocrf as vto
    pc_range = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
    grid = {'x': [-51.2, 51.2, 0.8], 'y': [-51.2, 51.2, 0.8], 'z': [-5, 3, 8], 'depth': [1.0, 60.0, 0.5]}
    m = nn.Module()
    m.image_encoder = ie.ImageEncoder(
        dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 2, 3), frozen_stages=-1,
             norm_cfg=dict(type='BN', requires_grad=True), norm_eval=False, with_cp=True, style='pytorch'),
        dict(type='CustomFPN', in_channels=[1024, 2048], out_channels=256, num_outs=1, start_level=0, out_ids=[0]))
    m.img_view_transformer = vto.OcRFViewTransformerFull(
        pc_range=pc_range, grid_config=grid, input_size=(256, 704), in_channels=256, out_channels=80,
        depthnet_cfg=dict(use_dcn=False, aspp_mid_channels=96, stereo=True, bias=5.), downsample=16)
    m.pre_process_net = be.build_pre_process(dict(type='CustomResNet', numC_input=80, num_layer=[2], num_channels=[80],
                                                  stride=[1], backbone_output_ids=[0]))
    m.bev_encoder = be.BEVEncoder(dict(type='CustomResNet', numC_input=160, num_channels=[160, 320, 640]),
                                  dict(type='FPN_LSS', in_channels=800, out_channels=256))
    tasks = [dict(num_class=1, class_names=['car']), dict(num_class=2, class_names=['truck', 'construction_vehicle']),
             dict(num_class=2, class_names=['bus', 'trailer']), dict(num_class=1, class_names=['barrier']),
             dict(num_class=2, class_names=['motorcycle', 'bicycle']),
             dict(num_class=2, class_names=['pedestrian', 'traffic_cone'])]
    m.pts_bbox_head = ch.CenterHead(in_channels=256, tasks=tasks, share_conv_channel=64,
                                    common_heads=dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2)),
                                    loss_bbox=dict(type='L1Loss', reduction='mean', loss_weight=0.25))
    return m


def _profile(fn, reps=3):
    """(launches per step, device ms per step, device ms per step by kernel or copy name)."""
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
        # kernels and copies only: torch's hook around Optimizer.step shows up as an annotation on the device timeline
        if e.device_type == torch.autograd.DeviceType.CUDA and e.name and not getattr(e, 'is_user_annotation', False) \
                and not e.name.startswith('Optimizer.'):
            us = e.device_time_total if hasattr(e, 'device_time_total') else e.cuda_time_total
            count += 1
            dev_us += us
            kernel = re.search(r'optim_\w+_kernel', e.name)
            own[kernel.group(0) if kernel else e.name[:60]] += us
    return count / reps, dev_us / 1e3 / reps, {k: v / 1e3 / reps for k, v in own.items()}


def run_case(case, iters):
    import math

    import torch
    from time_bev_encoder import _wall
    from ocrfdet_amd import optim
    assert torch.cuda.is_available(), 'timing needs the GPU: there is no CPU fallback for a measurement'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    base = reference_modules().to(dev)
    models = [base, copy.deepcopy(base), copy.deepcopy(base)]
    grads = [torch.randn_like(p) for p in base.parameters()]
    n_tensors, n_elements = len(grads), sum(g.numel() for g in grads)
    floats = [v for v in base.state_dict().values() if v.dtype.is_floating_point]
    n_ema, ema_elements = len(floats), sum(v.numel() for v in floats)
    for k, m in enumerate(models):
        for p, g in zip(m.parameters(), grads):
            p.grad = g if k == 2 else g.clone()                        # arms 1 and 2 scale their gradients in place
    groups = [optim.paramwise_groups(m, LR, WD, CUSTOM_KEYS) for m in models]
    strip = lambda gs: [{k: v for k, v in g.items() if k != 'name'} for g in gs]  # noqa: E731
    decay = lambda x: EMA_DECAY * (1 - math.exp(-x / 2000))  # noqa: E731

    # arm 1
    opt1 = torch.optim.AdamW(strip(groups[0]), lr=LR, weight_decay=WD)
    ema1, state1 = copy.deepcopy(models[0]).eval(), dict(updates=EMA_UPDATES)

    def reference():
        float(torch.nn.utils.clip_grad_norm_(models[0].parameters(), MAX_NORM))
        opt1.step()
        with torch.no_grad():
            state1['updates'] += 1
            d = decay(state1['updates'])
            msd = models[0].state_dict()
            for k, v in ema1.state_dict().items():
                if v.dtype.is_floating_point:
                    v *= d
                    v += (1.0 - d) * msd[k].detach()

    # arm 2
    opt2 = torch.optim.AdamW(strip(groups[1]), lr=LR, weight_decay=WD, fused=True)
    ema2, state2 = copy.deepcopy(models[1]).eval(), dict(updates=EMA_UPDATES)
    ema2_f = [v for v in ema2.state_dict().values() if v.dtype.is_floating_point]
    src2_f = [v for v in models[1].state_dict().values() if v.dtype.is_floating_point]
    params2 = list(models[1].parameters())

    def torch_best():
        torch.nn.utils.clip_grad_norm_(params2, MAX_NORM, foreach=True)
        opt2.step()
        with torch.no_grad():
            state2['updates'] += 1
            d = decay(state2['updates'])
            torch._foreach_mul_(ema2_f, d)
            torch._foreach_add_(ema2_f, src2_f, alpha=1.0 - d)

    # arm 3
    opt3 = optim.FusedAdamW(groups[2], lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)
    ema3 = optim.ModelEMA(models[2], decay=EMA_DECAY, updates=EMA_UPDATES)
    opt3.attach_ema(ema3)

    def fused():
        opt3.step()

    arms = [('1 reference formulation', reference), ('2 torch fused / foreach', torch_best), ('3 FusedAdamW + EMA', fused)]
    for _, fn in arms:
        for _ in range(3):
            fn()
    walls = _wall([fn for _, fn in arms], iters)
    print(f'{case}: {n_tensors} parameter tensors, {n_elements} elements ({n_elements / 1e6:.1f} M); EMA over {n_ema} '
          f'floating state_dict entries, {ema_elements} elements')
    print('    clip_grad_norm_ scales the gradients of arms 1 and 2 in place, so they shrink until the norm is below '
          'max_norm; torch multiplies by the clamped coefficient either way, so the work per step does not change')
    results = []
    for k, (name, fn) in enumerate(arms):
        launches, dev_ms, own = _profile(fn)
        best, median = walls[k]
        results.append((median, dev_ms))
        print(f'    arm {name}: wall best {best:.4f} / median {median:.4f} ms per step, device {dev_ms:.4f} ms, '
              f'{launches:.0f} launches')
        if k == 2:
            print('        ' + ', '.join(f'{kn} {ms:.4f} ms' for kn, ms in sorted(own.items())))
    nbytes = 40 * n_elements
    dev3 = results[2][1]
    print(f'    arm 3: 40 B x {n_elements} elements = {nbytes / 1e6:.1f} MB in {dev3:.4f} ms device -> '
          f'{nbytes / dev3 / 1e9:.2f} TB/s, {nbytes / dev3 / 1e9 / HBM_TBS:.0%} of the {HBM_TBS} TB/s copy rate '
          f'(at that rate: {nbytes / HBM_TBS / 1e9:.4f} ms)')
    print(f'    arm 1 / arm 3: wall {results[0][0] / results[2][0]:.2f}x, device {results[0][1] / results[2][1]:.2f}x; '
          f'arm 2 / arm 3: wall {results[1][0] / results[2][0]:.2f}x, device {results[1][1] / results[2][1]:.2f}x')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--limit', type=int, default=300, help='seconds per case')
    ap.add_argument('--case', type=int, default=None, help='(internal) run this one case in this process')
    a = ap.parse_args()
    if a.case is not None:
        run_case(CASES[a.case], a.iters)
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
            f.write(f'torch {torch.__version__}; iters {a.iters} x 5 blocks, alternating; device time and launch counts '
                    'from the torch profiler\n' + ''.join(lines))
    return 0


if __name__ == '__main__':
    sys.exit(main())
