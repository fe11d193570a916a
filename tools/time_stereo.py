"""Timing of the stereo cost volume at the reference shape (B = 2, 6 cameras, C = 256, 64 x 176 stereo features,
D = 118): ``ocrf_stereo_cost_volume`` against the torch formulation (device time, launches and host synchronisations
from the torch profiler), the kernel's algorithmic bytes and FLOP against the MI355X peaks, and the whole stereo
``DepthNet(256, 256, 80, 120, aspp_mid 96, bias 5)`` forward and forward + backward with either.

    python tools/time_stereo.py [--iters N] [--out profiles/stereo_timing.json]

``--dtype bf16``: the same shape with bfloat16 features, as an image encoder under bf16 autocast hands them over.  What
runs by default (two casts to float32 + ``ocrf_stereo_cost_volume``) against the opt-in path (two
``ocrf_stereo_pack_bf16`` + ``ocrf_stereo_cost_volume_bf16``), the arms alternating in one process: device time per arm
and per kernel from the torch profiler, and the stereo ``DepthNet`` eval forward under autocast with the switch off and
on.  The output is a text table:

    python tools/time_stereo.py --dtype bf16 [--iters N] [--out profiles/stereo_bf16_time.txt]
"""
import argparse
import collections
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ocrfdet_amd import depthnet  # noqa: E402
from tests.test_stereo_gpu import full_metas  # noqa: E402

HBM_TBS, FP32_TFLOPS = 6.29, 157.3          # MI355X_MICROARCH: measured float4 copy rate, FP32 vector peak (spec)
FLOP_PER_TERM = 8                           # 4 bilinear products + 3 adds + |a - b| accumulate (sub, add)


def _best(fn, iters, blocks=5):
    out = []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / iters)
    out.sort()
    return out[0], out[len(out) // 2]


def _profile(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as p:
        fn()
        torch.cuda.synchronize()
    names, dev_us = collections.Counter(), 0.0
    for e in p.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and e.name:
            names[e.name] += 1
            dev_us += e.device_time_total if hasattr(e, 'device_time_total') else e.cuda_time_total
    return sum(names.values()), dev_us / 1e3, names


def _syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    return sum('synchroniz' in str(x.message) for x in w)


def _kernels(fn, iters):
    """Mean device ms per call of ``fn`` over ``iters`` calls, in all and per kernel name, and launches per call."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as p:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    per, n = collections.defaultdict(float), 0
    for e in p.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and e.name:
            per[e.name] += (e.device_time_total if hasattr(e, 'device_time_total') else e.cuda_time_total) / 1e3 / iters
            n += 1
    return sum(per.values()), dict(per), n / iters


def _short(name):
    name = name.replace('(anonymous namespace)::', '').split('(')[0]
    return name if len(name) <= 70 else name[:67] + '...'


def main_bf16(a):
    dev = torch.device('cuda:0')
    metas = full_metas(dev)
    metas = dict(metas, cv_feat_list=[f.bfloat16() for f in metas['cv_feat_list']])
    BN, C, H, W = metas['cv_feat_list'][1].shape
    D = metas['frustum'].shape[0]
    arms = collections.OrderedDict(
        cast_f32=lambda: depthnet.stereo_cost_volume(metas, 5.0),                     # what autocast runs by default
        pack_bf16=lambda: depthnet.stereo_cost_volume(metas, 5.0, keep_bf16=True))
    lines = [f'stereo cost volume, bfloat16 features: BN = {BN}, C = {C}, {H} x {W}, D = {D}; device ms per call '
             f'(torch profiler, {a.iters} calls per block, {a.blocks} alternating blocks, median block)', '']
    with torch.no_grad():
        same = torch.equal(arms['cast_f32']().view(torch.int32), arms['pack_bf16']().view(torch.int32))
        lines.append(f'outputs bit-equal: {same}')
        runs = {k: [] for k in arms}
        for _ in range(a.blocks):
            for k, fn in arms.items():
                runs[k].append(_kernels(fn, a.iters))
        total = {}
        for k in arms:
            runs[k].sort(key=lambda r: r[0])
            tot, per, launches = runs[k][len(runs[k]) // 2]
            total[k] = tot
            lines.append(f'{k}: {tot:.3f} ms in {launches:.0f} launches, {_syncs(arms[k])} host syncs '
                         f'(blocks: {" ".join(f"{r[0]:.3f}" for r in runs[k])})')
            for name, ms in sorted(per.items(), key=lambda kv: -kv[1]):
                lines.append(f'    {ms:8.3f} ms  {_short(name)}')
        lines.append(f'ratio cast_f32 / pack_bf16: {total["cast_f32"] / total["pack_bf16"]:.3f}')
        lines.append('')
        net = depthnet.DepthNet(256, 256, 80, 120, use_dcn=False, stereo=True, bias=5.0, aspp_mid_channels=96).to(dev)
        net.eval()
        x = torch.randn(BN, 256, H // 4, W // 4, device=dev)
        mlp = torch.randn(BN // 6, 6, 27, device=dev)

        def forward(flag):
            net.fused_cost_volume_bf16 = flag
            with torch.autocast('cuda', dtype=torch.bfloat16):
                return net(x, mlp, metas)
        fwd = {}
        for flag in (False, True):
            forward(flag)
        for _ in range(a.blocks):
            for flag in (False, True):
                fwd.setdefault(flag, []).append((_kernels(lambda: forward(flag), a.iters)[0],
                                                 _best(lambda: forward(flag), a.iters, blocks=1)[0]))
        for flag in (False, True):
            dev_ms = sorted(r[0] for r in fwd[flag])[len(fwd[flag]) // 2]
            wall = sorted(r[1] for r in fwd[flag])[len(fwd[flag]) // 2]
            lines.append(f'DepthNet(256, 256, 80, 120) eval forward under bf16 autocast, fused_cost_volume_bf16 = {flag}: '
                         f'{dev_ms:.3f} ms device, {wall:.3f} ms wall')
        lines.append(f'ratio off / on (device): '
                     f'{sorted(r[0] for r in fwd[False])[len(fwd[False]) // 2] / sorted(r[0] for r in fwd[True])[len(fwd[True]) // 2]:.3f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--blocks', type=int, default=5, help='--dtype bf16: alternating blocks per arm')
    ap.add_argument('--dtype', choices=('f32', 'bf16'), default='f32')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.dtype == 'bf16':
        return main_bf16(a)
    dev = torch.device('cuda:0')
    metas = full_metas(dev)
    prev, curr = metas['cv_feat_list']
    BN, C, H, W = curr.shape
    D = metas['frustum'].shape[0]
    res = dict(shape=dict(BN=BN, C=C, H=H, W=W, D=D))
    fused = lambda: depthnet.stereo_cost_volume_hip(metas, 5.0)       # noqa: E731
    torch_ = lambda: depthnet.stereo_cost_volume_torch(metas, 5.0)    # noqa: E731
    with torch.no_grad():
        for name, fn in (('fused', fused), ('torch', torch_)):
            fn()
            best, med = _best(fn, a.iters)
            launches, dev_ms, _ = _profile(fn)
            res[name] = dict(wall_ms_best=best, wall_ms_median=med, device_ms=dev_ms, launches=launches,
                             host_syncs=_syncs(fn))
    nbytes = (prev.numel() + curr.numel() + BN * D * H * W) * 4
    flop = BN * D * H * W * 4 * (C // 4) * FLOP_PER_TERM
    t_bw, t_fl = nbytes / (HBM_TBS * 1e12) * 1e3, flop / (FP32_TFLOPS * 1e12) * 1e3
    bound = 'FP32 compute' if t_fl > t_bw else 'HBM'
    k_ms = res['fused']['device_ms']
    res['roofline'] = dict(bytes=nbytes, flop=flop, hbm_ms=t_bw, fp32_ms=t_fl, bound=bound,
                           fraction_of_bound=max(t_bw, t_fl) / k_ms,
                           speedup_device=res['torch']['device_ms'] / k_ms)

    net = depthnet.DepthNet(256, 256, 80, 120, use_dcn=False, stereo=True, bias=5.0, aspp_mid_channels=96).to(dev)
    x = torch.randn(BN, 256, H // 4, W // 4, device=dev)
    mlp = torch.randn(BN // 6, 6, 27, device=dev)
    for flag in (True, False):
        net.fused_cost_volume = flag
        key = 'depthnet_fused' if flag else 'depthnet_torch'
        net.eval()
        with torch.no_grad():
            fwd = lambda: net(x, mlp, metas)                               # noqa: E731
            fwd()
            f_best, f_med = _best(fwd, a.iters)
        net.train()

        def fb():
            net.zero_grad(set_to_none=True)
            net(x, mlp, metas).square().mean().backward()
        fb()
        b_best, b_med = _best(fb, a.iters)
        res[key] = dict(forward_ms_best=f_best, forward_ms_median=f_med, fwd_bwd_ms_best=b_best, fwd_bwd_ms_median=b_med)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
