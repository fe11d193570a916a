"""Timing of the stereo cost volume at the reference shape (B = 2, 6 cameras, C = 256, 64 x 176 stereo features,
D = 118): ``ocrf_stereo_cost_volume`` against the torch formulation (device time, launches and host synchronisations
from the torch profiler), the kernel's algorithmic bytes and FLOP against the MI355X peaks, and the whole stereo
``DepthNet(256, 256, 80, 120, aspp_mid 96, bias 5)`` forward and forward + backward with either.

    python tools/time_stereo.py [--iters N] [--out profiles/stereo_timing.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
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
