"""Times the detection head's training path at the reference shape (B = 8, 256 -> 128 x 128, six tasks, nuScenes-like
synthetic boxes): get_targets + loss forward + backward, fused (csrc/center_head.hip) against the torch formulation,
with the device launches and host synchronisations of each, and the head forward alone.

    python tools/time_center_head.py [--iters 20] [--out profiles/center_head_timing.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ocrfdet_amd import center_head as ch  # noqa: E402
from ocrfdet_amd import synthetic  # noqa: E402
from tests.test_center_head_gpu import full_head  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return dict(median_ms=ts[len(ts) // 2], min_ms=ts[0], iters=iters)


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(ev)


def syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    return sum('synchroniz' in str(x.message) for x in w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default='profiles/center_head_timing.json')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    head = full_head().to(dev)
    head.init_weights()
    x = torch.randn(8, 256, 128, 128, device=dev)
    bx, lab = synthetic.nuscenes_boxes(8, seed=0, device=dev)
    with torch.no_grad():
        outs = head([x])
    leaves = [{k: v.detach().clone().requires_grad_(True) for k, v in p[0].items()} for p in outs]

    def train(fused):
        def fn():
            head.fused_loss = fused
            pd = tuple([dict(p)] for p in leaves)
            ld = head.loss(bx, lab, pd)
            sum(ld.values()).backward()
        return fn

    def forward():
        with torch.no_grad():
            head([x])

    def forward_backward():
        y = head([x])
        sum(v.float().sum() for p in y for v in p[0].values()).backward()

    res = dict(shape=dict(B=8, in_channels=256, H=128, W=128, tasks=6, boxes=[int(b.shape[0]) for b in bx]))
    for name, fn in (('fused', train(True)), ('torch', train(False))):
        res[name] = dict(timed(fn, a.iters), launches=launches(fn), host_syncs=syncs(fn))
    res['head_forward'] = timed(forward, a.iters)
    res['head_forward_backward'] = timed(forward_backward, max(5, a.iters // 2))
    res['speedup_fused_vs_torch'] = res['torch']['median_ms'] / res['fused']['median_ms']
    res['fused_share_of_head_train'] = res['fused']['median_ms'] / (res['fused']['median_ms'] +
                                                                      res['head_forward_backward']['median_ms'])
    res['torch_share_of_head_train'] = res['torch']['median_ms'] / (res['torch']['median_ms'] +
                                                                      res['head_forward_backward']['median_ms'])
    res['reference_syncs_derived'] = ('per drawn object about 10 (width/length tests, radius min/int, range test, '
                                      'int(center) x2, numpy window H2D copy, assert), plus 2 .item() per task in '
                                      'loss: at B = 8 and ~35 boxes per sample about 2 800 + 12 per iteration')
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
