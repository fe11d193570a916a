"""Diagnostic: where the cfg2 step's time goes, on the device clock (ocrf_diag_stamp, 100 MHz): the step's two chains
re-issued here with a stamp after every stage — main stream: HOA-1/2 -> LSS pool -> HT pool -> HOA-3; side stream: per
frame update -> blend.     python tools/timeline_hotpath.py [--bw auto|N] [--ht panel --lss panel] [--fuse-hoa-stats 0|1]

Two more modes for the kernel timeline of the REAL step (hp.step, one host call), one rocprofv3 run of its own per arm:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o x -- \
        python tools/timeline_hotpath.py --ht panel --lss panel --fuse-hoa-stats 0|1 --steps 80
    python tools/timeline_hotpath.py --reduce DIR/.../x_kernel_trace.csv      (no GPU: the median step, kernel by kernel)"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ocrfdet_amd import _lib, hotpath, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--bw', default='auto')
ap.add_argument('--ht', default='mfma')
ap.add_argument('--lss', default='tile')
ap.add_argument('--lss-group', type=int, default=2)
ap.add_argument('--fuse-hoa-stats', type=int, default=1, help='HotPath(fuse_hoa_stats=...): the A/B arm')
ap.add_argument('--steps', type=int, default=0, help='issue this many whole steps (hp.step) and exit: what a kernel trace wraps')
ap.add_argument('--reduce', metavar='CSV', default=None, help='print the median step of a rocprofv3 kernel-trace CSV and exit')
a = ap.parse_args()


def reduce_trace(path, mark='bev_pool_cell_weights_kernel'):
    """A step = from one cell-weight pre-pass (the main chain's first kernel) to the next; the step of median period of the
    trace's second half, its kernels relative to the step's first start."""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    nm = lambda r: r['Kernel_Name'].replace('(anonymous namespace)::', '').split('(')[0][:64]  # noqa: E731
    idx = [i for i, r in enumerate(rows) if mark in r['Kernel_Name']]
    idx = idx[len(idx) // 2:]
    steps = sorted(((int(rows[j]['Start_Timestamp']) - int(rows[i]['Start_Timestamp']), rows[i:j]) for i, j in zip(idx, idx[1:])),
                   key=lambda s: s[0])
    print('%d steps; period us: min %.1f median %.1f max %.1f' % (len(steps), steps[0][0] / 1e3, steps[len(steps) // 2][0] / 1e3,
                                                                  steps[-1][0] / 1e3))
    # (the render stream's head now and then starts ahead of the pre-pass and its blend falls into the step before: only
    # the steps with the usual number of kernels are looked at)
    counts = [len(sg) for _, sg in steps]
    usual = max(set(counts), key=counts.count)
    steps = [s for s in steps if len(s[1]) == usual]
    span, seg = steps[len(steps) // 2]
    print('step of %d kernels, %.1f us from its first start to the next step\'s first start' % (len(seg), span / 1e3))
    t0 = int(seg[0]['Start_Timestamp'])
    for r in seg:
        s, e = int(r['Start_Timestamp']) - t0, int(r['End_Timestamp']) - t0
        print('%8.1f -> %8.1f  (%6.1f us)  q%-3s %s' % (s / 1e3, e / 1e3, (e - s) / 1e3, r['Queue_Id'], nm(r)))
    # every step of the second half: duration of the kernels the A/B is about, and where the two chains end
    by = {}
    for _, sg in steps:
        pools = [r for r in sg if 'bev_pool_panel_kernel' in r['Kernel_Name']]
        for key, r in (('LSS bev_pool_panel_kernel', pools[0] if pools else None), ('HT bev_pool_panel_kernel', pools[1] if len(pools) > 1 else None),
                       ('hoa_channel_stats_kernel', next((r for r in sg if 'hoa_channel_stats' in r['Kernel_Name']), None)),
                       ('hoa_mask_gate_kernel', next((r for r in sg if 'hoa_mask_gate' in r['Kernel_Name']), None))):
            if r is not None:
                by.setdefault(key, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
        s0 = int(sg[0]['Start_Timestamp'])
        gate = [int(r['End_Timestamp']) for r in sg if 'hoa_mask_gate' in r['Kernel_Name']]
        blend = [int(r['End_Timestamp']) for r in sg if 'raster_' in r['Kernel_Name']]
        if gate and blend:
            by.setdefault('main chain ends (hoa_mask_gate) after the step\'s start', []).append((gate[-1] - s0) / 1e3)
            by.setdefault('render stream ends (last raster kernel) after the step\'s start', []).append((max(blend) - s0) / 1e3)
            by.setdefault('main chain ends after the render stream', []).append((gate[-1] - max(blend)) / 1e3)
    for key, v in by.items():
        print('median over %d steps: %-66s %7.1f us' % (len(v), key, float(np.median(v))))


if a.reduce:
    reduce_trace(a.reduce)
    sys.exit(0)
dev = torch.device('cuda:0')
cfg = synthetic.CONFIGS['cfg2_6cam_2frame_bev200x200_render_hoa']
hp = hotpath.HotPath(cfg, dev, ht_pool_backend=a.ht, blend_workgroups='auto' if a.bw == 'auto' else int(a.bw),
                     lss_pool_backend=a.lss, lss_mfma_group=a.lss_group, fuse_hoa_stats=bool(a.fuse_hoa_stats))
depth, feat = hp.make_inputs(0)
if a.steps:
    for _ in range(a.steps):
        hp.step(depth, feat)
    torch.cuda.synchronize()
    hp.check_render_plans()
    print('issued', a.steps, 'steps; fuse_hoa_stats', hp.fuse_hoa_stats, '; one host call:', bool(hp._compiled), hp.one_call_refused)
    sys.exit(0)
for _ in range(10):
    hp.step(depth, feat)
torch.cuda.synchronize()
side = hotpath.shared_stream(dev, 'render')
cur = torch.cuda.current_stream(dev)
names = ['start', 'hoa12 (after the pools)', 'lss', 'ht', 'hoa3', 's_start', 'update (fused) | upd0+blend0', 'blend (fused) | upd1+blend1']
N = 60
stamps = torch.zeros(N, len(names), dtype=torch.int64, device=dev)
for it in range(N):
    row = stamps[it]
    _lib.diag_stamp(row, 0)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        _lib.diag_stamp(row, 5)
        plans = hp._plans()               # one fused plan (both frames) by default, or one per frame
        for k, entry in enumerate(plans):
            if len(plans) == 1:
                o = hp._render_planned(entry, phase='update')
                _lib.diag_stamp(row, 6)
                hp._render_planned(entry, phase='blend', out=o)
                _lib.diag_stamp(row, 7)
            else:
                hp._render_planned(entry)
                _lib.diag_stamp(row, 6 + k)
    lss = hp.pool(hp.lss, depth, feat)
    _lib.diag_stamp(row, 2)
    st = hp._fused_stats()
    ht = hp.pool(hp.ht, depth, feat, stats=st)
    _lib.diag_stamp(row, 3)
    ob = hp.hoa_opacity_bev()
    _lib.diag_stamp(row, 1)
    hp.hoa_step(ht, ob, stats=st)
    _lib.diag_stamp(row, 4)
    cur.wait_stream(side)
torch.cuda.synchronize()
s = stamps.cpu().numpy().astype(np.float64)
rel = (s - s[:, :1]) / 100.0        # us at 100 MHz
med = np.median(rel[20:], 0)
print('steady-state period %.1f us' % np.median(np.diff(s[20:, 0]) / 100.0))
for n, v in zip(names, med):
    print(f'{n:32s} {v:8.1f} us')
print('step end       %8.1f us' % max(med[4], med[7]))
