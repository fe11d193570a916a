"""A/B of HotPath(fuse_hoa_stats=...) at cfg2 in ONE process: HOA-3's channel statistics written by the HT pooling's
epilogue (on) against a statistics launch of their own (off: the parent's launches).  Both instances take the defaults
bench.py takes ('init' Gaussians, cached rank vectors, panel poolings, renders on the side stream) and are warmed; a
full-size step of each is compared bit for bit first; then PAIRS alternating blocks of STEPS steps are timed, every
block bracketed by a synchronise on both sides like bench.py's `timed`.
    python tools/ab_hoa_stats.py [--pairs 9] [--steps 200] [--out profiles/hoa_stats_fused_ab.txt]
The gain counts as shown if the fused arm is faster in every adjacent pair but at most one AND the median gain exceeds
the off arm's own block-to-block range (max - min); the file says which."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ocrfdet_amd import hotpath, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--pairs', type=int, default=9)
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--warmup', type=int, default=20)
ap.add_argument('--config', default='cfg2_6cam_2frame_bev200x200_render_hoa')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hoa_stats_fused_ab.txt'))
a = ap.parse_args()
assert a.pairs >= 7, 'at least 7 pairs of blocks'
dev = torch.device('cuda:0')
cfg = synthetic.CONFIGS[a.config]
arms = {'off': hotpath.HotPath(cfg, dev, fuse_hoa_stats=False), 'on': hotpath.HotPath(cfg, dev, fuse_hoa_stats=True)}
depth, feat = arms['on'].make_inputs(seed=0)
lines = [f'{a.config}: HotPath(fuse_hoa_stats=False) [off = the parent\'s launches] against True [on], one process, '
         f'{a.pairs} alternating pairs of blocks of {a.steps} steps, ms per step']


def say(s):
    print(s, flush=True)
    lines.append(s)


# ---- same results first: every output of a full-size step, call by call (step 1) and replayed (step 3) -------------
for k in range(3):
    outs = {}
    for name, hp in arms.items():
        outs[name] = list(hotpath.HotPath._flat_outputs(hp.step(depth, feat)))
    torch.cuda.synchronize()
    same = len(outs['on']) == len(outs['off']) and all(torch.equal(x, y) for x, y in zip(outs['on'], outs['off']))
    say(f'step {k + 1}: {len(outs["on"])} output tensors, torch.equal between the arms: {same}')
    if not same:
        sys.exit('the arms disagree')
for name, hp in arms.items():
    hp.check_render_plans()
    names = next(iter(hp._compiled.values())).step.names if hp._compiled else ()
    say(f'{name}: one host call per step: {bool(hp._compiled)} ({hp.one_call_refused}); recorded calls: {len(names)}, '
        f'ocrf_hoa_channel_stats x {names.count("ocrf_hoa_channel_stats")}, '
        f'ocrf_bev_pool_v2_nchw_panel_stats x {names.count("ocrf_bev_pool_v2_nchw_panel_stats")}')


def timed(hp, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        hp.step(depth, feat)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


for hp in arms.values():
    timed(hp, a.warmup)
ms = {'off': [], 'on': []}
for p in range(a.pairs):
    order = ('off', 'on') if p % 2 == 0 else ('on', 'off')          # neither arm always runs behind the other
    for name in order:
        ms[name].append(timed(arms[name], a.steps))
    say(f'pair {p + 1}: off {ms["off"][-1]:.4f}  on {ms["on"][-1]:.4f}  off - on {1e3 * (ms["off"][-1] - ms["on"][-1]):+.2f} us'
        f'  (first: {order[0]})')
for name in ('off', 'on'):
    v = ms[name]
    say(f'{name:3s}: median {statistics.median(v):.4f}  min {min(v):.4f}  max {max(v):.4f}  range {1e3 * (max(v) - min(v)):.2f} us')
diffs = [x - y for x, y in zip(ms['off'], ms['on'])]
gain = statistics.median(ms['off']) - statistics.median(ms['on'])
off_range = max(ms['off']) - min(ms['off'])
faster = sum(d > 0 for d in diffs)
say(f'on faster in {faster} of {len(diffs)} pairs; median gain {1e3 * gain:+.2f} us ({100 * gain / statistics.median(ms["off"]):+.2f} %); '
    f'median of the per-pair differences {1e3 * statistics.median(diffs):+.2f} us; off arm\'s own range {1e3 * off_range:.2f} us')
shown = faster >= len(diffs) - 1 and gain > off_range
say('GAIN SHOWN (faster in all pairs but at most one, median gain beyond the off arm\'s range)' if shown else
    'NO GAIN SHOWN by the rule (faster in all pairs but at most one AND median gain beyond the off arm\'s range)')
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
