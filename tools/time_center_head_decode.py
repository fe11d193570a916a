"""Times CenterHead.get_bboxes_padded at the reference shape (128 x 128, six tasks, the reference config's coder and
test_cfg, K = 500) at B = 1 and B = 8 on a peaked and an at-initialisation heatmap: fused (csrc/center_decode.hip)
against the torch formulation, with the device launches and host synchronisations of each.

    python tools/time_center_head_decode.py [--iters 20] [--out profiles/center_head_decode_timing.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.test_center_head_decode_gpu import full_preds  # noqa: E402
from tools.time_center_head import launches, syncs, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default='profiles/center_head_decode_timing.json')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(shape=dict(H=128, W=128, tasks=6, max_num=500, pre_max_size=1000, post_max_size=83))
    for B in (1, 8):
        for kind in ('peaked', 'init'):
            head, pd = full_preds(dev, kind, B=B)
            cell = {}
            for name, fused in (('fused', True), ('torch', False)):
                head.fused_decode = fused

                def fn():
                    head.get_bboxes_padded(pd)
                iters = a.iters if fused else max(3, a.iters // 4)
                cell[name] = dict(timed(fn, iters), launches=launches(fn), host_syncs=syncs(fn))
            head.fused_decode = True
            cell['kept'] = head.get_bboxes_padded(pd)[3].tolist()
            cell['speedup_fused_vs_torch'] = cell['torch']['median_ms'] / cell['fused']['median_ms']
            res[f'B{B}_{kind}'] = cell
    res['reference_syncs_derived'] = (
        'counted from the reference code, not measured: per task the coder decode makes 1 (post_center_range '
        'torch.tensor from a list is a host-to-device copy) and per sample the boolean-mask indexing 3; per sample '
        'and rotate task get_task_detections makes about 6 (mask indexing, the nms_rotated keep readback, post-range '
        'indexing), per circle task 2 (.cpu().numpy() and the keep list back); at B = 8 and six tasks about '
        '6 + 8 * 6 * 3 + 8 * (5 * 6 + 2) = 406 per call')
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
