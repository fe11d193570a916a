"""Generates ``tests/golden/center_head.npz``: the reference's own ``CenterHead`` (mmdet3d/models/dense_heads/
centerpoint_head.py) and ``LiDARInstance3DBoxes``, run on the CPU.

    python tests/golden/make_golden_center_head.py

Imports the reference behind the stubs of ``_ref_import.py`` (read-only tree, nothing copied) and the few more this
head needs, restated here from mmcv 1.x / mmdet 2.x (neither is part of the reference tree): ``ConvModule`` (conv, bn,
ReLU), ``multi_apply``, ``reduce_mean`` (identity without torch.distributed), ``GaussianFocalLoss`` and ``L1Loss`` with
``weight_reduce_loss`` (``loss.sum() / (avg_factor + finfo(float32).eps)`` under reduction 'mean', mmdet 2.19 and
later).  gaussian_radius / draw_heatmap_gaussian and clip_sigmoid are the reference's own.

Small case: the reference config's six tasks and ten classes on a 32 x 24 map (W != H; grid 128 x 96, voxel 0.125,
out_size_factor 4), max_objs 8, min_radius 2, B = 3:

* sample 0: two boxes on the same cell, a centre in (-1, 0) cells, centres outside the map, a zero-width box, two
  corners, interleaved classes of tasks 1 and 2, large boxes (radii above min_radius), more than max_objs boxes of task 5;
* sample 1: no boxes;
* sample 2: boxes at all four borders, centres outside the map, a negative length, random boxes (more than max_objs
  cars in all, so the last of them are truncated).  Task 3 (barrier) has no box.

Stored: the boxes, labels, targets of every task, the heatmap == 1 counts, the head forward (seeded state_dict, eval
mode) and its state_dict, the losses with task_specific True and False and the gradients w.r.t. the five head outputs and
the logits of both, and the reference config's head dict (JSON) with its state_dict keys and shapes.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402

REF = _ref_import.REF
B = 3
IN_CH, SHARE, HEAD_CONV = 16, 8, 8
CFG = dict(point_cloud_range=[-8.0, -6.0, -5.0, 8.0, 6.0, 3.0], grid_size=[128, 96, 40], voxel_size=[0.125, 0.125, 0.2],
           out_size_factor=4, dense_reg=1, gaussian_overlap=0.1, max_objs=8, min_radius=2,
           code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2])
TASKS = [dict(num_class=1, class_names=['car']), dict(num_class=2, class_names=['truck', 'construction_vehicle']),
         dict(num_class=2, class_names=['bus', 'trailer']), dict(num_class=1, class_names=['barrier']),
         dict(num_class=2, class_names=['motorcycle', 'bicycle']),
         dict(num_class=2, class_names=['pedestrian', 'traffic_cone'])]
COMMON = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2))


class ConvModule(nn.Module):
    """mmcv 1.x ConvModule with norm_cfg BN2d, default ReLU, order conv -> norm -> act, bias='auto'."""

    def __init__(self, c_in, c_out, kernel_size, stride=1, padding=0, bias='auto', conv_cfg=None, norm_cfg=None,
                 **kw):
        super().__init__()
        self.conv = nn.Conv2d(c_in, c_out, kernel_size, stride=stride, padding=padding,
                              bias=(norm_cfg is None) if bias == 'auto' else bias)
        self.bn = nn.BatchNorm2d(c_out)
        self.activate = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.activate(self.bn(self.conv(x)))


class BaseModule(nn.Module):
    """mmcv 1.x BaseModule's constructor (init_cfg kept, not applied: the golden weights are set explicitly)."""

    def __init__(self, init_cfg=None):
        super().__init__()
        self.init_cfg = init_cfg


def multi_apply(func, *args, **kwargs):
    return tuple(map(list, zip(*map(lambda *a: func(*a, **kwargs), *args))))


def weight_reduce_loss(loss, weight=None, reduction='mean', avg_factor=None):
    if weight is not None:
        loss = loss * weight
    if avg_factor is None:
        return loss.mean() if reduction == 'mean' else (loss.sum() if reduction == 'sum' else loss)
    if reduction == 'mean':
        return loss.sum() / (avg_factor + torch.finfo(torch.float32).eps)
    return loss


class GaussianFocalLoss(nn.Module):
    def __init__(self, alpha=2.0, gamma=4.0, reduction='mean', loss_weight=1.0, **kw):
        super().__init__()
        self.alpha, self.gamma, self.reduction, self.loss_weight = alpha, gamma, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        eps = 1e-12
        pos_weights = target.eq(1)
        neg_weights = (1 - target).pow(self.gamma)
        pos_loss = -(pred + eps).log() * (1 - pred).pow(self.alpha) * pos_weights
        neg_loss = -(1 - pred + eps).log() * pred.pow(self.alpha) * neg_weights
        return self.loss_weight * weight_reduce_loss(pos_loss + neg_loss, weight, self.reduction, avg_factor)


class L1Loss(nn.Module):
    def __init__(self, reduction='mean', loss_weight=1.0, **kw):
        super().__init__()
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        if target.numel() == 0:
            loss = pred.sum() * 0
        else:
            loss = torch.abs(pred - target)
        return self.loss_weight * weight_reduce_loss(loss, weight, self.reduction, avg_factor)


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def import_reference():
    _ref_import.install()
    import importlib
    mods = {}
    mods['gauss'] = _load('mmdet3d.core.utils.gaussian', REF + '/mmdet3d/core/utils/gaussian.py')
    mods['clip'] = _load('mmdet3d.models.utils.clip_sigmoid', REF + '/mmdet3d/models/utils/clip_sigmoid.py')
    core = _ref_import._pkg('mmdet3d.core', REF + '/mmdet3d/core')
    core.circle_nms = core.xywhr2xyxyr = None
    core.draw_heatmap_gaussian = mods['gauss'].draw_heatmap_gaussian
    core.gaussian_radius = mods['gauss'].gaussian_radius
    _ref_import._mod('mmdet3d.core.post_processing', nms_bev=None)
    _ref_import._mod('mmdet3d.core.utils', array_converter=lambda *a, **k: (lambda f: f))
    _ref_import._mod('mmdet3d.core.points', BasePoints=object)
    _ref_import._pkg('mmdet3d.core.bbox', REF + '/mmdet3d/core/bbox')
    _ref_import._pkg('mmdet3d.core.bbox.structures', REF + '/mmdet3d/core/bbox/structures')
    _ref_import._mod('mmcv.ops', box_iou_rotated=None, points_in_boxes_all=None, points_in_boxes_part=None)
    _ref_import._mod('mmdet3d.models.utils', clip_sigmoid=mods['clip'].clip_sigmoid)
    sys.modules['mmcv.cnn'].ConvModule = ConvModule
    sys.modules['mmcv.runner'].BaseModule = BaseModule
    _ref_import._mod('mmdet.core', build_bbox_coder=lambda cfg: None, multi_apply=multi_apply,
                     reduce_mean=lambda t: t)
    losses = dict(GaussianFocalLoss=GaussianFocalLoss, L1Loss=L1Loss)
    builder = sys.modules['mmdet3d.models.builder']
    builder.HEADS = _ref_import._Registry()
    builder.build_loss = lambda cfg: losses[cfg['type']](**{k: v for k, v in cfg.items() if k != 'type'})
    _ref_import._pkg('mmdet3d.models.dense_heads', REF + '/mmdet3d/models/dense_heads')
    cph = importlib.import_module('mmdet3d.models.dense_heads.centerpoint_head')
    builder.build_head = lambda cfg: getattr(cph, cfg['type'])(**{k: v for k, v in cfg.items() if k != 'type'})
    lidar = importlib.import_module('mmdet3d.core.bbox.structures.lidar_box3d')
    return cph, lidar.LiDARInstance3DBoxes


def make_boxes(rng):
    """(boxes (n, 9) float32 with bottom-centre z, labels) per sample."""
    cell = 0.5                                 # metres per map cell
    x0, y0 = -8.0, -6.0

    def box(cx, cy, w, l, label, z=-1.0, h=1.5):
        return [x0 + cx * cell, y0 + cy * cell, z, w, l, h, rng.uniform(-3.1, 3.1), rng.normal(), rng.normal()], label

    s0 = [box(5.3, 4.2, 1.9, 4.5, 0), box(5.6, 4.7, 2.0, 4.0, 0),                    # two cars on one cell
          box(-0.5, 11.5, 2.0, 4.0, 0),                                              # centre in (-1, 0) cells: kept
          box(-1.2, 5.5, 2.0, 4.0, 0), box(8.5, 26.5, 2.0, 4.0, 0),                  # out of range in x, in y
          box(9.5, 19.5, 0.0, 4.0, 0),                                               # width 0
          box(0.3, 0.2, 1.8, 4.2, 0), box(31.7, 23.6, 1.9, 4.4, 0),                  # corners
          box(10.5, 8.5, 2.5, 7.0, 2), box(12.2, 9.1, 2.6, 8.0, 1), box(14.8, 3.3, 2.4, 6.5, 2),  # task 1 interleaved
          box(20.1, 10.2, 2.9, 12.0, 4), box(22.4, 14.6, 3.0, 11.0, 3), box(18.3, 6.6, 2.8, 10.5, 4),  # task 2
          box(26.0, 4.0, 15.0, 20.0, 1)]                                             # very large: radius > 2
    for k in range(10):                                                              # task 5: 10 > max_objs boxes
        s0.append(box(rng.uniform(2, 30), rng.uniform(2, 22), 0.7, 0.8, 8 + (k % 2)))
    for k in range(3):
        s0.append(box(rng.uniform(2, 30), rng.uniform(2, 22), 0.8, 1.9, 6 + (k % 2)))
    s2 = [box(6.5, 6.5, 2.0, 4.5, 0), box(20.5, 12.5, 0.6, 0.7, 9), box(25.3, 18.9, 2.5, 9.0, 2),
          box(0.6, 12.2, 2.0, 4.0, 0), box(16.2, 23.4, 2.0, 4.0, 0),                 # left / bottom borders
          box(31.4, 2.2, 2.0, 4.0, 0), box(14.2, 0.4, 2.0, 4.0, 0),                  # right / top borders
          box(33.5, 5.5, 2.0, 4.0, 0), box(8.5, -2.5, 2.0, 4.0, 0),                  # out of range in x, in y
          box(11.5, 19.5, 2.0, -1.0, 0)]                                             # negative length
    for _ in range(12):
        lab = int(rng.choice([0, 1, 2, 4, 6, 7, 8, 9]))
        s2.append(box(rng.uniform(-3, 35), rng.uniform(-3, 27), rng.uniform(0.5, 3), rng.uniform(0.5, 9), lab,
                      z=rng.uniform(-2, 0), h=rng.uniform(0.8, 3)))
    out = []
    for s in (s0, [], s2):
        b = np.array([v[0] for v in s], np.float32).reshape(-1, 9)
        lab = np.array([v[1] for v in s], np.int64)
        out.append((b, lab))
    return out


def head_cfg(task_specific):
    return dict(in_channels=IN_CH, tasks=TASKS, common_heads=COMMON, share_conv_channel=SHARE,
                separate_head=dict(type='SeparateHead', init_bias=-2.19, final_kernel=3, head_conv=HEAD_CONV),
                loss_cls=dict(type='GaussianFocalLoss', reduction='mean'),
                loss_bbox=dict(type='L1Loss', reduction='mean', loss_weight=0.25), norm_bbox=True,
                train_cfg=CFG, task_specific=task_specific)


def reference_config():
    """The reference config's pts_bbox_head with train_cfg.pts and test_cfg.pts, as the model builder merges them."""
    ns = {}
    src = open(REF + '/configs/ocrfdet/ocrfdet.py').read()
    exec(compile(src, 'ocrfdet.py', 'exec'), ns)
    head = dict(ns['model']['pts_bbox_head'])
    head['train_cfg'] = ns['model']['train_cfg']['pts']
    head['test_cfg'] = ns['model']['test_cfg']['pts']
    return head


def main():
    cph, Boxes = import_reference()
    rng = np.random.default_rng(20261015)
    samples = make_boxes(rng)
    out = {}
    for b, (bx, lab) in enumerate(samples):
        out[f'boxes{b}'] = bx
        out[f'labels{b}'] = lab
    gt_boxes = [Boxes(torch.from_numpy(bx), box_dim=9) for bx, _ in samples]
    gt_labels = [torch.from_numpy(lab) for _, lab in samples]

    torch.manual_seed(0)
    head = cph.CenterHead(**head_cfg(True))
    gen = torch.Generator().manual_seed(1)
    state = {}
    for k, v in head.state_dict().items():
        if v.dtype.is_floating_point:
            w = torch.randn(v.shape, generator=gen) * (0.5 if 'weight' in k else 0.2)
            if k.endswith('running_var'):
                w = 0.5 + torch.rand(v.shape, generator=gen)
            v = w.half().float()
        state[k] = v
    head.load_state_dict(state)
    head.eval()
    for k, v in state.items():
        out['state.' + k] = v.numpy()
    x = (torch.randn(B, IN_CH, 24, 32, generator=gen)).half().float()
    out['x'] = x.numpy()
    with torch.no_grad():
        preds = head([x])
    names = list(COMMON) + ['heatmap']
    for t in range(len(TASKS)):
        for n in names:
            out[f'fwd.t{t}.{n}'] = preds[t][0][n].numpy()

    hm, anno, ind, mask = head.get_targets(gt_boxes, gt_labels)
    for t in range(len(TASKS)):
        out[f'heatmap{t}'] = hm[t].numpy()
        out[f'anno_box{t}'] = anno[t].numpy()
        out[f'ind{t}'] = ind[t].numpy()
        out[f'mask{t}'] = mask[t].numpy()
        out[f'num_pos{t}'] = np.float32(hm[t].eq(1).float().sum().item())

    for ts in (True, False):
        tag = 'ts' if ts else 'all'
        head.task_specific = ts
        leaves, dicts = [], []
        for t in range(len(TASKS)):
            d = {}
            for n in names:
                leaf = torch.from_numpy(out[f'fwd.t{t}.{n}'].copy()).requires_grad_(True)
                leaves.append((t, n, leaf))
                d[n] = leaf.clone()            # the reference's clip_sigmoid runs sigmoid_ in place
            dicts.append([d])
        ld = head.loss(gt_boxes, gt_labels, tuple(dicts))
        total = sum(v for v in ld.values())
        total.backward()
        keys = sorted(ld)
        out[f'loss_keys.{tag}'] = np.array(json.dumps(keys))
        out[f'losses.{tag}'] = np.array([float(ld[k]) for k in keys], np.float64)
        out[f'losses32.{tag}'] = np.array([ld[k].detach().float().item() for k in keys], np.float32)
        for t, n, leaf in leaves:
            out[f'grad.{tag}.t{t}.{n}'] = leaf.grad.numpy()

    ref_cfg = reference_config()
    out['ref_config'] = np.array(json.dumps(ref_cfg))
    ref_head = cph.CenterHead(**{k: v for k, v in ref_cfg.items() if k != 'type'})
    out['ref_keys'] = np.array(json.dumps({k: list(v.shape) for k, v in ref_head.state_dict().items()}))
    out['small_keys'] = np.array(json.dumps({k: list(v.shape) for k, v in state.items()}))
    out['cfg'] = np.array(json.dumps(dict(train_cfg=CFG, tasks=TASKS, in_ch=IN_CH, share=SHARE, head_conv=HEAD_CONV)))
    path = os.path.join(HERE, 'center_head.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    for t in range(len(TASKS)):
        print(t, 'mask', out[f'mask{t}'].sum(1), 'num_pos', out[f'num_pos{t}'])


if __name__ == '__main__':
    main()
