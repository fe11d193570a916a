"""Generates ``tests/golden/bev_align.npz``: the reference's own ``BEVDet4D.gen_grid`` / ``shift_feature``
(mmdet3d/models/detectors/bevdet.py:305-376), run on the CPU, beside a float64 restatement of the same formula.

    python tests/golden/make_golden_bev_align.py

``bevdet.py`` is imported from where it lies (read-only tree, nothing copied) behind module shells of this script's own:
``mmcv.runner.force_fp32`` as the identity, the ``DETECTORS`` registry as a no-op, and empty stand-ins for
``mmdet.models.backbones.resnet.ResNet``, ``mmdet3d.models.builder``, ``...detectors.centerpoint.CenterPoint``,
``mmdet3d.ops.bev_pool_v2.bev_pool.TRTBEVPoolv2``, ``mmdet3d.models.utils.grid_mask.GridMask`` and
``mmdet3d.core.bbox3d2result``.  The two methods are called unbound on a plain object with ``grid = None`` and an
``img_view_transformer`` that holds ``grid_interval`` / ``grid_lower_bound``.

Cases (n = 3 samples, v = 2 cameras, c = 2 channels): ``a`` 13 x 10 and ``b`` 16 x 24 with one BEV augmentation,
``c`` 16 x 24 with ``bda_adj != bda``, ``d`` 13 x 10 with flips in the augmentation.  Poses: a random rigid camera
mount, ego motion of up to 2.5 m and +-8 degrees of yaw between the frames, augmentation rotation +-22.5 degrees and
scale 0.95 ... 1.05; all float32, as the reference takes them.

Per case: the inputs; the reference's float32 normalised grid and output (``ref_grid``, ``ref_out``); the restatement
of gen_grid's formula in float64 with ``torch.linalg.inv`` on the float32 inputs (``tf``, ``grid``, ``out``: the
truth); and the reference's measured deviations from the truth, ``grid_err_px`` (pixels) and ``out_err``.  The script
asserts ``grid_err_px < 1e-3``: the restatement is the reference's formula.  The archive is written with fixed
timestamps: it regenerates byte for byte.
"""
import importlib.util
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402  (REF and the module-shell helpers only; install() is not called)
from make_golden_bev_encoder import save  # noqa: E402

REF = _ref_import.REF
GRID_INTERVAL = (0.8, 0.8, 8.0)


def import_reference():
    identity = lambda *a, **k: (lambda f: f)   # noqa: E731
    reg = _ref_import._Registry()
    _ref_import._mod('mmcv')
    _ref_import._mod('mmcv.runner', force_fp32=identity)
    _ref_import._mod('mmdet')
    _ref_import._mod('mmdet.models', DETECTORS=reg)
    _ref_import._mod('mmdet.models.backbones')
    _ref_import._mod('mmdet.models.backbones.resnet', ResNet=object)
    _ref_import._pkg('mmdet3d', REF + '/mmdet3d')
    models = _ref_import._pkg('mmdet3d.models', REF + '/mmdet3d/models')
    models.builder = _ref_import._mod('mmdet3d.models.builder')
    _ref_import._pkg('mmdet3d.models.detectors', REF + '/mmdet3d/models/detectors')
    _ref_import._mod('mmdet3d.models.detectors.centerpoint', CenterPoint=type('CenterPoint', (), {}))
    _ref_import._mod('mmdet3d.ops')
    _ref_import._mod('mmdet3d.ops.bev_pool_v2')
    _ref_import._mod('mmdet3d.ops.bev_pool_v2.bev_pool', TRTBEVPoolv2=object)
    _ref_import._mod('mmdet3d.models.utils')
    _ref_import._mod('mmdet3d.models.utils.grid_mask', GridMask=object)
    _ref_import._mod('mmdet3d.core', bbox3d2result=None)
    name = 'mmdet3d.models.detectors.bevdet'
    spec = importlib.util.spec_from_file_location(name, REF + '/mmdet3d/models/detectors/bevdet.py')
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m.BEVDet4D


def rot_z(a):
    c, s = torch.cos(a), torch.sin(a)
    m = torch.eye(3, dtype=torch.float64).repeat(a.shape[0], 1, 1)
    m[:, 0, 0], m[:, 0, 1], m[:, 1, 0], m[:, 1, 1] = c, -s, s, c
    return m


def rigid(rot, trans):
    m = torch.eye(4, dtype=torch.float64).repeat(rot.shape[0], 1, 1)
    m[:, :3, :3], m[:, :3, 3] = rot, trans
    return m


def random_rotation(n, gen):
    q, r = torch.linalg.qr(torch.randn(n, 3, 3, generator=gen, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1))[:, None, :]
    return q * torch.sign(torch.linalg.det(q))[:, None, None]


def uniform(n, lo, hi, gen):
    return lo + (hi - lo) * torch.rand(n, generator=gen, dtype=torch.float64)


def augmentation(n, gen, flips):
    m = rot_z(uniform(n, -math.pi / 8, math.pi / 8, gen)) * uniform(n, 0.95, 1.05, gen)[:, None, None]
    if flips:                                       # flip_dx / flip_dy of the reference's bev_transform
        m[0, 0] = -m[0, 0]
        m[1, 1] = -m[1, 1]
        m[2, 0], m[2, 1] = -m[2, 0], -m[2, 1]
    return m


def make_inputs(n, v, c, h, w, gen, other_adj, flips):
    mount = rigid(random_rotation(n * v, gen), uniform(n * v * 3, -1.5, 1.5, gen).view(-1, 3)).view(n, v, 4, 4)
    yaw = uniform(n, -8 * math.pi / 180, 8 * math.pi / 180, gen)
    move = torch.cat([uniform(n * 2, -2.5, 2.5, gen).view(n, 2), uniform(n, -0.1, 0.1, gen).view(n, 1)], 1)
    adj2key = rigid(rot_z(yaw), move)[:, None]
    inputs = dict(x=torch.randn(n, c, h, w, generator=gen, dtype=torch.float64),
                  curr=mount, adj=adj2key @ mount, bda=augmentation(n, gen, flips))
    if other_adj:
        inputs['bda_adj'] = augmentation(n, gen, False)
    inputs = {k: t.float() for k, t in inputs.items()}
    inputs['grid_interval'] = torch.tensor(GRID_INTERVAL)
    inputs['grid_lower_bound'] = torch.tensor([-0.5 * w * GRID_INTERVAL[0], -0.5 * h * GRID_INTERVAL[1], -5.0])
    return inputs


def truth(inp):
    """gen_grid's formula (bevdet.py:322-370) and grid_sample on the float32 inputs, in float64."""
    d = {k: t.double() for k, t in inp.items()}
    n, c, h, w = d['x'].shape

    def bda4(m):
        out = torch.zeros(n, 4, 4, dtype=torch.float64)
        out[:, :3, :3], out[:, 3, 3] = m, 1
        return out
    c02l0 = bda4(d['bda']) @ d['curr'][:, 0]
    c12l0 = bda4(d.get('bda_adj', d['bda'])) @ d['adj'][:, 0]
    l02l1 = c02l0 @ torch.linalg.inv(c12l0)
    keep = [0, 1, 3]
    l02l1 = l02l1[:, keep][:, :, keep]
    feat2bev = torch.zeros(3, 3, dtype=torch.float64)
    feat2bev[0, 0], feat2bev[1, 1] = d['grid_interval'][0], d['grid_interval'][1]
    feat2bev[0, 2], feat2bev[1, 2], feat2bev[2, 2] = d['grid_lower_bound'][0], d['grid_lower_bound'][1], 1
    tf = torch.linalg.inv(feat2bev) @ l02l1 @ feat2bev
    xs = torch.arange(w, dtype=torch.float64).view(1, w).expand(h, w)
    ys = torch.arange(h, dtype=torch.float64).view(h, 1).expand(h, w)
    pix = torch.stack([xs, ys, torch.ones_like(xs)], -1).view(1, h, w, 3, 1)
    pos = (tf.view(n, 1, 1, 3, 3) @ pix)[..., :2, 0]
    grid = pos / torch.tensor([w - 1.0, h - 1.0], dtype=torch.float64) * 2.0 - 1.0
    return tf, grid, F.grid_sample(d['x'], grid, align_corners=True)


CASES = dict(a=dict(h=13, w=10, other_adj=False, flips=False), b=dict(h=16, w=24, other_adj=False, flips=False),
             c=dict(h=16, w=24, other_adj=True, flips=False), d=dict(h=13, w=10, other_adj=False, flips=True))


def main():
    torch.set_num_threads(1)
    BEVDet4D = import_reference()
    gen = torch.Generator().manual_seed(20261018)
    out = {}
    for tag, cfg in CASES.items():
        inp = make_inputs(3, 2, 2, cfg['h'], cfg['w'], gen, cfg['other_adj'], cfg['flips'])
        det = type('Detector', (), {})()
        det.grid = None
        det.img_view_transformer = type('ViewTransformer', (), {})()
        det.img_view_transformer.grid_interval = inp['grid_interval']
        det.img_view_transformer.grid_lower_bound = inp['grid_lower_bound']
        det.gen_grid = lambda *a, _d=det, **k: BEVDet4D.gen_grid(_d, *a, **k)
        args = (inp['x'], [inp['curr'], inp['adj']], inp['bda'])
        ref_grid = BEVDet4D.gen_grid(det, *args, bda_adj=inp.get('bda_adj'))
        ref_out = BEVDet4D.shift_feature(det, *args, bda_adj=inp.get('bda_adj'))
        tf, grid, want = truth(inp)
        h, w = cfg['h'], cfg['w']
        scale = torch.tensor([(w - 1) / 2.0, (h - 1) / 2.0], dtype=torch.float64)
        grid_err_px = float(((ref_grid.double() - grid).abs() * scale).max())
        out_err = float((ref_out.double() - want).abs().max())
        assert grid_err_px < 1e-3, (tag, grid_err_px)
        for k, t in inp.items():
            out[f'{tag}.{k}'] = t.numpy()
        out[f'{tag}.ref_grid'], out[f'{tag}.ref_out'] = ref_grid.numpy(), ref_out.numpy()
        out[f'{tag}.tf'], out[f'{tag}.grid'], out[f'{tag}.out'] = tf.numpy(), grid.numpy(), want.numpy()
        out[f'{tag}.grid_err_px'], out[f'{tag}.out_err'] = np.float64(grid_err_px), np.float64(out_err)
        print(f'{tag}: {h} x {w}  grid_err_px {grid_err_px:.3e}  out_err {out_err:.3e}')
    path = os.path.join(HERE, 'bev_align.npz')
    save(path, out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
