"""Generates ``tests/golden/distill.npz``: the reference's own ``OcRFDet4DVGGT.build_cost_volume(method='group_corr')``
and ``get_pair_indices`` (mmdet3d/models/detectors/ocrfdet_vggt.py:166-230) and ``CrossAttentionAlign``
(bevdet_vggt.py:16-49), run on the CPU.

    python tests/golden/make_golden_distill.py

``bevdet_vggt.py`` and ``ocrfdet_vggt.py`` are imported from where they lie (read-only tree, nothing copied) behind the
module shells of this script: ``mmcv.runner.force_fp32``, the ``DETECTORS`` registry as a no-op, empty ``ResNet``,
``CenterPoint``, ``GridMask``, ``TRTBEVPoolv2`` and ``Aggregator`` classes, ``mmdet3d.models.builder``,
``bbox3d2result``, ``cv2`` and ``matplotlib.pyplot``.  ``build_cost_volume`` and ``get_pair_indices`` use nothing of
``self`` and are called on the class.  The two losses are the torch calls of ocrfdet_vggt.py:476-480 on a recorded
volume pair.  ``README_distill.md`` lists the arrays.  The archive is written with fixed timestamps: it regenerates
byte for byte.
"""
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import REF  # noqa: E402  (where the reference tree lies; nothing else of that module is used)

SEED = 20261020
ALIGN = dict(res_dim=6, vit_dim=16, num_heads=2)
VOLUMES = dict(a=dict(shape=(2, 2, 12, 3, 7), max_disp=4, groups=4),        # Cg = 3
               b=dict(shape=(1, 2, 6, 2, 3), max_disp=4, groups=3))         # W < D: columns clamp


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _pkg(name, path):
    m = _mod(name)
    m.__path__ = [path]
    return m


def import_reference():
    registry = type('Registry', (), dict(register_module=lambda self, *a, **k: (lambda cls: cls)))()
    empty = lambda name: type(name, (), {})                                   # noqa: E731
    _mod('mmcv')
    _mod('mmcv.runner', force_fp32=lambda *a, **k: (lambda f: f))
    _mod('mmdet')
    _mod('mmdet.models', DETECTORS=registry)
    _mod('mmdet.models.backbones')
    _mod('mmdet.models.backbones.resnet', ResNet=empty('ResNet'))
    _pkg('mmdet3d', REF + '/mmdet3d')
    _mod('mmdet3d.core', bbox3d2result=None)
    _mod('mmdet3d.ops')
    _mod('mmdet3d.ops.bev_pool_v2')
    _mod('mmdet3d.ops.bev_pool_v2.bev_pool', TRTBEVPoolv2=object)
    models = _pkg('mmdet3d.models', REF + '/mmdet3d/models')
    models.builder = _mod('mmdet3d.models.builder')
    _mod('mmdet3d.models.utils')
    _mod('mmdet3d.models.utils.grid_mask', GridMask=object)
    for name in ('backbones', 'backbones.vggt', 'backbones.vggt.vggt', 'backbones.vggt.vggt.models'):
        _mod('mmdet3d.models.' + name)
    _mod('mmdet3d.models.backbones.vggt.vggt.models.aggregator', Aggregator=empty('Aggregator'))
    _pkg('mmdet3d.models.detectors', REF + '/mmdet3d/models/detectors')
    _mod('mmdet3d.models.detectors.centerpoint', CenterPoint=empty('CenterPoint'))
    _mod('cv2')
    if 'matplotlib.pyplot' not in sys.modules:
        _mod('matplotlib')
        _mod('matplotlib.pyplot')
    mods = {}
    for name in ('bevdet_vggt', 'ocrfdet_vggt'):
        full = 'mmdet3d.models.detectors.' + name
        spec = importlib.util.spec_from_file_location(full, f'{REF}/mmdet3d/models/detectors/{name}.py')
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[full] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods['ocrfdet_vggt'].OcRFDet4DVGGT, mods['bevdet_vggt'].CrossAttentionAlign


def main():
    torch.set_num_threads(1)
    from make_golden_bev_encoder import save
    Detector, CrossAttentionAlign = import_reference()
    gen = torch.Generator().manual_seed(SEED)
    out = {}
    for tag, cfg in VOLUMES.items():
        feats = torch.randn(*cfg['shape'], generator=gen)
        out[f'vol.{tag}.feats'] = feats.numpy()
        out[f'vol.{tag}.out'] = Detector.build_cost_volume(None, feats, max_disp=cfg['max_disp'], method='group_corr',
                                                           groups=cfg['groups']).numpy()
    # the aligner: one state, its input pair and its output
    torch.manual_seed(SEED)
    aligner = CrossAttentionAlign(**ALIGN).eval()
    res_feat = torch.randn(1, 2, ALIGN['res_dim'], 2, 3, generator=gen)
    vit_feat = torch.randn(1, 2, ALIGN['vit_dim'], 3, 5, generator=gen)
    with torch.no_grad():
        out['align.out'] = aligner(res_feat, vit_feat).numpy()
    out['align.res_feat'], out['align.vit_feat'] = res_feat.numpy(), vit_feat.numpy()
    for k, v in aligner.state_dict().items():
        out['align.state.' + k] = v.numpy()
    # the two losses of ocrfdet_vggt.py:476-480 for a volume pair; differences around the smooth-L1 kink included
    F_ts = [torch.randn(2, 4, 5, 3, 7, generator=gen), torch.randn(2, 4, 5, 3, 7, generator=gen)]
    out['kd.volume_t'], out['kd.volume_s'] = F_ts[0].numpy(), F_ts[1].numpy()
    loss_Smoothl1_KD = F.smooth_l1_loss(F_ts[0], F_ts[1], beta=1.0) * 0.1
    loss_cos_KD = 1 - F.cosine_similarity(F_ts[0].flatten(1), F_ts[1].flatten(1), dim=1).mean()
    out['kd.losses'] = np.array([loss_Smoothl1_KD.item(), loss_cos_KD.item()], np.float32)
    # the pair draw under a seed
    random.seed(SEED)
    out['pairs'] = np.array([Detector.get_pair_indices(None) for _ in range(24)], np.int64)
    path = os.path.join(HERE, 'distill.npz')
    save(path, out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays; pairs', sorted(set(map(tuple, out['pairs']))))


if __name__ == '__main__':
    main()
