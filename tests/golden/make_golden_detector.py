"""Generates ``tests/golden/detector.npz``: the reference's own ``BEVDet4D.prepare_inputs(stereo=True)``
(mmdet3d/models/detectors/bevdet.py:412-476) and ``OcRFDet4D.extract_img_feat`` (ocrfdet.py:206-279), run on the CPU.

    python tests/golden/make_golden_detector.py

``bevdet.py`` and ``ocrfdet.py`` are imported from where they lie (read-only tree, nothing copied) behind module shells:
``_ref_import.install()`` (which also gives the reference's ``get_mlp_input``), and on top of it, in this script, the
``DETECTORS`` registry as a no-op, an empty ``ResNet`` class, ``mmdet3d.models.builder``, ``CenterPoint``,
``TRTBEVPoolv2``, ``GridMask``, ``bbox3d2result``, ``cv2`` and ``matplotlib.pyplot``.  The detector is made with
``__new__`` and given its attributes by hand (``num_frame = 3``, ``temporal_frame = 2``, ``extra_ref_frames = 1``: what
``BEVStereo4D.__init__`` sets for ``num_adj = 1``).

Inputs (``make_inputs``, seeded): B = 2 samples, N = 2 cameras, F = 3 frames, images 3 x 8 x 8.  Camera mounts and ego
poses have random rotations that are not axis-aligned; ``ego2global`` translations are about 1e3 m, as nuScenes global
poses are, with a few metres of ego motion between the frames and a few centimetres between the cameras of a frame.
Everything is float32, as the reference takes it.

The sub-modules are the parameter-free stand-ins below; ``tests/test_detector_host.py`` runs this package's detector
with the same classes.  ``README_detector.md`` lists the arrays.  The archive is written with fixed timestamps: it
regenerates byte for byte.
"""
import importlib.util
import math
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
B, N, F, T, H, W = 2, 2, 3, 2, 8, 8
SEED = 20261019


# ------------------------------------------------------------------------------------------------ stand-ins
class Fn(nn.Module):
    """A parameter-free layer from a function; ``log`` (a list) receives ``name`` on every call."""

    def __init__(self, fn, name=None, log=None):
        super().__init__()
        self.fn, self.name, self.log = fn, name, log

    def forward(self, x):
        if self.log is not None:
            self.log.append(self.name)
        return self.fn(x)


class StandInBackbone(nn.Module):
    """Has what ``BEVDet.image_encoder`` and ``BEVStereo4D.extract_stereo_ref_feat`` touch of a ResNet: ``forward`` ->
    [stereo feature, feature], and the stem (``conv1``, ``norm1``, ``relu``, ``maxpool``) with ``layer1``.  ``log``
    records 'forward' per full forward and 'layer1' per evaluation of the stereo feature."""
    deep_stem = False
    res_layers = ['layer1']

    def __init__(self):
        super().__init__()
        self.log = []
        self.conv1 = Fn(lambda x: torch.cat([x[:, :1] + x[:, 1:2], 0.5 * x[:, 2:3] - 0.25 * x[:, :1]], 1))
        self.norm1 = Fn(lambda x: x - 0.125)
        self.relu = Fn(torch.tanh)
        self.maxpool = nn.AvgPool2d(2)
        self.layer1 = Fn(lambda x: 1.5 * x + 0.25, 'layer1', self.log)
        self.pool = nn.AvgPool2d(4)

    def forward(self, x):
        self.log.append('forward')
        stereo = self.layer1(self.maxpool(self.relu(self.norm1(self.conv1(x)))))
        return [stereo, torch.sin(self.pool(x)) + 0.5 * self.pool(x * x)]


class StandInNeck(nn.Module):
    def forward(self, feats):
        assert len(feats) == 1
        return [2.0 * feats[0] - 1.0]


def _fold(t, k):
    """(B, ...) -> (B,) float64: a weighted sum that depends on the order of the entries and on ``k``."""
    t = t.double().reshape(t.shape[0], -1)
    w = torch.cos(0.37 * (k + 1) * torch.arange(1, t.shape[1] + 1, dtype=torch.float64))
    return (t * w).sum(1) / t.shape[1]


class StandInViewTransformer(nn.Module):
    """Folds EVERY argument it receives into its outputs, each with a pattern and a coefficient of its own, so that a
    swapped, missing or stale argument changes them.  Poses enter with a small coefficient: the outputs stay O(1), and
    one float32 ulp in a pose moves them by less than 1e-7.  ``log`` records, per call, whether autograd was enabled and
    whether ``cv_feat_list[0]`` was None."""
    downsample = 16
    C, h, w = 2, 4, 4

    def __init__(self):
        super().__init__()
        self.log = []
        self.grid_config = dict(depth=[1.0, 60.0, 0.5])
        self.cv_frustum = torch.arange(24, dtype=torch.float32).view(2, 2, 2, 3) / 24
        self.grid_interval = torch.tensor([0.8, 0.8, 8.0])
        self.grid_lower_bound = torch.tensor([-1.6, -1.6, -5.0])

    def forward(self, inputs, metas):
        x, rot, tran, intrin, post_rot, post_tran, bda, mlp_input, img, wo_norm, wo_aug, c2w = inputs
        prev, stereo = metas['cv_feat_list']
        self.log.append(dict(grad=torch.is_grad_enabled(), prev_is_none=prev is None))
        nb = x.shape[0]
        per_view = lambda t: t.reshape(nb, -1)     # noqa: E731  ((B * N, ...) features -> per sample)
        terms = [(1.0, x), (0.01, rot), (0.01, tran), (1e-3, intrin), (0.1, post_rot), (0.01, post_tran), (0.1, bda),
                 (1e-3, mlp_input), (0.1, img), (0.1, wo_norm), (0.1, wo_aug), (0.01, c2w),
                 (0.01, metas['k2s_sensor']), (1e-3, metas['intrins']), (0.1, metas['post_rots']),
                 (0.01, metas['post_trans']), (1.0, per_view(stereo)),
                 (1.0, metas['frustum'].reshape(1, -1).expand(nb, -1))]
        if prev is not None:
            terms.append((1.0, per_view(prev)))
        n = self.C * self.h * self.w
        pos = torch.arange(n, dtype=torch.float64)
        out = torch.zeros(nb, n, dtype=torch.float64)
        for k, (coef, t) in enumerate(terms):
            out = out + coef * _fold(t, k)[:, None] * torch.sin(0.1 * (k + 1) * pos + k)
        scalars = metas['cv_downsample'] + 0.5 * metas['downsample'] + metas['grid_config']['depth'][2]
        out = out + (0.01 * scalars + (0.75 if prev is None else 0.0)) * torch.cos(0.3 * pos)
        bev = out.view(nb, self.C, self.h, self.w).to(x.dtype)
        depth = torch.sigmoid(bev[:, :1] + x.reshape(nb, -1).mean(1).view(nb, 1, 1, 1))
        bev_mask = (bev[:, 1:] * 2.0, torch.sigmoid(bev.flip(1)))
        extras = [bev * 0.5, img[:, 0], None, None, None, [0] * nb, None, None, None]
        return bev, depth, bev_mask, extras


class StandInPreProcess(nn.Module):
    def forward(self, x):
        return [0.5 * x + 0.125, x]


class StandInBEVBackbone(nn.Module):
    def forward(self, x):
        return [x]


class StandInBEVNeck(nn.Module):
    def forward(self, feats):
        return feats[0]


# ------------------------------------------------------------------------------------------------ inputs
def _rotation(n, gen):
    q, r = torch.linalg.qr(torch.randn(n, 3, 3, generator=gen, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1))[:, None, :]
    return q * torch.sign(torch.linalg.det(q))[:, None, None]


def _rigid(rot, trans):
    m = torch.eye(4, dtype=torch.float64).repeat(rot.shape[0], 1, 1)
    m[:, :3, :3], m[:, :3, 3] = rot, trans
    return m


def _small_motion(n, gen, angle, shift):
    """Rigid maps near the identity: a rotation of up to ``angle`` radians about a random axis, a shift of up to
    ``shift`` metres per axis."""
    axis = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    axis = axis / axis.norm(dim=1, keepdim=True) * (2 * torch.rand(n, 1, generator=gen, dtype=torch.float64) - 1) * angle
    K = torch.zeros(n, 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -axis[:, 2], axis[:, 1], -axis[:, 0]
    K = K - K.transpose(1, 2)
    return _rigid(torch.linalg.matrix_exp(K), (2 * torch.rand(n, 3, generator=gen, dtype=torch.float64) - 1) * shift)


def make_inputs(seed=SEED, b=B, n=N, f=F, h=H, w=W, scale=1e3):
    """The 12-entry ``img_inputs`` (float32): images (b, n * f, 3, h, w) camera-major, everything else (b, f * n, ...)
    frame-major, as ``prepare_inputs`` views them."""
    gen = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)      # noqa: E731
    imgs = torch.randn(b, n * f, 3, h, w, generator=gen, dtype=torch.float64)
    mount = _rigid(_rotation(b * n, gen), 3 * rand(b * n, 3) - 1.5).view(b, 1, n, 4, 4).expand(b, f, n, 4, 4)
    key = _rigid(_rotation(b, gen), scale * (2 * rand(b, 3) - 1)).view(b, 1, 1, 4, 4)
    motion = _small_motion(b * f * n, gen, 8 * math.pi / 180, 0.05).view(b, f, n, 4, 4)
    step = _small_motion(b * f, gen, 8 * math.pi / 180, 2.5).view(b, f, 1, 4, 4).clone()
    step[:, 0] = torch.eye(4, dtype=torch.float64)
    ego2globals = key @ step @ motion
    intrins = torch.zeros(b, f * n, 3, 3, dtype=torch.float64)
    intrins[:, :, 0, 0], intrins[:, :, 1, 1] = 1200 + 100 * rand(b, f * n), 1200 + 100 * rand(b, f * n)
    intrins[:, :, 0, 2], intrins[:, :, 1, 2], intrins[:, :, 2, 2] = 800 + 20 * rand(b, f * n), 450 + 20 * rand(b, f * n), 1
    post_rots = torch.eye(3, dtype=torch.float64).repeat(b, f * n, 1, 1)
    post_rots[:, :, :2, :2] = 0.44 * (torch.eye(2, dtype=torch.float64) + 0.1 * torch.randn(b, f * n, 2, 2, generator=gen,
                                                                                         dtype=torch.float64))
    post_trans = torch.cat([40 * rand(b, f * n, 2) - 20, torch.zeros(b, f * n, 1, dtype=torch.float64)], -1)
    bda = _rotation(b, gen) * (0.95 + 0.1 * rand(b, 1, 1))
    c2w = _rigid(_rotation(b * f * n, gen), 10 * rand(b * f * n, 3) - 5).view(b, f * n, 4, 4)
    out = [imgs, mount[..., :3, :3].reshape(b, f * n, 3, 3), mount[..., :3, 3].reshape(b, f * n, 3), intrins, post_rots,
           post_trans, bda, mount.reshape(b, f * n, 4, 4), ego2globals.reshape(b, f * n, 4, 4),
           0.5 * imgs + 0.5, 0.25 * imgs.flip(-1) + 0.5, c2w]
    return [t.float().contiguous() for t in out]


INPUT_NAMES = ('imgs', 'rots', 'trans', 'intrins', 'post_rots', 'post_trans', 'bda', 'sensor2egos', 'ego2globals',
               'imgs_wo_norm', 'imgs_wo_aug', 'c2w')
TUPLE_NAMES = ('imgs', 'rots', 'trans', 'intrins', 'post_rots', 'post_trans', 'bda', 'sensor2keyegos', 'ego2globals',
               'curr2adjsensor', 'imgs_wo_norm', 'imgs_wo_aug', 'c2w')


def give_stand_ins(det, with_prev, align=False):
    """The attributes ``extract_img_feat`` reads, on a reference detector or on this package's."""
    det.img_backbone, det.img_neck = StandInBackbone(), StandInNeck()
    det.img_view_transformer = StandInViewTransformer()
    det.pre_process, det.pre_process_net = True, StandInPreProcess()
    det.img_bev_encoder_backbone, det.img_bev_encoder_neck = StandInBEVBackbone(), StandInBEVNeck()
    det.with_prev, det.align_after_view_transfromation = with_prev, align
    return det


# ------------------------------------------------------------------------------------------------ the reference
def import_reference():
    import _ref_import
    vt = _ref_import.install()[0]
    REF = _ref_import.REF
    reg = _ref_import._Registry()
    sys.modules['mmdet.models'].DETECTORS = reg
    resnet = type('ResNet', (), {})
    sys.modules['mmdet.models.backbones.resnet'].ResNet = resnet
    sys.modules['mmdet3d.models'].builder = sys.modules['mmdet3d.models.builder']
    _ref_import._pkg('mmdet3d.models.detectors', REF + '/mmdet3d/models/detectors')
    _ref_import._mod('mmdet3d.models.detectors.centerpoint', CenterPoint=type('CenterPoint', (), {}))
    sys.modules['mmdet3d.ops.bev_pool_v2.bev_pool'].TRTBEVPoolv2 = object
    _ref_import._mod('mmdet3d.models.utils')
    _ref_import._mod('mmdet3d.models.utils.grid_mask', GridMask=object)
    _ref_import._mod('mmdet3d.core', bbox3d2result=None)
    _ref_import._mod('cv2')                                    # what ocrfdet.py imports on top of bevdet.py
    if 'matplotlib.pyplot' not in sys.modules:
        _ref_import._mod('matplotlib')
        _ref_import._mod('matplotlib.pyplot')
    mods = {}
    for name in ('bevdet', 'ocrfdet'):
        full = 'mmdet3d.models.detectors.' + name
        spec = importlib.util.spec_from_file_location(full, f'{REF}/mmdet3d/models/detectors/{name}.py')
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[full] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods['ocrfdet'].OcRFDet4D, resnet, vt.LSSViewTransformerBEVDepth.get_mlp_input


def reference_detector(OcRFDet4D, resnet, get_mlp_input, with_prev, training):
    det = give_stand_ins(OcRFDet4D.__new__(OcRFDet4D), with_prev)
    # the reference asks its view transformer for mlp_input, frame by frame: the reference's own function
    det.img_view_transformer = type('RefViewTransformer', (StandInViewTransformer,), dict(get_mlp_input=get_mlp_input))()
    # extract_stereo_ref_feat takes the ResNet branch for an instance of the class bevdet.py imported
    det.img_backbone = type('RefBackbone', (StandInBackbone, resnet), {})()
    det.num_frame, det.temporal_frame, det.extra_ref_frames = F, T, 1
    det.grid_mask, det.with_img_neck, det.training, det.grid = None, True, training, None
    return det


def main():
    torch.set_num_threads(1)
    sys.path.insert(0, HERE)
    from make_golden_bev_encoder import save
    OcRFDet4D, resnet, get_mlp_input = import_reference()
    inputs = make_inputs()
    out = {'in.' + k: t.numpy() for k, t in zip(INPUT_NAMES, inputs)}

    det = reference_detector(OcRFDet4D, resnet, get_mlp_input, True, True)
    ret = det.prepare_inputs(inputs, stereo=True)
    assert len(ret) == 13
    for name, entry in zip(TUPLE_NAMES, ret):
        if name == 'bda':
            out['pi.bda'] = entry.numpy()
        elif name == 'curr2adjsensor':
            assert len(entry) == F and all(e is None for e in entry[T:])
            out['pi.curr2adjsensor'] = torch.stack(entry[:T]).numpy()
        else:
            assert len(entry) == F
            out['pi.' + name] = torch.stack(entry).numpy()
    rots, trans, intrins, post_rots, post_trans, bda = ret[1:7]
    out['pi.mlp_input'] = torch.stack([get_mlp_input(None, rots[0], trans[0], intrins[f], post_rots[f], post_trans[f], bda)
                                       for f in range(F)]).numpy()
    # the float64 requirement: the same products in float32 miss the reference by far more than one float32 ulp
    s2e, e2g = inputs[7].view(B, F, N, 4, 4), inputs[8].view(B, F, N, 4, 4)
    f32 = torch.inverse(e2g[:, 0, 0])[:, None, None] @ e2g @ s2e
    out['pi.float32_error'] = np.float64((f32 - torch.stack(ret[7], 1)).abs().max())

    for tag, with_prev in (('prev', True), ('noprev', False)):
        for mode, training in (('train', True), ('eval', False)):
            det = reference_detector(OcRFDet4D, resnet, get_mlp_input, with_prev, training)
            got = det.extract_img_feat(inputs, None)
            assert len(got) == (4 if training else 3)
            x, depth, bev_mask = got[:3]
            pre = f'eif.{tag}.{mode}.'
            out[pre + 'x'], out[pre + 'depth'] = x[0].numpy(), depth.numpy()
            out[pre + 'bev_mask0'], out[pre + 'bev_mask1'] = bev_mask[0].numpy(), bev_mask[1].numpy()
            if training:
                out[pre + 'extras0'] = got[3][0].numpy()
            log = det.img_view_transformer.log
            out[pre + 'vt_grad'] = np.array([e['grad'] for e in log])
            out[pre + 'vt_prev_is_none'] = np.array([e['prev_is_none'] for e in log])
            out[pre + 'backbone_log'] = np.array(det.img_backbone.log)
            print(pre, tuple(x[0].shape), 'vt calls', len(log), 'backbone', det.img_backbone.log)
    path = os.path.join(HERE, 'detector.npz')
    save(path, out)
    print('float32 evaluation misses the reference by', out['pi.float32_error'])
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
