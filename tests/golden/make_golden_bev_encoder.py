"""Generates ``tests/golden/bev_encoder.npz``: the reference's own ``CustomResNet`` (mmdet3d/models/backbones/resnet.py)
and ``FPN_LSS`` (mmdet3d/models/necks/lss_fpn.py), run on the CPU.

    python tests/golden/make_golden_bev_encoder.py

The two files are imported from where they lie (read-only tree, nothing copied) behind stubs of this script's own:
``mmcv.cnn.build_norm_layer`` as ``('bn', nn.BatchNorm2d(C))``, the ``NECKS`` / ``BACKBONES`` registries as no-ops, and
``mmdet.models.backbones.resnet.{BasicBlock, Bottleneck}`` as the restatement of mmdet 2.x below (mmdet is not part of
the reference tree).  The fixture therefore pins ``FPN_LSS`` completely and ``CustomResNet``'s wiring against the
reference's own code; it does NOT pin the two block classes, which are this script's reading of mmdet 2.x.

Cases (B = 2):

* ``resnet``: ``CustomResNet(8, num_channels=[16, 32, 64])`` on (2, 8, 16, 24) -> three feature maps;
* ``pre``: the ``pre_process`` form, ``CustomResNet(8, num_layer=[2], num_channels=[8], stride=[1],
  backbone_output_ids=[0])``;
* ``bottle``: ``CustomResNet(8, num_layer=[2, 1], num_channels=[16, 32], stride=[2, 2], block_type='BottleNeck')``;
* ``fpn``: ``FPN_LSS(in_channels=80, out_channels=12)`` on the three feature maps of ``resnet`` (eval mode);
  ``fpn_noextra`` with ``extra_upsample=None``, ``fpn_lateral`` with ``lateral=16``, ``fpn_inconv`` with
  ``use_input_conv=True``.

Per case: the seeded ``state_dict`` (weights on a power-of-two grid scaled by the fan-in, so that they compress;
non-trivial BatchNorm running statistics), the inputs, and in ``eval()`` and in ``train()``: the outputs, the gradients
of ``sum(out * R)`` for a fixed random ``R`` w.r.t. the inputs and the parameters, and the BatchNorm running statistics
after the ``train()`` forward.  Of a parameter gradient every k-th element of the flattened tensor is stored
(``k = ceil(numel / FULL)``: all of a tensor of at most ``FULL`` elements) and its Euclidean norm.  The inputs are
stored once (``x``; the ``fpn*`` cases read ``resnet.eval.out0..2``).  Also the ``state_dict`` keys and shapes of the
reference config's ``img_bev_encoder_backbone``, ``img_bev_encoder_neck`` and ``pre_process`` dicts, built at full
channel counts.  The archive is written with fixed timestamps: it regenerates byte for byte.
"""
import importlib.util
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402  (REF and the module-shell helpers only; install() is not called)

REF = _ref_import.REF
FULL = 256


# ---------------------------------------------------------------------------------------- mmdet 2.x, restated
def build_norm_layer(cfg, num_features, postfix=''):
    return 'bn' + str(postfix), nn.BatchNorm2d(num_features)


class BasicBlock(nn.Module):
    """mmdet 2.x ``mmdet.models.backbones.resnet.BasicBlock`` (conv_cfg None, no dcn, no plugins)."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style='pytorch', with_cp=False,
                 conv_cfg=None, norm_cfg=dict(type='BN'), dcn=None, plugins=None, init_cfg=None):
        super().__init__()
        assert dcn is None and plugins is None
        self.norm1_name, norm1 = build_norm_layer(norm_cfg, planes, postfix=1)
        self.norm2_name, norm2 = build_norm_layer(norm_cfg, planes, postfix=2)
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.add_module(self.norm1_name, norm1)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.add_module(self.norm2_name, norm2)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride, self.dilation, self.with_cp = stride, dilation, with_cp

    @property
    def norm1(self):
        return getattr(self, self.norm1_name)

    @property
    def norm2(self):
        return getattr(self, self.norm2_name)

    def forward(self, x):
        identity = x
        out = self.conv1(x)
        out = self.norm1(out)
        out = self.relu(out)
        out = self.conv2(out)
        out = self.norm2(out)
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


class Bottleneck(nn.Module):
    """mmdet 2.x ``Bottleneck``: with ``style='pytorch'`` the 3x3 conv carries the stride."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style='pytorch', with_cp=False,
                 conv_cfg=None, norm_cfg=dict(type='BN'), dcn=None, plugins=None, init_cfg=None):
        super().__init__()
        assert style in ('pytorch', 'caffe') and dcn is None and plugins is None
        conv1_stride, conv2_stride = (1, stride) if style == 'pytorch' else (stride, 1)
        self.norm1_name, norm1 = build_norm_layer(norm_cfg, planes, postfix=1)
        self.norm2_name, norm2 = build_norm_layer(norm_cfg, planes, postfix=2)
        self.norm3_name, norm3 = build_norm_layer(norm_cfg, planes * self.expansion, postfix=3)
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, stride=conv1_stride, bias=False)
        self.add_module(self.norm1_name, norm1)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=conv2_stride, padding=dilation, dilation=dilation,
                               bias=False)
        self.add_module(self.norm2_name, norm2)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.add_module(self.norm3_name, norm3)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(getattr(self, self.norm1_name)(self.conv1(x)))
        out = self.relu(getattr(self, self.norm2_name)(self.conv2(out)))
        out = getattr(self, self.norm3_name)(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def import_reference():
    reg = _ref_import._Registry()
    _ref_import._mod('mmcv')
    _ref_import._mod('mmcv.cnn', build_norm_layer=build_norm_layer)
    _ref_import._mod('mmdet')
    _ref_import._mod('mmdet.models', NECKS=reg, BACKBONES=reg)
    _ref_import._mod('mmdet.models.backbones')
    _ref_import._mod('mmdet.models.backbones.resnet', BasicBlock=BasicBlock, Bottleneck=Bottleneck)
    fpn = _load('ref_lss_fpn', REF + '/mmdet3d/models/necks/lss_fpn.py')
    res = _load('ref_resnet', REF + '/mmdet3d/models/backbones/resnet.py')
    return res.CustomResNet, fpn.FPN_LSS


# ---------------------------------------------------------------------------------------- seeded state
def seeded_state(module, gen):
    """Conv weights = (integers in [-8, 8] from a normal) / 4 * 2^round(log2(fan_in^-1/2)); BatchNorm weight and
    running_var in [0.5, 1.5), biases and running_mean in [-0.5, 0.5), on a 1/64 grid (coarse grids compress)."""
    state = {}
    for k, v in module.state_dict().items():
        if not v.dtype.is_floating_point:
            state[k] = v.clone()
            continue
        if v.dim() == 4:
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]
            scale = 2.0 ** round(float(np.log2(fan_in ** -0.5)))
            w = torch.clamp(torch.round(torch.randn(v.shape, generator=gen) * 4), -8, 8) / 4 * scale
        else:
            u = torch.floor(torch.rand(v.shape, generator=gen) * 64) / 64
            w = u + 0.5 if k.endswith(('running_var', '.weight')) else u - 0.5
        state[k] = w.float()
    return state


def flat(tensors):
    return np.concatenate([np.asarray(t, np.float32).reshape(-1) for t in tensors])


def run_case(out, tag, module, state, inputs, call):
    """``call(module, leaves)`` -> list of output tensors.  Per case the float entries of the state_dict are one flat
    array in state_dict order, as float16, which holds the grid exactly (``.keys``: [key, shape, is_float] of every entry; integer entries are 0), the parameter
    gradients one flat array in ``named_parameters`` order."""
    out[f'{tag}.keys'] = np.array(json.dumps([[k, list(v.shape), bool(v.dtype.is_floating_point)]
                                              for k, v in state.items()]))
    assert all(v.dtype.is_floating_point or int(v) == 0 for v in state.values())
    out[f'{tag}.state'] = flat(v.numpy() for v in state.values() if v.dtype.is_floating_point).astype(np.float16)
    assert np.array_equal(out[f'{tag}.state'].astype(np.float32),
                          flat(v.numpy() for v in state.values() if v.dtype.is_floating_point))
    rgen = torch.Generator().manual_seed(7)
    weights = None
    for mode in ('eval', 'train'):
        module.load_state_dict(state)
        module.train(mode == 'train')
        module.zero_grad(set_to_none=True)
        leaves = [x.clone().requires_grad_(True) for x in inputs]
        outs = call(module, leaves)
        if weights is None:
            weights = [torch.round(torch.randn(o.shape, generator=rgen) * 4) / 4 for o in outs]
            for i, r in enumerate(weights):
                out[f'{tag}.R{i}'] = r.numpy()
        sum((o * r).sum() for o, r in zip(outs, weights)).backward()
        for i, o in enumerate(outs):
            out[f'{tag}.{mode}.out{i}'] = o.detach().numpy()
        for i, x in enumerate(leaves):
            if x.grad is not None:                 # FPN_LSS reads two of the three maps
                out[f'{tag}.{mode}.gx{i}'] = x.grad.numpy()
        grads, norms = [], []
        for k, p in module.named_parameters():
            g = p.grad.reshape(-1)
            norms.append(g.double().norm().item())
            grads.append(g[::-(-g.numel() // FULL)].numpy())
        out[f'{tag}.{mode}.gp'] = flat(grads)
        out[f'{tag}.{mode}.gnorm'] = np.array(norms, np.float64)
        if mode == 'train':
            out[f'{tag}.train.stat'] = flat(v.numpy() for k, v in module.state_dict().items() if 'running_' in k)
    return [out[f'{tag}.eval.out{i}'] for i in range(len(weights))]


def reference_config():
    ns = {}
    exec(compile(open(REF + '/configs/ocrfdet/ocrfdet.py').read(), 'ocrfdet.py', 'exec'), ns)
    return {k: dict(ns['model'][k]) for k in ('img_bev_encoder_backbone', 'img_bev_encoder_neck', 'pre_process')}


def save(path, arrays):
    """``np.savez_compressed`` with fixed timestamps (numpy stamps the members with the current time)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


RESNETS = dict(resnet=dict(numC_input=8, num_channels=[16, 32, 64]),
               pre=dict(numC_input=8, num_layer=[2], num_channels=[8], stride=[1], backbone_output_ids=[0]),
               bottle=dict(numC_input=8, num_layer=[2, 1], num_channels=[16, 32], stride=[2, 2],
                           block_type='BottleNeck'))
FPNS = dict(fpn=dict(in_channels=80, out_channels=12),
            fpn_noextra=dict(in_channels=80, out_channels=12, extra_upsample=None),
            fpn_lateral=dict(in_channels=80, out_channels=12, lateral=16),
            fpn_inconv=dict(in_channels=80, out_channels=12, use_input_conv=True))


def main():
    torch.set_num_threads(1)
    CustomResNet, FPN_LSS = import_reference()
    gen = torch.Generator().manual_seed(20261018)
    out = {}
    x = (torch.round(torch.randn(2, 8, 16, 24, generator=gen) * 64) / 64).float()
    out['x'] = x.numpy()
    feats = None
    for tag, cfg in RESNETS.items():
        torch.manual_seed(0)
        m = CustomResNet(**cfg)
        res = run_case(out, tag, m, seeded_state(m, gen), [x], lambda mod, lv: mod(lv[0]))
        if tag == 'resnet':
            feats = [torch.from_numpy(f.copy()) for f in res]
    for tag, cfg in FPNS.items():
        torch.manual_seed(0)
        m = FPN_LSS(**cfg)
        run_case(out, tag, m, seeded_state(m, gen), feats, lambda mod, lv: [mod(lv)])
    out['cases'] = np.array(json.dumps(dict(resnets=RESNETS, fpns=FPNS, full=FULL)))
    ref_cfg = reference_config()
    out['ref_config'] = np.array(json.dumps(ref_cfg))
    keys = {}
    for name, cfg in ref_cfg.items():
        cls = dict(CustomResNet=CustomResNet, FPN_LSS=FPN_LSS)[cfg['type']]
        mod = cls(**{k: v for k, v in cfg.items() if k != 'type'})
        keys[name] = {k: list(v.shape) for k, v in mod.state_dict().items()}
    out['ref_keys'] = np.array(json.dumps(keys))
    path = os.path.join(HERE, 'bev_encoder.npz')
    save(path, out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
