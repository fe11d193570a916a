"""The mmdet 2.x / mmcv building blocks every native module of the detector is made of: ``BasicBlock`` and ``Bottleneck``
(``mmdet.models.backbones.resnet``), ``ConvModule``, ``build_norm_layer``, ``kaiming_init`` and the registry's
``build``, restated for the arguments the reference passes and close neighbours, with mmdet's attribute names and
``state_dict`` keys.  mmdet and mmcv are not part of the reference tree, so the restatement could not be checked against
them; ``tests/resnet_oracle.py`` is an independent float64 evaluation of the blocks from the ``state_dict`` alone.

The residual tail ``relu(out + identity)`` of a block is ``plane_ops.add_relu`` (one HIP launch) for CUDA float32
contiguous maps while the block's ``fused_tail`` is True, else ``add_relu_torch``.  Under bf16 autocast ``out`` and
``identity`` are both bfloat16 and take the op's bf16 kernels while ``fused_tail_bf16`` is True as well; a mixed pair
stays on torch, which promotes.  ``with_cp=True`` checkpoints the whole block (tail included) in the non-reentrant form.

``fused_norm`` (off by default; ``fuse_norms`` sets it) moves the batch norms into ``norm_ops.bn_act`` as well: with it
on, ``relu(bn(conv(x)))`` is one op, the last norm takes the residual tail with it (``relu(bn(x) + identity)``), and a
``ConvModule`` runs its norm with its ReLU, or alone when it has no activation, wherever ``bn_act_fusable`` accepts
the operands.  Everything else (the flag off, the CPU, other dtypes, ``SyncBN``, another activation, a residual of
another dtype) runs the expressions it runs with the flag off.
"""
import torch
from torch import nn
from torch.nn.modules.batchnorm import _BatchNorm
from torch.utils.checkpoint import checkpoint

from .norm_ops import bn_act, bn_act_fusable
from .plane_ops import FUSED_TAIL_BF16_DEFAULT, FUSED_TAIL_DEFAULT, add_relu, add_relu_fusable, add_relu_torch


def build_norm(norm_cfg, channels):
    """mmcv ``build_norm_layer(norm_cfg, channels)[1]`` for the batch norms."""
    cfg = dict(norm_cfg)
    kind = cfg.pop('type', None)
    if kind not in ('BN', 'BN2d', 'SyncBN'):
        raise NotImplementedError(f'norm_cfg {norm_cfg}: only BN, BN2d and SyncBN')
    requires_grad = cfg.pop('requires_grad', True)
    cfg.setdefault('eps', 1e-5)
    layer = (nn.SyncBatchNorm if kind == 'SyncBN' else nn.BatchNorm2d)(channels, **cfg)
    for p in layer.parameters():
        p.requires_grad = requires_grad
    return layer


def build(cfg, kind, cls):
    """``cls(**cfg)`` for a config dict whose ``type``, if it has one, is ``kind``."""
    cfg = dict(cfg)
    got = cfg.pop('type', kind)
    if got != kind:
        raise NotImplementedError(f'type {got}: only {kind}')
    return cls(**cfg)


def kaiming_init(module, mode='fan_out'):
    """mmcv's ``kaiming_init`` (normal) on every ``Conv2d`` of ``module`` and (1, 0) on its norms.  ``fan_out``: for
    ReLU, conv biases to 0; ``fan_in``: ``kaiming_normal_``'s defaults, biases left alone."""
    fan_out = mode == 'fan_out'
    kw = dict(a=0, mode='fan_out', nonlinearity='relu') if fan_out else {}
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, **kw)
            if fan_out and m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, (_BatchNorm, nn.GroupNorm)):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)


# ------------------------------------------------------------------------------------------------ residual blocks
class _Block(nn.Module):
    """What the two mmdet 2.x blocks share: the ``norm{i}`` properties, checkpointing and the residual tail."""
    fused_tail = FUSED_TAIL_DEFAULT
    fused_tail_bf16 = FUSED_TAIL_BF16_DEFAULT      # bfloat16 operands take the op too (only while fused_tail is on)
    fused_norm = False                             # the norms run norm_ops.bn_act where it takes them (fuse_norms)
    with_cp = False

    def _norm_relu(self, bn, x):
        """``relu(bn(x))`` of the fused forward."""
        if bn_act_fusable(bn, x):
            return bn_act(bn, x)
        return self.relu(bn(x))

    def _norm_tail(self, bn, x, identity):
        """``relu(bn(x) + identity)`` of the fused forward."""
        if bn_act_fusable(bn, x, identity):
            return bn_act(bn, x, residual=identity)
        return self._tail(bn(x), identity)

    def _tail(self, out, identity):
        if (self.fused_tail and (self.fused_tail_bf16 or out.dtype != torch.bfloat16)
                and add_relu_fusable(out, identity)):
            return add_relu(out, identity)
        return add_relu_torch(out, identity)

    def forward(self, x):
        if self.with_cp and x.requires_grad:
            return checkpoint(self._forward, x, use_reentrant=False)
        return self._forward(x)

    @property
    def norm1(self):
        return self.bn1

    @property
    def norm2(self):
        return self.bn2


class BasicBlock(_Block):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style='pytorch', with_cp=False,
                 norm_cfg=dict(type='BN')):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn1 = build_norm(norm_cfg, planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = build_norm(norm_cfg, planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride, self.dilation, self.with_cp = stride, dilation, with_cp

    @property
    def last_norm(self):
        return self.bn2

    def _forward(self, x):
        if self.fused_norm:
            return self._forward_fused_norm(x)
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self._tail(out, identity)

    def _forward_fused_norm(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self._norm_relu(self.bn1, self.conv1(x))
        return self._norm_tail(self.bn2, self.conv2(out), identity)


class Bottleneck(_Block):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style='pytorch', with_cp=False,
                 norm_cfg=dict(type='BN')):
        super().__init__()
        assert style in ('pytorch', 'caffe')
        # 'pytorch': the 3 x 3 convolution carries the stride; 'caffe': the first 1 x 1
        self.conv1_stride, self.conv2_stride = (1, stride) if style == 'pytorch' else (stride, 1)
        self.conv1 = nn.Conv2d(inplanes, planes, 1, stride=self.conv1_stride, bias=False)
        self.bn1 = build_norm(norm_cfg, planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=self.conv2_stride, padding=dilation, dilation=dilation,
                               bias=False)
        self.bn2 = build_norm(norm_cfg, planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = build_norm(norm_cfg, planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride, self.dilation, self.style, self.with_cp = stride, dilation, style, with_cp

    @property
    def norm3(self):
        return self.bn3

    @property
    def last_norm(self):
        return self.bn3

    def _forward(self, x):
        if self.fused_norm:
            return self._forward_fused_norm(x)
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self._tail(out, identity)

    def _forward_fused_norm(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self._norm_relu(self.bn1, self.conv1(x))
        out = self._norm_relu(self.bn2, self.conv2(out))
        return self._norm_tail(self.bn3, self.conv3(out), identity)


def fuse_bf16_tails(module, flag=True):
    """Set ``fused_tail_bf16`` on every block inside ``module``."""
    for m in module.modules():
        if isinstance(m, _Block):
            m.fused_tail_bf16 = bool(flag)


def fuse_norms(module, flag=True):
    """Set ``fused_norm`` on every block and every ``ConvModule`` inside ``module``."""
    for m in module.modules():
        if isinstance(m, (_Block, ConvModule)):
            m.fused_norm = bool(flag)


def unfuse_tails(module):
    """Set ``fused_tail = False`` on every block inside ``module``: its tails then run ``add_relu_torch``."""
    for m in module.modules():
        if isinstance(m, _Block):
            m.fused_tail = False


# ------------------------------------------------------------------------------------------------ ConvModule
_ACTIVATIONS = dict(ReLU=nn.ReLU, LeakyReLU=nn.LeakyReLU, Sigmoid=nn.Sigmoid, Tanh=nn.Tanh, GELU=nn.GELU)


class ConvModule(nn.Module):
    """mmcv ``ConvModule`` in its default order conv -> norm -> act: with ``bias='auto'``, ``conv`` has a bias exactly
    when there is no norm; the norm is ``bn``, the activation ``activate``."""
    fused_norm = False                             # as _Block.fused_norm: the norm and a ReLU behind it run bn_act

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias='auto', conv_cfg=None,
                 norm_cfg=None, act_cfg=None, inplace=True):
        super().__init__()
        if conv_cfg is not None and conv_cfg.get('type', 'Conv2d') not in (None, 'Conv2d', 'Conv'):
            raise NotImplementedError(f'conv_cfg {conv_cfg}: only Conv2d')
        self.with_norm, self.with_activation = norm_cfg is not None, act_cfg is not None
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding,
                              bias=(not self.with_norm) if bias == 'auto' else bool(bias))
        if self.with_norm:
            self.bn = build_norm(norm_cfg, out_channels)
        if self.with_activation:
            cfg = dict(act_cfg)
            kind = cfg.pop('type', None)
            if kind not in _ACTIVATIONS:
                raise NotImplementedError(f'act_cfg {act_cfg}: only {sorted(_ACTIVATIONS)}')
            if kind in ('ReLU', 'LeakyReLU'):
                cfg.setdefault('inplace', inplace)
            self.activate = _ACTIVATIONS[kind](**cfg)

    def forward(self, x):
        x = self.conv(x)
        if (self.fused_norm and self.with_norm and (not self.with_activation or type(self.activate) is nn.ReLU)
                and bn_act_fusable(self.bn, x)):
            return bn_act(self.bn, x, relu=self.with_activation)
        if self.with_norm:
            x = self.bn(x)
        if self.with_activation:
            x = self.activate(x)
        return x
