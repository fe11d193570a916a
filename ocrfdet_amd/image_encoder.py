"""The image encoder of the reference config (configs/ocrfdet/ocrfdet.py:48-65): ``ResNet`` (mmdet 2.x
``mmdet.models.backbones.ResNet``), ``CustomFPN`` (mmdet3d/models/necks/fpn.py:13-224) and ``ImageEncoder``, which is
``BEVDet.image_encoder`` (bevdet.py:44-64, without ``grid_mask``) and ``BEVStereo4D.extract_stereo_ref_feat``
(bevdet.py:600-614) over the detector's two attributes ``img_backbone`` and ``img_neck``: with them images reach the
neck's 256-channel input and the stereo feature of ``DepthNet`` inside this package.

``ResNet`` restates mmdet 2.x for the arguments the reference passes and close neighbours: constructor keywords,
attribute names and the torchvision ``state_dict`` layout (what ``pretrained='torchvision://resnet50'`` loads).  Its
residual blocks and ``CustomFPN``'s ``ConvModule`` are those of ``blocks.py``.  Deliberate deviations:

* no checkpoint is ever fetched: ``pretrained`` and ``init_cfg`` are stored and otherwise ignored; loading weights is the
  caller's ``load_state_dict``;
* ``deep_stem``, ``avg_down``, ``dcn``, ``plugins``, a ``conv_cfg`` other than ``Conv2d`` and norms other than the batch
  norms raise ``NotImplementedError``;
* ``CustomFPN``'s top-down step returns a new tensor instead of adding in place; ``ConvModule``'s activations are
  ``ReLU`` / ``LeakyReLU`` / ``Sigmoid`` / ``Tanh`` / ``GELU``; ``init_weights()`` is the reference's ``init_cfg``
  (Xavier-uniform on the ``Conv2d``s) and, as in mmcv, is the caller's to invoke.

The convolutions stay with MIOpen.  What is fused are the memory-bound passes between them, ``add_relu`` (the residual
tail of every block) and ``upsample_add`` (``CustomFPN``'s top-down step), both of ``plane_ops.py`` and re-exported
here.  CUDA float32 contiguous tensors of equal shape (``add_relu``) or with matching B and C and a target no smaller
than the source (``upsample_add``) take the kernels while ``ResNet.fused_tail`` / ``CustomFPN.fused_merge`` is True;
everything else (the CPU, other dtypes, non-contiguous maps, other interpolation modes) takes the torch formulation.
Under ``torch.autocast('cuda', dtype=torch.bfloat16)`` the maps between the convolutions are bfloat16: they take the
ops' bf16 kernels while ``ResNet.fused_tail_bf16`` / ``CustomFPN.fused_merge_bf16`` are True as well.
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.modules.batchnorm import _BatchNorm

from .blocks import BasicBlock, Bottleneck, ConvModule, _Block, build, build_norm, fuse_bf16_tails, kaiming_init
from .plane_ops import (FUSED_MERGE_BF16_DEFAULT, FUSED_MERGE_DEFAULT, FUSED_TAIL_BF16_DEFAULT,  # noqa: F401 (re-exported)
                        FUSED_TAIL_DEFAULT, add_relu, add_relu_torch, upsample_add, upsample_add_fusable,
                        upsample_add_torch)


# ------------------------------------------------------------------------------------------------ ResNet
def _res_layer(block, inplanes, planes, num_blocks, stride, dilation, style, with_cp, norm_cfg):
    """mmdet 2.x ``ResLayer`` without ``avg_down``: the first block carries the stride and the downsample."""
    downsample = None
    if stride != 1 or inplanes != planes * block.expansion:
        downsample = nn.Sequential(nn.Conv2d(inplanes, planes * block.expansion, 1, stride=stride, bias=False),
                                   build_norm(norm_cfg, planes * block.expansion))
    kw = dict(dilation=dilation, style=style, with_cp=with_cp, norm_cfg=norm_cfg)
    layers = [block(inplanes, planes, stride=stride, downsample=downsample, **kw)]
    layers += [block(planes * block.expansion, planes, stride=1, **kw) for _ in range(1, num_blocks)]
    return nn.Sequential(*layers)


class ResNet(nn.Module):
    arch_settings = {18: (BasicBlock, (2, 2, 2, 2)), 34: (BasicBlock, (3, 4, 6, 3)), 50: (Bottleneck, (3, 4, 6, 3)),
                     101: (Bottleneck, (3, 4, 23, 3)), 152: (Bottleneck, (3, 8, 36, 3))}

    def __init__(self, depth, in_channels=3, stem_channels=None, base_channels=64, num_stages=4, strides=(1, 2, 2, 2),
                 dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), style='pytorch', deep_stem=False, avg_down=False,
                 frozen_stages=-1, conv_cfg=None, norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True,
                 dcn=None, stage_with_dcn=(False, False, False, False), plugins=None, with_cp=False,
                 zero_init_residual=True, pretrained=None, init_cfg=None):
        super().__init__()
        if depth not in self.arch_settings:
            raise KeyError(f'invalid depth {depth} for resnet')
        if deep_stem:
            raise NotImplementedError('deep_stem=True: only the 7 x 7 stem')
        if avg_down:
            raise NotImplementedError('avg_down=True: only the strided 1 x 1 downsample')
        if dcn is not None:
            raise NotImplementedError('dcn: deformable convolution is not part of this package')
        if plugins is not None:
            raise NotImplementedError('plugins: none are part of this package')
        if conv_cfg is not None and conv_cfg.get('type', 'Conv2d') not in (None, 'Conv2d', 'Conv'):
            raise NotImplementedError(f'conv_cfg {conv_cfg}: only Conv2d')
        if style not in ('pytorch', 'caffe'):
            raise ValueError(f'style {style}: pytorch or caffe')
        assert 1 <= num_stages <= 4 and len(strides) == len(dilations) == num_stages
        assert max(out_indices) < num_stages
        stem_channels = base_channels if stem_channels is None else stem_channels
        self.depth, self.stem_channels, self.base_channels = depth, stem_channels, base_channels
        self.num_stages, self.strides, self.dilations, self.out_indices = num_stages, strides, dilations, out_indices
        self.style, self.deep_stem, self.avg_down, self.frozen_stages = style, deep_stem, avg_down, frozen_stages
        self.conv_cfg, self.norm_cfg, self.norm_eval, self.with_cp = conv_cfg, norm_cfg, norm_eval, with_cp
        self.zero_init_residual, self.pretrained, self.init_cfg = zero_init_residual, pretrained, init_cfg
        self.block, stage_blocks = self.arch_settings[depth]
        self.stage_blocks = stage_blocks[:num_stages]

        self.conv1 = nn.Conv2d(in_channels, stem_channels, 7, stride=2, padding=3, bias=False)
        self.norm1_name = 'bn1'
        self.bn1 = build_norm(norm_cfg, stem_channels)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.res_layers, inplanes = [], stem_channels
        for i, num_blocks in enumerate(self.stage_blocks):
            planes = base_channels * 2 ** i
            name = f'layer{i + 1}'
            self.add_module(name, _res_layer(self.block, inplanes, planes, num_blocks, strides[i], dilations[i], style,
                                             with_cp, norm_cfg))
            inplanes = planes * self.block.expansion
            self.res_layers.append(name)
        self.feat_dim = self.block.expansion * base_channels * 2 ** (len(self.stage_blocks) - 1)
        self._freeze_stages()

    @property
    def norm1(self):
        return getattr(self, self.norm1_name)

    @property
    def fused_tail(self):
        """Whether the residual tails run as ``add_relu``; setting it applies to every block."""
        return all(m.fused_tail for m in self.modules() if isinstance(m, _Block))

    @fused_tail.setter
    def fused_tail(self, flag):
        for m in self.modules():
            if isinstance(m, _Block):
                m.fused_tail = bool(flag)

    @property
    def fused_tail_bf16(self):
        """Whether bfloat16 tails (bf16 autocast) run as ``add_relu`` while ``fused_tail`` is on; setting it applies to
        every block."""
        return all(m.fused_tail_bf16 for m in self.modules() if isinstance(m, _Block))

    @fused_tail_bf16.setter
    def fused_tail_bf16(self, flag):
        fuse_bf16_tails(self, flag)

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.norm1.eval()
            for m in (self.conv1, self.norm1):
                for p in m.parameters():
                    p.requires_grad = False
        for i in range(1, min(self.frozen_stages, self.num_stages) + 1):
            m = getattr(self, f'layer{i}')
            m.eval()
            for p in m.parameters():
                p.requires_grad = False

    def init_weights(self):
        """mmcv's ``kaiming_init`` (fan_out, relu, normal) on the convolutions, (1, 0) on the norms and, with
        ``zero_init_residual``, 0 on the last norm of every block.  Fetches nothing."""
        kaiming_init(self, mode='fan_out')
        if self.zero_init_residual:
            for m in self.modules():
                if isinstance(m, _Block):
                    nn.init.constant_(m.last_norm.weight, 0)

    def forward(self, x):
        x = self.maxpool(self.relu(self.norm1(self.conv1(x))))
        outs = []
        for i, name in enumerate(self.res_layers):
            x = getattr(self, name)(x)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, _BatchNorm):
                    m.eval()
        return self


# ------------------------------------------------------------------------------------------------ CustomFPN
class CustomFPN(nn.Module):
    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, out_ids=[],
                 add_extra_convs=False, relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None,
                 norm_cfg=None, act_cfg=None, upsample_cfg=dict(mode='nearest'),
                 init_cfg=dict(type='Xavier', layer='Conv2d', distribution='uniform')):
        super().__init__()
        assert isinstance(in_channels, list)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.num_ins, self.num_outs = len(in_channels), num_outs
        self.relu_before_extra_convs, self.no_norm_on_lateral = relu_before_extra_convs, no_norm_on_lateral
        self.fp16_enabled = False
        self.upsample_cfg = upsample_cfg.copy()
        self.out_ids, self.init_cfg = out_ids, init_cfg
        self.fused_merge = FUSED_MERGE_DEFAULT
        self.fused_merge_bf16 = FUSED_MERGE_BF16_DEFAULT           # bfloat16 laterals too (only while fused_merge is on)
        if end_level == -1:
            self.backbone_end_level = self.num_ins
        else:
            self.backbone_end_level = end_level
            assert end_level <= len(in_channels)
            assert num_outs == end_level - start_level
        self.start_level, self.end_level = start_level, end_level
        assert isinstance(add_extra_convs, (str, bool))
        if isinstance(add_extra_convs, str):
            assert add_extra_convs in ('on_input', 'on_lateral', 'on_output')
        elif add_extra_convs:
            add_extra_convs = 'on_input'
        self.add_extra_convs = add_extra_convs

        self.lateral_convs, self.fpn_convs = nn.ModuleList(), nn.ModuleList()
        kw = dict(conv_cfg=conv_cfg, act_cfg=act_cfg, inplace=False)
        for i in range(self.start_level, self.backbone_end_level):
            self.lateral_convs.append(ConvModule(in_channels[i], out_channels, 1,
                                                 norm_cfg=None if no_norm_on_lateral else norm_cfg, **kw))
            if i in self.out_ids:
                self.fpn_convs.append(ConvModule(out_channels, out_channels, 3, padding=1, norm_cfg=norm_cfg, **kw))
        extra_levels = num_outs - self.backbone_end_level + self.start_level
        if self.add_extra_convs and extra_levels >= 1:
            for i in range(extra_levels):
                c_in = in_channels[self.backbone_end_level - 1] if i == 0 and self.add_extra_convs == 'on_input' \
                    else out_channels
                self.fpn_convs.append(ConvModule(c_in, out_channels, 3, stride=2, padding=1, norm_cfg=norm_cfg, **kw))

    def init_weights(self):
        """The reference's ``init_cfg``: Xavier-uniform weights and zero biases on every ``Conv2d``."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight, gain=1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def _merge(self, dst, src):
        """``dst += F.interpolate(src, ...)`` of the top-down path, as a new tensor."""
        cfg = dict(self.upsample_cfg)
        if 'scale_factor' not in cfg:
            cfg['size'] = tuple(dst.shape[2:])
        fused = self.fused_merge and (self.fused_merge_bf16 or dst.dtype != torch.bfloat16)
        if fused and set(cfg) <= {'mode', 'size', 'scale_factor'} and cfg.get('mode', 'nearest') == 'nearest':
            size, scale = cfg.get('size'), cfg.get('scale_factor')
            if upsample_add_fusable(dst, src, size, scale):
                return upsample_add(dst, src, size=size, scale_factor=scale)
        return upsample_add_torch(dst, src, **cfg)

    def forward(self, inputs):
        assert len(inputs) == len(self.in_channels)
        laterals = [conv(inputs[i + self.start_level]) for i, conv in enumerate(self.lateral_convs)]
        used_backbone_levels = len(laterals)
        for i in range(used_backbone_levels - 1, 0, -1):
            laterals[i - 1] = self._merge(laterals[i - 1], laterals[i])
        outs = [self.fpn_convs[i](laterals[i]) for i in self.out_ids]
        if self.num_outs > len(outs):
            if not self.add_extra_convs:
                for i in range(self.num_outs - used_backbone_levels):
                    outs.append(F.max_pool2d(outs[-1], 1, stride=2))
            else:
                if self.add_extra_convs == 'on_input':
                    extra_source = inputs[self.backbone_end_level - 1]
                elif self.add_extra_convs == 'on_lateral':
                    extra_source = laterals[-1]
                else:
                    extra_source = outs[-1]
                outs.append(self.fpn_convs[used_backbone_levels](extra_source))
                for i in range(used_backbone_levels + 1, self.num_outs):
                    outs.append(self.fpn_convs[i](F.relu(outs[-1]) if self.relu_before_extra_convs else outs[-1]))
        return outs[0]


# ------------------------------------------------------------------------------------------------ the encoder
class ImageEncoder(nn.Module):
    """``BEVDet.image_encoder`` (bevdet.py:44-64, no ``grid_mask``) and ``BEVStereo4D.extract_stereo_ref_feat``
    (:600-614) over ``img_backbone`` (a ``ResNet``) and ``img_neck`` (a ``CustomFPN`` or None).  The submodule names are
    the detector's attributes, so its checkpoint keys match with an empty prefix."""

    def __init__(self, img_backbone, img_neck=None):
        super().__init__()
        self.img_backbone = build(img_backbone, 'ResNet', ResNet)
        if img_neck is not None:
            self.img_neck = build(img_neck, 'CustomFPN', CustomFPN)

    @property
    def with_img_neck(self):
        return getattr(self, 'img_neck', None) is not None

    def image_encoder(self, img, stereo=False):
        B, N, C, imH, imW = img.shape
        x = self.img_backbone(img.view(B * N, C, imH, imW))
        stereo_feat = None
        if stereo:
            stereo_feat = x[0]
            x = x[1:]
        if self.with_img_neck:
            x = self.img_neck(x)
            if type(x) in (list, tuple):
                x = x[0]
        _, output_dim, output_H, output_W = x.shape
        return x.view(B, N, output_dim, output_H, output_W), stereo_feat

    def extract_stereo_ref_feat(self, x):
        B, N, C, imH, imW = x.shape
        x = x.view(B * N, C, imH, imW)
        net = self.img_backbone
        x = net.maxpool(net.relu(net.norm1(net.conv1(x))))
        return getattr(net, net.res_layers[0])(x)

    forward = image_encoder
