"""The BEV encoder of the reference config: ``CustomResNet`` (mmdet3d/models/backbones/resnet.py:11-84), ``FPN_LSS``
(mmdet3d/models/necks/lss_fpn.py:11-100) and the two mmdet 2.x residual blocks they are built from, with the
reference's constructor signatures, attribute names and ``state_dict`` keys, so that its checkpoints load with
``strict=True``.  ``BEVEncoder`` is ``BEVDet.bev_encoder`` (bevdet.py:66-72) over the detector's two attributes, and
``build_pre_process`` the detector's ``pre_process_net``: with them the output of ``OcRFViewTransformerFull`` reaches
``CenterHead`` inside this package.

The residual blocks are those of ``blocks.py`` with ``style='pytorch'`` and ``dilation=1``.

The convolutions stay with MIOpen.  What is fused is ``FPN_LSS.forward``'s ``cat([x2, up(x1)], 1)`` and ``up2[0]``, as
``upsample_cat`` of ``plane_ops.py`` (re-exported here).  CUDA float32 contiguous inputs with an integer
``scale_factor`` take it while ``fused_upsample`` is True, and bfloat16 ones its ``_bf16`` kernels while
``fused_upsample_bf16`` is True as well; everything else (the CPU, other dtypes, a non-integer factor) takes
``upsample_cat_torch``.

``BEVEncoder`` computes in float32, as the reference's ``@force_fp32`` has it.  ``autocast_bf16=True`` is the opt-in
that lets it run as bf16 autocast runs it: bfloat16 convolutions, a bfloat16 ``_up_cat`` and a bfloat16 result.
"""
import torch
from torch import nn
from torch.utils.checkpoint import checkpoint

from .blocks import BasicBlock, Bottleneck, build, build_norm, unfuse_tails
from .plane_ops import (FUSED_UPSAMPLE_BF16_DEFAULT, upsample_cat, upsample_cat_bf16_fusable, upsample_cat_fusable,
                        upsample_cat_torch)


class CustomResNet(nn.Module):
    def __init__(self, numC_input, num_layer=[2, 2, 2], num_channels=None, stride=[2, 2, 2], backbone_output_ids=None,
                 norm_cfg=dict(type='BN'), with_cp=False, block_type='Basic'):
        super().__init__()
        assert len(num_layer) == len(stride)
        if num_channels is None:
            num_channels = [numC_input * 2 ** (i + 1) for i in range(len(num_layer))]
        self.backbone_output_ids = range(len(num_layer)) if backbone_output_ids is None else backbone_output_ids
        if block_type == 'BottleNeck':
            block, div = Bottleneck, Bottleneck.expansion
        elif block_type == 'Basic':
            block, div = BasicBlock, 1
        else:
            raise NotImplementedError(f'block_type {block_type}: only Basic and BottleNeck')
        layers, c_in = [], numC_input
        for n, c_out, s in zip(num_layer, num_channels, stride):
            stage = [block(c_in, c_out // div, stride=s, downsample=nn.Conv2d(c_in, c_out, 3, s, 1), norm_cfg=norm_cfg)]
            stage += [block(c_out, c_out // div, norm_cfg=norm_cfg) for _ in range(n - 1)]
            layers.append(nn.Sequential(*stage))
            c_in = c_out
        self.layers = nn.Sequential(*layers)
        # off because the tail is unmeasured at these shapes; flipping it is a separate change with its own
        # tools/time_bev_encoder.py row
        unfuse_tails(self.layers)
        self.with_cp = with_cp

    def forward(self, x):
        feats = []
        for lid, layer in enumerate(self.layers):
            x = checkpoint(layer, x, use_reentrant=False) if self.with_cp else layer(x)
            if lid in self.backbone_output_ids:
                feats.append(x)
        return feats


# ------------------------------------------------------------------------------------------------ FPN_LSS
class FPN_LSS(nn.Module):
    def __init__(self, in_channels, out_channels, scale_factor=4, input_feature_index=(0, 2), norm_cfg=dict(type='BN'),
                 extra_upsample=2, lateral=None, use_input_conv=False):
        super().__init__()
        self.input_feature_index = input_feature_index
        self.extra_upsample = extra_upsample is not None
        self.fused_upsample = True
        self.fused_upsample_bf16 = FUSED_UPSAMPLE_BF16_DEFAULT    # for bfloat16 operands, while fused_upsample is on
        self.up = nn.Upsample(scale_factor=scale_factor, mode='bilinear', align_corners=True)
        mid = out_channels * (2 if self.extra_upsample else 1)
        self.input_conv = nn.Sequential(
            nn.Conv2d(in_channels, mid, kernel_size=1, padding=0, bias=False), build_norm(norm_cfg, mid),
            nn.ReLU(inplace=True)) if use_input_conv else None
        if use_input_conv:
            in_channels = mid
        self.conv = nn.Sequential(
            nn.Conv2d(in_channels, mid, kernel_size=3, padding=1, bias=False), build_norm(norm_cfg, mid),
            nn.ReLU(inplace=True),
            nn.Conv2d(mid, mid, kernel_size=3, padding=1, bias=False), build_norm(norm_cfg, mid), nn.ReLU(inplace=True))
        if self.extra_upsample:
            self.up2 = nn.Sequential(
                nn.Upsample(scale_factor=extra_upsample, mode='bilinear', align_corners=True),
                nn.Conv2d(mid, out_channels, kernel_size=3, padding=1, bias=False), build_norm(norm_cfg, out_channels),
                nn.ReLU(inplace=True),
                nn.Conv2d(out_channels, out_channels, kernel_size=1, padding=0))
        self.lateral = lateral is not None
        if self.lateral:
            self.lateral_conv = nn.Sequential(
                nn.Conv2d(lateral, lateral, kernel_size=1, padding=0, bias=False), build_norm(norm_cfg, lateral),
                nn.ReLU(inplace=True))

    def _up_cat(self, x2, x1, scale):
        if self.fused_upsample and (upsample_cat_fusable(x2, x1, scale) or (
                self.fused_upsample_bf16 and upsample_cat_bf16_fusable(x2, x1, scale))):
            return upsample_cat(x2, x1, scale)
        return upsample_cat_torch(x2, x1, scale)

    def forward(self, feats):
        x2, x1 = feats[self.input_feature_index[0]], feats[self.input_feature_index[1]]
        if self.lateral:
            x2 = self.lateral_conv(x2)
        x = self._up_cat(x2, x1, self.up.scale_factor)
        if self.input_conv is not None:
            x = self.input_conv(x)
        x = self.conv(x)
        if self.extra_upsample:
            x = self._up_cat(None, x, self.up2[0].scale_factor)
            for layer in self.up2[1:]:
                x = layer(x)
        return x


# ------------------------------------------------------------------------------------------------ the encoder
def build_pre_process(cfg):
    """The detector's ``pre_process_net`` (bevdet.py ``builder.build_backbone(pre_process)``): a ``CustomResNet``; the
    detector takes ``[0]`` of what it returns."""
    return build(cfg, 'CustomResNet', CustomResNet)


class BEVEncoder(nn.Module):
    """``BEVDet.bev_encoder`` (bevdet.py:66-72): backbone, neck, ``[0]`` of a list or tuple, in float32.  The submodule
    names are the detector's attributes, so its checkpoint keys match with an empty prefix.

    ``autocast_bf16`` (default False: the reference's ``@force_fp32``): while bfloat16 autocast is active on the input's
    device, autocast is left on and the input is not widened (a float32 one is narrowed once to bfloat16), so the
    convolutions and batch norms run as autocast runs them, ``FPN_LSS._up_cat`` sees bfloat16 and the result is
    bfloat16.  The parameters stay float32.  Outside bfloat16 autocast the flag changes nothing."""

    def __init__(self, backbone_cfg, neck_cfg, autocast_bf16=False):
        super().__init__()
        self.img_bev_encoder_backbone = build(backbone_cfg, 'CustomResNet', CustomResNet)
        self.img_bev_encoder_neck = build(neck_cfg, 'FPN_LSS', FPN_LSS)
        self.autocast_bf16 = autocast_bf16

    def forward(self, x):
        device = x.device.type if x.device.type in ('cuda', 'cpu') else 'cuda'
        if (self.autocast_bf16 and torch.is_autocast_enabled(device)
                and torch.get_autocast_dtype(device) == torch.bfloat16):
            x = self.img_bev_encoder_neck(self.img_bev_encoder_backbone(x.to(torch.bfloat16)))
            return x[0] if type(x) in (list, tuple) else x
        with torch.autocast(device, enabled=False):
            x = self.img_bev_encoder_backbone(x.float())
            x = self.img_bev_encoder_neck(x)
        if type(x) in (list, tuple):
            x = x[0]
        return x
