"""The BEV encoder of the reference config: ``CustomResNet`` (mmdet3d/models/backbones/resnet.py:11-84), ``FPN_LSS``
(mmdet3d/models/necks/lss_fpn.py:11-100) and the two mmdet 2.x residual blocks they are built from, with the
reference's constructor signatures, attribute names and ``state_dict`` keys, so that its checkpoints load with
``strict=True``.  ``BEVEncoder`` is ``BEVDet.bev_encoder`` (bevdet.py:66-72) over the detector's two attributes, and
``build_pre_process`` the detector's ``pre_process_net``: with them the output of ``OcRFViewTransformerFull`` reaches
``CenterHead`` inside this package.

``BasicBlock`` and ``Bottleneck`` restate ``mmdet.models.backbones.resnet`` (mmdet 2.x, ``style='pytorch'``) for the
arguments ``CustomResNet`` passes; mmdet is not part of the reference tree, so the restatement could not be checked
against it.

The convolutions stay with MIOpen.  What is fused is ``FPN_LSS.forward``'s ``cat([x2, up(x1)], 1)`` and ``up2[0]``:
bilinear upsampling with ``align_corners=True`` by an integer factor, written straight into its channels of the
concatenation by ``csrc/upsample_cat.hip`` in one launch (``upsample_cat``; the backward is one gather launch without
atomics).  CUDA float32 contiguous inputs with an integer ``scale_factor`` take it while ``fused_upsample`` is True;
everything else (the CPU, other dtypes, a non-integer factor) takes ``upsample_cat_torch``.  The kernel's interpolation
weights come from integer arithmetic with one rounding, torch's from a float product: the two differ in the last bits.
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.utils.checkpoint import checkpoint

from . import _lib


def _norm(norm_cfg, channels):
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


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, norm_cfg=dict(type='BN')):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = _norm(norm_cfg, planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = _norm(norm_cfg, planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + identity)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, norm_cfg=dict(type='BN')):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = _norm(norm_cfg, planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = _norm(norm_cfg, planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = _norm(norm_cfg, planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + identity)


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
        self.with_cp = with_cp

    def forward(self, x):
        feats = []
        for lid, layer in enumerate(self.layers):
            x = checkpoint(layer, x, use_reentrant=False) if self.with_cp else layer(x)
            if lid in self.backbone_output_ids:
                feats.append(x)
        return feats


# ------------------------------------------------------------------------------------------------ upsample + cat
def upsample_cat_torch(x2, x1, scale):
    """``cat([x2, interpolate(x1, scale_factor=scale, mode='bilinear', align_corners=True)], 1)``; ``x2`` None: the
    upsampling alone."""
    up = F.interpolate(x1, scale_factor=scale, mode='bilinear', align_corners=True)
    return up if x2 is None else torch.cat([x2, up], dim=1)


class _UpsampleCat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, x1, scale):
        B, C1, Hin, Win = x1.shape
        C2 = 0 if x2 is None else x2.shape[1]
        out = torch.empty(B, C2 + C1, Hin * scale, Win * scale, dtype=torch.float32, device=x1.device)
        _lib.launch('ocrf_upsample_cat_forward', x1.device, B, C2, C1, Hin, Win, scale, x2, x1, out)
        ctx.shape = (B, C2, C1, Hin, Win, scale)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        B, C2, C1, Hin, Win, scale = ctx.shape
        grad_out = grad_out.contiguous()
        grad_x2 = grad_x1 = None
        if ctx.needs_input_grad[0] and C2:
            grad_x2 = grad_out[:, :C2]
        if ctx.needs_input_grad[1]:
            grad_x1 = torch.empty(B, C1, Hin, Win, dtype=torch.float32, device=grad_out.device)
            _lib.launch('ocrf_upsample_cat_backward', grad_out.device, B, C2, C1, Hin, Win, scale, grad_out, grad_x1)
        return grad_x2, grad_x1, None


def _fusable(x2, x1, scale):
    if not isinstance(scale, (int, float)) or scale != int(scale) or scale < 1:
        return False
    for t in (x1, x2):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()):
            return False
    return x2 is None or (x2.shape[0] == x1.shape[0] and x2.shape[2] == x1.shape[2] * int(scale)
                          and x2.shape[3] == x1.shape[3] * int(scale))


def upsample_cat(x2, x1, scale):
    """``upsample_cat_torch`` as one HIP launch (``ocrf_upsample_cat_forward`` / ``_backward``): ``x1`` (B, C1, H, W)
    upsampled by the integer ``scale`` behind the channels of ``x2`` (B, C2, H*scale, W*scale), or alone with ``x2``
    None.  CUDA float32 contiguous tensors only: anything else raises (``FPN_LSS`` dispatches)."""
    _lib.require_cuda(x1, x2)
    if not _fusable(x2, x1, scale):
        raise _lib.OcrfHipError('upsample_cat takes contiguous float32 NCHW tensors, x2 scale times the size of x1, '
                                'and an integer scale')
    return _UpsampleCat.apply(x2, x1, int(scale))


class FPN_LSS(nn.Module):
    def __init__(self, in_channels, out_channels, scale_factor=4, input_feature_index=(0, 2), norm_cfg=dict(type='BN'),
                 extra_upsample=2, lateral=None, use_input_conv=False):
        super().__init__()
        self.input_feature_index = input_feature_index
        self.extra_upsample = extra_upsample is not None
        self.fused_upsample = True
        self.up = nn.Upsample(scale_factor=scale_factor, mode='bilinear', align_corners=True)
        mid = out_channels * (2 if self.extra_upsample else 1)
        self.input_conv = nn.Sequential(
            nn.Conv2d(in_channels, mid, kernel_size=1, padding=0, bias=False), _norm(norm_cfg, mid),
            nn.ReLU(inplace=True)) if use_input_conv else None
        if use_input_conv:
            in_channels = mid
        self.conv = nn.Sequential(
            nn.Conv2d(in_channels, mid, kernel_size=3, padding=1, bias=False), _norm(norm_cfg, mid),
            nn.ReLU(inplace=True),
            nn.Conv2d(mid, mid, kernel_size=3, padding=1, bias=False), _norm(norm_cfg, mid), nn.ReLU(inplace=True))
        if self.extra_upsample:
            self.up2 = nn.Sequential(
                nn.Upsample(scale_factor=extra_upsample, mode='bilinear', align_corners=True),
                nn.Conv2d(mid, out_channels, kernel_size=3, padding=1, bias=False), _norm(norm_cfg, out_channels),
                nn.ReLU(inplace=True),
                nn.Conv2d(out_channels, out_channels, kernel_size=1, padding=0))
        self.lateral = lateral is not None
        if self.lateral:
            self.lateral_conv = nn.Sequential(
                nn.Conv2d(lateral, lateral, kernel_size=1, padding=0, bias=False), _norm(norm_cfg, lateral),
                nn.ReLU(inplace=True))

    def _up_cat(self, x2, x1, scale):
        if self.fused_upsample and _fusable(x2, x1, scale):
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
def _build(cfg, kind, cls):
    cfg = dict(cfg)
    got = cfg.pop('type', kind)
    if got != kind:
        raise NotImplementedError(f'type {got}: only {kind}')
    return cls(**cfg)


def build_pre_process(cfg):
    """The detector's ``pre_process_net`` (bevdet.py ``builder.build_backbone(pre_process)``): a ``CustomResNet``; the
    detector takes ``[0]`` of what it returns."""
    return _build(cfg, 'CustomResNet', CustomResNet)


class BEVEncoder(nn.Module):
    """``BEVDet.bev_encoder`` (bevdet.py:66-72): backbone, neck, ``[0]`` of a list or tuple, in float32.  The submodule
    names are the detector's attributes, so its checkpoint keys match with an empty prefix."""

    def __init__(self, backbone_cfg, neck_cfg):
        super().__init__()
        self.img_bev_encoder_backbone = _build(backbone_cfg, 'CustomResNet', CustomResNet)
        self.img_bev_encoder_neck = _build(neck_cfg, 'FPN_LSS', FPN_LSS)

    def forward(self, x):
        device = x.device.type if x.device.type in ('cuda', 'cpu') else 'cuda'
        with torch.autocast(device, enabled=False):
            x = self.img_bev_encoder_backbone(x.float())
            x = self.img_bev_encoder_neck(x)
        if type(x) in (list, tuple):
            x = x[0]
        return x
