"""The small building blocks of the reference's neck (mmdet3d/models/necks/view_transformer_ocrf.py:36-228, :272-380,
:520-575): structure, attribute names and ``state_dict`` keys fixed by the reference; eval mode on the GPU takes the fused
HIP passes of ``neck_ops`` / ``hoa``.  ``view_transformer_ocrf`` re-exports every name of this file."""
import torch
import torch.nn.functional as F
from torch import nn

from . import hoa, neck_ops


def _conv_bn(cin, cout, k=1, relu=False):
    layers = [nn.Conv2d(cin, cout, kernel_size=k, stride=1, padding=k // 2), nn.BatchNorm2d(cout)]
    return layers + [nn.ReLU(inplace=True)] if relu else layers


class MS_CAM(nn.Module):
    """Multi-scale channel attention (:36-66).  The pooling modules are kept for the Sequential's
    indices (state_dict keys); the reductions themselves are ``mean`` / ``amax`` — PyTorch's
    adaptive-pool kernels run one thread per output element, 3.4 ms per call on a 200x200 map."""

    def __init__(self, input_channel=64, output_channel=64, r=4):
        super().__init__()
        mid = int(input_channel // r)
        self.local_att = nn.Sequential(*_conv_bn(input_channel, mid, relu=True), *_conv_bn(mid, output_channel))
        self.global_att = nn.Sequential(nn.AdaptiveAvgPool2d(1), *_conv_bn(input_channel, mid, relu=True),
                                        *_conv_bn(mid, output_channel))
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        g = x.mean((2, 3), keepdim=True)
        for layer in list(self.global_att)[1:]:
            g = layer(g)
        return self.sigmoid(self.local_att(x) + g)


class ChannelAttention(nn.Module):
    def __init__(self, input_channel, output_channel, ratio=16):
        super().__init__()
        self.avg_pool, self.max_pool = nn.AdaptiveAvgPool2d(1), nn.AdaptiveMaxPool2d(1)
        self.fc = nn.Sequential(nn.Conv2d(input_channel, input_channel // ratio, 1, bias=False), nn.ReLU(),
                                nn.Conv2d(input_channel // ratio, output_channel, 1, bias=False))
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        # (the maximum with its index, as the reference's AdaptiveMaxPool2d(1), :72-83 — see hoa.HeightAttention._forward_torch)
        peak = x.flatten(2).max(-1)[0].unsqueeze(-1).unsqueeze(-1)
        return self.sigmoid(self.fc(x.mean((2, 3), keepdim=True)) + self.fc(peak))


def _tensors_of(owner, name, modules, buffers=True):
    """The parameter (+ buffer) tensors of ``modules`` as a list cached on ``owner``: enumerating them through
    ``Module.parameters()`` costs ~0.1 ms per call, a third of the host time of an eager forward.  The weight-pack
    caches key on these tensors' versions / addresses, which ``load_state_dict``, optimizer steps and ``.to()``
    all change while the tensor OBJECTS stay; ``OcRFViewTransformerFull`` drops the lists on ``_apply`` /
    ``load_state_dict`` / ``train`` anyway.  Assigning a NEW ``nn.Parameter`` to a sub-module needs
    ``invalidate_packs()``."""
    cache = owner.__dict__.setdefault('_tensor_lists', {})
    lst = cache.get(name)
    if lst is None:
        lst = cache[name] = [t for m in modules
                             for t in list(m.parameters()) + (list(m.buffers()) if buffers else [])]
    return lst


def _drop_tensor_lists(root):
    for m in root.modules():
        m.__dict__.pop('_tensor_lists', None)


_ZEROS = {}


def _zeros(shape, like):
    """A persistent all-zero tensor per (shape, device, dtype): read-only operand of fused kernels.  Not
    ``torch.zeros`` per call: that is a memset, and memset NODES make a captured hipGraph of the step
    fault on replay after any intervening copy (csrc/launch.h, zero_async)."""
    key = (tuple(shape), like.device, like.dtype)
    t = _ZEROS.get(key)
    if t is None:
        t = _ZEROS[key] = torch.zeros(shape, device=like.device, dtype=like.dtype)
    return t


def _spatial_logits(x, conv):
    return conv(torch.cat((x.mean(1, keepdim=True), torch.max(x, dim=1, keepdim=True)[0]), 1))    # (:94-96: max with indices)


class SpatialAttention(nn.Module):
    def __init__(self, kernel_size=7):
        super().__init__()
        self.conv1 = nn.Conv2d(2, 1, kernel_size, padding=kernel_size // 2, bias=False)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        return self.sigmoid(_spatial_logits(x, self.conv1))


class ResCBAMBlock(nn.Module):
    """:100-137.  Note the reference feeds ``conv2`` with ``inplanes`` channels (== planes here)."""

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.ca, self.sa = ChannelAttention(planes, planes), SpatialAttention()
        self.downsample, self.stride = downsample, stride

    def forward(self, x):
        out = self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x)))))
        out = self.ca(out) * out
        if out.is_cuda and not torch.is_grad_enabled():
            out = hoa.spatial_gate(self.sa.conv1.weight, out, _zeros((out.shape[0], 1) + out.shape[2:], out), True)[1]
        else:
            out = self.sa(out) * out
        res = x if self.downsample is None else self.downsample(x)
        return self.relu(out + res)


class DiceLoss(nn.Module):
    def __init__(self, use_sigmoid=True, loss_weight=1.):
        super().__init__()
        self.use_sigmoid, self.loss_weight = use_sigmoid, loss_weight

    def forward(self, inputs, targets, smooth=1e-5):
        p = (torch.sigmoid(inputs) if self.use_sigmoid else inputs).reshape(-1)
        t = targets.reshape(-1)
        dice = (2. * (p * t).sum() + smooth) / (p.sum() + t.sum() + smooth)
        return self.loss_weight * (1 - dice)


class ProbNet(nn.Module):
    """BEV foreground-probability head (:139-201); the losses keep their buffers so checkpoints load."""

    def __init__(self, in_channels=512, scale_factor=1, with_centerness=False, loss_weight=6.0, bev_size=None):
        super().__init__()
        self.loss_weight, self.loss_weight_opacity = loss_weight, 6.0
        mid = in_channels // 2
        self.base_conv = nn.Sequential(*_conv_bn(in_channels, mid, k=3, relu=True))
        self.prob_conv = nn.Sequential(ResCBAMBlock(mid, mid))
        self.mask_net = nn.Conv2d(mid, 1, kernel_size=1, padding=0, stride=1)
        self.with_centerness = with_centerness
        if with_centerness:
            n = bev_size[0]
            g = torch.stack(torch.meshgrid(torch.arange(n), torch.arange(n), indexing='ij'), -1)
            g = (g - n // 2) / (n // 2)
            self.centerness = ((g[..., 0] ** 2 + g[..., 1] ** 2) / 2).sqrt() + 1       # plain attribute (:167)
        self.dice_loss = DiceLoss(use_sigmoid=True, loss_weight=self.loss_weight)
        self.dice_loss_opacity = DiceLoss(use_sigmoid=True, loss_weight=self.loss_weight_opacity)
        self.ce_loss = nn.BCEWithLogitsLoss(pos_weight=torch.tensor([2.13]))

    def _fusable(self, x):
        blk = self.prob_conv[0]
        return (x.is_cuda and not self.training and not torch.is_grad_enabled() and len(self.prob_conv) == 1
                and blk.downsample is None and blk.stride == 1 and self.mask_net.out_channels == 1)

    def forward(self, input):
        if self._fusable(input):
            # eval on the GPU: MIOpen's three convolutions with the BatchNorms folded + six HIP launches
            # (neck_ops.probnet_forward) instead of ~33 launches
            ts = _tensors_of(self, 'prob', (self,))
            key = tuple((t._version, t.data_ptr()) for t in ts)
            if self.__dict__.get('_pack_key') != key:
                self.__dict__['_pack'] = neck_ops.pack_probnet(self)
                self.__dict__['_pack_key'] = key
            return neck_ops.probnet_forward(input, self.__dict__['_pack'])
        return self.mask_net(self.prob_conv(self.base_conv(input)))

    def _centerness_on(self, device):
        """``centerness`` on the loss's device, copied once per device (the reference keeps it on the GPU, :166)."""
        c = self.__dict__.get('_centerness_dev')
        if c is None or c.device != device:
            c = self.__dict__['_centerness_dev'] = self.centerness.to(device)
        return c

    def _mask_losses(self, gt_bev_mask, pred_bev_mask, dice):
        """Centerness-weighted BCE with logits (pos_weight 2.13) + Dice over B x Y x X maps (:177-201), without the
        reference's switch of ``ce_loss.reduction`` as a side effect."""
        bs, bev_h, bev_w = gt_bev_mask.shape
        b = gt_bev_mask.reshape(bs, bev_w * bev_h).permute(1, 0).to(torch.float)
        a = pred_bev_mask.reshape(bs, bev_w * bev_h).permute(1, 0)
        if self.with_centerness:
            tmp = F.binary_cross_entropy_with_logits(a, b, pos_weight=self.ce_loss.pos_weight, reduction='none')
            ce = (tmp * self._centerness_on(a.device).reshape(bev_w * bev_h, 1)).mean()
        else:
            ce = self.ce_loss(a, b)
        return ce, dice(pred_bev_mask.reshape(bs, -1), gt_bev_mask.reshape(bs, -1))

    def get_bev_mask_loss(self, gt_bev_mask, pred_bev_mask):
        ce, dice = self._mask_losses(gt_bev_mask, pred_bev_mask, self.dice_loss)
        return dict(mask_ce_loss=self.loss_weight * ce, mask_dice_loss=dice)

    def get_bev_opacity_loss(self, gt_bev_mask, pred_bev_mask):
        ce, dice = self._mask_losses(gt_bev_mask, pred_bev_mask, self.dice_loss_opacity)
        return dict(mask_ce_opacity_loss=self.loss_weight_opacity * ce, mask_dice_opacity_loss=dice)


class DualFeatFusion(nn.Module):
    """:203-213.  Eval mode on the GPU: one HIP pass (``ocrf_dual_feat_fusion``) instead of cat + two
    1x1 convolutions + two BatchNorms + ReLU + seven elementwise passes over the BEV."""

    def __init__(self, input_channel, output_channel):
        super().__init__()
        self.ca = MS_CAM(input_channel, output_channel)

    def _fusable(self, x1):
        la = self.ca.local_att
        c, m = la[3].out_channels, la[0].out_channels
        return (x1.is_cuda and not self.training and not torch.is_grad_enabled() and la[0].in_channels == 2 * c
                and (c, m) in ((80, 40), (64, 32)))

    def forward(self, x1, x2, addend=None):
        """``addend`` (eval mode on the GPU only): also return ``addend + out``, written by the same pass."""
        if self._fusable(x1):
            ca = self.ca
            ts = _tensors_of(self, 'fuser', (ca.local_att, ca.global_att))
            key = tuple((t._version, t.data_ptr()) for t in ts)
            if self.__dict__.get('_pack_key') != key:
                self.__dict__['_pack'] = (neck_ops.pack_fusion_params(ca), neck_ops.pack_global_att(ca))
                self.__dict__['_pack_key'] = key
            local, glob = self.__dict__['_pack']
            g = neck_ops.global_att_vector(x1, x2, glob)
            return neck_ops.dual_feat_fusion(x1, x2, local, g, ca.local_att[0].out_channels, addend=addend)
        cf = self.ca(torch.cat((x1, x2), 1))
        out = cf * x1 + (1 - cf) * x2
        return out if addend is None else (out, addend + out)


class BEVGeomAttention(nn.Module):
    def __init__(self, kernel_size=7):
        super().__init__()
        self.conv1 = nn.Conv2d(2, 1, kernel_size, padding=kernel_size // 2, bias=False)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x, bev_prob):
        if x.is_cuda and not torch.is_grad_enabled():
            return hoa.spatial_gate(self.conv1.weight, x, bev_prob, False)[0]
        return self.sigmoid(_spatial_logits(x, self.conv1) + bev_prob)

    def gate(self, x, bev_prob):
        """-> x * forward(x, bev_prob) (:1190) in two HBM passes."""
        if x.is_cuda and not torch.is_grad_enabled():
            return hoa.spatial_gate(self.conv1.weight, x, bev_prob, True)[1]
        return self.forward(x, bev_prob) * x


_TallLinear, _linear = neck_ops.TallLinear, neck_ops.tall_linear


class _Head(nn.Module):
    """fc1 -> ReLU -> fc2 -> ``act``; ``extra`` widens fc1's input by the sampled RGB (:272-380)."""
    extra = 0

    def __init__(self, input_dim, hidden_dim, output_dim):
        super().__init__()
        self.fc1 = nn.Linear(input_dim + self.extra, hidden_dim)
        self.fc2 = nn.Linear(hidden_dim, output_dim)

    def act(self, x):
        return x

    def forward(self, x):
        return self.act(_linear(self.fc2, torch.relu(_linear(self.fc1, x))))


class ScaleFactorMLP(_Head):
    def __init__(self, input_dim, hidden_dim, output_dim):
        super().__init__(input_dim, hidden_dim, output_dim)
        self.softplus = nn.Softplus()

    def act(self, x):
        return self.softplus(x)


class RotationFactorMLP(_Head):
    def act(self, x):
        return F.normalize(x, dim=-1)


class OpacityFactorMLP(_Head):
    def __init__(self, input_dim, hidden_dim, output_dim):
        super().__init__(input_dim, hidden_dim, output_dim)
        self.sigmoid = nn.Sigmoid()

    def act(self, x):
        return self.sigmoid(x)


class ColorFactorMLPGaussian(OpacityFactorMLP):
    extra = 3


class ColorFactorMLPNerf(OpacityFactorMLP):
    extra = 3


class DepthFactorMLPNerf(_Head):
    extra = 3

    def act(self, x):
        return torch.relu(x)


class ImgFeatResize1(DepthFactorMLPNerf):
    pass


class ImgFeatResize2(DepthFactorMLPNerf):
    pass


class VoxelFeatureExtractor(nn.Module):
    def __init__(self, in_planes=1, out_planes=13):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv3d(in_planes, out_planes, kernel_size=1), nn.BatchNorm3d(out_planes),
                                  nn.ReLU(inplace=True))

    def forward(self, x):
        conv, bn = self.conv[0], self.conv[1]
        if (x.is_cuda and x.dim() == 5 and x.shape[1] == 1 and conv.in_channels == 1 and conv.kernel_size == (1, 1, 1)
                and type(bn) is nn.BatchNorm3d and bn.affine and bn.track_running_stats):
            # (a converted nn.SyncBatchNorm needs cross-rank statistics: it takes the layer path below)
            return self._lift(x)
        return self.conv(x)

    def _lift(self, x):
        """Conv3d(1 -> Zh, k = 1) + BatchNorm3d + ReLU in closed form: channel h of the convolution is
        ``w_h x + b_h``, so its batch statistics are ``w_h mean(x) + b_h`` and ``w_h^2 var(x)`` and the three layers
        are ONE broadcast multiply-add + ReLU.  MIOpen runs the 1-channel Conv3d and the BatchNorm over the
        (B,Zh,Y,X,C) tensor at 0.8 + 2.0 ms and 4.0 + 2.8 ms (forward + backward) at 200x200."""
        conv, bn = self.conv[0], self.conv[1]
        w, b = conv.weight.reshape(-1), conv.bias
        if b is None:
            b = torch.zeros_like(w)
        if bn.training:
            n = x.numel()
            var, mean = torch.var_mean(x, unbiased=False)
            mean_h, var_h = w * mean + b, w * w * var
            with torch.no_grad():
                bn.num_batches_tracked += 1
                mom = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
                bn.running_mean.mul_(1 - mom).add_(mean_h, alpha=mom)
                bn.running_var.mul_(1 - mom).add_(var_h * (n / max(n - 1, 1)), alpha=mom)
        else:
            mean_h, var_h = bn.running_mean, bn.running_var
        a = bn.weight * torch.rsqrt(var_h + bn.eps)
        shape = (1, -1, 1, 1, 1)
        out = torch.addcmul((a * (b - mean_h) + bn.bias).view(shape), x, (a * w).view(shape))
        return out.relu_()


class ResizeNetwork(nn.Module):
    """256 -> output_channel, x16 up-sampling, purely linear (:534-554)."""

    def __init__(self, output_channel):
        super().__init__()
        self.conv1 = nn.Conv2d(256, 128, kernel_size=3, padding=1)
        self.upsample1 = nn.ConvTranspose2d(128, 64, kernel_size=2, stride=2)
        self.conv2 = nn.Conv2d(64, 32, kernel_size=3, padding=1)
        self.upsample2 = nn.ConvTranspose2d(32, output_channel, kernel_size=2, stride=2)
        self.upsample3 = nn.ConvTranspose2d(output_channel, output_channel, kernel_size=4, stride=4)

    def stem(self, x):
        """Everything up to conv2's output — what the composed NeRF kernels consume."""
        return self.conv2(self.upsample1(self.conv1(x)))

    def forward(self, x):
        return self.upsample3(self.upsample2(self.stem(x)))


class _LinearWeighted(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.tensor(0.5))

    def forward(self, a1, a2):
        if a1.is_cuda and not torch.is_grad_enabled():
            return torch.lerp(a2, a1, self.w)       # a2 + w (a1 - a2): one launch instead of four
        return self.w * a1 + (1 - self.w) * a2


class LinearWeightedImage(_LinearWeighted):
    pass


class LinearWeightedDepth(_LinearWeighted):
    pass


class LearnedPositionalEncoding(nn.Module):
    """mmdet 2.x ``LearnedPositionalEncoding`` (not in the reference tree; imported at :12):
    ``forward(mask (B,H,W)) -> (B, 2*num_feats, H, W)`` = cat(col_embed(x) over rows, row_embed(y)
    over columns)."""

    def __init__(self, num_feats, row_num_embed=50, col_num_embed=50):
        super().__init__()
        self.row_embed = nn.Embedding(row_num_embed, num_feats)
        self.col_embed = nn.Embedding(col_num_embed, num_feats)
        self.num_feats, self.row_num_embed, self.col_num_embed = num_feats, row_num_embed, col_num_embed
        nn.init.uniform_(self.row_embed.weight)
        nn.init.uniform_(self.col_embed.weight)

    def forward(self, mask):
        h, w = mask.shape[-2:]
        xe = self.col_embed(torch.arange(w, device=mask.device))
        ye = self.row_embed(torch.arange(h, device=mask.device))
        pos = torch.cat((xe.unsqueeze(0).expand(h, -1, -1), ye.unsqueeze(1).expand(-1, w, -1)), -1)
        return pos.permute(2, 0, 1).unsqueeze(0).repeat(mask.shape[0], 1, 1, 1)
