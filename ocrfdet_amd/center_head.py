"""The detector's box head: the reference's ``CenterHead`` and ``SeparateHead`` (mmdet3d/models/dense_heads/
centerpoint_head.py) with their constructor arguments, attribute names and ``state_dict`` keys, built without mmcv or
mmdet.  ``ConvBNReLU`` is ``blocks.ConvModule`` with a ReLU, for batch norms (mmcv's naming: ``conv`` / ``bn``,
``bias='auto'`` = no conv bias under BN).

The training path (``get_targets`` + ``loss``) has two formulations of the same arithmetic:

* the fused one -- ``csrc/center_head.hip``: the targets of every sample and task in one call (a memset and two
  launches), the Gaussian focal loss of every task in two launches (backward one), the L1 regression loss gathered at
  ``ind`` straight from the five head outputs in two launches (backward one).  No host synchronisation; reruns are
  bit-identical;
* the torch one (``*_torch``) -- the CPU path, and the fallback when ``fused_loss`` is False or an input is not float32.
  It is vectorised over boxes (no per-object Python loop) and reads nothing back to the host.

bfloat16 head outputs (``forward`` under bf16 autocast) are cast to float32 in ``loss`` and ``get_bboxes``: they take
the fused kernels, losses and boxes are float32, and autograd's cast hands a bf16 prediction a bf16 gradient.  The
reference runs the head's loss in whatever dtype arrives; float16 outputs keep the torch formulation.

Both keep the reference's integer outcomes (slot, radius, centre cell) and heatmap values bit for bit: the radius in
float32 in the reference's operation order, the Gaussian in float64 as numpy computes it.

``get_bboxes`` (top-K decode, circle and rotated BEV NMS, merge) is in ``center_decode.py``: fused by
``csrc/center_decode.hip`` in four launches with no host synchronisation (``get_bboxes_padded``), or by its torch
formulation on the CPU, for inputs that are not float32 CUDA tensors and with ``fused_decode = False``.  A head built
without ``bbox_coder`` or ``test_cfg`` (training only) cannot decode and raises ``NotImplementedError``.

``DCNSeparateHead`` (``separate_head=dict(type='DCNSeparateHead', dcn_config=dict(type='DCN', ...))``) is built on
``deform_conv.DeformConv2dPack``; a ``dcn_config`` of any other type raises ``NotImplementedError``.
"""
import copy
import ctypes

import torch
import torch.nn as nn

from . import _lib
from . import center_decode as cd
from .blocks import ConvModule, kaiming_init
from .deform_conv import build_dcn

__all__ = ['ConvBNReLU', 'SeparateHead', 'DCNSeparateHead', 'CenterHead', 'HeatmapLoss', 'RegLoss', 'clip_sigmoid',
           'gaussian_focal_loss', 'targets_torch', 'heatmap_loss_torch', 'reg_loss_torch', 'pack_boxes', 'reduce_counts']

F32_EPS = float(torch.finfo(torch.float32).eps)
GROUPS = ('xy', 'z', 'whl', 'yaw', 'vel')
CLIP_INDEX = (0, 2, 3, 6, 8, 10)
HEADS = ('reg', 'height', 'dim', 'rot', 'vel')


class ConvBNReLU(ConvModule):
    """mmcv ``ConvModule(c_in, c_out, k, padding=..., norm_cfg=BN2d)``: conv (no bias under BN), ``bn``, ReLU."""

    def __init__(self, c_in, c_out, kernel_size, stride=1, padding=0, bias='auto', conv_cfg=None,
                 norm_cfg=dict(type='BN2d'), **kwargs):
        if conv_cfg not in (None, dict(type='Conv2d')):
            raise NotImplementedError(f'conv_cfg {conv_cfg}: only Conv2d')
        if norm_cfg is not None and norm_cfg.get('type') not in ('BN', 'BN2d'):
            raise NotImplementedError(f'norm_cfg {norm_cfg}: only BN2d')
        super().__init__(c_in, c_out, kernel_size, stride=stride, padding=padding, bias=bias, conv_cfg=conv_cfg,
                         norm_cfg=norm_cfg, act_cfg=dict(type='ReLU'), inplace=True)


class SeparateHead(nn.Module):
    """The reference's ``SeparateHead``: per head ``num_conv - 1`` ConvModules and a final plain Conv2d with bias."""

    def __init__(self, in_channels, heads, head_conv=64, final_kernel=1, init_bias=-2.19, conv_cfg=dict(type='Conv2d'),
                 norm_cfg=dict(type='BN2d'), bias='auto', init_cfg=None, **kwargs):
        assert init_cfg is None, 'To prevent abnormal initialization behavior, init_cfg is not allowed to be set'
        super().__init__()
        self.heads = heads
        self.init_bias = init_bias
        for head in self.heads:
            classes, num_conv = self.heads[head]
            layers, c_in = [], in_channels
            for _ in range(num_conv - 1):
                layers.append(ConvBNReLU(c_in, head_conv, final_kernel, padding=final_kernel // 2, bias=bias,
                                         conv_cfg=conv_cfg, norm_cfg=norm_cfg))
                c_in = head_conv
            layers.append(nn.Conv2d(head_conv, classes, final_kernel, stride=1, padding=final_kernel // 2, bias=True))
            self.__setattr__(head, nn.Sequential(*layers))

    def init_weights(self):
        kaiming_init(self)
        for head in self.heads:
            if head == 'heatmap':
                self.__getattr__(head)[-1].bias.data.fill_(self.init_bias)

    def forward(self, x):
        return {head: self.__getattr__(head)(x) for head in self.heads}


class DCNSeparateHead(nn.Module):
    """The reference's ``DCNSeparateHead`` (centerpoint_head.py:125-240): one deformable convolution in front of the
    heatmap head (``feature_adapt_cls`` -> ``cls_head``) and one in front of the regression heads (``feature_adapt_reg``
    -> ``task_head``, a ``SeparateHead`` without the heatmap).  ``dcn_config``: ``dict(type='DCN', in_channels=...,
    out_channels=..., kernel_size=..., padding=..., groups=..., ...)``, built by ``deform_conv.build_dcn``; any other
    type (or none) raises ``NotImplementedError``.

    ``init_weights`` does what the reference's ``init_cfg = dict(type='Kaiming', layer='Conv2d')`` does: every
    ``nn.Conv2d`` inside the head, the ``conv_offset`` of the two deformable convolutions included, gets Kaiming-normal
    weights; the deformable weights themselves keep their construction-time initialisation."""

    def __init__(self, in_channels, num_cls, heads, dcn_config, head_conv=64, final_kernel=1, init_bias=-2.19,
                 conv_cfg=dict(type='Conv2d'), norm_cfg=dict(type='BN2d'), bias='auto', init_cfg=None, **kwargs):
        assert init_cfg is None, 'To prevent abnormal initialization behavior, init_cfg is not allowed to be set'
        super().__init__()
        heads = dict(heads)
        heads.pop('heatmap', None)
        self.feature_adapt_cls = build_dcn(dcn_config)
        self.feature_adapt_reg = build_dcn(dcn_config)
        self.cls_head = nn.Sequential(
            ConvBNReLU(in_channels, head_conv, 3, padding=1, conv_cfg=conv_cfg, bias=bias, norm_cfg=norm_cfg),
            nn.Conv2d(head_conv, num_cls, 3, stride=1, padding=1, bias=bool(bias)))
        self.init_bias = init_bias
        self.task_head = SeparateHead(in_channels, heads, head_conv=head_conv, final_kernel=final_kernel, bias=bias)

    def init_weights(self):
        kaiming_init(self)
        self.cls_head[-1].bias.data.fill_(self.init_bias)

    def forward(self, x):
        ret = self.task_head(self.feature_adapt_reg(x))
        ret['heatmap'] = self.cls_head(self.feature_adapt_cls(x))
        return ret


def clip_sigmoid(x, eps=1e-4):
    """The reference's clip_sigmoid without its in-place ``sigmoid_`` on the logits."""
    return torch.clamp(x.sigmoid(), min=eps, max=1 - eps)


def gaussian_focal_loss(pred, target, alpha=2.0, gamma=4.0):
    """mmdet 2.x gaussian_focal_loss, elementwise."""
    eps = 1e-12
    pos_weights = target.eq(1)
    neg_weights = (1 - target).pow(gamma)
    pos_loss = -(pred + eps).log() * (1 - pred).pow(alpha) * pos_weights
    neg_loss = -(1 - pred + eps).log() * pred.pow(alpha) * neg_weights
    return pos_loss + neg_loss


def _divisor(avg_factor):
    """weight_reduce_loss's ``avg_factor + eps``: the reference's avg_factor is a Python float (the float32 count read
    back by ``.item()``, plus 1e-4 for the task-specific regression), so the sum is float64, rounded to float32 where
    the division happens."""
    return (avg_factor.double() + F32_EPS).float()


# --------------------------------------------------------------------------------------------- boxes
def pack_boxes(gt_bboxes_3d, gt_labels_3d, device):
    """(boxes (N, D) f32, labels (N,) int64, offsets (B + 1,) int64) on ``device``.  Boxes are objects with ``.tensor``
    (LiDARInstance3DBoxes) or plain (N, >= 7) tensors, bottom-centre z.  What is on the host travels in one pinned
    non-blocking copy."""
    tens = [(b.tensor if hasattr(b, 'tensor') else b) for b in gt_bboxes_3d]
    widths = {int(t.shape[-1]) for t in tens if t.dim() == 2}
    if len(widths) > 1:
        raise ValueError(f'all boxes must have the same width, got {sorted(widths)}')
    D = widths.pop() if widths else 9
    offs = [0]
    for t in tens:
        offs.append(offs[-1] + int(t.shape[0]))
    N = offs[-1]
    dev = torch.device(device)
    if dev.type == 'cuda' and not any(t.is_cuda for t in tens) and not any(l.is_cuda for l in gt_labels_3d):
        nb = N * D + (N * D) % 2                    # int64 words start 8-byte aligned
        buf = torch.empty(nb + 2 * (N + len(offs)), dtype=torch.float32, pin_memory=True)
        ints = buf[nb:].view(torch.int64)
        if N:
            buf[:N * D] = torch.cat([t.reshape(-1, D).float() for t in tens]).reshape(-1)
            ints[:N] = torch.cat([l.reshape(-1).long() for l in gt_labels_3d])
        ints[N:] = torch.tensor(offs, dtype=torch.int64)
        d = buf.to(dev, non_blocking=True)
        di = d[nb:].view(torch.int64)
        return d[:N * D].view(N, D), di[:N], di[N:]
    boxes = torch.cat([t.reshape(-1, D).to(dev, torch.float32) for t in tens]) if N else torch.zeros(0, D, device=dev)
    labels = torch.cat([l.reshape(-1).to(dev, torch.int64) for l in gt_labels_3d]) if N else \
        torch.zeros(0, dtype=torch.int64, device=dev)
    if dev.type == 'cuda':
        ob = torch.tensor(offs, dtype=torch.int64).pin_memory()
        offsets = ob.to(dev, non_blocking=True)
    else:
        offsets = torch.tensor(offs, dtype=torch.int64)
    return boxes, labels, offsets


# --------------------------------------------------------------------------------------------- torch formulation
def _const(values, dtype, dev):
    """A small constant tensor on ``dev`` without a host synchronisation (pinned, non-blocking)."""
    t = torch.tensor(values, dtype=dtype)
    return t.pin_memory().to(dev, non_blocking=True) if dev.type == 'cuda' else t


def _radius_torch(height, width, o):
    """gaussian_radius on tensors with the reference's float32 operation order and Python min()."""
    b1 = height + width
    c1 = width * height * (1 - o) / (1 + o)
    r1 = (b1 + torch.sqrt(b1 ** 2 - 4 * c1)) / 2
    b2 = 2 * (height + width)
    c2 = (1 - o) * width * height
    r2 = (b2 + torch.sqrt(b2 ** 2 - 16 * c2)) / 2
    a3 = 4 * o
    b3 = -2 * o * (height + width)
    c3 = (o - 1) * width * height
    r3 = (b3 + torch.sqrt(b3 ** 2 - 4 * a3 * c3)) / 2
    r = torch.where(r2 < r1, r2, r1)
    return torch.where(r3 < r, r3, r)


def targets_torch(boxes, labels, offsets, table, ncls, cfg, with_velocity, norm_bbox):
    """Torch formulation of the batch's targets -> (heat (sum of B * ncls * H * W,) f32 flat, anno (T, B, M, C),
    ind (T, B, M) int64, mask (T, B, M) uint8, counts (2T,) f32).  ``table`` (n_labels, 2) int32: task, class."""
    dev = boxes.device
    T, B = len(ncls), offsets.numel() - 1
    W, H = (int(g) // int(cfg['out_size_factor']) for g in cfg['grid_size'][:2])
    M = int(cfg['max_objs']) * int(cfg['dense_reg'])
    C = 10 if with_velocity else 8
    osf = int(cfg['out_size_factor'])
    vs = _const(cfg['voxel_size'], torch.float32, dev)
    pc = _const(cfg['point_cloud_range'], torch.float32, dev)
    N = boxes.shape[0]
    idx = torch.arange(N, device=dev)
    sample = torch.searchsorted(offsets[1:].contiguous(), idx, right=True)
    lab = labels.long()
    inrange_lab = (lab >= 0) & (lab < table.shape[0])
    tc = table.to(dev).long()[lab.clamp(0, table.shape[0] - 1)]
    task = torch.where(inrange_lab, tc[:, 0], torch.full_like(lab, -1))
    cls = tc[:, 1]
    # slot: rank within (sample, task) after the class-by-class regrouping, ties by original order
    key = ((sample * (T + 1) + (task + 1)) * 64 + cls) * (N + 1) + idx
    order = torch.argsort(key)
    rank = torch.empty_like(idx)
    rank[order] = idx
    gkey = sample * (T + 1) + (task + 1)
    sorted_g = gkey[order]
    first = torch.searchsorted(sorted_g, gkey)
    slot = rank - first
    width = boxes[:, 3] / vs[0] / osf
    length = boxes[:, 4] / vs[1] / osf
    ok = (task >= 0) & (slot < M) & (width > 0) & (length > 0)
    radius = _radius_torch(length, width, float(cfg['gaussian_overlap']))
    radius = torch.clamp(torch.nan_to_num(radius, nan=0.0).clamp(max=65536.0).to(torch.int32),
                         min=int(cfg['min_radius']))
    cx = (boxes[:, 0] - pc[0]) / vs[0] / osf
    cy = (boxes[:, 1] - pc[1]) / vs[1] / osf
    ix, iy = cx.to(torch.int32), cy.to(torch.int32)
    drawn = ok & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    # rows
    z = boxes[:, 2] + boxes[:, 5] * 0.5
    dims = boxes[:, 3:6].log() if norm_bbox else boxes[:, 3:6]
    cols = [cx - ix, cy - iy, z[:, None], dims, torch.sin(boxes[:, 6:7]), torch.cos(boxes[:, 6:7])]
    if with_velocity:
        cols.append(boxes[:, 7:9])
    rows = torch.cat([c if c.dim() == 2 else c[:, None] for c in cols], 1)
    dump = T * B * M
    dest = torch.where(drawn, (task.clamp(min=0) * B + sample) * M + slot.clamp(max=M - 1), torch.full_like(idx, dump))
    anno = torch.zeros(dump + 1, C, device=dev)
    ind = torch.zeros(dump + 1, dtype=torch.int64, device=dev)
    mask = torch.zeros(dump + 1, dtype=torch.uint8, device=dev)
    if N:                                           # undrawn boxes all land in the discarded row `dump`
        anno.index_copy_(0, dest, rows)
        ind.index_copy_(0, dest, (iy.long() * W + ix.long()))
        mask.index_copy_(0, dest, drawn.to(torch.uint8))
    anno, ind, mask = anno[:dump].view(T, B, M, C), ind[:dump].view(T, B, M), mask[:dump].view(T, B, M)
    # heatmap: max over objects of numpy's float64 Gaussian, per (task, sample, class) plane
    P = sum(ncls)
    cls0 = _const([sum(ncls[:t]) for t in range(T)], torch.int64, dev)
    plane = torch.where(drawn, sample * P + cls0[task.clamp(min=0)] + cls, torch.full_like(idx, B * P))
    heat = torch.zeros(B * P + 1, H, W, dtype=torch.float32, device=dev)
    yy = torch.arange(H, device=dev, dtype=torch.float64)[None, :, None]
    xx = torch.arange(W, device=dev, dtype=torch.float64)[None, None, :]
    r = radius.double()[:, None, None]
    sigma = (2 * r + 1) / 6
    for s0 in range(0, N, 64):
        sl = slice(s0, s0 + 64)
        dx = xx - ix[sl].double()[:, None, None]
        dy = yy - iy[sl].double()[:, None, None]
        g = torch.exp(-(dx * dx + dy * dy) / (2 * sigma[sl] * sigma[sl]))
        g = torch.where((g < torch.finfo(torch.float64).eps) | (dx.abs() > r[sl]) | (dy.abs() > r[sl]),
                        torch.zeros_like(g), g).float()
        heat.index_reduce_(0, plane[sl], g, 'amax', include_self=True)
    heat = heat[:B * P].view(B, P, H, W)
    flat = torch.cat([heat[:, sum(ncls[:t]):sum(ncls[:t + 1])].reshape(-1) for t in range(T)])
    ones = torch.stack([heat[:, sum(ncls[:t]):sum(ncls[:t + 1])].eq(1).float().sum() for t in range(T)])
    msum = mask.float().sum((1, 2))
    return flat, anno, ind, mask, torch.cat([ones, msum])


def heatmap_loss_torch(logits, heatmaps, counts, loss_weight=1.0):
    """Per task: (clip_sigmoid(logits), loss_weight * gaussian focal sum / (max(count, 1) + eps))."""
    clipped, out = [], []
    for t, (x, g) in enumerate(zip(logits, heatmaps)):
        p = clip_sigmoid(x)
        clipped.append(p)
        out.append(loss_weight * (gaussian_focal_loss(p, g).sum() / _divisor(torch.clamp(counts[t], min=1))))
    return clipped, out


def _gather_pred(preds, ind, with_velocity):
    keys = HEADS if with_velocity else HEADS[:4]
    pred = torch.cat([preds[k] for k in keys], 1).permute(0, 2, 3, 1).contiguous()
    pred = pred.view(pred.size(0), -1, pred.size(3))
    return pred.gather(1, ind.unsqueeze(2).expand(ind.size(0), ind.size(1), pred.size(2)))


def reg_loss_torch(preds, anno, ind, mask, num, code_weights, loss_weight=0.25, task_specific=True, reduction='mean'):
    """One task's L1 regression loss -> a list of the five group losses (task_specific) or one loss."""
    C = anno.shape[-1]
    pred = _gather_pred(preds, ind, C == 10)
    m = mask.unsqueeze(2).expand_as(anno).float()
    m = m * (~torch.isnan(anno)).float()
    w = m * _const(code_weights[:C], torch.float32, m.device)
    num = torch.clamp(num, min=1e-4)

    def l1(p, t, wt, avg):
        loss = torch.abs(p - t) * wt
        if reduction == 'none':
            return loss_weight * loss
        return loss_weight * (loss.sum() / _divisor(avg))
    if task_specific:
        return [l1(pred[..., a:b], anno[..., a:b], w[..., a:b], num.double() + 1e-4) for a, b in zip(CLIP_INDEX, CLIP_INDEX[1:])]
    return [l1(pred, anno, w, num)]


# --------------------------------------------------------------------------------------------- fused
def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t is not None and t.numel() else 0 for t in tensors])


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def targets_fused(boxes, labels, offsets, table, ncls, cfg, with_velocity, norm_bbox):
    """``targets_torch`` by ``ocrf_center_head_targets``."""
    dev = boxes.device
    T, B = len(ncls), offsets.numel() - 1
    W, H = (int(g) // int(cfg['out_size_factor']) for g in cfg['grid_size'][:2])
    M = int(cfg['max_objs']) * int(cfg['dense_reg'])
    C = 10 if with_velocity else 8
    N, D = boxes.shape
    heat = torch.empty(B * sum(ncls) * H * W, device=dev)
    anno = torch.empty(T, B, M, C, device=dev)
    ind = torch.empty(T, B, M, dtype=torch.int64, device=dev)
    mask = torch.empty(T, B, M, dtype=torch.uint8, device=dev)
    counts = torch.empty(2 * T, device=dev)
    ws = _lib.workspace.get(dev, _lib.lib().ocrf_center_head_targets_workspace_bytes(N), 'center_head_targets')
    vs = (ctypes.c_float * 2)(*[float(v) for v in cfg['voxel_size'][:2]])
    pc = (ctypes.c_float * 2)(*[float(v) for v in cfg['point_cloud_range'][:2]])
    boxes, labels = boxes.contiguous(), labels.contiguous()
    _lib.launch('ocrf_center_head_targets', dev, B, T, _ints(ncls), table.shape[0], table, N, D, boxes, labels, offsets,
                H, W, M, int(with_velocity), int(norm_bbox), vs, pc, int(cfg['out_size_factor']),
                float(cfg['gaussian_overlap']), int(cfg['min_radius']), heat, anno, ind, mask, counts, ws, ws.numel())
    return heat, anno, ind, mask, counts


class HeatmapLoss(torch.autograd.Function):
    """(heat flat, counts, loss_weight, *logits) -> (losses (T,), *clip_sigmoid outputs) by
    ``ocrf_center_head_heatmap_loss`` / ``_backward``; the clipped outputs carry no gradient."""

    @staticmethod
    def forward(ctx, heat, counts, loss_weight, *logits):
        x = [l.detach().contiguous() for l in logits]
        B, HW = x[0].shape[0], x[0].shape[2] * x[0].shape[3]
        ncls = [int(l.shape[1]) for l in x]
        dev = x[0].device
        clipped = [torch.empty_like(l) for l in x]
        out = torch.empty(len(x), device=dev)
        dens = torch.empty(len(x), device=dev)
        ws = _lib.workspace.get(dev, _lib.lib().ocrf_center_head_heatmap_loss_workspace_bytes(B, len(x), _ints(ncls), HW),
                                'center_head_hm')
        _lib.launch('ocrf_center_head_heatmap_loss', dev, B, len(x), _ints(ncls), HW, _ptrs(x), heat, counts,
                    float(loss_weight), _ptrs(clipped), out, dens, ws, ws.numel())
        ctx.save_for_backward(heat, dens, *x)
        ctx.loss_weight = float(loss_weight)
        ctx.mark_non_differentiable(*clipped)
        return (out, *clipped)

    @staticmethod
    def backward(ctx, g_out, *_):
        heat, dens, *x = ctx.saved_tensors
        B, HW = x[0].shape[0], x[0].shape[2] * x[0].shape[3]
        ncls = [int(l.shape[1]) for l in x]
        dev = x[0].device
        grads = [torch.empty_like(l) for l in x]
        go = g_out.float().contiguous()
        _lib.launch('ocrf_center_head_heatmap_loss_backward', dev, B, len(x), _ints(ncls), HW, _ptrs(x), heat, dens, go,
                    ctx.loss_weight, _ptrs(grads))
        return (None, None, None, *grads)


class RegLoss(torch.autograd.Function):
    """(anno, ind, mask, counts, code_weights, loss_weight, with_velocity, *heads (5 per task)) -> losses (T, 6) by
    ``ocrf_center_head_reg_loss`` / ``_backward``: columns 0-4 the task-specific groups, 5 the single sum."""

    @staticmethod
    def forward(ctx, anno, ind, mask, counts, code_weights, loss_weight, with_velocity, *heads):
        T, B, M, C = anno.shape
        h = [v.detach().contiguous() if v is not None else None for v in heads]
        HW = h[0].shape[2] * h[0].shape[3]
        dev = anno.device
        out = torch.empty(T, 6, device=dev)
        dens = torch.empty(T, 2, device=dev)
        cw = (ctypes.c_float * C)(*[float(v) for v in code_weights[:C]])
        ws = _lib.workspace.get(dev, _lib.lib().ocrf_center_head_reg_loss_workspace_bytes(B, T), 'center_head_reg')
        _lib.launch('ocrf_center_head_reg_loss', dev, B, T, HW, M, int(with_velocity), _ptrs(h), anno, ind, mask, cw, counts,
                    float(loss_weight), out, dens, ws, ws.numel())
        ctx.save_for_backward(anno, ind, mask, dens, *[v for v in h if v is not None])
        ctx.present = [v is not None for v in h]
        ctx.args = ([float(v) for v in code_weights[:C]], float(loss_weight), int(with_velocity))
        return out

    @staticmethod
    def backward(ctx, g_out):
        anno, ind, mask, dens, *hs = ctx.saved_tensors
        it = iter(hs)
        h = [next(it) if p else None for p in ctx.present]
        T, B, M, C = anno.shape
        HW = h[0].shape[2] * h[0].shape[3]
        dev = anno.device
        sizes = [v.numel() if v is not None else 0 for v in h]
        flat = torch.zeros(sum(sizes), device=dev)              # one fill for every gradient
        grads, o = [], 0
        for v, n in zip(h, sizes):
            grads.append(flat[o:o + n].view_as(v) if v is not None else None)
            o += n
        cw, lw, wv = ctx.args
        go = g_out.float().contiguous()
        _lib.launch('ocrf_center_head_reg_loss_backward', dev, B, T, HW, M, wv, _ptrs(h), anno, ind, mask,
                    (ctypes.c_float * C)(*cw), dens, go, lw, _ptrs(grads))
        return (None,) * 7 + tuple(grads)


def reduce_counts(counts):
    """mmdet's reduce_mean of every count at once: one async all_reduce of the (2T,) vector when distributed."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return counts
    counts = counts.clone()
    dist.all_reduce(counts.div_(dist.get_world_size()), op=dist.ReduceOp.SUM, async_op=True).wait()
    return counts


# --------------------------------------------------------------------------------------------- head
class CenterHead(nn.Module):
    """The reference's ``CenterHead`` (same arguments, attributes and state_dict).  ``fused_loss`` (default True)
    selects the HIP targets and losses when the inputs are float32 CUDA tensors.

    ``fused_decode_bf16`` (class attribute, default False): head outputs that are all CUDA bfloat16 (a head under bf16
    autocast) are decoded in place by ``ocrf_center_decode_bf16`` instead of being cast to float32 first, one cast
    launch per head tensor; the results are the same bits."""

    fused_decode_bf16 = False

    def __init__(self, in_channels=[128], tasks=None, train_cfg=None, test_cfg=None, bbox_coder=None,
                 common_heads=dict(), loss_cls=dict(type='GaussianFocalLoss', reduction='mean'),
                 loss_bbox=dict(type='L1Loss', reduction='none', loss_weight=0.25),
                 separate_head=dict(type='SeparateHead', init_bias=-2.19, final_kernel=3), share_conv_channel=64,
                 num_heatmap_convs=2, conv_cfg=dict(type='Conv2d'), norm_cfg=dict(type='BN2d'), bias='auto',
                 norm_bbox=True, init_cfg=None, task_specific=True):
        assert init_cfg is None, 'To prevent abnormal initialization behavior, init_cfg is not allowed to be set'
        super().__init__()
        num_classes = [len(t['class_names']) for t in tasks]
        self.class_names = [t['class_names'] for t in tasks]
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.norm_bbox = norm_bbox
        if loss_cls.get('type') != 'GaussianFocalLoss' or loss_cls.get('reduction', 'mean') != 'mean':
            raise NotImplementedError(f'loss_cls {loss_cls}: only GaussianFocalLoss with reduction mean')
        if loss_bbox.get('type') != 'L1Loss' or loss_bbox.get('reduction', 'mean') not in ('mean', 'none'):
            raise NotImplementedError(f'loss_bbox {loss_bbox}: only L1Loss with reduction mean or none')
        self.loss_cls_cfg, self.loss_bbox_cfg = dict(loss_cls), dict(loss_bbox)
        if isinstance(bbox_coder, dict):
            coder = dict(bbox_coder)
            kind = coder.pop('type', 'CenterPointBBoxCoder')
            if kind != 'CenterPointBBoxCoder':
                raise NotImplementedError(f'bbox_coder type {kind}: only CenterPointBBoxCoder')
            bbox_coder = cd.CenterPointBBoxCoder(**coder)
        self.bbox_coder = bbox_coder
        self.fused_decode = True
        self.num_anchor_per_locs = [n for n in num_classes]
        self.fp16_enabled = False
        self.fused_loss = True
        self.shared_conv = ConvBNReLU(in_channels, share_conv_channel, 3, padding=1, conv_cfg=conv_cfg,
                                      norm_cfg=norm_cfg, bias=bias)
        self.task_heads = nn.ModuleList()
        separate_head = dict(separate_head)
        kind = separate_head.pop('type', 'SeparateHead')
        for num_cls in num_classes:
            heads = copy.deepcopy(common_heads)
            heads.update(dict(heatmap=(num_cls, num_heatmap_convs)))
            separate_head.update(in_channels=share_conv_channel, heads=heads, num_cls=num_cls)
            if kind == 'DCNSeparateHead':
                self.task_heads.append(DCNSeparateHead(**separate_head))
            elif kind != 'SeparateHead':
                raise NotImplementedError(f'separate_head type {kind}')
            else:
                self.task_heads.append(SeparateHead(**separate_head))
        self.with_velocity = 'vel' in common_heads.keys()
        self.task_specific = task_specific
        # label -> (task, class in task), the regrouping of get_targets_single
        table = [(t, c) for t, names in enumerate(self.class_names) for c in range(len(names))]
        self.register_buffer('_class_table', torch.tensor(table, dtype=torch.int32).view(-1, 2), persistent=False)

    def init_weights(self):
        kaiming_init(self.shared_conv)
        for h in self.task_heads:
            h.init_weights()

    def forward_single(self, x):
        x = self.shared_conv(x)
        return [task(x) for task in self.task_heads]

    def forward(self, feats):
        outs = [self.forward_single(f) for f in feats]
        return tuple(map(list, zip(*outs)))

    # ----------------------------------------------------------------------------------------- targets
    def _fused(self, *tensors):
        return self.fused_loss and all(t.is_cuda and t.dtype == torch.float32 for t in tensors)

    def _targets(self, gt_bboxes_3d, gt_labels_3d, device=None, fused=None):
        if device is None:                          # the reference builds the targets on the labels' device
            device = gt_labels_3d[0].device if len(gt_labels_3d) else torch.device('cpu')
        boxes, labels, offsets = pack_boxes(gt_bboxes_3d, gt_labels_3d, device)
        table = self._class_table.to(device)
        if fused is None:
            fused = self.fused_loss and device.type == 'cuda'
        if fused:
            return targets_fused(boxes, labels, offsets, table, self.num_classes, self.train_cfg, self.with_velocity,
                                 self.norm_bbox)
        return targets_torch(boxes, labels, offsets, table, self.num_classes, self.train_cfg, self.with_velocity,
                             self.norm_bbox)

    def _split_heat(self, heat, B):
        W, H = (int(g) // int(self.train_cfg['out_size_factor']) for g in self.train_cfg['grid_size'][:2])
        out, o = [], 0
        for n in self.num_classes:
            out.append(heat[o:o + B * n * H * W].view(B, n, H, W))
            o += B * n * H * W
        return out

    def get_targets(self, gt_bboxes_3d, gt_labels_3d):
        """(heatmaps, anno_boxes, inds, masks), each a list over tasks, as the reference's."""
        heat, anno, ind, mask, _ = self._targets(gt_bboxes_3d, gt_labels_3d)
        return self._split_heat(heat, len(gt_labels_3d)), list(anno.unbind(0)), list(ind.unbind(0)), \
            list(mask.unbind(0))

    def loss(self, gt_bboxes_3d, gt_labels_3d, preds_dicts, **kwargs):
        """The reference's loss dict: task{i}.loss_{xy,z,whl,yaw,vel,heatmap}, or 'loss' without task_specific."""
        B = len(gt_labels_3d)
        cast = cd.bf16_as_float32(preds_dicts)      # read from these; the caller's dicts get 'heatmap' and 'anno_box'
        logits = [p[0]['heatmap'] for p in cast]
        heat, anno, ind, mask, counts = self._targets(gt_bboxes_3d, gt_labels_3d, device=logits[0].device)
        counts = reduce_counts(counts)
        T = len(self.num_classes)
        heads = [[p[0].get(k) for k in HEADS] for p in cast]
        w_cls = float(self.loss_cls_cfg.get('loss_weight', 1.0))
        w_box = float(self.loss_bbox_cfg.get('loss_weight', 1.0))
        cw = list(self.train_cfg['code_weights'])
        red = self.loss_bbox_cfg.get('reduction', 'mean')
        used = [h for hs in heads for h in (hs if self.with_velocity else hs[:4])]
        W, H = (int(g) // int(self.train_cfg['out_size_factor']) for g in self.train_cfg['grid_size'][:2])
        for t, x in enumerate(logits):
            if tuple(x.shape) != (B, self.num_classes[t], H, W) or any(
                    h.dim() != 4 or tuple(h.shape[::2]) != (B, H) or h.shape[3] != W for h in used):
                raise ValueError(f'task {t}: head outputs must be (B={B}, C, {H}, {W}) as the targets, got '
                                 f'{tuple(x.shape)}')
        fused = self._fused(*logits, *used) and heat.is_cuda and red == 'mean'
        if fused:
            hm_out, *clipped = HeatmapLoss.apply(heat, counts, w_cls, *logits)
            hm = list(hm_out.unbind(0))
            flat = [h if (self.with_velocity or i % 5 < 4) else None for i, h in enumerate(x for hs in heads for x in hs)]
            reg = RegLoss.apply(anno, ind, mask, counts, cw, w_box, self.with_velocity, *flat)
            regs = [list(reg[t, :5].unbind(0)) if self.task_specific else [reg[t, 5]] for t in range(T)]
        else:
            clipped, hm = heatmap_loss_torch(logits, self._split_heat(heat, B), counts, w_cls)
            regs = [reg_loss_torch(p[0], anno[t], ind[t], mask[t], counts[T + t], cw, w_box, self.task_specific, red)
                    for t, p in enumerate(cast)]
        loss_dict = dict()
        if not self.task_specific:
            loss_dict['loss'] = 0
        for task_id, preds_dict in enumerate(preds_dicts):
            preds_dict[0]['heatmap'] = clipped[task_id]
            keys = HEADS if self.with_velocity else HEADS[:4]
            preds_dict[0]['anno_box'] = torch.cat([preds_dict[0][k] for k in keys], dim=1)
            if self.task_specific:
                for name, v in zip(GROUPS, regs[task_id]):
                    loss_dict[f'task{task_id}.loss_{name}'] = v
                loss_dict[f'task{task_id}.loss_heatmap'] = hm[task_id]
            else:
                loss_dict['loss'] += regs[task_id][0]
                loss_dict['loss'] += hm[task_id]
        return loss_dict

    # ----------------------------------------------------------------------------------------- decode
    def _decode_cfg(self):
        if self.bbox_coder is None or self.test_cfg is None:
            raise NotImplementedError('CenterHead decoding needs both bbox_coder and test_cfg; this head was built '
                                      'for training only')
        return cd.DecodeConfig(self.bbox_coder, self.test_cfg, self.num_classes)

    def get_bboxes_padded(self, preds_dicts):
        """Every sample's detections, padded and without a host synchronisation: boxes (B, M, 9 | 7) f32 with
        bottom-centre z, scores (B, M) f32, labels (B, M) int32 and counts (B,) int32, M = T * post_max_size; rows past
        a sample's count are zero."""
        cfg = self._decode_cfg()
        if self.fused_decode and self.fused_decode_bf16 and cd.fused_ok(preds_dicts, torch.bfloat16):
            return cd.decode_fused(preds_dicts, cfg, self.norm_bbox)        # read in place: no casts
        preds_dicts = cd.bf16_as_float32(preds_dicts)
        if self.fused_decode and cd.fused_ok(preds_dicts):
            return cd.decode_fused(preds_dicts, cfg, self.norm_bbox)
        return cd.decode_torch(preds_dicts, cfg, self.norm_bbox)

    def get_bboxes(self, preds_dicts, img_metas, img=None, rescale=False):
        """The reference's list over samples of [bboxes, scores, labels]: bboxes through ``img_metas[i]['box_type_3d']``
        (box_dim 9, or 7 without velocity) when the metas provide it, else a plain (n, 9 | 7) float32 tensor; labels
        int32.  Reads the B counts back once."""
        boxes, scores, labels, counts = self.get_bboxes_padded(preds_dicts)
        ret = []
        for i, n in enumerate(cd.read_counts(counts)):
            b = boxes[i, :n]
            meta = img_metas[i] if img_metas is not None and i < len(img_metas) else None
            if isinstance(meta, dict) and 'box_type_3d' in meta:
                b = meta['box_type_3d'](b, b.shape[1])
            ret.append([b, scores[i, :n], labels[i, :n]])
        return ret
