"""Training losses of the neck: the reference's ``get_loss`` (view_transformer_ocrf.py:1354-1417) with its helpers
``get_downsampled_gt_depth_and_semantic`` (:1203-1282), ``get_depth_and_semantic_loss`` (:1284-1314), ``Box2dtoMask``
(:1337-1352) and MVSGaussian's SSIM (lib/train/losses/ssim_loss.py).

Two formulations of the same arithmetic:

* the fused one — ``csrc/losses.hip`` behind ``depth_labels``, ``DepthSemanticLoss`` and ``RenderLosses``: labels in one
  launch, the depth / semantic BCE in two (backward one), the masked MSE + 1 - SSIM + depth L1 of every sample and render
  in three (backward one).  No host synchronisation, no data-dependent shapes, deterministic;
* the torch one (``*_torch``) — the CPU path, and the fallback when a gt tensor requires grad or the module's
  ``fused_losses`` is False.  It keeps the reference's values without its host reads: masks are weights, the depth range
  is reduced on the device.

Neither writes the caller's gt tensors (the reference zeroes out-of-range depths in place).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

__all__ = ['MASK_AFTER_ITERATION', 'box_bounds', 'box_mask', 'depth_labels', 'depth_labels_torch',
           'depth_semantic_loss', 'depth_semantic_loss_torch', 'render_losses', 'render_losses_torch', 'pack_boxes',
           'SSIM', 'ssim', 'ssim_torch', 'gaussian_window']

MASK_AFTER_ITERATION = 3862 * 2         # the box mask applies while the call counter is above this (:1375)
_ORIG_W, _Y_SHIFT, _MAX_BOXES = 1600, 158, 256


# --------------------------------------------------------------------------------------------- labels
def _patches(t, ds):
    BN, H, W = t.shape[0], t.shape[-2], t.shape[-1]
    return t.reshape(BN, H // ds, ds, W // ds, ds).permute(0, 1, 3, 2, 4).reshape(-1, ds * ds)


def _bins(v, d0, step, D):
    """(v - (d0 - step)) / step with both scalars rounded to float32 once, kept where 0 <= bin < D + 1, else 0."""
    b = (v - (d0 - step)) / step
    return torch.where((b < D + 1) & (b >= 0.0), b, torch.zeros_like(b))


def _check_labels_shapes(gt_depth, gt_semantic, ds):
    if gt_depth.dim() != 4 or gt_depth.shape != gt_semantic.shape:
        raise ValueError(f'gt_depth and gt_semantic must both be (B,N,H,W), got {tuple(gt_depth.shape)} and '
                         f'{tuple(gt_semantic.shape)}')
    H, W = gt_depth.shape[-2:]
    if H % ds or W % ds:
        raise ValueError(f'H and W ({H}, {W}) must be multiples of the downsample factor {ds}')


def depth_labels_torch(gt_depth, gt_semantic, depth_cfg, D, ds):
    """Torch formulation of ``get_downsampled_gt_depth_and_semantic`` without writing its inputs -> (depth_labels
    (B*N*h*w, D), semantic_labels (B*N*h*w, 2)).  Rows whose semantic max is 1 hold the normalised histogram of the
    patch's depth x semantic bins (NaN when none is valid), the others the one-hot of the patch's nearest depth."""
    _check_labels_shapes(gt_depth, gt_semantic, ds)
    d0, d1, step = (float(v) for v in depth_cfg[:3])
    out = (gt_depth < d0) | (gt_depth > d1)
    gd = gt_depth.masked_fill(out, 0.0)
    gs = gt_semantic.masked_fill(out, 0.0)
    sd = gd * gs
    B, N, H, W = gd.shape
    gd, gs, sd = (t.reshape(B * N, H, W) for t in (gd, gs, sd))
    sem = _patches(gs, ds).max(-1).values
    sem_labels = F.one_hot(sem.long(), num_classes=2).float()
    dp = _patches(gd, ds)
    nearest = torch.where(dp == 0.0, torch.full_like(dp, 1e5), dp).min(-1).values
    hard = F.one_hot(_bins(nearest, d0, step, D).long(), num_classes=D + 1)[:, 1:].float()
    sp = _patches(sd, ds)
    sb = _bins(torch.where(sp == 0.0, torch.full_like(sp, 1e5), sp), d0, step, D).long()
    cnt = torch.zeros(sb.shape[0], D + 1, dtype=torch.long, device=sb.device).scatter_add_(1, sb, torch.ones_like(sb))
    soft = cnt[:, 1:] / cnt[:, 1:].sum(-1, keepdim=True)
    return torch.where((sem_labels[:, 1] > 0)[:, None], soft, hard), sem_labels


def depth_labels(gt_depth, gt_semantic, depth_cfg, D, ds):
    """``depth_labels_torch`` by ``ocrf_depth_labels`` (one launch, bit for bit the same labels)."""
    _lib.require_cuda(gt_depth, gt_semantic)
    _check_labels_shapes(gt_depth, gt_semantic, ds)
    B, N, H, W = gt_depth.shape
    gd, gs = gt_depth.detach().float().contiguous(), gt_semantic.detach().float().contiguous()
    R = B * N * (H // ds) * (W // ds)
    labels = torch.empty(R, D, device=gd.device)
    sem = torch.empty(R, 2, device=gd.device)
    d0, d1, step = (float(v) for v in depth_cfg[:3])
    _lib.launch('ocrf_depth_labels', gd.device, B * N, H, W, ds, D, d0, d1, step, gd, gs, labels, sem)
    return labels, sem


# --------------------------------------------------------------------------------------------- depth / semantic BCE
def depth_semantic_loss_torch(depth_labels, depth_preds, semantic_labels, semantic_preds, w_depth, w_semantic):
    """Torch formulation of ``get_depth_and_semantic_loss``: the row mask (label max > 0; NaN rows out) as a weight."""
    D = depth_preds.shape[1]
    dp = depth_preds.permute(0, 2, 3, 1).reshape(-1, D)
    sp = semantic_preds.permute(0, 2, 3, 1).reshape(-1, 2)
    mask = depth_labels.max(1).values > 0.0
    w = torch.where(semantic_labels[:, 1:2] > 0, torch.full_like(semantic_labels[:, 1:2], 0.9),
                    torch.full_like(semantic_labels[:, 1:2], 0.1))
    wm = w * mask[:, None]
    dl = torch.where(mask[:, None], depth_labels, torch.zeros_like(depth_labels))
    depth_loss = (F.binary_cross_entropy(dp, dl, reduction='none') * wm).sum() / wm.sum().clamp(min=0.1)
    t = semantic_labels
    pt = (1 - sp) * t + sp * (1 - t)
    focal = (0.25 * t + 0.75 * (1 - t)) * pt.pow(2)
    sem = F.binary_cross_entropy(sp, t, reduction='none') * focal * mask[:, None]
    semantic_loss = sem.sum() / mask.sum().clamp(min=1)
    return w_depth * depth_loss, w_semantic * semantic_loss


class DepthSemanticLoss(torch.autograd.Function):
    """(depth (BN,D,h,w), semantic (BN,2,h,w)) -> (w_depth * depth BCE, w_semantic * focal BCE) by
    ``ocrf_depth_semantic_loss`` / ``_backward``; the labels are constants."""

    @staticmethod
    def forward(ctx, depth, semantic, depth_labels, semantic_labels, w_depth, w_semantic):
        BN, D, h, w = depth.shape
        dev = depth.device
        dl, sl = depth_labels.contiguous(), semantic_labels.contiguous()
        d, s = depth.detach().contiguous(), semantic.detach().contiguous()
        out = torch.empty(2, device=dev)
        denoms = torch.empty(2, device=dev)
        ws = _lib.workspace.get(dev, _lib.lib().ocrf_depth_semantic_loss_workspace_bytes(BN * h * w), 'losses_ds')
        _lib.launch('ocrf_depth_semantic_loss', dev, BN, h * w, D, dl, sl, d, s, float(w_depth), float(w_semantic), out,
                    denoms, ws, ws.numel())
        ctx.save_for_backward(d, s, dl, sl, denoms)
        ctx.weights = (float(w_depth), float(w_semantic))
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_depth, g_sem):
        d, s, dl, sl, denoms = ctx.saved_tensors
        BN, D, h, w = d.shape
        dev = d.device
        go = torch.stack((g_depth.reshape(()), g_sem.reshape(()))).float().contiguous()
        gd, gs = torch.empty_like(d), torch.empty_like(s)
        _lib.launch('ocrf_depth_semantic_loss_backward', dev, BN, h * w, D, dl, sl, d, s, *ctx.weights, denoms, go, gd, gs)
        return gd, gs, None, None, None, None


def depth_semantic_loss(depth_labels, depth_preds, semantic_labels, semantic_preds, w_depth, w_semantic):
    _lib.require_cuda(depth_labels, depth_preds, semantic_labels, semantic_preds)
    BN, D, h, w = depth_preds.shape
    R = BN * h * w
    if (semantic_preds.shape != (BN, 2, h, w) or tuple(depth_labels.shape) != (R, D)
            or tuple(semantic_labels.shape) != (R, 2)):
        raise ValueError(f'shapes do not match: depth {tuple(depth_preds.shape)}, semantic {tuple(semantic_preds.shape)}, '
                         f'depth labels {tuple(depth_labels.shape)}, semantic labels {tuple(semantic_labels.shape)}')
    return DepthSemanticLoss.apply(depth_preds.float(), semantic_preds.float(), depth_labels.detach().float(),
                                   semantic_labels.detach().float(), w_depth, w_semantic)


# --------------------------------------------------------------------------------------------- box mask
def box_bounds(boxes, W, H):
    """Box2dtoMask's slices of (n,4) boxes for an image of W x H: (y0, y1, x0, x1) long tensors after the float32
    scaling by W / 1600 (the y coordinates too), int() truncation, the -158 shift of y and Python's slice rules.
    NaN and anything below -9e18 count as -9e18, anything above 9e18 as 9e18 (``trunc_ll`` of csrc/losses.hip): the
    conversion of such a float to an integer differs between devices, and INT64_MIN - 158 would wrap to a large
    positive bound."""
    scale = torch.tensor(W / _ORIG_W, dtype=torch.float32, device=boxes.device)
    s = torch.nan_to_num(boxes.float() * scale, nan=-9e18, posinf=9e18, neginf=-9e18).clamp(-9e18, 9e18).trunc().long()

    def norm(v, L):
        v = torch.where(v < 0, v + L, v)
        return v.clamp(0, L)
    return norm(s[:, 1] - _Y_SHIFT, H), norm(s[:, 3] - _Y_SHIFT, H), norm(s[:, 0], W), norm(s[:, 2], W)


def box_mask(boxes, W, H, device=None):
    """(H, W) float mask of Box2dtoMask for (n,4) boxes, without a host loop: the union of the boxes' row and column
    ranges as a (H,n) x (n,W) product of indicators."""
    device = boxes.device if device is None else device
    boxes = boxes.to(device)
    y0, y1, x0, x1 = box_bounds(boxes.reshape(-1, 4), W, H)
    ys = torch.arange(H, device=device)[:, None]
    xs = torch.arange(W, device=device)[:, None]
    rows = ((ys >= y0) & (ys < y1)).float()                         # (H, n)
    cols = ((xs >= x0) & (xs < x1)).float()                         # (W, n)
    return ((rows @ cols.t()) > 0).float()


def pack_boxes(boxes_per_sample, cam_idx, device):
    """(B, n_max, 4) float boxes on ``device`` + int32 meta (counts | cameras) for the fused render losses.  Boxes on
    the host travel with the meta in ONE pinned non-blocking copy; boxes on the device are padded there."""
    B = len(boxes_per_sample)
    bx = [b.reshape(-1, 4) for b in boxes_per_sample]
    counts = [int(b.shape[0]) for b in bx]
    n_max = max(counts + [0])
    if n_max > _MAX_BOXES:
        raise ValueError(f'at most {_MAX_BOXES} boxes per sample, got {n_max}')
    cams = cam_idx if torch.is_tensor(cam_idx) else None
    on_host = all(not b.is_cuda for b in bx)
    nbox = B * n_max * 4
    host = torch.empty(nbox + 2 * B, dtype=torch.int32, pin_memory=True)
    host[nbox:nbox + B] = torch.tensor(counts, dtype=torch.int32)
    if cams is None:
        host[nbox + B:] = torch.tensor([int(c) for c in cam_idx], dtype=torch.int32)
    if on_host and n_max:
        hb = host[:nbox].view(torch.float32).view(B, n_max, 4)
        hb.zero_()
        for i, b in enumerate(bx):
            hb[i, :counts[i]] = b.float()
    dev = host.to(device, non_blocking=True)
    meta = dev[nbox:]
    if cams is not None:
        meta = torch.cat((meta[:B], cams.to(device=device, dtype=torch.int32).reshape(B)))
    if on_host:
        packed = dev[:nbox].view(torch.float32).view(B, n_max, 4)
    else:
        packed = torch.nn.utils.rnn.pad_sequence([b.to(device).float() for b in bx], batch_first=True) if n_max else \
            torch.empty(B, 0, 4, device=device)
    return packed.contiguous(), meta.contiguous(), n_max


# --------------------------------------------------------------------------------------------- SSIM
def gaussian_window(window_size, channel, sigma=1.5, device=None, dtype=torch.float32):
    """MVSGaussian's window: the float32 1-D Gaussian normalised in float32, its float32 outer product, per channel."""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)],
                     dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    w2 = g.mm(g.t()).float()
    return w2.expand(channel, 1, window_size, window_size).contiguous().to(device=device, dtype=dtype)


def ssim_torch(img1, img2, window_size=11, size_average=True, window=None):
    C = img1.shape[1]
    if window is None:
        window = gaussian_window(window_size, C, device=img1.device, dtype=img1.dtype)
    pad = window_size // 2

    def blur(x):
        return F.conv2d(x, window, padding=pad, groups=C)
    mu1, mu2 = blur(img1), blur(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = blur(img1 * img1) - mu1_sq
    s2 = blur(img2 * img2) - mu2_sq
    s12 = blur(img1 * img2) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m.mean() if size_average else m.mean(1).mean(1).mean(1)


def _fused_ssim_ok(img1, img2, window_size, size_average):
    return (window_size == 11 and size_average and img1.is_cuda and img2.is_cuda and img1.dim() == 4
            and img1.shape == img2.shape and not img1.requires_grad and img1.dtype == img2.dtype == torch.float32)


def ssim(img1, img2, window_size=11, size_average=True):
    """MVSGaussian's ``ssim(img1, img2)``: fused (``ocrf_render_losses``, one render, no mask / depth term) for window 11
    with ``size_average``; gradients flow to ``img2``.  Otherwise — or when ``img1`` requires grad — the torch
    formulation."""
    if _fused_ssim_ok(img1, img2, window_size, size_average):
        B, C, H, W = img1.shape
        _, s, _ = RenderLosses.apply(img1, img2, None, None, None, None, None, None, None, 0, 0, False, None,
                                     (0.0, 0.0), (0.0, 1.0, 0.0), (B, 1, C, H, W))
        return 1.0 - s
    return ssim_torch(img1, img2, window_size, size_average)


class SSIM(nn.Module):
    """MVSGaussian's ``SSIM(window_size=11, size_average=True)`` module (see ``ssim``)."""

    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        self.window_size, self.size_average = window_size, size_average
        self.channel, self.window = 1, None

    def forward(self, img1, img2):
        if _fused_ssim_ok(img1, img2, self.window_size, self.size_average):
            return ssim(img1, img2, self.window_size, self.size_average)
        C = img1.shape[1]
        if self.window is None or self.channel != C or self.window.device != img1.device \
                or self.window.dtype != img1.dtype:
            self.window = gaussian_window(self.window_size, C, device=img1.device, dtype=img1.dtype)
            self.channel = C
        return ssim_torch(img1, img2, self.window_size, self.size_average, self.window)


# --------------------------------------------------------------------------------------------- render losses
def render_losses_torch(gt_images, renders, render_depths, gt_depth, cam_idx_list, masks, depth_range):
    """Torch formulation of the per-sample loop of ``get_loss`` (:1370-1414) -> (color, ssim, depth) losses.
    ``renders`` / ``render_depths``: the three (B,3,H,W) / (B,1,H,W) tensors; ``masks``: per sample a (H,W) mask or
    None (before the iteration threshold); ``gt_depth`` (B,N,H,W) as given (range-zeroed here, on a copy)."""
    B = renders[0].shape[0]
    d0, d1 = float(depth_range[0]), float(depth_range[1])
    color, ssim_l, depth = [], [], []
    for b in range(B):
        m = masks[b]
        gt_b = gt_images[b:b + 1] if m is None else gt_images[b:b + 1] * m
        rs = [r[b:b + 1] if m is None else r[b:b + 1] * m for r in renders]
        color.append(sum(F.mse_loss(gt_b, r) for r in rs) / 3)
        ssim_l.append(sum(1 - ssim_torch(gt_b, r) for r in rs) / 3)
        g = gt_depth[b, int(cam_idx_list[b])].unsqueeze(0)
        g = g.masked_fill((g < d0) | (g > d1), 0.0)
        lo, hi = g.min(), g.max()
        den = (hi.double() - lo.double() + 0.01).float()
        target = (g - lo) / den
        depth.append(sum(F.l1_loss(rd[b], target) for rd in render_depths) / 3)
    return (torch.sum(torch.stack(color), dim=0) / B * 20, torch.sum(torch.stack(ssim_l), dim=0) / B * 1,
            torch.sum(torch.stack(depth) / B * 1))


class RenderLosses(torch.autograd.Function):
    """Masked MSE, 1 - SSIM and depth L1 of B samples x K renders by ``ocrf_render_losses`` / ``_backward``.
    Gradients for the renders and the render depths given as differentiable (the gt tensors are constants)."""

    @staticmethod
    def forward(ctx, gt, r0, r1, r2, rd0, rd1, rd2, boxes, meta, n_max, use_mask, has_depth, gt_depth, depth_range,
                weights, dims):
        B, K, C, H, W = dims
        dev = gt.device
        rs = [t.detach().contiguous() if t is not None else None for t in (r0, r1, r2)]
        rds = [t.detach().contiguous() if t is not None else None for t in (rd0, rd1, rd2)]
        gt = gt.detach().contiguous()
        gd = gt_depth.detach().contiguous() if has_depth else None
        out = torch.empty(3, device=dev)
        saved = torch.empty(B * C * K * 3 * H * W, device=dev)
        stats = torch.empty(2 * B, device=dev)
        ws = _lib.workspace.get(dev, _lib.lib().ocrf_render_losses_workspace_bytes(B, C, H, W), 'losses_render')
        n_cams = gd.shape[1] if has_depth else 0
        args = [B, K, C, H, W, gt, *rs, boxes, meta, n_max, int(use_mask), gd, n_cams, *rds,
                float(depth_range[0]), float(depth_range[1])] + [float(w) for w in weights]
        _lib.launch('ocrf_render_losses', dev, *args, out, saved, stats, ws, ws.numel())
        keep = [gt, boxes, meta, gd, saved, stats] + rs + rds
        ctx.save_for_backward(*[t if t is not None else torch.empty(0) for t in keep])
        ctx.present = [t is not None for t in keep]
        ctx.args = (B, K, C, H, W, n_max, int(use_mask), n_cams, depth_range, weights)
        ctx.need = [ctx.needs_input_grad[i] for i in range(1, 7)]
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_color, g_ssim, g_depth):
        saved_t = [t if p else None for t, p in zip(ctx.saved_tensors, ctx.present)]
        gt, boxes, meta, gd, saved, stats = saved_t[:6]
        rs, rds = saved_t[6:9], saved_t[9:12]
        B, K, C, H, W, n_max, use_mask, n_cams, depth_range, weights = ctx.args
        dev = gt.device
        go = torch.stack((g_color.reshape(()), g_ssim.reshape(()), g_depth.reshape(()))).float().contiguous()
        grads = [torch.empty_like(r) if (r is not None and need) else None for r, need in zip(rs, ctx.need[:3])]
        dgrads = [torch.empty_like(r) if (r is not None and need and gd is not None) else None
                  for r, need in zip(rds, ctx.need[3:])]
        args = [B, K, C, H, W, gt, *rs, boxes, meta, n_max, use_mask, gd, n_cams, *rds,
                float(depth_range[0]), float(depth_range[1])] + [float(w) for w in weights]
        _lib.launch('ocrf_render_losses_backward', dev, *args, saved, stats, go, *grads, *dgrads)
        return (None, *grads, *dgrads) + (None,) * 9


def render_losses(gt_images, renders, render_depths, gt_depth, cam_idx_list, boxes_per_sample, use_mask, depth_range):
    """Fused ``render_losses_torch``: ``boxes_per_sample`` the (n_b,4) boxes of each sample's camera.  Every render depth
    that requires grad gets a gradient; the second (``render_depth_G_all``) requires one only when the rasteriser rendered
    it differentiable (``depth_mode='mean', depth_grad=True``: ``OcRFViewTransformerFull.render_depth_grad``)."""
    r0, r1, r2 = renders
    _lib.require_cuda(gt_images, r0, r1, r2, *render_depths, gt_depth)
    B, C, H, W = r0.shape
    for r in (r1, r2):
        if r.shape != r0.shape:
            raise ValueError(f'renders must share one shape, got {tuple(r0.shape)} and {tuple(r.shape)}')
    for rd in render_depths:
        if rd.numel() != B * H * W or rd.shape[0] != B:
            raise ValueError(f'render depths must be {(B, 1, H, W)}, got {tuple(rd.shape)}')
    rd0, rd1, rd2 = (rd.reshape(B, 1, H, W) for rd in render_depths)
    if gt_images.dim() != 4 or gt_images.shape[0] < B or tuple(gt_images.shape[1:]) != (C, H, W):
        raise ValueError(f'gt_images must be (>= {B}, {C}, {H}, {W}), got {tuple(gt_images.shape)}')
    if gt_depth.dim() != 4 or gt_depth.shape[0] < B or tuple(gt_depth.shape[2:]) != (H, W):
        raise ValueError(f'gt_depth must be ({B}, N, {H}, {W}), got {tuple(gt_depth.shape)}')
    if len(boxes_per_sample) != B or len(cam_idx_list) != B:
        raise ValueError(f'need one box set and one camera per sample ({B})')
    if not torch.is_tensor(cam_idx_list) and any(not 0 <= int(c) < gt_depth.shape[1] for c in cam_idx_list):
        raise ValueError(f'camera indices {list(cam_idx_list)} outside [0, {gt_depth.shape[1]})')
    dev = r0.device
    boxes, meta, n_max = pack_boxes(boxes_per_sample, cam_idx_list, dev)
    f = lambda t: t.float()                    # noqa: E731
    return RenderLosses.apply(f(gt_images), f(r0), f(r1), f(r2), f(rd0), f(rd1), f(rd2), boxes, meta,
                              n_max, bool(use_mask), True, f(gt_depth), tuple(float(v) for v in depth_range[:2]),
                              (20.0, 1.0, 1.0), (B, 3, C, H, W))
