"""Test-time decode and NMS of the detection head: the reference's ``CenterHead.get_bboxes`` / ``get_task_detections``
(mmdet3d/models/dense_heads/centerpoint_head.py), ``CenterPointBBoxCoder`` (core/bbox/coders/centerpoint_bbox_coders.py),
``circle_nms`` and ``nms_bev`` (core/post_processing/box3d_nms.py) with mmcv's ``nms_rotated``, built without mmcv,
mmdet or numba.

Two formulations of the same arithmetic, both writing padded per-sample results -- boxes (B, M, 9 | 7) with
bottom-centre z, scores (B, M), int32 labels (B, M) with the task's class offset, int32 counts (B,), M = T *
post_max_size:

* the fused one -- ``csrc/center_decode.hip`` (``ocrf_center_decode``): four launches for every sample and task, no
  memset, no atomics on results, nothing read back to the host;
* the torch one (``decode_torch``) -- the CPU path, and the fallback for inputs that are not float32 CUDA tensors or
  ``head.fused_decode = False``.  Vectorised over samples, tasks and boxes; its greedy scan loops over candidate rank
  for every (sample, task) at once and reads nothing back.

bfloat16 head outputs (bf16 autocast) are cast to float32 first (``bf16_as_float32``), so they decode in float32 on
either path; float16 ones take the torch formulation as they are.  Opt-in (``CenterHead.fused_decode_bf16``) head
outputs that are ALL CUDA bfloat16 skip the casts: ``ocrf_center_decode_bf16`` reads them in place, widens each load
exactly and returns the bits the float32 call returns on ``.float()`` of the same heads.

Rules both keep:

* ties: equal scores go in ascending (class, cell) order and every later sort is stable;
* the top K of a task's ncls * H * W sigmoid scores is the reference's two-stage top K (per class, then over the
  ncls * K survivors);
* box arithmetic in float32, one operation at a time in the reference's order; the NMS box is the decoded one with
  dims 3:6 times ``nms_rescale_factor``, through ``xywhr2xyxyr`` and back; the output dims are fl(fl(d * f) / f);
* rotated IoU (mmcv 1.4.8-1.6.0 ``box_iou_rotated_utils.hpp``): intersection over area1 + area2 - inter, 0 when an
  area is below 1e-14, centres shifted to their mean; here in float64, the intersection by polygon clipping.  The
  corners are c + R(a) (+-w/2, +-h/2) with R counter-clockwise in x-right / y-up coordinates (``box_corners``, and
  ``box_corners`` in the HIP source); that sense is not verified against mmcv;
* circle NMS suppresses at squared centre distance <= min_radius (the radius as written, a reference quirk), the
  distance in float32 and the comparison in float64, as the reference's numba loop.
"""
import ctypes

import numpy as np
import torch

from . import _lib

__all__ = ['CenterPointBBoxCoder', 'DecodeConfig', 'box_corners', 'box_iou_rotated_bev', 'iou_rotated_pairs',
           'nms_bev', 'circle_nms', 'xywhr2xyxyr', 'decode_torch', 'decode_fused', 'MAX_CLASSES']

MAX_TASKS = _lib.OCRF_CD_MAX_TASKS
MAX_CLASSES = _lib.OCRF_CD_MAX_CLASSES
MAX_NUM = _lib.OCRF_CD_MAX_NUM
HEAD_KEYS = ('heatmap', 'reg', 'height', 'dim', 'rot', 'vel')
_POLY_CAP = 12


class CenterPointBBoxCoder:
    """The reference's ``CenterPointBBoxCoder``: same constructor, attributes and ``decode`` return value (a list over
    samples of dicts ``bboxes`` (n, 9 | 7), ``scores`` (n,), float ``labels`` (n,)), by the torch formulation."""

    def __init__(self, pc_range, out_size_factor, voxel_size, post_center_range=None, max_num=100,
                 score_threshold=None, code_size=9):
        self.pc_range = pc_range
        self.out_size_factor = out_size_factor
        self.voxel_size = voxel_size
        self.post_center_range = post_center_range
        self.max_num = max_num
        self.score_threshold = score_threshold
        self.code_size = code_size

    def encode(self):
        pass

    def decode(self, heat, rot_sine, rot_cosine, hei, dim, vel, reg=None, task_id=-1):
        """``heat`` is the sigmoid heatmap (B, ncls, H, W) and ``dim`` already exponentiated, as the reference's."""
        if self.post_center_range is None:
            raise NotImplementedError('Need to reorganize output as a batch, only support post_center_range is not '
                                      'None for now!')
        rows, scores, cls, ok = _decode_rows(self, heat, reg, hei, dim, rot_sine, rot_cosine, vel)
        return [dict(bboxes=rows[i][ok[i]], scores=scores[i][ok[i]], labels=cls[i][ok[i]].float())
                for i in range(rows.shape[0])]


def _topk(heat, K):
    """(scores, flat index c * HW + cell) of the top K of (B, ncls, H, W): descending, ties in ascending index."""
    B = heat.shape[0]
    flat = heat.reshape(B, -1)
    if K > heat.shape[2] * heat.shape[3]:
        raise ValueError(f'max_num {K} exceeds the map size {heat.shape[2]} x {heat.shape[3]}')
    s, i = torch.sort(flat, dim=1, descending=True, stable=True)
    return s[:, :K].contiguous(), i[:, :K].contiguous()


def _gather(x, cell):
    """(B, C, H, W) gathered at cell (B, K) -> (B, K, C)."""
    B, C = x.shape[:2]
    return x.reshape(B, C, -1).gather(2, cell[:, None, :].expand(B, C, cell.shape[1])).transpose(1, 2)


def _decode_rows(coder, heat, reg, hei, dim, rot_sine, rot_cosine, vel):
    """The coder's decode before its boolean indexing: rows (B, K, 9 | 7), scores (B, K), class (B, K) int64 and the
    coder's keep mask (B, K)."""
    K = int(coder.max_num)
    H, W = heat.shape[2:]
    scores, idx = _topk(heat, K)
    cls = idx // (H * W)
    cell = idx % (H * W)
    xs = (cell % W).to(heat.dtype)
    ys = (cell // W).to(heat.dtype)
    if reg is not None:
        r = _gather(reg, cell)
        xs = xs + r[..., 0]
        ys = ys + r[..., 1]
    else:
        xs = xs + 0.5
        ys = ys + 0.5
    rot = torch.atan2(_gather(rot_sine, cell)[..., 0], _gather(rot_cosine, cell)[..., 0])
    osf = coder.out_size_factor
    xs = xs * osf * coder.voxel_size[0] + coder.pc_range[0]
    ys = ys * osf * coder.voxel_size[1] + coder.pc_range[1]
    cols = [xs[..., None], ys[..., None], _gather(hei, cell), _gather(dim, cell), rot[..., None]]
    if vel is not None:
        cols.append(_gather(vel, cell))
    rows = torch.cat(cols, 2)
    ok = torch.ones_like(scores, dtype=torch.bool)
    if coder.score_threshold:
        ok = ok & (scores > coder.score_threshold)
    if coder.post_center_range is not None:
        rng = _const(list(coder.post_center_range), rows.dtype, rows.device)
        ok = ok & (rows[..., :3] >= rng[:3]).all(-1) & (rows[..., :3] <= rng[3:]).all(-1)
    return rows, scores, cls, ok


def _const(values, dtype, dev):
    """A small constant tensor on ``dev`` without a host synchronisation (pinned, non-blocking)."""
    t = torch.as_tensor(values, dtype=dtype)
    return t.pin_memory().to(dev, non_blocking=True) if dev.type == 'cuda' else t


# --------------------------------------------------------------------------------------------- geometry
def xywhr2xyxyr(boxes_xywhr):
    """mmdet3d's xywhr2xyxyr."""
    boxes = torch.zeros_like(boxes_xywhr)
    half_w = boxes_xywhr[..., 2] / 2
    half_h = boxes_xywhr[..., 3] / 2
    boxes[..., 0] = boxes_xywhr[..., 0] - half_w
    boxes[..., 1] = boxes_xywhr[..., 1] - half_h
    boxes[..., 2] = boxes_xywhr[..., 0] + half_w
    boxes[..., 3] = boxes_xywhr[..., 1] + half_h
    boxes[..., 4] = boxes_xywhr[..., 4]
    return boxes


def _xyxyr2xywhr(b):
    """nms_bev's way back."""
    return torch.stack(((b[..., 0] + b[..., 2]) / 2, (b[..., 1] + b[..., 3]) / 2, b[..., 2] - b[..., 0],
                        b[..., 3] - b[..., 1], b[..., 4]), dim=-1)


def box_corners(cx, cy, w, h, a):
    """The one torch place that fixes the rotation sense (mirrors ``box_corners`` in csrc/center_decode.hip): corners
    c + R(a) (+-w/2, +-h/2), R counter-clockwise in x-right / y-up coordinates, listed counter-clockwise.  Float64
    tensors of one shape -> (..., 4, 2)."""
    c, s = torch.cos(a), torch.sin(a)
    lx = torch.stack([-0.5 * w, 0.5 * w, 0.5 * w, -0.5 * w], -1)
    ly = torch.stack([-0.5 * h, -0.5 * h, 0.5 * h, 0.5 * h], -1)
    px = cx[..., None] + (c[..., None] * lx - s[..., None] * ly)
    py = cy[..., None] + (s[..., None] * lx + c[..., None] * ly)
    return torch.stack([px, py], -1)


def iou_rotated_pairs(a, b):
    """Rotated IoU of box pairs a[k], b[k] ((..., 5) xywhr, float32 values) in float64 -> (...): Sutherland-Hodgman
    clipping of a by the edges of b, the operations of ``iou_rotated`` in csrc/center_decode.hip."""
    shape = a.shape[:-1]
    a = a.reshape(-1, 5).double()
    b = b.reshape(-1, 5).double()
    N = a.shape[0]
    area_a, area_b = a[:, 2] * a[:, 3], b[:, 2] * b[:, 3]
    sx, sy = 0.5 * (a[:, 0] + b[:, 0]), 0.5 * (a[:, 1] + b[:, 1])
    pa = box_corners(a[:, 0] - sx, a[:, 1] - sy, a[:, 2], a[:, 3], a[:, 4])
    pb = box_corners(b[:, 0] - sx, b[:, 1] - sy, b[:, 2], b[:, 3], b[:, 4])
    dev = a.device
    P = torch.zeros(N, _POLY_CAP, 2, dtype=torch.float64, device=dev)
    P[:, :4] = pa
    n = torch.full((N,), 4, dtype=torch.int64, device=dev)
    k = torch.arange(_POLY_CAP, device=dev)
    for e in range(4):
        o, ed = pb[:, e], pb[:, (e + 1) % 4] - pb[:, e]
        dc = ed[:, None, 0] * (P[..., 1] - o[:, None, 1]) - ed[:, None, 1] * (P[..., 0] - o[:, None, 0])
        valid = k[None] < n[:, None]
        prev_i = torch.where(k[None] == 0, n[:, None] - 1, k[None] - 1).clamp(min=0)
        prev = P.gather(1, prev_i[..., None].expand(N, _POLY_CAP, 2))
        dp = dc.gather(1, prev_i)
        cin, pin = dc >= 0, dp >= 0
        e_int = valid & (cin != pin)
        e_cur = valid & cin
        t = torch.where(e_int, dp / torch.where(e_int, dp - dc, torch.ones_like(dc)), torch.zeros_like(dc))
        ip = prev + t[..., None] * (P - prev)
        cnt = e_int.long() + e_cur.long()
        pos = torch.cumsum(cnt, 1) - cnt
        out = torch.zeros(N, _POLY_CAP + 1, 2, dtype=torch.float64, device=dev)
        dump = torch.full_like(pos, _POLY_CAP)
        i_int = torch.where(e_int & (pos < _POLY_CAP), pos, dump)
        i_cur = torch.where(e_cur & (pos + e_int.long() < _POLY_CAP), pos + e_int.long(), dump)
        out.scatter_(1, i_int[..., None].expand(N, _POLY_CAP, 2), ip)
        out.scatter_(1, i_cur[..., None].expand(N, _POLY_CAP, 2), P)
        P = out[:, :_POLY_CAP]
        n = cnt.sum(1).clamp(max=_POLY_CAP)
    nxt = torch.where(k[None] + 1 >= n[:, None], torch.zeros_like(k[None]), k[None] + 1).expand(N, _POLY_CAP)
    Q = P.gather(1, nxt[..., None].expand(N, _POLY_CAP, 2))
    cross = (P[..., 0] * Q[..., 1] - Q[..., 0] * P[..., 1]) * (k[None] < n[:, None])
    inter = torch.where(n >= 3, (0.5 * cross.sum(1)).abs(), torch.zeros_like(area_a))
    iou = inter / (area_a + area_b - inter)
    iou = torch.where((area_a < 1e-14) | (area_b < 1e-14), torch.zeros_like(iou), iou)
    return iou.reshape(shape)


def box_iou_rotated_bev(a, b):
    """(N, 5) x (M, 5) xywhr boxes -> (N, M) float64 rotated IoU (mmcv's box_iou_rotated arithmetic in float64)."""
    N, M = a.shape[0], b.shape[0]
    return iou_rotated_pairs(a[:, None, :].expand(N, M, 5), b[None, :, :].expand(N, M, 5))


def _greedy(sup, n, post_max):
    """Greedy NMS over a suppression matrix for every leading index at once: sup (..., P, P) bool (j > i only
    matters), n (...) candidate counts -> keep (..., P) bool, at most post_max per row.  Loops over rank."""
    P = sup.shape[-1]
    rank = torch.arange(P, device=sup.device)
    alive = rank < n[..., None]
    removed = torch.zeros_like(alive)
    keep = torch.zeros_like(alive)
    kept = torch.zeros_like(n)
    for i in range(P):
        k = alive[..., i] & ~removed[..., i] & (kept < post_max)
        keep[..., i] = k
        kept = kept + k.long()
        removed = removed | (k[..., None] & sup[..., i, :])
    return keep


def _pair_chunks(a, b, fn, rows=64):
    """fn over (..., P, P) pairs of a[..., i] and b[..., j], in row chunks to bound the memory."""
    P = a.shape[-2]
    outs = []
    for i0 in range(0, P, rows):
        ai = a[..., i0:i0 + rows, None, :]
        outs.append(fn(ai.expand(*ai.shape[:-3], ai.shape[-3], P, a.shape[-1]),
                       b[..., None, :, :].expand(*b.shape[:-2], ai.shape[-3], P, b.shape[-1])))
    return torch.cat(outs, -2)


def nms_bev(boxes, scores, thresh, pre_max_size=None, post_max_size=None):
    """The reference's nms_bev: (N, 5) xyxyr boxes, (N,) scores -> kept indices (int64), best first."""
    assert boxes.size(1) == 5, 'Input boxes shape should be [N, 5]'
    order = scores.sort(dim=0, descending=True, stable=True)[1]
    if pre_max_size is not None:
        order = order[:pre_max_size]
    b = _xyxyr2xywhr(boxes[order].contiguous())
    n = b.shape[0]
    sup = box_iou_rotated_bev(b, b) > thresh if n else torch.zeros(0, 0, dtype=torch.bool, device=b.device)
    keep = _greedy(sup, torch.tensor(n, device=b.device), n)
    keep = order[keep]
    if post_max_size is not None:
        keep = keep[:post_max_size]
    return keep


def circle_nms(dets, thresh, post_max_size=83):
    """The reference's circle_nms: (N, 3) [x, y, score] (numpy or tensor) -> list of kept indices, best first."""
    d = torch.as_tensor(np.asarray(dets) if not torch.is_tensor(dets) else dets)
    order = torch.sort(d[:, 2], descending=True, stable=True)[1]
    x, y = d[order, 0], d[order, 1]
    dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
    sup = (dx * dx + dy * dy).double() <= thresh
    n = d.shape[0]
    keep = _greedy(sup, torch.tensor(n), n)
    out = order[keep].tolist()
    return out[:post_max_size] if post_max_size < len(out) else out


# --------------------------------------------------------------------------------------------- config
class DecodeConfig:
    """What decoding reads from the coder and ``test_cfg``, per task where the reference allows a list."""

    def __init__(self, coder, test_cfg, ncls):
        T = len(ncls)
        if T > MAX_TASKS or max(ncls) > MAX_CLASSES:
            raise ValueError(f'at most {MAX_TASKS} tasks of {MAX_CLASSES} classes, got {ncls}')
        self.ncls = list(ncls)
        self.K = int(coder.max_num)
        if not 0 < self.K <= MAX_NUM:
            raise ValueError(f'max_num must be in [1, {MAX_NUM}], got {self.K}')
        self.coder = coder
        nms_type = test_cfg.get('nms_type')
        self.circle = [(nms_type[t] if isinstance(nms_type, list) else nms_type) == 'circle' for t in range(T)]
        thr = test_cfg.get('nms_thr')
        self.thr = []
        for t in range(T):
            if self.circle[t]:
                self.thr.append(float(test_cfg['min_radius'][t]))
            else:
                self.thr.append(float(thr[t] if isinstance(thr, list) else thr))
        factors = test_cfg.get('nms_rescale_factor', [1.0] * T)
        self.factor = np.ones((T, MAX_CLASSES), np.float32)
        for t in range(T):
            f = factors[t]
            if isinstance(f, list):
                for c, v in enumerate(f[:MAX_CLASSES]):
                    self.factor[t, c] = v
            else:
                self.factor[t, :] = f
        st = test_cfg['score_threshold']
        self.score_thr = float(st) if st > 0.0 else None
        pre, post = test_cfg.get('pre_max_size'), test_cfg.get('post_max_size')
        self.pre_max = self.K if pre is None else min(int(pre), self.K)
        self.post_max = self.K if post is None else int(post)
        lim = test_cfg.get('post_center_limit_range')
        self.limit = list(lim) if lim is not None and len(lim) > 0 else None
        self.coder_thr = float(coder.score_threshold) if coder.score_threshold else None
        self.center = list(coder.post_center_range) if coder.post_center_range is not None else None
        self.offsets = [sum(ncls[:t]) for t in range(T)]


# --------------------------------------------------------------------------------------------- torch formulation
def _task_inputs(pd, norm_bbox):
    heat = pd['heatmap'].sigmoid()
    dim = torch.exp(pd['dim']) if norm_bbox else pd['dim']
    return heat, pd['reg'], pd['height'], dim, pd['rot'][:, 0:1], pd['rot'][:, 1:2], pd.get('vel')


def decode_torch(preds_dicts, cfg, norm_bbox=True):
    """The torch formulation of get_bboxes -> padded (boxes, scores, labels int32, counts int32)."""
    T = len(preds_dicts)
    K, post = cfg.K, cfg.post_max
    rows_t, bev_t, score_t, label_t, n_t = [], [], [], [], []
    for t, p in enumerate(preds_dicts):
        heat, reg, hei, dim, rs, rc, vel = _task_inputs(p[0], norm_bbox)
        rows, scores, cls, ok = _decode_rows(cfg.coder, heat, reg, hei, dim, rs, rc, vel)
        B, C, dev = rows.shape[0], rows.shape[2], rows.device
        if cfg.circle[t]:
            cut = K
            bev = torch.cat([rows[..., :2], torch.zeros_like(rows[..., :3])], -1)
        else:
            cut = cfg.pre_max
            if cfg.score_thr is not None:
                ok = ok & (scores >= cfg.score_thr)
            f = _const(cfg.factor[t], torch.float32, dev)[cls.clamp(max=MAX_CLASSES - 1)]
            ds = rows[..., 3:6] * f[..., None]
            bev = _xyxyr2xywhr(xywhr2xyxyr(torch.stack([rows[..., 0], rows[..., 1], ds[..., 0], ds[..., 1],
                                                        rows[..., 6]], -1)))
            rows = torch.cat([rows[..., :3], ds / f[..., None], rows[..., 6:]], -1)
        pos = torch.cumsum(ok.long(), 1) - 1
        dest = torch.where(ok & (pos < cut), pos, torch.full_like(pos, K))
        n_t.append(torch.clamp(ok.long().sum(1), max=cut))

        def compact(x, fill=0):
            out = torch.full((B, K + 1) + tuple(x.shape[2:]), fill, dtype=x.dtype, device=dev)
            out.scatter_(1, dest.view(B, K, *([1] * (x.dim() - 2))).expand(x.shape), x)
            return out[:, :K]
        rows_t.append(compact(rows))
        bev_t.append(compact(bev))
        score_t.append(compact(scores))
        label_t.append(compact(cls + cfg.offsets[t]))
    rows, bev = torch.stack(rows_t, 1), torch.stack(bev_t, 1)           # (B, T, K, C), (B, T, K, 5)
    scores, labels, n = torch.stack(score_t, 1), torch.stack(label_t, 1), torch.stack(n_t, 1)
    B, C, dev = rows.shape[0], rows.shape[3], rows.device
    circle = _const(cfg.circle, torch.bool, dev)
    thr = _const(cfg.thr, torch.float64, dev)

    def suppress(a, b):
        dx, dy = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1]
        near = (dx * dx + dy * dy).double() <= thr[:, None, None]
        over = iou_rotated_pairs(a, b) > thr[:, None, None]
        return torch.where(circle[:, None, None], near, over)
    sup = _pair_chunks(bev, bev, suppress) if K else torch.zeros(B, T, 0, 0, dtype=torch.bool, device=dev)
    keep = _greedy(sup, n, post)
    if cfg.limit is not None:
        lim = _const(cfg.limit, rows.dtype, dev)
        inside = (rows[..., :3] >= lim[:3]).all(-1) & (rows[..., :3] <= lim[3:]).all(-1)
        keep = keep & (inside | circle[:, None])
    M = T * post
    flat = keep.reshape(B, T * K)
    pos = torch.cumsum(flat.long(), 1) - 1
    dest = torch.where(flat, pos, torch.full_like(pos, M))
    rows = rows.reshape(B, T * K, C)
    rows = torch.cat([rows[..., :2], (rows[..., 2] - rows[..., 5] * 0.5)[..., None], rows[..., 3:]], -1)
    out_b = torch.zeros(B, M + 1, C, dtype=rows.dtype, device=dev).scatter_(1, dest[..., None].expand(B, T * K, C), rows)
    out_s = torch.zeros(B, M + 1, dtype=scores.dtype, device=dev).scatter_(1, dest, scores.reshape(B, T * K))
    out_l = torch.zeros(B, M + 1, dtype=torch.int64, device=dev).scatter_(1, dest, labels.reshape(B, T * K))
    return out_b[:, :M], out_s[:, :M], out_l[:, :M].int(), flat.sum(1).int()


# --------------------------------------------------------------------------------------------- fused
def bf16_as_float32(preds_dicts):
    """``preds_dicts`` with every bfloat16 head output (a head that ran under bf16 autocast) cast to float32, in new
    dicts; the same object when there is none.  float16 outputs stay as they are."""
    if not any(v.dtype == torch.bfloat16 for p in preds_dicts for k, v in p[0].items() if k in HEAD_KEYS):
        return preds_dicts
    return [[{k: v.float() if k in HEAD_KEYS and v.dtype == torch.bfloat16 else v for k, v in p[0].items()}]
            for p in preds_dicts]


def fused_ok(preds_dicts, dtype=torch.float32):
    """The kernel takes these heads: all on the GPU and all of ``dtype`` (float32, or bfloat16 for the ``_bf16`` entry
    point; a mixed list is refused), every task with a ``reg`` head."""
    ts = [v for p in preds_dicts for k, v in p[0].items() if k in HEAD_KEYS]
    return all(t.is_cuda and t.dtype == dtype for t in ts) and all('reg' in p[0] for p in preds_dicts)


_ENTRY = {torch.float32: 'ocrf_center_decode', torch.bfloat16: 'ocrf_center_decode_bf16'}


def decode_fused(preds_dicts, cfg, norm_bbox=True):
    """``decode_torch`` by ``ocrf_center_decode``, or by ``ocrf_center_decode_bf16`` when every head is bfloat16 (read in
    place; the float32 results are bit-equal to those on ``.float()`` of the heads).  A list of mixed dtypes is
    refused."""
    T = len(preds_dicts)
    p0 = preds_dicts[0][0]
    B, _, H, W = p0['heatmap'].shape
    if cfg.K > H * W:
        raise ValueError(f'max_num {cfg.K} exceeds the map size {H} x {W}')
    dev = p0['heatmap'].device
    with_vel = 'vel' in p0
    keys = HEAD_KEYS if with_vel else HEAD_KEYS[:5]
    heads = []
    for t, p in enumerate(preds_dicts):
        d = p[0]
        if tuple(d['heatmap'].shape) != (B, cfg.ncls[t], H, W):
            raise ValueError(f'task {t}: heatmap must be ({B}, {cfg.ncls[t]}, {H}, {W}), got {tuple(d["heatmap"].shape)}')
        for k, c in zip(keys[1:], (2, 1, 3, 2, 2)):
            if tuple(d[k].shape) != (B, c, H, W):
                raise ValueError(f'task {t}: {k} must be ({B}, {c}, {H}, {W}), got {tuple(d[k].shape)}')
        heads.append([d[k].detach().contiguous() for k in keys] + ([] if with_vel else [None]))
    flat = [h for hs in heads for h in hs]
    dtype = p0['heatmap'].dtype
    if dtype not in _ENTRY or any(h is not None and h.dtype != dtype for h in flat):
        raise _lib.OcrfHipError('decode_fused takes head outputs that are all float32 or all bfloat16, got '
                                f'{sorted({str(h.dtype) for h in flat if h is not None})}')
    C = 9 if with_vel else 7
    M = T * cfg.post_max
    boxes = torch.empty(B, M, C, dtype=torch.float32, device=dev)
    scores = torch.empty(B, M, dtype=torch.float32, device=dev)
    labels = torch.empty(B, M, dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    ws = _lib.workspace.get(dev, _lib.lib().ocrf_center_decode_workspace_bytes(B, T, cfg.K, cfg.post_max), 'center_decode')
    coder = cfg.coder
    f2 = lambda v: (ctypes.c_float * len(v))(*[float(x) for x in v])  # noqa: E731
    ptrs = (ctypes.c_void_p * len(flat))(*[t.data_ptr() if t is not None else 0 for t in flat])
    _lib.launch(_ENTRY[dtype], dev,
                B, T, (ctypes.c_int * T)(*cfg.ncls), H, W, ptrs, int(with_vel), int(norm_bbox), cfg.K, cfg.pre_max,
                cfg.post_max, float(coder.out_size_factor), f2(coder.voxel_size[:2]), f2(coder.pc_range[:2]),
                int(cfg.coder_thr is not None), cfg.coder_thr or 0.0, f2(cfg.center) if cfg.center else None,
                int(cfg.score_thr is not None), cfg.score_thr or 0.0, f2(cfg.limit) if cfg.limit else None,
                (ctypes.c_int * T)(*[int(c) for c in cfg.circle]), (ctypes.c_double * T)(*cfg.thr),
                cfg.factor.ctypes.data_as(ctypes.c_void_p), boxes, scores, labels, counts, ws, ws.numel())
    return boxes, scores, labels, counts


def read_counts(counts):
    """The B counts on the host: one copy through pinned memory for CUDA tensors."""
    if not counts.is_cuda:
        return counts.tolist()
    host = torch.empty(counts.shape, dtype=counts.dtype, pin_memory=True)
    host.copy_(counts, non_blocking=True)
    torch.cuda.current_stream(counts.device).synchronize()
    return host.tolist()

