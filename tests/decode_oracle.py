"""A plain float64 oracle of ``CenterHead.get_bboxes`` (padded outputs) and the decode test cases built on it.

``decode(preds, ncls, coder, test_cfg, norm_bbox)`` restates the rules of ``ocrfdet_amd/center_decode.py`` and INTEGRATION
3d in NumPy, one (sample, task) at a time, without sharing code with either formulation:

* the key of a cell is its sigmoid in float64, rounded once to float32 (a float32 sigmoid is within ``SCORE_ULPS`` of
  it); the top K over ncls * H * W by (key descending, flat index ascending);
* box arithmetic in float32, one ``np.float32`` step at a time in the reference's order;
* the coder's ``score > threshold`` and centre range, the test cfg's ``score >= threshold`` (rotate tasks), the per-class
  ``nms_rescale_factor`` with the ``xywhr2xyxyr`` round trip, ``pre_max_size`` (rotate tasks; circle tasks cut at K);
* greedy NMS: rotated IoU > nms_thr in float64 by mmcv's construction (corners of each box inside the other plus every
  edge-edge intersection, deduplicated, sorted by angle around their centroid, shoelace area; 0 below an area of 1e-14;
  centres shifted to their mean), or circle NMS at float32 squared distance <= min_radius compared in float64; only the
  pairs the greedy scan decides on are computed, and pairs whose enclosing circles are disjoint are 0;
* ``post_max_size``, the limit range on rotate tasks, z - dz / 2, the class offsets, rows past the count zero.

Corners follow the project's convention: c + R(a) (+-w/2, +-h/2), R counter-clockwise.

``build(name)`` makes one named case of ``CASES``: the head outputs, the coder and test cfg, and the oracle's result.  It
redraws (a new seed) while a decided IoU lies within 1e-6 of its threshold or a circle distance within 1e-6 relative of
its radius, and asserts that the case reaches what its name claims (mask-row spill, ties across the K boundary, more
than one mask word, ...).
"""
import numpy as np

f32 = np.float32
MARGIN = 1e-6
# A float32 sigmoid fl(1 / fl(1 + fl(exp(-x)))) is not correctly rounded: one ulp of exp moves fl(1 + e) by a rounding
# step of 2^-23, two ulp of a score in [0.5, 1).  Scores are compared within SCORE_ULPS, and keys the order or a
# threshold depends on are kept KEY_GAP_ULPS apart unless they are equal by construction.
SCORE_ULPS = 2
KEY_GAP_ULPS = 8
SCAN_LDS_BYTES = 64 * 1024


def lds_rows(K, n):
    """Mask rows the greedy scan keeps in LDS (the rest it reads from global memory): the kernel's formula."""
    nw = (K + 63) // 64
    return min(n, SCAN_LDS_BYTES // (8 * nw))


def sigmoid_key(x):
    x = np.asarray(x, np.float64)
    return (1.0 / (1.0 + np.exp(-x))).astype(f32)


# --------------------------------------------------------------------------------------------- rotated IoU
def corners(cx, cy, w, h, a):
    """(m,) float64 arrays -> (m, 4, 2), counter-clockwise."""
    c, s = np.cos(a), np.sin(a)
    lx = np.stack([-0.5 * w, 0.5 * w, 0.5 * w, -0.5 * w], -1)
    ly = np.stack([-0.5 * h, -0.5 * h, 0.5 * h, 0.5 * h], -1)
    return np.stack([cx[:, None] + c[:, None] * lx - s[:, None] * ly,
                     cy[:, None] + s[:, None] * lx + c[:, None] * ly], -1)


def _inside(p, q):
    """Points p (m, k, 2) in rectangles q (m, 4, 2), edges included (a relative tolerance of 1e-12)."""
    ab, ad = q[:, 1] - q[:, 0], q[:, 3] - q[:, 0]
    ap = p - q[:, None, 0]
    u, uu = (ap * ab[:, None]).sum(-1), (ab * ab).sum(-1)[:, None]
    v, vv = (ap * ad[:, None]).sum(-1), (ad * ad).sum(-1)[:, None]
    eu, ev = 1e-12 * uu, 1e-12 * vv
    return (u >= -eu) & (u <= uu + eu) & (v >= -ev) & (v <= vv + ev)


def iou_one_to_many(a, bs):
    """Rotated IoU of box a (5,) with boxes bs (m, 5), xywhr, in float64 by mmcv's construction."""
    a = np.asarray(a, np.float64)
    bs = np.asarray(bs, np.float64).reshape(-1, 5)
    m = bs.shape[0]
    if m == 0:
        return np.zeros(0)
    area_a, area_b = a[2] * a[3], bs[:, 2] * bs[:, 3]
    sx, sy = 0.5 * (a[0] + bs[:, 0]), 0.5 * (a[1] + bs[:, 1])
    pa = corners(a[0] - sx, a[1] - sy, np.full(m, a[2]), np.full(m, a[3]), np.full(m, a[4]))
    pb = corners(bs[:, 0] - sx, bs[:, 1] - sy, bs[:, 2], bs[:, 3], bs[:, 4])
    pts = [pa, pb]
    ok = [_inside(pa, pb), _inside(pb, pa)]
    # edge k of a against edge l of b: p + t r = q + u s
    p, r = pa, np.roll(pa, -1, 1) - pa
    q, s = pb, np.roll(pb, -1, 1) - pb
    p, r = p[:, :, None], r[:, :, None]
    q, s = q[:, None], s[:, None]
    den = r[..., 0] * s[..., 1] - r[..., 1] * s[..., 0]
    qp = q - p
    par = np.abs(den) <= 1e-14 * np.sqrt((r * r).sum(-1) * (s * s).sum(-1))
    safe = np.where(par, 1.0, den)
    t = (qp[..., 0] * s[..., 1] - qp[..., 1] * s[..., 0]) / safe
    u = (qp[..., 0] * r[..., 1] - qp[..., 1] * r[..., 0]) / safe
    e = 1e-12
    hit = ~par & (t >= -e) & (t <= 1 + e) & (u >= -e) & (u <= 1 + e)
    pts.append((p + t[..., None] * r).reshape(m, 16, 2))
    ok.append(hit.reshape(m, 16))
    P = np.concatenate(pts, 1)
    V = np.concatenate(ok, 1)
    # deduplicate: a point within 1e-9 of an earlier valid one goes
    scale = 1.0 + np.maximum(np.abs(a[2:4]).max(), np.abs(bs[:, 2:4]).max(1))
    d2 = ((P[:, :, None] - P[:, None]) ** 2).sum(-1)
    near = (d2 <= (1e-9 * scale[:, None, None]) ** 2) & V[:, :, None] & np.triu(np.ones((24, 24), bool), 1)[None]
    V = V & ~near.any(1)
    n = V.sum(1)
    cnt = np.maximum(n, 1)[:, None]
    cx = np.where(V, P[..., 0], 0.0).sum(1, keepdims=True) / cnt
    cy = np.where(V, P[..., 1], 0.0).sum(1, keepdims=True) / cnt
    ang = np.where(V, np.arctan2(P[..., 1] - cy, P[..., 0] - cx), np.inf)
    order = np.argsort(ang, 1, kind='stable')
    P = np.take_along_axis(P, order[..., None], 1)
    k = np.arange(24)[None]
    nxt = np.where(k + 1 < n[:, None], k + 1, 0)
    Q = np.take_along_axis(P, nxt[..., None], 1)
    cross = np.where(k < n[:, None], P[..., 0] * Q[..., 1] - Q[..., 0] * P[..., 1], 0.0)
    inter = np.where(n >= 3, np.abs(0.5 * cross.sum(1)), 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = inter / (area_a + area_b - inter)
    return np.where((area_a < 1e-14) | (area_b < 1e-14), 0.0, iou)


# --------------------------------------------------------------------------------------------- oracle
def _per_task(v, T):
    return list(v) if isinstance(v, (list, tuple)) else [v] * T


def greedy(bev, circle, thr, post_max, stats=None):
    """Greedy NMS of n candidates (best first): bev (n, 5) float32 -> kept candidate indices.  ``stats`` collects the
    smallest distance of a decided pair from its threshold and the (kept, suppressed) pairs."""
    n = bev.shape[0]
    removed = np.zeros(n, bool)
    kept = []
    b64 = bev.astype(np.float64)
    rad = 0.5 * np.sqrt(b64[:, 2] ** 2 + b64[:, 3] ** 2)
    for i in range(n):
        if removed[i]:
            continue
        if len(kept) >= post_max:
            break
        kept.append(i)
        js = i + 1 + np.nonzero(~removed[i + 1:])[0]
        if js.size == 0:
            continue
        if circle:
            dx, dy = bev[i, 0] - bev[js, 0], bev[i, 1] - bev[js, 1]
            d2 = (dx * dx + dy * dy).astype(np.float64)
            sup = d2 <= thr
            gap = np.abs(d2 - thr) / thr if thr > 0 else np.abs(d2)
        else:
            dd = (b64[i, 0] - b64[js, 0]) ** 2 + (b64[i, 1] - b64[js, 1]) ** 2
            rr = (rad[i] + rad[js]) * (1.0 + 1e-9) + 1e-9
            close = dd <= rr * rr
            iou = np.zeros(js.size)
            iou[close] = iou_one_to_many(b64[i], b64[js[close]])
            sup = iou > thr
            gap = np.abs(iou - thr)
        if stats is not None:
            stats['gap'] = min(stats.get('gap', np.inf), float(gap.min()))
            stats.setdefault('sup', []).extend((i, int(j)) for j in js[sup])
        removed[js[sup]] = True
    return np.array(kept, np.int64)


def decode(preds, ncls, coder, test_cfg, norm_bbox=True, stats=None):
    """Padded (boxes (B, M, 9 | 7) f32, scores (B, M) f32, labels (B, M) int32, counts (B,) int32), M = T *
    post_max_size.  ``preds``: one dict of numpy head outputs per task.  ``stats`` (a dict) receives per (sample, task)
    the candidate count, the cut, the keys and the NMS record."""
    T = len(preds)
    K = int(coder['max_num'])
    with_vel = 'vel' in preds[0]
    C = 9 if with_vel else 7
    nms_type = _per_task(test_cfg.get('nms_type'), T)
    nms_thr = _per_task(test_cfg.get('nms_thr'), T)
    factors = test_cfg.get('nms_rescale_factor', [1.0] * T)
    pre = test_cfg.get('pre_max_size')
    post = test_cfg.get('post_max_size')
    pre = K if pre is None else min(int(pre), K)
    post = K if post is None else int(post)
    st = test_cfg['score_threshold']
    score_thr = f32(st) if st > 0.0 else None
    coder_thr = f32(coder['score_threshold']) if coder.get('score_threshold') else None
    crange = np.asarray(coder['post_center_range'], f32)
    lim = test_cfg.get('post_center_limit_range')
    lim = np.asarray(lim, f32) if lim is not None and len(lim) > 0 else None
    osf, vs, pc = f32(coder['out_size_factor']), [f32(v) for v in coder['voxel_size']], [f32(v) for v in coder['pc_range']]
    B = preds[0]['heatmap'].shape[0]
    M = T * post
    boxes = np.zeros((B, M, C), f32)
    scores = np.zeros((B, M), f32)
    labels = np.zeros((B, M), np.int32)
    counts = np.zeros(B, np.int32)
    for b in range(B):
        out = 0
        for t in range(T):
            p = preds[t]
            n_c = ncls[t]
            H, W = p['heatmap'].shape[2:]
            HW = H * W
            if K > HW:
                raise ValueError('max_num exceeds the map')
            key = sigmoid_key(p['heatmap'][b].reshape(-1))
            idx = np.lexsort((np.arange(key.size), -key.astype(np.float64)))[:K]
            sc = key[idx]
            cls, cell = idx // HW, idx % HW
            g = lambda name, ch: p[name][b, ch].reshape(-1)[cell]  # noqa: E731
            xs = (cell % W).astype(f32) + g('reg', 0)
            ys = (cell // W).astype(f32) + g('reg', 1)
            xs = xs * osf
            xs = xs * vs[0]
            xs = xs + pc[0]
            ys = ys * osf
            ys = ys * vs[1]
            ys = ys + pc[1]
            dims = np.stack([g('dim', k) for k in range(3)], 1)
            if norm_bbox:
                dims = np.exp(dims.astype(np.float64)).astype(f32)
            rot = np.arctan2(g('rot', 0).astype(np.float64), g('rot', 1).astype(np.float64)).astype(f32)
            rows = np.zeros((K, 9), f32)
            rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3:6], rows[:, 6] = xs, ys, g('height', 0), dims, rot
            if with_vel:
                rows[:, 7], rows[:, 8] = g('vel', 0), g('vel', 1)
            ok = np.ones(K, bool)
            if coder_thr is not None:
                ok &= sc > coder_thr
            ok &= (rows[:, :3] >= crange[:3]).all(1) & (rows[:, :3] <= crange[3:]).all(1)
            circle = nms_type[t] == 'circle'
            if circle:
                thr = float(test_cfg['min_radius'][t])
                bev = np.zeros((K, 5), f32)
                bev[:, :2] = rows[:, :2]
                cut = K
            else:
                thr = float(nms_thr[t])
                if score_thr is not None:
                    ok &= sc >= score_thr
                ft = factors[t]
                fac = np.asarray([float(ft[c]) if isinstance(ft, (list, tuple)) else float(ft) for c in range(n_c)],
                                 f32)[cls]
                ds = rows[:, 3:6] * fac[:, None]
                hw, hh = ds[:, 0] / f32(2), ds[:, 1] / f32(2)
                x1, y1, x2, y2 = rows[:, 0] - hw, rows[:, 1] - hh, rows[:, 0] + hw, rows[:, 1] + hh
                bev = np.stack([(x1 + x2) / f32(2), (y1 + y2) / f32(2), x2 - x1, y2 - y1, rows[:, 6]], 1)
                rows[:, 3:6] = ds / fac[:, None]
                cut = pre
            cand = np.nonzero(ok)[0][:cut]
            st_bt = {}
            kept = cand[greedy(bev[cand], circle, thr, post, st_bt)]
            if stats is not None:
                stats[(b, t)] = dict(n=int(cand.size), n_pass=int(ok.sum()), key=key, idx=idx, circle=circle, thr=thr,
                                     kept=kept, **st_bt)
            if lim is not None and not circle:
                kept = kept[(rows[kept, :3] >= lim[:3]).all(1) & (rows[kept, :3] <= lim[3:]).all(1)]
            if stats is not None:
                stats[(b, t)]['out'] = kept
            r = rows[kept, :C].copy()
            r[:, 2] = r[:, 2] - r[:, 5] * f32(0.5)
            boxes[b, out:out + kept.size] = r
            scores[b, out:out + kept.size] = sc[kept]
            labels[b, out:out + kept.size] = cls[kept] + sum(ncls[:t])
            out += kept.size
        counts[b] = out
    return boxes, scores, labels, counts


# --------------------------------------------------------------------------------------------- comparison
def ulp_close(got, want, ulps, what=''):
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    sp = np.spacing(np.maximum(np.abs(want), f32(1e-30)).astype(f32))
    bad = np.abs(got.astype(np.float64) - want.astype(np.float64)) > ulps * sp
    assert not bad.any(), f'{what}: {bad.sum()} values beyond {ulps} ulp: got {got[bad][:5]} want {want[bad][:5]}'


def assert_padded_close(got, want, score_ulps=SCORE_ULPS):
    """Counts, labels and order exactly; scores within ``score_ulps``; x / y / vel within 1 ulp, dims and yaw within 2 ulp and z
    within the bound of ``check_padded``; rows past the count zero."""
    gb, gs, gl, gc = (np.asarray(x.cpu().numpy() if hasattr(x, 'cpu') else x) for x in got)
    wb, ws, wl, wc = want
    assert gb.shape == wb.shape and gs.shape == ws.shape and gl.shape == wl.shape
    assert gl.dtype == np.int32 and gc.dtype == np.int32
    np.testing.assert_array_equal(gc, wc, err_msg='counts')
    xyv = [0, 1, 7, 8] if wb.shape[-1] == 9 else [0, 1]
    for i, n in enumerate(wc):
        np.testing.assert_array_equal(gl[i, :n], wl[i, :n], err_msg=f'sample {i}: labels or order')
        ulp_close(gs[i, :n], ws[i, :n], score_ulps, f'sample {i} scores')
        g, w = gb[i, :n], wb[i, :n]
        ulp_close(g[:, xyv], w[:, xyv], 1, f'sample {i} x, y, vel')
        ulp_close(g[:, 3:7], w[:, 3:7], 2, f'sample {i} dims, yaw')
        dz = np.abs(w[:, 5] * f32(0.5))
        tol = np.spacing(np.abs(w[:, 2])) + 2 * np.spacing(dz) + np.spacing(np.abs(w[:, 2] + w[:, 5] * f32(0.5)))
        assert (np.abs(g[:, 2].astype(np.float64) - w[:, 2]) <= tol).all(), f'sample {i}: z'
        assert not gb[i, n:].any() and not gs[i, n:].any() and not gl[i, n:].any(), f'sample {i}: padding not zero'


# --------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, name, preds, ncls, coder, test_cfg, norm_bbox, want, stats):
        self.name, self.preds, self.ncls, self.coder, self.test_cfg = name, preds, ncls, coder, test_cfg
        self.norm_bbox, self.want, self.stats = norm_bbox, want, stats

    @property
    def K(self):
        return int(self.coder['max_num'])

    def torch_preds(self, device='cpu'):
        import torch
        return tuple([{k: torch.from_numpy(v).to(device) for k, v in p.items()}] for p in self.preds)

    def head(self, device='cpu'):
        from ocrfdet_amd import center_head as ch
        tasks = [dict(num_class=n, class_names=[f't{t}c{c}' for c in range(n)]) for t, n in enumerate(self.ncls)]
        common = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2))
        if 'vel' in self.preds[0]:
            common['vel'] = (2, 2)
        return ch.CenterHead(in_channels=4, tasks=tasks, common_heads=common, share_conv_channel=4,
                             separate_head=dict(type='SeparateHead', init_bias=-2.19, final_kernel=1, head_conv=4),
                             bbox_coder=dict(self.coder), test_cfg=dict(self.test_cfg),
                             norm_bbox=self.norm_bbox).to(device)


def _base(K, T=1, pre=None, post=None, circle=(), thr=0.2, radius=1.0, factor=1.0, coder_thr=0.1, score_thr=0.1,
          crange=(-1e3, -1e3, -10.0, 1e3, 1e3, 10.0), limit=None, H=32, W=32):
    coder = dict(type='CenterPointBBoxCoder', pc_range=[-W / 2.0, -H / 2.0], post_center_range=list(crange), max_num=K,
                 score_threshold=coder_thr, out_size_factor=4, voxel_size=[0.25, 0.25], code_size=9)
    test = dict(pc_range=coder['pc_range'], post_center_limit_range=list(limit) if limit else [], max_per_img=K,
                max_pool_nms=False, min_radius=[radius] * T, score_threshold=score_thr, out_size_factor=4,
                voxel_size=[0.25, 0.25], pre_max_size=K if pre is None else pre, post_max_size=K if post is None else post,
                nms_type=['circle' if t in circle else 'rotate' for t in range(T)], nms_thr=[thr] * T,
                nms_rescale_factor=[factor] * T)
    return coder, test


def _heads(rng, B, ncls, H, W, size=(1.0, 2.5), logits='distinct', vel=True, norm_bbox=True):
    """Random head outputs.  logits 'distinct': every cell's key from a shuffled grid in (0.02, 0.98), so that distinct
    keys are thousands of ulp apart; 'quant': multiples of 1/8 in [-1, 2]; boxes of side ``size`` metres on 1 m
    cells with any yaw."""
    out = []
    for n in ncls:
        N = n * H * W
        if logits == 'distinct':
            p = 0.02 + 0.96 * (rng.permutation(B * N).reshape(B, N) + 0.5) / (B * N)
            hm = np.log(p / (1 - p))
        else:
            hm = rng.integers(-8, 17, (B, N)) / 8.0
        sides = rng.uniform(size[0], size[1], (B, 2, H, W))
        d = dict(heatmap=hm.reshape(B, n, H, W), reg=rng.uniform(0, 1, (B, 2, H, W)),
                 height=rng.uniform(-1, 1, (B, 1, H, W)),
                 dim=np.concatenate([sides, rng.uniform(0.5, 2.0, (B, 1, H, W))], 1))
        if norm_bbox:
            d['dim'] = np.log(d['dim'])
        yaw, r = rng.uniform(-np.pi, np.pi, (B, H, W)), rng.uniform(0.5, 2.0, (B, H, W))
        d['rot'] = np.stack([r * np.sin(yaw), r * np.cos(yaw)], 1)
        if vel:
            d['vel'] = rng.normal(0, 1, (B, 2, H, W))
        out.append(d)
    return out


def _set_box(d, b, x, y, cx, cy, dims, yaw, c=0, logit=None, norm_bbox=True, sincos=None):
    """Box of task head d at cell (x, y): centre (cx, cy) in cells, dims (w, l, h) metres."""
    if logit is not None:
        d['heatmap'][b, c, y, x] = logit
    d['reg'][b, :, y, x] = (cx - x, cy - y)
    d['dim'][b, :, y, x] = [(np.log(v) if v > 0 else -100.0) if norm_bbox else v for v in dims]
    d['rot'][b, :, y, x] = sincos if sincos is not None else (np.sin(yaw), np.cos(yaw))


# every case: (spec builder, claims).  A spec builder takes rng -> (preds as float64 arrays, ncls, coder, test, norm_bbox)
def _simple(K, B=2, ncls=(1,), H=32, W=32, logits='distinct', size=(1.0, 2.5), **kw):
    def make(rng):
        coder, test = _base(K, T=len(ncls), H=H, W=W, **kw)
        return _heads(rng, B, ncls, H, W, size=size, logits=logits), list(ncls), coder, test, True
    return make


def _spill(K, **kw):
    """Every cell passes the filters.  Cells pair up along a row: the second box of a pair sits on the first, with
    nearly its size and yaw, and the two take neighbouring ranks, so that overlapping clusters are spread over the whole
    score range and a kept box at any rank suppresses the next one."""
    def make(rng):
        B, H, W = 2, 32, 32
        coder, test = _base(K, coder_thr=None, score_thr=0.0, post=K, **kw)
        preds = _heads(rng, B, [1], H, W, size=(1.2, 2.4))
        d = preds[0]
        N = H * W
        grid = np.log((np.arange(N) + 0.5) / N * 0.96 + 0.02) - np.log(1 - ((np.arange(N) + 0.5) / N * 0.96 + 0.02))
        for b in range(B):
            rank = rng.permutation(N // 2)
            for m in range(N // 2):
                y, x = divmod(2 * m, W)
                lead = rng.integers(0, 2)
                xl, xp = x + lead, x + 1 - lead
                d['heatmap'][b, 0, y, xl] = grid[2 * rank[m] + 1]
                d['heatmap'][b, 0, y, xp] = grid[2 * rank[m]]
                d['reg'][b, 0, y, xp] = xl + d['reg'][b, 0, y, xl] - xp + rng.uniform(-0.05, 0.05)
                d['reg'][b, 1, y, xp] = d['reg'][b, 1, y, xl] + rng.uniform(-0.05, 0.05)
                d['dim'][b, :, y, xp] = d['dim'][b, :, y, xl] + rng.uniform(-0.05, 0.05, 3)
                d['rot'][b, :, y, xp] = d['rot'][b, :, y, xl] + rng.uniform(-0.02, 0.02, 2)
        return preds, [1], coder, test, True
    return make


def _ties(kind):
    def make(rng):
        B, H, W = 2, 24, 24
        if kind == 'quant':
            ncls = [3]
            preds = _heads(rng, B, ncls, H, W, logits='quant')
            coder, test = _base(300, H=H, W=W, pre=1000, post=300)
        else:
            ncls = [2]
            H = W = 32
            preds = _heads(rng, B, ncls, H, W)
            hm = preds[0]['heatmap']
            if kind == 'saturated':     # 500 cells with key 1.0f; the rest below
                for b in range(B):
                    flat = hm[b].reshape(-1)
                    flat[rng.choice(flat.size, 500, replace=False)] = rng.uniform(20.0, 40.0, 500)
                coder, test = _base(300, H=H, W=W)
            else:                       # 'zero': keys 0 and denormal, no thresholds
                for b in range(B):
                    flat = hm[b].reshape(-1)
                    flat[:] = -120.0
                    sel = rng.choice(flat.size, 150, replace=False)
                    flat[sel] = rng.choice([-87.5, -88.0, -88.5], 150)
                coder, test = _base(300, H=H, W=W, coder_thr=None, score_thr=0.0)
        return preds, ncls, coder, test, True
    return make


def _circle(K):
    def make(rng):
        B = 2
        preds = _heads(rng, B, [1], 32, 32)
        coder, test = _base(K, circle=(0,), radius=1.0, post=K)
        d = preds[0]
        for b in range(B):         # pairs at 0.99 and 1.01 of min_radius (squared metres), ranks 1-4
            _set_box(d, b, 2, 2, 2.5, 2.5, (1, 1, 1), 0.0, logit=8.0)
            _set_box(d, b, 3, 2, 2.5 + np.sqrt(0.99), 2.5, (1, 1, 1), 0.0, logit=7.9)
            _set_box(d, b, 20, 20, 20.5, 20.5, (1, 1, 1), 0.0, logit=7.8)
            _set_box(d, b, 20, 21, 20.5, 20.5 + np.sqrt(1.01), (1, 1, 1), 0.0, logit=7.7)
        return preds, [1], coder, test, True
    return make


def _geometry(rng):
    B, H, W = 1, 24, 24
    preds = _heads(rng, B, [1], H, W, size=(0.2, 0.4))
    coder, test = _base(64, H=H, W=W, thr=0.3, pre=64, post=64)
    d = preds[0]
    L = iter(np.arange(10.0, 5.0, -0.1))
    box = lambda x, y, cx, cy, dims, yaw, **kw: _set_box(d, 0, x, y, cx, cy, dims, yaw, logit=next(L), **kw)  # noqa
    box(2, 2, 2.5, 2.5, (2, 2, 1), 0.0)                  # A
    box(3, 2, 2.5, 2.5, (2, 2, 1), 0.0)                  # identical to A: suppressed
    box(2, 3, 2.5, 2.5, (0.0, 2, 1), 0.0)                # zero area (dim logit -100 below) on A: kept
    box(8, 2, 8.5, 2.5, (4, 4, 1), 0.3)                  # B
    box(9, 2, 8.5, 2.5, (2, 2, 1), 0.3)                  # inside B, IoU 0.25: kept
    box(8, 3, 8.5, 2.5, (3, 3, 1), 0.3)                  # inside B, IoU 0.5625: suppressed
    box(14, 2, 14.5, 2.5, (1, 1, 1), 0.0)                # D
    box(15, 2, 15.5, 2.5, (1, 1, 1), 0.0)                # shares an edge with D: kept
    box(14, 8, 14.5, 8.5, (1, 1, 1), 0.0)                # E
    box(15, 9, 15.5, 9.5, (1, 1, 1), 0.0)                # touches E at a corner: kept
    box(2, 8, 2.5, 8.5, (1.6, 1.6, 1), 0.0)              # square
    box(3, 8, 2.5, 8.5, (1.6, 1.6, 1), np.pi / 2, sincos=(1.0, 0.0))   # the square turned 90 degrees: suppressed
    box(8, 14, 8.5, 14.5, (6, 0.2, 1), 0.1)              # long thin
    box(9, 14, 8.5, 14.5, (6, 0.2, 1), 1.2)              # crossing it: kept
    box(8, 15, 8.5, 14.55, (6, 0.2, 1), 0.1)             # parallel, 0.05 off: suppressed
    box(2, 20, 2.5, 20.5, (3, 1, 1), np.pi, sincos=(0.0, -1.0))     # yaw +pi
    box(3, 20, 2.5, 20.5, (3, 1, 1), -np.pi, sincos=(-0.0, -1.0))   # yaw -pi, the same rectangle: suppressed
    box(4, 20, 2.5, 20.5, (3, 1, 1), 0.0)                # yaw 0, the same rectangle: suppressed
    return preds, [1], coder, test, True


def _thresholds(which):
    def make(rng):
        B, H, W = 2, 16, 16
        ncls = [2, 1]
        preds = _heads(rng, B, ncls, H, W)
        for d in preds:             # keys mostly below 0.5, so that the cells at key 0.5 are in the top K
            d['heatmap'] -= 2.0
        if which == 'coder':        # key 0.5 exactly, strict > drops it
            coder, test = _base(100, T=2, H=H, W=W, circle=(1,), coder_thr=0.5, score_thr=0.2)
        else:                       # key 0.5 exactly, >= keeps it (rotate task only)
            coder, test = _base(100, T=2, H=H, W=W, circle=(1,), coder_thr=0.1, score_thr=0.5)
        for d in preds:
            for b in range(B):
                flat = d['heatmap'][b].reshape(-1)
                flat[rng.choice(flat.size, 12, replace=False)] = 0.0
        return preds, ncls, coder, test, True
    return make


def _outputs(which):
    def make(rng):
        B, H, W = 2, 16, 16
        ncls = [2, 1]
        kw = dict(T=2, H=H, W=W, circle=(1,), radius=2.0)
        preds = _heads(rng, B, ncls, H, W, vel=which != 'no_vel', norm_bbox=which != 'raw_dims')
        if which == 'post1':
            kw['post'] = 1
        elif which == 'post_big':
            kw['post'] = 300
        elif which == 'limit':
            kw.update(crange=(-7.0, -1e3, -10.0, 1e3, 1e3, 10.0), limit=(-4.0, -5.0, -0.5, 5.0, 6.0, 0.5))
        return preds, ncls, _base(100, **kw)[0], _base(100, **kw)[1], which != 'raw_dims'
    return make


def _limits(B):
    def make(rng):
        H, W = 12, 12
        ncls = [1, 2, 3, 4, 5, 6, 7, 8]
        preds = _heads(rng, B, ncls, H, W)
        coder, test = _base(100, T=8, H=H, W=W, pre=80, post=50, circle=(3, 6), radius=1.5)
        test['nms_thr'] = [0.1, 0.2, 0.3, 0.4, 0.5, 0.15, 0.25, 0.35]
        test['nms_rescale_factor'] = [1.0, [0.7, 1.3], [0.5, 1.0, 2.0], 1.1, [1.5, 0.8, 1.0, 0.6, 1.2],
                                      [1.0 + 0.1 * c for c in range(6)], 0.9, [0.6 + 0.1 * c for c in range(8)]]
        return preds, ncls, coder, test, True
    return make


def _map(ncls, H, W, K):
    return _simple(K, ncls=ncls, H=H, W=W, post=K)


CASES = {}
for _k in (1, 63, 64, 65, 128, 129, 513, 641):
    CASES[f'words_K{_k}'] = (_simple(_k, pre=max(_k, 1000), post=_k, size=(1.5, 3.0)), {'words'})
for _k in (705, 769, 1000, 1024):
    CASES[f'spill_K{_k}'] = (_spill(_k), {'spill'})
for _p in (64, 65, 300):
    CASES[f'pre_K500_{_p}'] = (_simple(500, pre=_p, post=500), {'pre'})
CASES['pre_K1024_700'] = (_spill(1024, pre=700), {'pre', 'spill'})
CASES['circle_K100'] = (_circle(100), {'circle', 'pairs'})
CASES['circle_K600'] = (_circle(600), {'circle', 'pairs'})
for _kind in ('quant', 'saturated', 'zero'):
    CASES[f'ties_{_kind}'] = (_ties(_kind), {'tie'})
CASES['map_1023'] = (_map((3,), 11, 31, 200), set())
CASES['map_1024'] = (_map((1,), 32, 32, 300), set())
CASES['map_1025'] = (_map((5,), 5, 41, 205), {'full'})
CASES['map_2049'] = (_map((3,), 1, 683, 400), set())
CASES['map_full_32x32'] = (_map((2,), 32, 32, 1024), {'full'})
CASES['limits_B1'] = (_limits(1), set())
CASES['limits_B16'] = (_limits(16), set())
CASES['geometry'] = (_geometry, {'geometry'})
CASES['thr_coder'] = (_thresholds('coder'), {'thr_coder'})
CASES['thr_test'] = (_thresholds('test'), {'thr_test'})
for _w in ('post1', 'post_big', 'limit', 'no_vel', 'raw_dims'):
    CASES[f'out_{_w}'] = (_outputs(_w), {_w})


def _check_keys(case, stats):
    """Keys next to each other in the top K + 1 are equal by construction (equal logits, or both saturated) or more
    than KEY_GAP_ULPS apart, and no top-K key is that close to a score threshold unless equal to it (logit 0, key 0.5),
    so that neither the order nor a filter hangs on how a sigmoid rounds."""
    thrs = [case.coder.get('score_threshold') or 0.0, case.test_cfg['score_threshold']]
    thrs = [f32(v) for v in thrs if v > 0]
    for (b, t), s in stats.items():
        logit = case.preds[t]['heatmap'][b].reshape(-1).astype(np.float64)
        key = s['key']
        order = np.lexsort((np.arange(key.size), -key.astype(np.float64)))[:case.K + 1]
        for i, j in zip(order[:-1], order[1:]):
            li, lj, ki, kj = logit[i], logit[j], key[i], key[j]
            if li == lj or (ki == kj == 1.0 and min(li, lj) >= 20.0) or (ki == kj == 0.0 and max(li, lj) <= -110.0):
                continue
            assert abs(float(ki) - float(kj)) > KEY_GAP_ULPS * np.spacing(max(ki, kj)), \
                f'{case.name} ({b}, {t}): keys {ki} and {kj} of logits {li}, {lj} are within {KEY_GAP_ULPS} ulp'
        for v in thrs:
            top = key[order[:-1]]
            near = (top != v) & (np.abs(top.astype(np.float64) - float(v)) <= KEY_GAP_ULPS * np.spacing(v))
            assert not near.any(), f'{case.name} ({b}, {t}): a key within {KEY_GAP_ULPS} ulp of the threshold {v}'


def _check_claims(case, claims, stats):
    K = case.K
    st = list(stats.values())
    if 'words' in claims:
        assert max(s['n'] for s in st) == K and (K == 1 or sum(len(s.get('sup', [])) for s in st) > 0)
    if 'spill' in claims:
        rows = lds_rows(K, K)
        assert rows < 1024 and any(s['n'] > lds_rows(K, s['n']) for s in st), 'no (sample, task) spills'
        assert any(i >= lds_rows(K, s['n']) for s in st for i, _ in s.get('sup', [])), \
            'no suppression comes from a mask row held in global memory'
    if 'pre' in claims:
        pre = case.test_cfg['pre_max_size']
        assert all(s['n'] == pre < s['n_pass'] for s in st) and (K + 63) // 64 > 1
    if 'circle' in claims:
        assert all(s['circle'] and s['n'] > 64 for s in st) and (K < 512 or all(s['n'] > 512 for s in st))
    if 'pairs' in claims:
        for s in st:
            sup = set(s['sup'])
            assert (0, 1) in sup and 2 in s['kept'] and 3 in s['kept'] and (2, 3) not in sup
    if 'tie' in claims:
        for s in st:
            key, idx = s['key'], s['idx']
            v = key[idx[K - 1]]
            eq = np.nonzero(key == v)[0]
            assert key[idx[K - 1]] == np.sort(key)[::-1][K], 'no tie across the K boundary'
            assert len(np.unique(eq // 1024)) > 1, 'the tie does not span two 1024-element chunks'
            H, W = case.preds[0]['heatmap'].shape[2:]
            assert len(np.unique(eq // (H * W))) > 1, 'the tie does not span two classes'
    if 'full' in claims:
        H, W = case.preds[0]['heatmap'].shape[2:]
        assert K == H * W
    if 'geometry' in claims:
        s = stats[(0, 0)]
        sup = set(s['sup'])
        want_sup = {(0, 1), (3, 5), (10, 11), (12, 14), (15, 16), (15, 17)}
        want_keep = {0, 2, 3, 4, 6, 7, 8, 9, 10, 12, 13, 15}
        assert want_sup <= sup and want_keep <= set(s['kept'].tolist()), (sorted(sup)[:20], s['kept'][:20])
    if 'thr_coder' in claims or 'thr_test' in claims:
        for (b, t), s in stats.items():
            top = s['key'][s['idx']]
            assert (top == 0.5).any()
            if t == 0 and 'thr_test' in claims:
                assert any(top[k] == 0.5 for k in s['kept'])
    if 'post1' in claims:
        assert all(len(s['kept']) == 1 for s in st)
    if 'post_big' in claims:
        assert all(len(s['kept']) < case.test_cfg['post_max_size'] for s in st)
    if 'limit' in claims:
        assert any(len(s['out']) < len(s['kept']) for s in st if not s['circle'])
        assert any(s['n_pass'] < K for s in st)


def build(name, seed=0, tries=20):
    make, claims = CASES[name]
    for k in range(tries):
        rng = np.random.default_rng([seed, k, sum(map(ord, name))])
        preds, ncls, coder, test, norm_bbox = make(rng)
        preds = [{h: np.ascontiguousarray(v, np.float32) for h, v in p.items()} for p in preds]
        stats = {}
        want = decode(preds, ncls, coder, test, norm_bbox, stats)
        gaps = [s['gap'] for s in stats.values() if 'gap' in s]
        if not gaps or min(gaps) > MARGIN:
            break
    else:
        raise AssertionError(f'{name}: no draw in {tries} keeps every decided pair {MARGIN} from its threshold')
    case = Case(name, preds, ncls, coder, test, norm_bbox, want, stats)
    _check_keys(case, stats)
    _check_claims(case, claims, stats)
    return case
