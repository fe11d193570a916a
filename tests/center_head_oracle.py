"""A plain oracle of the detection head's training targets and losses, and the test cases built on it.

It restates ``get_targets_single`` and ``loss`` of the reference's CenterHead from what tests/test_center_head_host.py
pins and include/ocrf_hip.h and DESIGN.md (4.10) describe, and shares no code with ``ocrfdet_amd/center_head.py`` or
the kernels (csrc/center_head.hip).

``targets``: one Python loop per sample, task and object, in the reference's order.

* A task's objects are regrouped class by class (every object of the task's first class in input order, then the
  second class, ...).  The k-th object of that list owns slot k.  A label outside the class table (-1, n_labels, ...)
  belongs to no task.  Objects from slot ``max_objs`` on are dropped before anything is drawn.
* What the reference computes on float32 tensors is computed with numpy float32 scalars, one operation at a time:
  width and length in cells (``/ voxel_size / out_size_factor``), the three roots of the radius formula with Python's
  ``min``, the centre in cells, the gravity-centre z, the centre's offset from its cell.  IEEE ``/`` and ``sqrt`` are
  correctly rounded, so the integer outcomes (skip, radius, cell) are defined exactly and no input needs excluding.
  log / sin / cos are taken in float64 and rounded once (a float32 implementation may differ by an ulp or two).
* An object is skipped, keeping its slot, unless width > 0 and length > 0, and again when its centre cell
  (``.to(int32)``: truncation toward zero, so a centre in (-1, 0) lands in cell 0) is off the map.
* radius = max(min_radius, int(r)).  Two rules go beyond the reference: a NaN r (an infinite
  dimension; the reference raises at ``int(nan)``) counts as 0, and r is capped at 65536.
* A draw is ``max`` of the plane's window, clipped to the map, with the float64 Gaussian exp(-(x^2 + y^2) /
  (2 sigma^2)), sigma = (2 radius + 1) / 6, zeroed below eps * max (max = 1, the centre) and then cast to float32.

``heatmap_loss`` / ``reg_loss``: float64 throughout, gradients by torch's float64 autograd of the plain operations
on the CPU.  clip_sigmoid clamps to the float32 values of 1e-4 and 1 - 1e-4 (the reference clamps a float32 tensor);
the heat-map divisor is float32(max(count, 1) + eps); the regression loss is |pred - target| * mask * isnotnan *
code_weight gathered at ``ind``, five group sums over (num + 1e-4) + eps and the single sum over num + eps,
num = max(mask sum, 1e-4), eps = float32's.  A NaN target code makes its loss NaN (NaN * 0) and its gradient 0
(autograd's sgn(NaN) = 0).

``build(name)`` makes one named case of ``CASES`` (seeded, cached) and asserts that it is what its name claims;
``check_targets`` / ``check_heatmap_loss`` / ``check_reg_loss`` hold a formulation's results to the oracle:

* targets: ind, mask, both counts, the heat map's cells equal to 0 and equal to 1 and anno columns 0, 1, 2, 8, 9
  exactly; other heat-map cells within 1 float32 ulp (a float64 exp off by one ulp may round the other way), anno
  columns 3:8 within 2 ulp;
* loss values within 1e-5 relative (the project's bar for fused losses), clip_sigmoid within 1e-6 absolute;
* gradients by region, each region held to 1e-5 of the ORACLE's largest entry in that region: heat-map logits under
  g == 1, 0 < g < 1, g == 0, and where the sigmoid is clipped (exactly 0 there); per regression head the cells the
  oracle writes (the non-zero set must be equal, every other cell 0).  A caller may pass the float32 torch
  formulation's own errors ``e_torch``: where one already exceeds 1e-5 the region's bar is 2 e_torch (a different
  summation order, the margin of tests/test_optim_gpu.py).
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

F32 = np.float32
F32_EPS = float(np.finfo(np.float32).eps)
F64_EPS = float(np.finfo(np.float64).eps)
CLIP_LO, CLIP_HI = float(F32(1e-4)), float(F32(1 - 1e-4))
GROUP_EDGES = (0, 2, 3, 6, 8, 10)
HEADS = (('reg', 2), ('height', 1), ('dim', 3), ('rot', 2), ('vel', 2))
CODE_WEIGHTS = [1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1]
RADIUS_CAP = 65536
RTOL = 1e-5


# --------------------------------------------------------------------------------------------- targets
def radius_f32(length, width, overlap):
    """gaussian_radius((length, width), overlap) on float32 scalars: the Python scalars folded in double and rounded
    to float32 where they meet a tensor, ``b ** 2`` as a product, Python's min (the first of the smallest; a NaN
    root is never smaller)."""
    h, w = F32(length), F32(width)
    o = float(overlap)
    omo, opo, om1 = F32(1 - o), F32(1 + o), F32(o - 1)
    with np.errstate(all='ignore'):
        b1 = h + w
        c1 = w * h * omo / opo
        r1 = (b1 + np.sqrt(b1 * b1 - F32(4) * c1)) / F32(2)
        b2 = F32(2) * (h + w)
        c2 = omo * w * h
        r2 = (b2 + np.sqrt(b2 * b2 - F32(16) * c2)) / F32(2)
        b3 = F32(-2 * o) * (h + w)
        c3 = om1 * w * h
        r3 = (b3 + np.sqrt(b3 * b3 - F32(4 * (4 * o)) * c3)) / F32(2)
    for r in (r1, r2, r3):
        assert type(r) is np.float32
    return min(r1, r2, r3)


def draw(plane, ix, iy, radius):
    """One draw_heatmap_gaussian: max of the clipped window with the float64 Gaussian cast to float32."""
    H, W = plane.shape
    sigma = (2 * radius + 1) / 6
    left, right = min(ix, radius), min(W - ix, radius + 1)
    top, bottom = min(iy, radius), min(H - iy, radius + 1)
    y = np.arange(-top, bottom, dtype=np.float64)[:, None]
    x = np.arange(-left, right, dtype=np.float64)[None, :]
    g = np.exp(-(x * x + y * y) / (2 * sigma * sigma))
    g[g < F64_EPS * 1.0] = 0                        # the whole window's max is its centre, exp(0) = 1
    win = plane[iy - top:iy + bottom, ix - left:ix + right]
    np.maximum(win, g.astype(np.float32), out=win)


def map_size(cfg):
    osf = int(cfg['out_size_factor'])
    return int(cfg['grid_size'][1]) // osf, int(cfg['grid_size'][0]) // osf          # H, W


def targets(boxes, labels, offsets, table, ncls, cfg, with_velocity, norm_bbox):
    """Namespace of heat (list over tasks of (B, ncls, H, W) f32), flat (the blocks back to back), anno (T, B, M, C)
    f32, ind (T, B, M) int64, mask (T, B, M) uint8, ones and msum (T,) (heat-map cells equal to 1, mask sums) and
    objs, one (b, t, cls, slot, ix, iy, radius) per drawn object."""
    boxes = np.asarray(boxes, np.float32)
    labels = np.asarray(labels, np.int64)
    offsets = [int(o) for o in offsets]
    table = np.asarray(table).reshape(-1, 2)
    T, B = len(ncls), len(offsets) - 1
    H, W = map_size(cfg)
    M = int(cfg['max_objs']) * int(cfg['dense_reg'])
    C = 10 if with_velocity else 8
    vs = [F32(v) for v in cfg['voxel_size']]
    pc = [F32(v) for v in cfg['point_cloud_range']]
    osf = F32(int(cfg['out_size_factor']))
    heat = [np.zeros((B, n, H, W), np.float32) for n in ncls]
    anno = np.zeros((T, B, M, C), np.float32)
    ind = np.zeros((T, B, M), np.int64)
    mask = np.zeros((T, B, M), np.uint8)
    objs = []
    for b in range(B):
        bx, lab = boxes[offsets[b]:offsets[b + 1]], labels[offsets[b]:offsets[b + 1]]
        where = [(int(table[v, 0]), int(table[v, 1])) if 0 <= v < len(table) else (-1, 0) for v in lab]
        for t in range(T):
            regrouped = [(i, c) for c in range(ncls[t]) for i in range(len(lab)) if where[i] == (t, c)]
            for k, (i, c) in enumerate(regrouped[:M]):
                row = bx[i]
                width = row[3] / vs[0] / osf
                length = row[4] / vs[1] / osf
                if not (width > 0 and length > 0):
                    continue
                r = radius_f32(length, width, cfg['gaussian_overlap'])
                radius = max(int(cfg['min_radius']), 0 if np.isnan(r) else int(min(r, F32(RADIUS_CAP))))
                cx = (row[0] - pc[0]) / vs[0] / osf
                cy = (row[1] - pc[1]) / vs[1] / osf
                ix, iy = int(cx), int(cy)
                if not (0 <= ix < W and 0 <= iy < H):
                    continue
                draw(heat[t][b, c], ix, iy, radius)
                ind[t, b, k] = iy * W + ix
                mask[t, b, k] = 1
                with np.errstate(all='ignore'):
                    dims = [F32(np.log(np.float64(d))) if norm_bbox else d for d in row[3:6]]
                    code = [cx - F32(ix), cy - F32(iy), row[2] + row[5] * F32(0.5), *dims,
                            F32(np.sin(np.float64(row[6]))), F32(np.cos(np.float64(row[6])))]
                if with_velocity:
                    code += [row[7], row[8]]
                assert all(type(v) is np.float32 for v in code)
                anno[t, b, k] = code
                objs.append((b, t, c, k, ix, iy, radius))
    ones = np.array([float((h == 1).sum()) for h in heat])
    msum = mask.reshape(T, -1).sum(1).astype(np.float64)
    return SimpleNamespace(heat=heat, flat=np.concatenate([h.reshape(-1) for h in heat]), anno=anno, ind=ind,
                           mask=mask, ones=ones, msum=msum, objs=objs, shape=(T, B, M, C, H, W))


# --------------------------------------------------------------------------------------------- losses
def heatmap_loss(logits, heat, ones, loss_weight, grad_out):
    """logits, heat: lists over tasks of (B, n, H, W) float32 arrays; ones (T,); grad_out (T,) -> namespace of out
    (T,) f64, clipped, grads, sig (the unclipped sigmoid), lists of f64 arrays."""
    out, clipped, grads, sig = [], [], [], []
    for t, (x, g) in enumerate(zip(logits, heat)):
        x = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
        g = torch.tensor(np.asarray(g), dtype=torch.float64)
        s = 1 / (1 + torch.exp(-x))
        p = torch.clamp(s, min=CLIP_LO, max=CLIP_HI)
        pos = (g == 1).double()
        loss = -torch.log(p + 1e-12) * (1 - p) ** 2 * pos - torch.log(1 - p + 1e-12) * p ** 2 * (1 - g) ** 4
        den = float(F32(max(float(ones[t]), 1.0) + F32_EPS))
        val = loss_weight * (loss.sum() / den)
        val.backward(torch.tensor(float(grad_out[t]), dtype=torch.float64))
        out.append(val.item())
        clipped.append(p.detach().numpy())
        grads.append(x.grad.numpy())
        sig.append(s.detach().numpy())
    return SimpleNamespace(out=np.array(out), clipped=clipped, grads=grads, sig=sig)


def reg_loss(heads, anno, ind, mask, msum, code_weights, loss_weight, grad_out):
    """heads: list over tasks of {name: (B, c, H, W) float32 array} (no 'vel' without velocity); grad_out (T, 6) ->
    namespace of out (T, 6) f64 (the five groups, then the single sum) and grads (list of {name: f64 array})."""
    T, B, M, C = anno.shape
    names = [n for n, _ in HEADS][:5 if C == 10 else 4]
    cw = torch.tensor(list(code_weights[:C]), dtype=torch.float64)
    rows, leaves = [], []
    for t in range(T):
        leaf = {n: torch.tensor(np.asarray(heads[t][n]), dtype=torch.float64, requires_grad=True) for n in names}
        leaves.append(leaf)
        pred = torch.cat([leaf[n] for n in names], 1).reshape(B, C, -1)
        p = torch.stack([pred[b][:, torch.from_numpy(ind[t, b])].T for b in range(B)])         # (B, M, C)
        tgt = torch.from_numpy(anno[t]).double()
        w = torch.from_numpy(mask[t]).double()[:, :, None] * (~torch.isnan(tgt)).double() * cw
        loss = (p - tgt).abs() * w
        num = max(float(msum[t]), 1e-4)
        row = [loss_weight * (loss[..., a:b].sum() / ((num + 1e-4) + F32_EPS))
               for a, b in zip(GROUP_EDGES, GROUP_EDGES[1:])]
        rows.append(torch.stack(row + [loss_weight * (loss.sum() / (num + F32_EPS))]))
    out = torch.stack(rows)
    out.backward(torch.tensor(np.asarray(grad_out), dtype=torch.float64))
    return SimpleNamespace(out=out.detach().numpy(),
                           grads=[{n: leaf[n].grad.numpy() for n in names} for leaf in leaves])


# --------------------------------------------------------------------------------------------- checks
def _ulps(a, b):
    """|a - b| in float32 ulps of the larger magnitude; 0 where both are the same infinity or both NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(all='ignore'):
        d = np.abs(a.astype(np.float64) - b) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)
    return np.where(same, 0.0, np.where(np.isfinite(d), d, np.inf))


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check_targets(got, want):
    """got = (flat heat, anno, ind, mask, counts (2T,)) as arrays, want = ``targets(...)``."""
    heat, anno, ind, mask, counts = (np.asarray(a) for a in got)
    T, C = want.shape[0], want.shape[3]
    assert ind.dtype == np.int64 and mask.dtype == np.uint8 and heat.dtype == np.float32 and anno.dtype == np.float32
    assert np.array_equal(mask, want.mask), f'mask differs in {int((mask != want.mask).sum())} slots'
    assert np.array_equal(ind, want.ind), f'ind differs in {int((ind != want.ind).sum())} slots'
    assert np.array_equal(counts[:T], want.ones.astype(np.float32)), (counts[:T], want.ones)
    assert np.array_equal(counts[T:], want.msum.astype(np.float32)), (counts[T:], want.msum)
    assert heat.shape == want.flat.shape
    assert np.array_equal(heat == 0, want.flat == 0), 'the sets of heat-map cells equal to 0 differ'
    assert np.array_equal(heat == 1, want.flat == 1), 'the sets of heat-map cells equal to 1 differ'
    u = _ulps(heat, want.flat)
    assert u.max() <= 1, f'heat map: {int((u > 1).sum())} cells off by more than 1 ulp, worst {u.max()}'
    exact = [0, 1, 2] + ([8, 9] if C == 10 else [])
    assert _same(anno[..., exact], want.anno[..., exact]), 'anno columns 0, 1, 2, 8, 9 differ'
    v = _ulps(anno[..., 3:8], want.anno[..., 3:8])
    assert v.max() <= 2, f'anno columns 3:8 off by {v.max()} ulp'
    return dict(heat_ulp=float(u.max()), heat_inexact=int((u > 0).sum()), anno_ulp=float(v.max()))


def _loss_close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f'{what}: NaN losses differ: {got} against {want}'
    ok = ~np.isnan(want)
    err = np.abs(got - want)[ok] / np.maximum(np.abs(want[ok]), 1e-30)
    assert np.all(err <= RTOL), f'{what}: {got} against {want}, relative error {err.max():.3e}'
    return float(err.max(initial=0.0))


def _region_errors(got, want, regions):
    """{name: max |got - want| over the region / the oracle's largest entry there}; a region whose oracle entries are
    all 0 must be 0 exactly (error inf otherwise)."""
    out = {}
    for name, sel in regions.items():
        if not sel.any():
            continue
        g, w = got[sel], want[sel]
        scale = np.abs(w).max()
        d = np.abs(g - w).max()
        out[name] = float(d / scale) if scale > 0 else (0.0 if d == 0 else float('inf'))
    return out


def _hold(errors, e_torch, what):
    for name, e in errors.items():
        bar = RTOL
        if e_torch is not None and e_torch.get(name, 0.0) > RTOL:
            bar = 2 * e_torch[name]
        assert np.isfinite(e) and e <= bar, f'{what}, region {name}: error {e:.3e} above {bar:.3e}'


def heat_regions(c):
    """Per task the four regions of the heat-map logits' gradient."""
    out = []
    for g, s in zip(c.tg.heat, c.hm.sig):
        clip = (s < CLIP_LO) | (s > CLIP_HI)
        out.append({'g==1': (g == 1) & ~clip, '0<g<1': (g > 0) & (g < 1) & ~clip, 'g==0': (g == 0) & ~clip,
                    'clipped': clip})
    return out


def heatmap_errors(grads, c):
    """{region: the worst error over the tasks} of a formulation's logit gradients (lists of arrays), unasserted."""
    worst = {}
    for t, regions in enumerate(heat_regions(c)):
        for k, e in _region_errors(np.asarray(grads[t], np.float64), c.hm.grads[t], regions).items():
            worst[k] = max(worst.get(k, 0.0), e)
    return worst


def reg_errors(grads, c, i):
    """{head: the worst error over the tasks, on the cells the oracle writes} for the case's i-th grad_out."""
    worst = {}
    for t, per_head in enumerate(c.reg[i].grads):
        for name, w in per_head.items():
            e = _region_errors(np.asarray(grads[t][name], np.float64), w, {name: w != 0})
            worst[name] = max(worst.get(name, 0.0), e.get(name, 0.0))
    return worst


def check_heatmap_loss(out, clipped, grads, c, e_torch=None):
    """out (T,), clipped and grads (lists of arrays) of a formulation against case ``c`` -> ``heatmap_errors``."""
    _loss_close(out, c.hm.out, 'heat-map loss')
    for t, regions in enumerate(heat_regions(c)):
        p = np.asarray(clipped[t], np.float64)
        assert np.abs(p - c.hm.clipped[t]).max() <= 1e-6, f'task {t}: clip_sigmoid'
        gr = np.asarray(grads[t])
        assert np.isfinite(gr).all()
        assert not gr[regions['clipped']].any(), f'task {t}: a clipped cell has a gradient'
    worst = heatmap_errors(grads, c)
    _hold(worst, e_torch, 'heat-map gradient')
    return worst


def check_reg_loss(out, grads, c, i, e_torch=None):
    """out (T, 6) and grads (list over tasks of {name: array}) for the case's i-th grad_out -> ``reg_errors``."""
    want = c.reg[i]
    _loss_close(out, want.out, 'regression loss')
    for t, per_head in enumerate(want.grads):
        assert sorted(grads[t]) == sorted(per_head)
        for name, w in per_head.items():
            g = np.asarray(grads[t][name])
            assert np.isfinite(g).all(), f'task {t}, {name}: non-finite gradient'
            assert np.array_equal(g != 0, w != 0), \
                f'task {t}, {name}: written cells differ in {int(((g != 0) != (w != 0)).sum())} places'
    worst = reg_errors(grads, c, i)
    _hold(worst, e_torch, 'regression gradient')
    return worst


# --------------------------------------------------------------------------------------------- cases
def make_cfg(W, H, max_objs, voxel=0.1, osf=8, min_radius=2, overlap=0.1):
    cell = voxel * osf
    return dict(point_cloud_range=[-cell * W / 2, -cell * H / 2, -5.0, cell * W / 2, cell * H / 2, 3.0],
                grid_size=[W * osf, H * osf, 40], voxel_size=[voxel, voxel, 0.2], out_size_factor=osf, dense_reg=1,
                gaussian_overlap=overlap, max_objs=max_objs, min_radius=min_radius, code_weights=list(CODE_WEIGHTS))


def box_at(cfg, cx, cy, w, l, rng, box_dim=9, z=-1.0, h=1.5):
    """A box whose centre is at (cx, cy) map cells, (w, l) metres."""
    cell = cfg['voxel_size'][0] * cfg['out_size_factor']
    row = [cfg['point_cloud_range'][0] + cx * cell, cfg['point_cloud_range'][1] + cy * cell, z, w, l, h,
           rng.uniform(-3.1, 3.1)]
    return row + list(rng.standard_normal(box_dim - 7))


def random_boxes(cfg, n, rng, box_dim=9, margin=0.0):
    """n boxes with centres up to ``margin`` cells off the map; one in six is large (radii above min_radius)."""
    H, W = map_size(cfg)
    rows = []
    for _ in range(n):
        w, l = (rng.uniform(5.0, 14.0), rng.uniform(8.0, 30.0)) if rng.random() < 1 / 6 else \
            (rng.uniform(0.5, 3.0), rng.uniform(0.5, 12.0))
        rows.append(box_at(cfg, rng.uniform(-margin, W + margin), rng.uniform(-margin, H + margin), w, l, rng, box_dim,
                           z=rng.uniform(-2, 0), h=rng.uniform(0.8, 3)))
    return rows


def _table(ncls):
    return np.array([(t, c) for t, n in enumerate(ncls) for c in range(n)], np.int32).reshape(-1, 2)


def _logits(rng, shape):
    """Logits around -2 with +-20 (clipped on both sides) and exact 0 mixed in."""
    x = (rng.standard_normal(shape) * 2 - 2).astype(np.float32)
    flat = x.reshape(-1)
    at = rng.choice(flat.size, min(flat.size, 3 * max(flat.size // 50, 2)), replace=False)
    for k, v in enumerate((20.0, -20.0, 0.0)):
        flat[at[k::3]] = v
    return x


def _heads(rng, B, H, W, with_velocity):
    return {n: rng.standard_normal((B, k, H, W)).astype(np.float32) for n, k in HEADS[:5 if with_velocity else 4]}


def _rank_rows(labels, label):
    """Rows of the boxes with ``label``, in input order: the r-th of them owns slot r of a one-class task."""
    return np.nonzero(np.asarray(labels) == label)[0]


def _dense(rng):
    ncls = [1, 2, 2, 1, 2, 2]
    cfg = make_cfg(40, 40, 300)
    odd = [-1, 10, 1000]
    lab0 = np.array([0] * 350 + odd * 4 + list(rng.integers(1, 10, 600 - 350 - 12)))
    rng.shuffle(lab0)
    lab1 = np.concatenate([rng.integers(0, 10, 257 - 6), odd * 2])
    rng.shuffle(lab1)
    bx0 = np.array(random_boxes(cfg, 600, rng, margin=3.0), np.float32)
    bx1 = np.array(random_boxes(cfg, 257, rng, margin=3.0), np.float32)
    cars = _rank_rows(lab0, 0)

    def put(slot, cx, cy, w=1.9, l=4.5):             # the car that owns ``slot`` of task 0
        bx0[cars[slot]] = np.array(box_at(cfg, cx, cy, w, l, rng), np.float32)

    put(9, -2.5, 7.5)                                # off the map: slot 9 stays empty (ind 0)
    put(10, 0.4, 0.3)                                # on cell 0, beside the empty slots 9 and 11
    put(11, 5.5, 5.5, w=0.0)                         # zero width
    put(20, 8.5, 8.5, l=-1.0)                        # negative length
    put(21, -0.5, 11.5)                              # a centre in (-1, 0) cells is kept in cell 0
    put(255, 17.3, 22.6)                             # one cell in slots 255 and 256
    put(256, 17.7, 22.2)
    put(40, 30.5, 30.5)                              # and one in slots 40, 270 and 299
    put(270, 30.2, 30.8)
    put(299, 30.6, 30.1)
    boxes = np.concatenate([bx0, bx1])
    labels = np.concatenate([lab0, lab1]).astype(np.int64)
    return dict(ncls=ncls, cfg=cfg, boxes=boxes, labels=labels, offsets=[0, 600, 857])


def _one_task(rng):
    cfg = make_cfg(7, 5, 4, voxel=0.125, osf=4, min_radius=0)
    rows = [box_at(cfg, 3.5, 2.5, 30.0, 30.0, rng),   # a radius beyond the map: clipped on all four sides
            box_at(cfg, 6.5, 0.5, 0.01, 0.01, rng),   # radius 0: a single cell
            box_at(cfg, 1.2, 4.6, 1.0, 2.0, rng)]
    return dict(ncls=[1], cfg=cfg, boxes=np.array(rows, np.float32), labels=np.zeros(3, np.int64), offsets=[0, 3])


def _max_planes(rng):
    ncls = [8] * 8
    cfg = make_cfg(16, 16, 32)
    labels = np.repeat(np.arange(64), 3)
    rng.shuffle(labels)
    return dict(ncls=ncls, cfg=cfg, boxes=np.array(random_boxes(cfg, 192, rng), np.float32),
                labels=labels.astype(np.int64), offsets=[0, 192])


def _wide(rng):
    cfg = make_cfg(300, 3, 16)
    rows, labels = [], []
    for b in range(2):
        rows += [box_at(cfg, 299.5, 2.5, 2.0, 4.0, rng), box_at(cfg, 256.5, 2.2, 2.5, 9.0, rng),
                 box_at(cfg, 255.5, 0.5, 1.0, 1.0, rng), box_at(cfg, 0.5, 2.9, 3.0, 11.0, rng)]
        rows += [box_at(cfg, rng.uniform(200, 300), rng.uniform(0, 3), rng.uniform(0.5, 3), rng.uniform(0.5, 12), rng)
                 for _ in range(14)]
        labels += list(rng.integers(0, 3, 18))
    return dict(ncls=[1, 2], cfg=cfg, boxes=np.array(rows, np.float32), labels=np.array(labels, np.int64),
                offsets=[0, 18, 36])


def _box_dims(rng, box_dim, with_velocity, norm_bbox):
    cfg = make_cfg(12, 10, 8)
    boxes = np.array(random_boxes(cfg, 24, rng, box_dim, margin=1.0), np.float32)
    return dict(ncls=[2, 1], cfg=cfg, boxes=boxes, labels=rng.integers(0, 3, 24).astype(np.int64), offsets=[0, 13, 24],
                with_velocity=with_velocity, norm_bbox=norm_bbox)


def _hm_blocks(rng, no_pos0):
    cfg = make_cfg(300, 300, 32)
    boxes = np.array(random_boxes(cfg, 40, rng), np.float32)
    labels = rng.integers(0, 4, 40).astype(np.int64)
    labels[:4] = [0, 1, 2, 3]
    if no_pos0:
        labels[labels == 0] = 1 + np.arange((labels == 0).sum()) % 3
    return dict(ncls=[1, 3], cfg=cfg, boxes=boxes, labels=labels, offsets=[0, 22, 40])


def _reg_exact(rng):
    cfg = make_cfg(8, 8, 6)
    boxes = np.array(random_boxes(cfg, 10, rng), np.float32)
    boxes[1] = np.array(box_at(cfg, 3.3, 4.4, 2.0, 4.0, rng), np.float32)      # two boxes of task 0 on one cell
    boxes[2] = np.array(box_at(cfg, 3.6, 4.7, 1.8, 4.2, rng), np.float32)
    labels = np.array([1, 0, 0, 1, 0, 0, 1, 1, 0, 1], np.int64)
    grad_outs = [np.zeros((2, 6), np.float32) for _ in range(6)]
    for j, go in enumerate(grad_outs):
        go[:, j] = [1.0, 0.75]
    return dict(ncls=[1, 1], cfg=cfg, boxes=boxes, labels=labels, offsets=[0, 5, 10], reg_grad_outs=grad_outs,
                exact=True)


def _nan_code(rng):
    cfg = make_cfg(8, 8, 4)
    boxes = np.array(random_boxes(cfg, 7, rng), np.float32)
    boxes[2, 7] = np.nan
    return dict(ncls=[1, 2], cfg=cfg, boxes=boxes, labels=np.array([0, 1, 0, 2, 1, 0, 2], np.int64), offsets=[0, 7])


def _inf_dim(rng):
    cfg = make_cfg(9, 7, 4)
    boxes = np.array(random_boxes(cfg, 6, rng), np.float32)
    boxes[1] = np.array(box_at(cfg, 4.5, 3.5, np.inf, 4.0, rng), np.float32)
    return dict(ncls=[1, 1], cfg=cfg, boxes=boxes, labels=np.array([0, 0, 1, 0, 1, 1], np.int64), offsets=[0, 6])


ALL = ('targets', 'hm', 'reg')
CASES = {                                             # name: (builder, the parts it runs)
    'dense': (lambda rng: _dense(rng), ALL),
    'one_task': (lambda rng: _one_task(rng), ALL),
    'max_planes': (lambda rng: _max_planes(rng), ALL),
    'wide': (lambda rng: _wide(rng), ALL),
    'box_dims_11_velocity': (lambda rng: _box_dims(rng, 11, True, True), ALL),
    'box_dims_7_plain': (lambda rng: _box_dims(rng, 7, False, False), ALL),
    'hm_blocks': (lambda rng: _hm_blocks(rng, False), ('targets', 'hm')),
    'hm_blocks_no_positive': (lambda rng: _hm_blocks(rng, True), ('targets', 'hm')),
    'reg_exact': (lambda rng: _reg_exact(rng), ('reg',)),
    'nan_code': (lambda rng: _nan_code(rng), ('targets', 'reg')),
    'inf_dim': (lambda rng: _inf_dim(rng), ('targets', 'hm')),
}


def cases_with(part):
    return [n for n, (_, parts) in CASES.items() if part in parts]


RERUN = ('dense', 'hm_blocks')


def _filled_cells(tg, t, b):
    return tg.ind[t, b][tg.mask[t, b] == 1]


def _expect(name, c):
    tg = c.tg
    T, B, M, C, H, W = tg.shape
    radii = [o[6] for o in tg.objs]
    n = np.diff(c.offsets)
    if name == 'dense':
        assert list(n) == [600, 257] and (c.labels[:600] == 0).sum() == 350 and H * W == 6 * 256 + 64 and M == 300
        assert all(v in c.labels[:600] and v in c.labels[600:] for v in (-1, 10, 1000))
        m, i = tg.mask[0, 0], tg.ind[0, 0]
        assert m[256:].sum() > 20 and m[255] == m[256] == 1 and i[255] == i[256] != 0          # slots past 256
        assert m[40] == m[270] == m[299] == 1 and i[40] == i[270] == i[299]
        assert list(m[9:12]) == [0, 1, 0] and list(i[9:12]) == [0, 0, 0]                       # cell 0 beside empty slots
        assert m[20] == 0 and m[21] == 1 and i[21] % W == 0 and tg.anno[0, 0, 21, 0] < 0
        assert (m == 0).sum() > 10                                                            # centres off the map
        assert len(_filled_cells(tg, 0, 0)) - len(np.unique(_filled_cells(tg, 0, 0))) >= 10    # shared cells
        assert all(tg.mask[t].any() for t in range(T)) and max(radii) > 2
    elif name == 'one_task':
        assert (T, B, H, W, M) == (1, 1, 5, 7, 4) and c.cfg['min_radius'] == 0
        assert radii[0] > 7 and radii[1] == 0 and not (tg.heat[0] == 0).any() and tg.ones[0] == 3
    elif name == 'max_planes':
        assert T == 8 and sum(c.ncls) == 64 and all(h[0, k].max() == 1 for h in tg.heat for k in range(8))
    elif name == 'wide':
        assert (H, W) == (3, 300)
        cells = np.concatenate([_filled_cells(tg, t, b) for t in range(T) for b in range(B)])
        assert (cells % W > 255).sum() > 10 and (cells // W == 2).any() and (cells % W == 299).any()
    elif name.startswith('box_dims'):
        assert c.boxes.shape[1] == (11 if c.with_velocity else 7) and C == (10 if c.with_velocity else 8)
        assert tg.mask.sum() > 10
    elif name.startswith('hm_blocks'):
        sizes = [B * k * H * W for k in c.ncls]
        assert sizes == [180000, 540000] and [-(-s // 2048) for s in sizes] == [88, 264]
        assert sizes[1] % 2048 % 256 == 96
        assert (tg.ones[0] == 0) == (name == 'hm_blocks_no_positive') and tg.ones[1] > 0
    elif name == 'reg_exact':
        assert len(np.unique(_filled_cells(tg, 0, 0))) < len(_filled_cells(tg, 0, 0))
    elif name == 'nan_code':
        assert np.isnan(tg.anno).sum() == 1 and np.isnan(tg.anno[0, 0, 1, 8]) and tg.mask[0, 0, 1] == 1
        assert np.isnan(c.reg[0].out).sum() == 2 and np.isnan(c.reg[0].out[0, [4, 5]]).all()
        assert all(np.isfinite(g).all() for per in c.reg[0].grads for g in per.values())
        cell = int(tg.ind[0, 0, 1])
        assert not c.reg[0].grads[0]['vel'][0, 0].reshape(-1)[cell] and c.reg[0].grads[0]['vel'][0, 1].reshape(-1)[cell]
    elif name == 'inf_dim':
        at = [o for o in tg.objs if o[1] == 0 and o[3] == 1]
        assert len(at) == 1 and at[0][6] == c.cfg['min_radius'] and np.isinf(tg.anno[0, 0, 1, 3])
        assert (tg.heat[0] == 0).any()
    if 'hm' in c.parts:
        clip = np.concatenate([((s < CLIP_LO) | (s > CLIP_HI)).reshape(-1) for s in c.hm.sig])
        x = np.concatenate([a.reshape(-1) for a in c.logits])
        assert (clip & (x > 0)).any() and (clip & (x < 0)).any() and (x == 0).any()
        # no sigmoid near a clip bound: which side a cell is on does not depend on float32 rounding
        s = np.concatenate([a.reshape(-1) for a in c.hm.sig])
        assert np.minimum(np.abs(s / CLIP_LO - 1), np.abs(s / CLIP_HI - 1)).min() > 1e-5
        assert all(r['g==1'].any() or not (g == 1).any() for r, g in zip(heat_regions(c), tg.heat))
    if c.exact:
        # grad_out column 1 (z) alone: the filled slot whose height prediction equals its target gets exactly 0, its
        # neighbour slot of the same task does not; column 5 reaches every code, columns 0..4 only their own heads
        cell = lambda k: int(tg.ind[1, 0, k])                                                   # noqa: E731
        gz = c.reg[1].grads[1]['height'][0, 0].reshape(-1)
        assert tg.mask[1, 0, 0] and tg.mask[1, 0, 1] and cell(0) != cell(1) and gz[cell(1)] == 0 and gz[cell(0)] != 0
        assert all(not c.reg[1].grads[t][n].any() for t in range(T) for n in ('reg', 'dim', 'rot', 'vel'))
        assert all(c.reg[5].grads[t][n].any() for t in range(T) for n, _ in HEADS)


@functools.lru_cache(maxsize=None)
def build(name):
    """The case ``name`` of ``CASES``: its inputs (float32 / int64 arrays), the oracle's targets ``tg``, and the
    oracle's losses ``hm`` and ``reg`` (one per grad_out) on the oracle's targets."""
    # hm_blocks_no_positive shares hm_blocks's seed: the same boxes and logits, only task 0's labels moved away
    rng = np.random.default_rng(20261019 + list(CASES).index(name.replace('_no_positive', '')))
    builder, parts = CASES[name]
    spec = dict(with_velocity=True, norm_bbox=True, parts=parts, reg_grad_outs=None, exact=False)
    spec.update(builder(rng))
    c = SimpleNamespace(name=name, **spec)
    c.offsets = np.array(c.offsets, np.int64)
    c.table = _table(c.ncls)
    c.tg = targets(c.boxes, c.labels, c.offsets, c.table, c.ncls, c.cfg, c.with_velocity, c.norm_bbox)
    T, B, M, C, H, W = c.tg.shape
    c.hm_weight, c.reg_weight = 0.75, 0.25
    c.hm = c.reg = None
    if 'hm' in c.parts:
        c.logits = [_logits(rng, (B, k, H, W)) for k in c.ncls]
        c.hm_grad_out = np.array([1.0 + 0.25 * t for t in range(T)], np.float32)
        c.hm = heatmap_loss(c.logits, c.tg.heat, c.tg.ones, c.hm_weight, c.hm_grad_out)
    if 'reg' in c.parts:
        c.heads = [_heads(rng, B, H, W, c.with_velocity) for _ in range(T)]
        if c.exact:                                   # predictions equal to their targets: the sign is 0
            for t, b, k, code in ((0, 0, 0, 0), (0, 0, 0, 3), (1, 0, 1, 2), (1, 1, 0, 9), (0, 1, 1, 6)):
                assert c.tg.mask[t, b, k]
                head, chan = [(n, j) for n, w in HEADS for j in range(w)][code]
                c.heads[t][head][b, chan].reshape(-1)[c.tg.ind[t, b, k]] = c.tg.anno[t, b, k, code]
        if c.reg_grad_outs is None:
            c.reg_grad_outs = [(0.5 + 0.1 * ((np.arange(T * 6) * 7) % 11)).reshape(T, 6).astype(np.float32)]
        c.reg = [reg_loss(c.heads, c.tg.anno, c.tg.ind, c.tg.mask, c.tg.msum, c.cfg['code_weights'], c.reg_weight, go)
                 for go in c.reg_grad_outs]
    _expect(name, c)
    return c
