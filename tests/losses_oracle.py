"""Cases, float64 evaluation and checker for the fused neck losses of csrc/losses.hip (``depth_labels``,
``depth_semantic_loss``, ``render_losses`` and ``ssim`` of ocrfdet_amd/losses.py).  Shared by
test_losses_oracle_host.py (the cases carry the edges they name, the bar rejects wrong formulations) and
test_losses_oracle_gpu.py (the fused ops through the same checker).

Oracle.  The ``*_torch`` functions of ocrfdet_amd/losses.py on the float32 inputs widened to float64 (the window is the
float32 window widened; ``den`` of the depth target is rounded to float32 once, as in the kernel); the masks come from
``losses.box_mask``, whose result is an integer.  The depth labels are the exception: their oracle is
``depth_labels_torch`` in float32 on the CPU and the condition is bit equality with the NaNs in the same places.

Bar.  ``e_torch`` is the largest absolute error of the float32 ``*_torch`` evaluation on the CPU against the oracle, per
quantity (each loss, each gradient tensor); the fused result must satisfy ``e_fused <= max(2 e_torch, floor)`` with a
floor of 8 * 2^-24 of the oracle gradient's largest magnitude for gradients (``bn_act``'s) and 1e-5 relative for
losses.  Where the oracle is exactly 0 the fused value must be exactly 0, element by element.

Ties.  A sign that flips between float32 and float64 is an error of the size of the gradient itself, so the builders
keep ``|render_depth - target|`` at 1e-4 or more except at the exact ties they place on purpose, and keep every gt depth
either exactly on ``d_min`` / ``d_max``, one float32 step off them, or far from them; they assert both.

Everything is seeded by the case's name; nothing reads a file but the kernel's source, for its constants.
"""
import dataclasses
import functools
import os
import re
import zlib

import numpy as np
import torch

from ocrfdet_amd import _lib, losses

EPS = 2.0 ** -24
D_MIN, D_MAX, STEP = 1.0, 60.0, 0.5
DEPTH_RANGE = (D_MIN, D_MAX)
TIE = 1e-4
W_DEPTH, W_SEMANTIC = 3.0, 25.0
DS_UPSTREAM = ((0.7, -1.3), (1.0, 0.0), (0.0, 1.0))
RENDER_UPSTREAM = (0.7, -1.3, 2.1)
N_CAMS = 3


def kernel_constants():
    """The tile, block and box constants of csrc/losses.hip, read from its source."""
    with open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'csrc', 'losses.hip')) as f:
        src = f.read()
    names = ('kTW', 'kTH', 'kR', 'kThreads', 'kL1Pixels', 'kMaxBoxes')
    return {k: int(re.search(r'\b%s = (\d+)' % k, src).group(1)) for k in names}


K = kernel_constants()


def assert_kernel_constants():
    """The shapes below rest on these; a change in the kernel must break the tests, not thin their coverage."""
    assert K == dict(kTW=64, kTH=16, kR=5, kThreads=256, kL1Pixels=8192, kMaxBoxes=256), K
    assert losses._MAX_BOXES == K['kMaxBoxes'] and 2 * K['kR'] + 1 == 11


def tiles(H, W):
    return -(-H // K['kTH']) * -(-W // K['kTW'])


def l1_blocks(H, W):
    return -(-H * W // K['kL1Pixels'])


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _next(v, up):
    """The float32 neighbour of ``v``."""
    return float(np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)))


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _leaf(t, dtype=torch.float32, device='cpu', requires=True):
    """A copy of a case's tensor to differentiate by: the cases are shared and stay as they were built."""
    return t.detach().to(device=device, dtype=dtype, copy=True).requires_grad_(requires)


# ------------------------------------------------------------------------------------------------ checker
@dataclasses.dataclass
class Figure:
    case: str
    name: str
    e_torch: float
    e_fused: float
    floor: float
    factor: float
    zeros_kept: bool

    @property
    def ok(self):
        return self.zeros_kept and self.e_fused <= max(self.factor * self.e_torch, self.floor)      # NaN fails

    def __str__(self):
        u = self.floor if self.floor > 0 else 1.0
        unit = f'units of the floor {self.floor:.3e}' if self.floor > 0 else 'absolute: the oracle is exactly 0'
        return (f'{self.case} {self.name}: torch {self.e_torch / u:.3f} fused {self.e_fused / u:.3f} ({unit})'
                + ('' if self.zeros_kept else ' NON-ZERO WHERE THE ORACLE IS EXACTLY 0')
                + ('' if self.ok else f' EXCEEDS max({self.factor:g} e_torch, floor)'))


def _cpu64(t):
    return t.detach().double().cpu()


def figures(case, got, factor=2.0):
    """One ``Figure`` per quantity of ``case.want``; ``got`` maps the same names to the results under test (a missing
    or ``None`` entry is an error).  Quantities named ``loss_*`` take the loss floor, the others the gradient floor;
    with ``case.per_element`` the gradients are held element by element to a relative 4 * 2^-24 instead."""
    out = []
    for name, want in case.want.items():
        assert got.get(name) is not None, f'{case.name}: no {name}'
        g, t = _cpu64(got[name]), _cpu64(case.torch32[name])
        assert g.shape == want.shape, (case.name, name, tuple(g.shape), tuple(want.shape))
        zero = want == 0
        zeros_kept = bool((g[zero] == 0).all())
        if name.startswith('loss_'):
            fig = Figure(case.name, name, float((t - want).abs()), float((g - want).abs()), 1e-5 * float(want.abs()),
                         factor, zeros_kept)
        elif case.per_element:
            scale = torch.where(zero, torch.ones_like(want), want.abs())
            fig = Figure(case.name, name + ' (per element, relative)', float(((t - want).abs() / scale).max()),
                         float(((g - want).abs() / scale).max()), 4 * EPS, 0.0, zeros_kept)
        else:
            fig = Figure(case.name, name, float((t - want).abs().max()), float((g - want).abs().max()),
                         8 * EPS * float(want.abs().max()), factor, zeros_kept)
        out.append(fig)
    return out


def check(case, got, factor=None):
    """Print every figure, then assert them all."""
    figs = figures(case, got, case.factor if factor is None else factor)
    for f in figs:
        print(f)
    bad = [str(f) for f in figs if not f.ok]
    assert not bad, '\n'.join(bad)
    return figs


def same_labels(got, want):
    """Bit equality of two (labels, semantic labels) pairs, NaNs in the same places."""
    for a, b in zip(got, want):
        a, b = a.detach().cpu(), b.detach().cpu()
        if a.shape != b.shape or a.dtype != b.dtype or not torch.equal(torch.isnan(a), torch.isnan(b)):
            return False
        if not torch.equal(a.nan_to_num(nan=-1.0).view(torch.int32), b.nan_to_num(nan=-1.0).view(torch.int32)):
            return False
    return True


# ------------------------------------------------------------------------------------------------ depth labels
LABEL_DS = (1, 3, 8, 16)
LABEL_D = (1, 63, 64, 65, 118)
LABEL_KINDS = ('none', 'all_valid', 'sem_outside', 'nan', 'soft')          # the first five patches, in this order
_LN, _LW = 3, 5                                                            # cameras and patches per row


@dataclasses.dataclass(frozen=True)
class LabelCase:
    name: str
    ds: int
    D: int
    cfg: tuple
    gt_depth: torch.Tensor                 # (1, 3, h ds, 5 ds)
    gt_semantic: torch.Tensor
    special: tuple                         # the depths every case holds, as float32 values
    want: tuple                            # depth_labels_torch in float32 on the CPU

    @property
    def rows(self):
        return self.want[0].shape[0]

    def patch(self, t, r):
        """The ds * ds values of patch ``r`` of a gt tensor."""
        return losses._patches(t.reshape(_LN, t.shape[-2], t.shape[-1]), self.ds)[r]


def _unpatch(p, h, ds):
    """(3 h 5, ds ds) patches -> (1, 3, h ds, 5 ds): the inverse of ``losses._patches``."""
    return p.reshape(_LN, h, _LW, ds, ds).permute(0, 1, 3, 2, 4).reshape(1, _LN, h * ds, _LW * ds).contiguous()


@functools.lru_cache(maxsize=None)
def label_case(ds, D, min_rows=0):
    """Finite gt depth / semantic whose patches hold: one of each ``LABEL_KINDS``; every bin edge ``d_min + k step``
    (``d_min`` and ``d_max`` among them) with both float32 neighbours, 0, a negative value and 1e5, once in patches
    without semantics (hard rows) and once in patches with (soft rows); random fill.  B N h w = 15 h is no multiple
    of 4."""
    name = f'labels_ds{ds}_D{D}' + (f'_rows{min_rows}' if min_rows else '')
    gen = _gen(name)
    P = ds * ds
    d0, step = D_MIN, STEP
    d1 = d0 + D * step
    special = []
    for k in range(D + 1):
        e = d0 + k * step                                  # multiples of 0.5: exact in float32
        special += [_next(e, False), e, _next(e, True)]
    special += [0.0, -3.0, 1e5]
    n_sp = -(-len(special) // P)
    rows = max(len(LABEL_KINDS) + 2 * n_sp + 6, min_rows, 45)
    h = -(-rows // (_LN * _LW))
    while (_LN * h * _LW) % 4 == 0:
        h += 1
    R = _LN * h * _LW
    # random fill: 60 % lidar hits between d_min - 1 and d_max + 1, a third of the patches without semantics
    depth = torch.where(torch.rand(R, P, generator=gen) < 0.6,
                        torch.rand(R, P, generator=gen) * (d1 - d0 + 2.0) + (d0 - 1.0), torch.zeros(()))
    sem = ((torch.rand(R, P, generator=gen) < 0.4) & (torch.rand(R, 1, generator=gen) < 0.67)).float()
    inside = torch.rand(P, generator=gen) * (d1 - d0) * 0.98 + d0 + 0.005 * (d1 - d0)
    # the five kinds
    depth[0] = _f32([0.0, d0 - 0.5, d1 + 1.0, -1.0])[torch.arange(P) % 4]
    sem[0] = 0.0
    depth[1], sem[1] = inside, (torch.arange(P) % 2 == 0).float()
    depth[2], sem[2] = inside, 0.0
    depth[2, 0], sem[2, 0] = d1 + 1.0, 1.0
    depth[3], sem[3] = inside, 0.0
    depth[3, 0], sem[3, 0] = d1, 1.0
    depth[4] = d0 + 0.1 + step * (torch.arange(P) % min(D, 7)).float()
    sem[4] = 1.0
    # the special depths, ascending, so that the nearest of each patch is one of them
    sp = _f32(sorted(special))
    pad = torch.full((2 * n_sp * P,), 0.0)
    pad[:len(sp)] = sp
    pad[n_sp * P:n_sp * P + len(sp)] = sp
    a = len(LABEL_KINDS)
    depth[a:a + 2 * n_sp] = pad.reshape(2 * n_sp, P)
    sem[a:a + n_sp] = 0.0
    sem[a + n_sp:a + 2 * n_sp] = (torch.arange(n_sp * P) % 5 != 4).float().reshape(n_sp, P)
    assert torch.isfinite(depth).all()
    gd, gs = _unpatch(depth, h, ds), _unpatch(sem, h, ds)
    cfg = (d0, d1, step)
    want = losses.depth_labels_torch(gd, gs, cfg, D, ds)
    case = LabelCase(name, ds, D, cfg, gd, gs, tuple(float(v) for v in sp), want)
    assert case.rows == R and R % 4 and torch.equal(case.patch(gd, 3), depth[3])
    return case


# ------------------------------------------------------------------------------------------------ depth / semantic BCE
@dataclasses.dataclass(frozen=True)
class DsCase:
    name: str
    BN: int
    h: int
    w: int
    D: int
    labels: torch.Tensor                   # (R, D) float32, NaN rows included
    sem_labels: torch.Tensor               # (R, 2)
    depth: torch.Tensor                    # (BN, D, h, w) predictions
    sem: torch.Tensor                      # (BN, 2, h, w)
    per_element: bool
    factor: float
    want: dict
    torch32: dict

    @property
    def rows(self):
        return self.BN * self.h * self.w

    def in_mask(self):
        return self.labels.max(1).values > 0.0


# name: (BN, h, w, D, rows taken from the label case, predictions)
DS_SPECS = {
    'ds_rows1_single_hard_row': (1, 1, 1, 5, 'one_hard', 'softmax'),
    'ds_rows255': (3, 5, 17, 5, 'first', 'softmax'),
    'ds_rows256': (1, 16, 16, 5, 'first', 'softmax'),
    'ds_rows257_D118': (1, 1, 257, 118, 'first', 'softmax'),
    'ds_rows513': (3, 9, 19, 5, 'first', 'softmax'),
    'ds_rows257_no_row_in_mask': (1, 1, 257, 5, 'unmasked', 'softmax'),
    'ds_exact_0_and_1': (2, 2, 2, 5, 'masked', 'exact'),
}


def ds_run(fn, c, dtype=torch.float32, device='cpu', upstream=DS_UPSTREAM):
    """Losses and, per upstream pair ``i``, the gradients ``g_depth@i`` / ``g_sem@i`` of ``fn`` (a
    ``depth_semantic_loss*`` of ocrfdet_amd/losses.py) on the case's operands as ``dtype`` on ``device``."""
    cast = lambda t: t.to(device=device, dtype=dtype)              # noqa: E731
    d, s = _leaf(c.depth, dtype, device), _leaf(c.sem, dtype, device)
    ls = fn(cast(c.labels), d, cast(c.sem_labels), s, W_DEPTH, W_SEMANTIC)
    out = {'loss_depth': ls[0].detach(), 'loss_sem': ls[1].detach()}
    for i, go in enumerate(upstream):
        gd, gs = torch.autograd.grad(ls, (d, s), [cast(_f32(g)) for g in go], retain_graph=True)
        out[f'g_depth@{i}'], out[f'g_sem@{i}'] = gd, gs
    return out


@functools.lru_cache(maxsize=None)
def ds_case(name):
    BN, h, w, D, take, preds = DS_SPECS[name]
    R = BN * h * w
    gen = _gen(name)
    lab = label_case(3, D, min_rows=R)
    labels, sem_labels = lab.want
    mask = labels.max(1).values > 0.0
    if take == 'one_hard':
        idx = torch.nonzero(mask & (sem_labels[:, 1] == 0))[:1, 0]
    elif take == 'unmasked':
        idx = torch.nonzero(~mask)[:, 0]
        idx = idx[torch.arange(R) % len(idx)]
    elif take == 'masked':
        idx = torch.nonzero(mask)[:R, 0]
    else:
        idx = torch.arange(R)
    labels, sem_labels = labels[idx].contiguous(), sem_labels[idx].contiguous()
    assert labels.shape == (R, D)
    depth = torch.randn(BN, D, h, w, generator=gen).softmax(1)
    sem = torch.randn(BN, 2, h, w, generator=gen).softmax(1)
    if preds == 'exact':
        # a third exactly 0, a third exactly 1; every pairing of {0, 1} with a zero and a non-zero label occurs
        for t in (depth, sem):
            pick = torch.randint(0, 3, t.shape, generator=gen)
            t[pick == 0], t[pick == 1] = 0.0, 1.0
        lab_nchw = labels.reshape(BN, h, w, D).permute(0, 3, 1, 2)
        for p in (0.0, 1.0):
            assert ((depth == p) & (lab_nchw > 0)).any() and ((depth == p) & (lab_nchw == 0)).any()
    c = DsCase(name, BN, h, w, D, labels, sem_labels, depth, sem, preds == 'exact', 2.0, {}, {})
    c.want.update({k: _cpu64(v) for k, v in ds_run(losses.depth_semantic_loss_torch, c, torch.float64).items()})
    c.torch32.update(ds_run(losses.depth_semantic_loss_torch, c, torch.float32))
    return c


def ds_fused(c, device):
    return ds_run(losses.depth_semantic_loss, c, torch.float32, device)


# ------------------------------------------------------------------------------------------------ box masks
MASK_VARIANTS = ('zero', 'full', 'tile_edges', 'wrap', 'empty', 'beyond', 'nan', 'many')
_NAN = -2 ** 62                            # a rectangle bound that stands for a NaN coordinate


def mask_rects(variant, H, W, gen):
    """Rectangles (y0, y1, x0, x1) as Python slice bounds of the (H, W) image, after the -158 shift and before the
    slice rules: what Box2dtoMask's ``mask[y0:y1, x0:x1] = 1`` would be handed."""
    if variant == 'zero':
        return []
    if variant == 'full':
        return [(0, H, 0, W)]
    if variant == 'tile_edges':            # one box ends on y = 16 and x = 64, one starts there, one in mid-tile
        return [(8, 16, 32, 64), (16, H, 64, W), (2, 6, 5, 20)]
    if variant == 'wrap':                  # y0 = -3 wraps to H - 3; y1 is clamped to H
        return [(-3, H + 5, 5, W - 5)]
    if variant == 'empty':                 # y1 <= y0 selects nothing; the other box is ordinary
        return [(9, 4, 5, 30), (5, 12, 10, 50)]
    if variant == 'beyond':
        return [(2, H - 2, W - 10, W + 50)]
    if variant == 'nan':                   # NaN counts as a very negative bound: x0 -> 0, y1 -> 0 (empty)
        return [(2, 10, _NAN, 30), (3, _NAN, 40, 60)]
    if variant == 'many':
        n = K['kMaxBoxes']
        y0, x0 = torch.randint(0, H, (n,), generator=gen), torch.randint(0, W, (n,), generator=gen)
        hh, ww = torch.randint(1, 4, (n,), generator=gen), torch.randint(1, 9, (n,), generator=gen)
        return [(int(a), int(a + b), int(c), int(c + d)) for a, b, c, d in zip(y0, hh, x0, ww)]
    raise KeyError(variant)


def boxes_of(rects, W):
    """(n, 4) float32 boxes (x0, y0, x1, y1) in the 1600-wide frame whose Box2dtoMask bounds are ``rects``: the
    coordinate half a pixel inside the integer it truncates to, so that no rounding of the scaling matters."""
    scale = float(np.float32(W / 1600))

    def coord(v, shift):
        if v == _NAN:
            return float('nan')
        v += shift
        return (v + (0.5 if v >= 0 else -0.5)) / scale
    rows = [[coord(x0, 0), coord(y0, 158), coord(x1, 0), coord(y1, 158)] for y0, y1, x0, x1 in rects]
    return torch.tensor(rows, dtype=torch.float32).reshape(-1, 4)


def slice_mask(rects, H, W):
    """The mask of ``rects`` by Python's own slices."""
    m = np.zeros((H, W), np.float32)
    for y0, y1, x0, x1 in rects:
        m[y0:y1, x0:x1] = 1.0
    return torch.from_numpy(m)


# ------------------------------------------------------------------------------------------------ render losses
SIZES = ((1, 1), (5, 7), (16, 64), (17, 65), (65, 127), (4161, 5))
MASK_SIZES = ((17, 65), (65, 127))


@dataclasses.dataclass(frozen=True)
class RenderSpec:
    H: int
    W: int
    masks: tuple = None                    # per sample a name of MASK_VARIANTS; None: mask off
    depths: tuple = ('textured',)          # per sample: textured | edges | outside
    image: str = 'textured'                # textured | smooth
    factor: float = 2.0

    @property
    def B(self):
        return len(self.depths)


def _render_specs():
    s = {}
    for H, W in SIZES:
        s[f'size_{H}x{W}'] = RenderSpec(H, W, depths=('edges' if H * W >= 16 else 'textured',))
    for H, W in MASK_SIZES:
        for v in MASK_VARIANTS:
            s[f'mask_{v}_{H}x{W}'] = RenderSpec(H, W, masks=(v,))
    s['depth_textured_17x65'] = RenderSpec(17, 65)
    s['depth_outside_17x65'] = RenderSpec(17, 65, depths=('outside',))
    s['smooth_17x65'] = RenderSpec(17, 65, image='smooth')
    s['batch3_17x65'] = RenderSpec(17, 65, masks=('full', 'wrap', 'zero'), depths=('textured', 'edges', 'outside'))
    return s


RENDER_SPECS = _render_specs()
SMOOTH_CASE = 'smooth_17x65'
EDGE_DEPTHS = (D_MIN, _next(D_MIN, False), _next(D_MIN, True), D_MAX, _next(D_MAX, True), _next(D_MAX, False))


@dataclasses.dataclass(frozen=True)
class RenderCase:
    name: str
    spec: RenderSpec
    gt_images: torch.Tensor                # (B + 1, 3, H, W)
    renders: tuple                         # 3 x (B, 3, H, W)
    render_depths: tuple                   # 3 x (B, 1, H, W)
    gt_depth: torch.Tensor                 # (B, 3, H, W)
    cams: tuple
    rects: tuple                           # per sample, or None with the mask off
    boxes: tuple                           # per sample (n, 4); empty with the mask off
    targets: torch.Tensor                  # (B, H, W) float64 depth targets
    want: dict
    torch32: dict
    per_element: bool = False

    @property
    def factor(self):
        return self.spec.factor

    @property
    def use_mask(self):
        return self.rects is not None

    def masks(self):
        H, W = self.spec.H, self.spec.W
        return [losses.box_mask(b, W, H) if self.use_mask else None for b in self.boxes]


def _depth_plane(kind, H, W, gen):
    g = torch.rand(H, W, generator=gen) * (D_MAX - D_MIN - 1.0) + (D_MIN + 0.5)
    if kind == 'edges':                    # the range's ends, one float32 step inside and outside them, far outside
        vals = _f32(list(EDGE_DEPTHS) + [0.0, -2.0, 1e5])
        g.view(-1)[torch.randperm(H * W, generator=gen)[:len(vals)]] = vals
    elif kind == 'outside':                # nothing in range: the target is exactly 0 and den = 0.01
        vals = _f32([0.0, 0.5, _next(D_MIN, False), _next(D_MAX, True), 70.0, -1.0, 1e5])
        g = vals[torch.randint(0, len(vals), (H, W), generator=gen)]
    else:
        assert kind == 'textured'
    return g


def depth_target(plane, dtype=torch.float64):
    """The depth target of ``render_losses_torch`` for one camera plane, restated for the builders' tie checks."""
    g = plane.to(dtype)
    g = g.masked_fill((g < D_MIN) | (g > D_MAX), 0.0)
    lo, hi = g.min(), g.max()
    return (g - lo) / (hi.double() - lo.double() + 0.01).float()


def render_run_torch(c, dtype, masks=None, gt_images=None, depth_range=DEPTH_RANGE, upstream=RENDER_UPSTREAM):
    """``render_losses_torch`` on the case's operands as ``dtype`` on the CPU: losses and the six gradients."""
    cast = lambda t: t.to(dtype)           # noqa: E731
    rs = [_leaf(r, dtype) for r in c.renders]
    rds = [_leaf(r, dtype) for r in c.render_depths]
    masks = c.masks() if masks is None else masks
    gt = cast(c.gt_images if gt_images is None else gt_images)
    ls = losses.render_losses_torch(gt, rs, rds, cast(c.gt_depth), list(c.cams),
                                    [None if m is None else cast(m) for m in masks], depth_range)
    grads = torch.autograd.grad(ls, rs + rds, [cast(_f32(g)) for g in upstream])
    return _render_result(ls, grads)


def _render_result(ls, grads):
    out = {f'loss_{n}': v.detach() for n, v in zip(('color', 'ssim', 'depth'), ls)}
    out.update({n: g for n, g in zip(('g_render0', 'g_render1', 'g_render2', 'g_depth0', 'g_depth1', 'g_depth2'), grads)})
    return out


def render_fused(c, device, requires=(True,) * 6, upstream=RENDER_UPSTREAM):
    """``losses.render_losses`` on ``device``; ``requires`` says which of the three renders and three render depths
    require grad (the others' gradients come back as ``None``)."""
    leaves = [_leaf(t, torch.float32, device, r) for t, r in zip(c.renders + c.render_depths, requires)]
    boxes = list(c.boxes) if c.use_mask else [torch.zeros(0, 4)] * c.spec.B
    ls = losses.render_losses(c.gt_images.to(device), leaves[:3], leaves[3:], c.gt_depth.to(device), list(c.cams), boxes,
                              c.use_mask, DEPTH_RANGE)
    torch.autograd.backward(ls, [_f32(g).to(device) for g in upstream])
    return _render_result(ls, [t.grad for t in leaves])


@functools.lru_cache(maxsize=None)
def render_case(name):
    spec = RENDER_SPECS[name]
    gen = _gen(name)
    B, H, W = spec.B, spec.H, spec.W
    if spec.image == 'smooth':             # e11 - mu1^2 cancels against C2 = 9e-4
        gt = 0.9 + 0.01 * torch.rand(B + 1, 3, H, W, generator=gen)
        renders = tuple(0.9 + 0.01 * torch.rand(B, 3, H, W, generator=gen) for _ in range(3))
    else:
        gt = torch.rand(B + 1, 3, H, W, generator=gen)
        renders = tuple((gt[:B] + 0.1 * torch.randn(B, 3, H, W, generator=gen)).clamp(0, 1) for _ in range(3))
    cams = tuple((2 + b) % N_CAMS for b in range(B))
    # the other cameras hold a narrower textured plane: the wrong camera gives another range
    gt_depth = torch.rand(B, N_CAMS, H, W, generator=gen) * 20.0 + 5.0
    for b in range(B):
        gt_depth[b, cams[b]] = _depth_plane(spec.depths[b], H, W, gen)
    v = gt_depth[torch.arange(B), list(cams)]
    on_edge = torch.zeros_like(v, dtype=torch.bool)
    for e in EDGE_DEPTHS:
        on_edge |= v == e
    assert (on_edge | (((v - D_MIN).abs() > 1e-3) & ((v - D_MAX).abs() > 1e-3))).all()
    targets = torch.stack([depth_target(gt_depth[b, cams[b]]) for b in range(B)])
    rds = [torch.rand(B, 1, H, W, generator=gen) for _ in range(3)]
    for b in range(B):
        if spec.depths[b] == 'outside':    # exact ties: render depth 0 opposite a target of exactly 0
            for rd in rds:
                rd[b, 0][torch.rand(H, W, generator=gen) < 0.25] = 0.0
                rd[b, 0].view(-1)[0] = 0.0
    for rd in rds:                         # off the ties that are not exact
        for _ in range(4):
            near = ((rd[:, 0].double() - targets).abs() < TIE) & (rd[:, 0].double() != targets)
            if not near.any():
                break
            rd[:, 0][near] += 2e-3
        d = (rd[:, 0].double() - targets).abs()
        assert ((d >= TIE) | (d == 0)).all()
        for b in range(B):
            assert bool((d[b] == 0).any()) == (spec.depths[b] == 'outside')
            t32 = depth_target(gt_depth[b, cams[b]], torch.float32)
            assert torch.equal(t32 == rd[b, 0], d[b] == 0), 'an exact tie must be one in float32 as well'
    if spec.masks is None:
        rects, boxes = None, (None,) * B
    else:
        rects = tuple(tuple(mask_rects(m, H, W, gen)) for m in spec.masks)
        boxes = tuple(boxes_of(r, W) for r in rects)
    c = RenderCase(name, spec, gt, renders, tuple(rds), gt_depth, cams, rects, boxes, targets, {}, {})
    c.want.update({k: _cpu64(t) for k, t in render_run_torch(c, torch.float64).items()})
    c.torch32.update(render_run_torch(c, torch.float32))
    return c


# ------------------------------------------------------------------------------------------------ ssim()
@dataclasses.dataclass(frozen=True)
class SsimCase:
    name: str
    img1: torch.Tensor                     # (2, 1, 17, 65)
    img2: torch.Tensor
    upstream: float
    want: dict
    torch32: dict
    per_element: bool = False
    factor: float = 2.0


def ssim_run(fn, c, dtype=torch.float32, device='cpu'):
    a, b = c.img1.to(device=device, dtype=dtype), _leaf(c.img2, dtype, device)
    s = fn(a, b)
    s.backward(_f32(c.upstream).to(device=device, dtype=dtype))
    return {'loss_ssim_value': s.detach(), 'g_img2': b.grad}


@functools.lru_cache(maxsize=None)
def ssim_case():
    """``losses.ssim`` on one channel: K = 1, no mask, no depth term."""
    gen = _gen('ssim_c1')
    a = torch.rand(2, 1, 17, 65, generator=gen)
    b = (a + 0.1 * torch.randn(2, 1, 17, 65, generator=gen)).clamp(0, 1)
    c = SsimCase('ssim_c1_17x65', a, b, -1.3, {}, {})
    c.want.update({k: _cpu64(t) for k, t in ssim_run(losses.ssim_torch, c, torch.float64).items()})
    c.torch32.update(ssim_run(losses.ssim_torch, c))
    return c

