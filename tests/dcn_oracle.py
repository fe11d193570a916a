"""Float64 oracle of the deformable convolution (DCN v1, mmcv 1.x ``deform_conv2d``) and an input generator that places
every sampling coordinate by construction.

The oracle restates the definition in plain numpy, vectorised over the output positions only: per (image, deformable
group, tap) the coordinates, the range test, ``floor``, the four corners; columns, output and the three gradients.

* ``offset`` channel ``g * 2K + 2k`` is the ROW offset of tap ``k = i * kw + j`` of group ``g``, ``2k + 1`` the COLUMN
  offset; input channel ``c`` uses ``g = c // (C // dg)``.
* ``h = ho * stride_h - pad_h + i * dil_h + off_h``; the sample is 0 unless ``h > -1 and w > -1 and h < H and w < W``.
* Inside: ``hl = floor(h)``, ``lh = h - hl``, corners ``(hl | hl + 1, wl | wl + 1)`` with ``(1 - lh | lh) (1 - lw | lw)``,
  a corner outside the map contributing 0.
* ``col[n, c * K + k, ho * Wo + wo]`` is the sample, ``out = weight (*) col`` grouped over ``groups``.
* ``gcol = weight^T grad_out``; ``grad_x`` scatters it through the corner weights; ``grad_offset_h = sum_c gcol *
  ((1 - lw) (x[hl+1, wl] - x[hl, wl]) + lw (x[hl+1, wl+1] - x[hl, wl+1]))`` (w alike); ``grad_weight = grad_out col^T``.

Everything is computed in float64 from the float32 inputs as they are (the offsets are float32 numbers; the coordinate
``base + offset`` is exact in float64).
"""
import functools

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def output_size(H, W, kernel, stride, padding, dilation):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel, stride, padding, dilation
    return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def base_coordinates(H, W, kernel, stride, padding, dilation):
    """Integer coordinates without the offsets: (base_h, base_w), each (K, Ho, Wo)."""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel, stride, padding, dilation
    Ho, Wo = output_size(H, W, kernel, stride, padding, dilation)
    bh = np.zeros((kh * kw, Ho, Wo), np.int64)
    bw = np.zeros((kh * kw, Ho, Wo), np.int64)
    for i in range(kh):
        for j in range(kw):
            bh[i * kw + j] = (np.arange(Ho) * sh - ph + i * dh)[:, None]
            bw[i * kw + j] = (np.arange(Wo) * sw - pw + j * dw)[None, :]
    return bh, bw


def coordinates(offset, H, W, kernel, stride, padding, dilation, dg):
    """(h, w) float64, each (n, dg, K, Ho, Wo), of the float32 ``offset`` (n, dg * 2K, Ho, Wo)."""
    n = offset.shape[0]
    K = kernel[0] * kernel[1]
    bh, bw = base_coordinates(H, W, kernel, stride, padding, dilation)
    off = offset.astype(np.float64).reshape(n, dg, K, 2, *offset.shape[2:])
    with np.errstate(invalid='ignore', over='ignore'):
        return bh + off[:, :, :, 0], bw + off[:, :, :, 1]


def _taps(h, w, H, W):
    """Per position (flat arrays h, w): ``inside`` and, for the four corners in the order (0,0) (0,1) (1,0) (1,1), the
    flat index (clamped), the weight (0 where the corner is not read), and the derivative factors of the weight."""
    with np.errstate(invalid='ignore'):
        inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    hs, ws = np.where(inside, h, 0.0), np.where(inside, w, 0.0)
    hl, wl = np.floor(hs), np.floor(ws)
    lh, lw = hs - hl, ws - wl
    corners = []
    for a in (0, 1):
        for b in (0, 1):
            r, c = hl + a, wl + b
            ok = inside & (r >= 0) & (r <= H - 1) & (c >= 0) & (c <= W - 1)
            idx = (np.clip(r, 0, H - 1) * W + np.clip(c, 0, W - 1)).astype(np.int64)
            wh, ww = (lh if a else 1 - lh), (lw if b else 1 - lw)
            dh, dw = (1.0 if a else -1.0), (1.0 if b else -1.0)      # d weight / d h = dh * ww, d weight / d w = dw * wh
            corners.append((idx, ok, wh * ww * ok, dh * ww * ok, dw * wh * ok))
    return inside, corners


def columns(x, offset, kernel, stride, padding, dilation, dg):
    """col (n, C * K, P) float64."""
    n, C, H, W = x.shape
    K = kernel[0] * kernel[1]
    h, w = coordinates(offset, H, W, kernel, stride, padding, dilation, dg)
    P = h.shape[3] * h.shape[4]
    cpg = C // dg
    xf = x.astype(np.float64).reshape(n, C, H * W)
    col = np.zeros((n, C, K, P))
    for b in range(n):
        for g in range(dg):
            for k in range(K):
                _, corners = _taps(h[b, g, k].ravel(), w[b, g, k].ravel(), H, W)
                for idx, ok, wgt, _, _ in corners:
                    v = np.where(ok[None], xf[b, g * cpg:(g + 1) * cpg][:, idx], 0.0)
                    col[b, g * cpg:(g + 1) * cpg, k] += v * wgt[None]
    return col.reshape(n, C * K, P)


def forward(x, offset, weight, stride, padding, dilation, groups, dg):
    """out (n, Cout, Ho, Wo) float64."""
    n, C, H, W = x.shape
    Cout, _, kh, kw = weight.shape
    Ho, Wo = output_size(H, W, (kh, kw), stride, padding, dilation)
    col = columns(x, offset, (kh, kw), stride, padding, dilation, dg)
    Kd = (C // groups) * kh * kw
    wm = weight.astype(np.float64).reshape(groups, Cout // groups, Kd)
    out = np.einsum('gmk,ngkp->ngmp', wm, col.reshape(n, groups, Kd, Ho * Wo))
    return out.reshape(n, Cout, Ho, Wo)


def backward(x, offset, weight, grad_out, stride, padding, dilation, groups, dg):
    """(grad_x, grad_offset, grad_weight) float64."""
    n, C, H, W = x.shape
    Cout, _, kh, kw = weight.shape
    kernel, K = (kh, kw), kh * kw
    Ho, Wo = output_size(H, W, kernel, stride, padding, dilation)
    P, cpg, Kd = Ho * Wo, C // dg, (C // groups) * K
    wm = weight.astype(np.float64).reshape(groups, Cout // groups, Kd)
    go = grad_out.astype(np.float64).reshape(n, groups, Cout // groups, P)
    col = columns(x, offset, kernel, stride, padding, dilation, dg).reshape(n, groups, Kd, P)
    grad_weight = np.einsum('ngmp,ngkp->gmk', go, col).reshape(weight.shape)
    gcol = np.einsum('gmk,ngmp->ngkp', wm, go).reshape(n, C, K, P)
    h, w = coordinates(offset, H, W, kernel, stride, padding, dilation, dg)
    xf = x.astype(np.float64).reshape(n, C, H * W)
    grad_x = np.zeros((n, C, H * W))
    grad_offset = np.zeros((n, dg, K, 2, P))
    for b in range(n):
        for g in range(dg):
            ch = slice(g * cpg, (g + 1) * cpg)
            for k in range(K):
                _, corners = _taps(h[b, g, k].ravel(), w[b, g, k].ravel(), H, W)
                for idx, ok, wgt, d_h, d_w in corners:
                    gc = gcol[b, ch, k]                                   # (cpg, P)
                    for c in range(cpg):
                        np.add.at(grad_x[b, g * cpg + c], idx, gc[c] * wgt)
                    v = np.where(ok[None], xf[b, ch][:, idx], 0.0)
                    grad_offset[b, g, k, 0] += (gc * v).sum(0) * d_h
                    grad_offset[b, g, k, 1] += (gc * v).sum(0) * d_w
    return grad_x.reshape(x.shape), grad_offset.reshape(offset.shape), grad_weight


# --------------------------------------------------------------------------------------------- inputs
CLASSES = ('fractional', 'integer', 'minus_one', 'at_size', 'just_inside_low', 'just_inside_high', 'far_low', 'far_high',
           'nan', 'plus_inf', 'minus_inf', 'plus_huge', 'minus_huge')
JUST = 2.0 ** -10               # distance of a "just inside" coordinate from the edge of the range: exact in float32


def make_offsets(rng, n, H, W, kernel, stride, padding, dilation, dg, special=True):
    """float32 ``offset`` (n, dg * 2K, Ho, Wo) built from wanted coordinates, and ``classes``: {name: (axis, flat
    indices)} into the (n, dg, K, Ho, Wo) coordinate array of that axis (0: rows, 1: columns).

    Every coordinate is ``integer + fraction`` with the integer in [-2, size] and the fraction in [0.05, 0.95], so that
    floor is the same in float32 and float64 and some taps fall outside; ``special`` then overwrites chosen taps of both
    axes with coordinates that are exactly an integer inside the map, exactly -1, exactly the size, just inside either
    end, far outside (3 max(H, W)), NaN, +-inf and +-1e30."""
    K = kernel[0] * kernel[1]
    bh, bw = base_coordinates(H, W, kernel, stride, padding, dilation)
    shape = (n, dg, K) + bh.shape[1:]
    total = int(np.prod(shape))
    target, classes = [], {}
    for size in (H, W):
        target.append(rng.integers(-2, size + 1, shape) + rng.uniform(0.05, 0.95, shape))
    off = [np.float32(target[0] - bh), np.float32(target[1] - bw)]
    if special:
        far = 3.0 * max(H, W)
        per = max(1, total // 40)
        for axis, size in ((0, H), (1, W)):
            picks = rng.permutation(total)
            base = np.broadcast_to(bh if axis == 0 else bw, shape).reshape(-1)
            flat = off[axis].reshape(-1)
            want = dict(integer=lambda m: rng.integers(0, size, m).astype(np.float64), minus_one=lambda m: np.full(m, -1.0),
                        at_size=lambda m: np.full(m, float(size)), just_inside_low=lambda m: np.full(m, -1.0 + JUST),
                        just_inside_high=lambda m: np.full(m, size - JUST), far_low=lambda m: np.full(m, -far),
                        far_high=lambda m: np.full(m, size + far))
            raw = dict(nan=np.nan, plus_inf=np.inf, minus_inf=-np.inf, plus_huge=1e30, minus_huge=-1e30)
            at = 0
            for name in CLASSES[1:]:
                m = per if name in want else max(1, per // 4)
                idx = picks[at:at + m]
                at += m
                if name in want:
                    flat[idx] = np.float32(want[name](m) - base[idx])      # integers and dyadic fractions: exact
                else:
                    flat[idx] = np.float32(raw[name])
                classes[(name, axis)] = idx
            classes[('fractional', axis)] = picks[at:]
    offset = np.stack(off, 3).reshape(n, dg * 2 * K, *bh.shape[1:]).astype(np.float32)
    return offset, classes


def check_classes(offset, classes, H, W, kernel, stride, padding, dilation, dg):
    """Assert that the float64 coordinates of ``offset`` are what ``make_offsets`` set out to place, and that every
    fractional one has the same floor in float32."""
    h, w = coordinates(offset, H, W, kernel, stride, padding, dilation, dg)
    bh, bw = base_coordinates(H, W, kernel, stride, padding, dilation)
    K = kernel[0] * kernel[1]
    off = offset.reshape(offset.shape[0], dg, K, 2, *offset.shape[2:])
    far = 3.0 * max(H, W)
    for axis, (coord, base, size) in enumerate(((h, bh, H), (w, bw, W))):
        flat = coord.reshape(-1)
        with np.errstate(invalid='ignore', over='ignore'):
            flat32 = (np.broadcast_to(base, coord.shape).astype(np.float32) + off[:, :, :, axis]).reshape(-1)
        get = lambda name: flat[classes[(name, axis)]]    # noqa: E731
        for name in CLASSES:
            assert len(classes[(name, axis)]) > 0, (name, axis)
        v = get('integer')
        assert np.all(v == np.round(v)) and np.all((v >= 0) & (v <= size - 1))
        assert np.all(get('minus_one') == -1.0) and np.all(get('at_size') == size)
        assert np.all(get('just_inside_low') == -1.0 + JUST) and np.all(get('just_inside_high') == size - JUST)
        assert np.all(get('far_low') == -far) and np.all(get('far_high') == size + far)
        assert np.all(np.isnan(get('nan'))) and np.all(get('plus_inf') == np.inf) and np.all(get('minus_inf') == -np.inf)
        assert np.all(get('plus_huge') > 1e29) and np.all(get('minus_huge') < -1e29)
        v = get('fractional')
        frac = v - np.floor(v)
        assert np.all((frac > 0.049) & (frac < 0.951)) and np.all((v > -2) & (v < size + 1))
        assert v.min() < -1 and v.max() > size and ((v > 0) & (v < size - 1)).any()
        # the float32 coordinate the kernels form has the same floor, and the exact classes are exact there too
        assert np.array_equal(np.floor(flat32[classes[('fractional', axis)]]), np.floor(v))
        for name in ('integer', 'minus_one', 'at_size', 'just_inside_low', 'just_inside_high'):
            assert np.array_equal(flat32[classes[(name, axis)]].astype(np.float64), get(name)), name


# --------------------------------------------------------------------------------------------- the shared cases
# (C, Cout, H, W, kernel, stride, padding, dilation, groups, dg), n = 2 each: the smallest shapes that can still go wrong
# (odd sizes, every (groups, dg) pairing, stride, dilation, a 1 x 1 and a non-square kernel) and one plane whose
# positions span more than one workgroup with a ragged tail
CASES = {
    '3x3 pad 1': (8, 8, 5, 7, (3, 3), (1, 1), (1, 1), (1, 1), 1, 1),
    'groups 2': (8, 8, 5, 7, (3, 3), (1, 1), (1, 1), (1, 1), 2, 1),
    'groups 4 dg 2': (8, 8, 5, 7, (3, 3), (1, 1), (1, 1), (1, 1), 4, 2),
    'dg 4': (8, 8, 5, 7, (3, 3), (1, 1), (1, 1), (1, 1), 1, 4),
    'stride 2': (8, 8, 5, 7, (3, 3), (2, 2), (1, 1), (1, 1), 2, 1),
    'dilation 2': (8, 8, 5, 7, (3, 3), (1, 1), (2, 2), (2, 2), 1, 2),
    '1x1': (8, 8, 5, 7, (1, 1), (1, 1), (0, 0), (1, 1), 2, 1),
    '3x1': (8, 8, 5, 7, (3, 1), (1, 1), (1, 0), (1, 1), 1, 1),
    'plane 16x44': (16, 16, 16, 44, (3, 3), (1, 1), (1, 1), (1, 1), 4, 1),
}


@functools.lru_cache(maxsize=None)
def problem(name, n=2):
    """(x, offset, weight, grad_out float32 numpy, classes, geometry) of a case, seeded by its name.  Shared: do not
    write into the arrays."""
    C, Cout, H, W, kernel, stride, padding, dilation, groups, dg = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    offset, classes = make_offsets(rng, n, H, W, kernel, stride, padding, dilation, dg)
    x = rng.standard_normal((n, C, H, W)).astype(np.float32)
    weight = rng.standard_normal((Cout, C // groups) + kernel).astype(np.float32)
    grad_out = rng.standard_normal((n, Cout) + offset.shape[2:]).astype(np.float32)
    for a in (x, offset, weight, grad_out):
        a.setflags(write=False)
    return x, offset, weight, grad_out, classes, (stride, padding, dilation, groups, dg)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(out, grad_x, grad_offset, grad_weight) float64 of a case, computed once."""
    x, offset, weight, grad_out, _, geo = problem(name)
    return (forward(x, offset, weight, *geo),) + backward(x, offset, weight, grad_out, *geo)
