"""What the tests of the temporal BEV alignment share (test_bev_align_host.py, test_bev_align_gpu.py): the float64 oracle,
the bounds, the brute-force statement of which output pixels read a source pixel, and the seeded transforms.

A transform is the (2, 3) float32 array of rows 0 and 1 of ``tf``: output pixel (row i, column j) samples the source at
``(sx, sy) = (t00 j + t01 i + t02, t10 j + t11 i + t12)``.

Bounds (the float32 epsilon is 2^-24):

* coordinates: rounding ``tf`` to float32 and the two fmaf per axis move a sample by at most
  ``dx = 4 * 2^-24 (|t00| (W - 1) + |t01| (H - 1) + |t02| + 1)`` (``dy`` alike);
* forward: bilinear interpolation with zero extension is ``2 max|x|``-Lipschitz per axis (so a floor that flips between
  the oracle and the kernel does not matter), and the value's own six roundings give ``8 * 2^-24 max|x|``:
  ``2 max|x| (dx + dy) + 8 * 2^-24 max|x|``;
* backward: a source pixel sums at most ``K`` terms ``weight * g`` whose weights move by ``2 (dx + dy)``:
  ``K max|g| 2 (dx + dy)``, ``K`` the largest number of readers of one source pixel (``readers``).
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24


def rows(tf):
    """(n, 2, 3) float64 of anything that holds (n, 3, 3) or (n, 2, 3) transforms."""
    return np.asarray(tf, np.float64)[:, :2, :]


def coordinate_error(tf, h, w):
    """``dx + dy``, the largest over the transforms of the batch."""
    t = np.abs(rows(tf))
    d = 4 * EPS * (t[:, :, 0] * (w - 1) + t[:, :, 1] * (h - 1) + t[:, :, 2] + 1)
    return float(d.sum(1).max())


def forward_bound(tf, h, w, xmax):
    return 2 * xmax * coordinate_error(tf, h, w) + 8 * EPS * xmax


def backward_bound(tf, h, w, gmax):
    k = max(int(readers(t, h, w).max()) for t in rows(tf))
    return k * gmax * 2 * coordinate_error(tf, h, w)


def sample(x, tf):
    """float64 ``grid_sample(bilinear, zeros, align_corners=True)`` of ``x`` (n, c, h, w) at the transforms ``tf``, on the
    CPU: a torch tensor that depends differentiably on ``x``."""
    n, c, h, w = x.shape
    t = torch.from_numpy(rows(tf))
    xs = torch.arange(w, dtype=torch.float64).view(1, 1, w)
    ys = torch.arange(h, dtype=torch.float64).view(1, h, 1)
    sx = t[:, 0, 0, None, None] * xs + t[:, 0, 1, None, None] * ys + t[:, 0, 2, None, None]
    sy = t[:, 1, 0, None, None] * xs + t[:, 1, 1, None, None] * ys + t[:, 1, 2, None, None]
    grid = torch.stack([sx / max(w - 1, 1) * 2 - 1, sy / max(h - 1, 1) * 2 - 1], -1)
    return F.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=True)


def oracle(x, tf, g):
    """(out, grad_x) as float64 numpy arrays for float arrays ``x``, ``g`` (n, c, h, w)."""
    x = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True)
    out = sample(x, tf)
    out.backward(torch.from_numpy(np.asarray(g, np.float64)))
    return out.detach().numpy(), x.grad.numpy()


def floors(t, h, w):
    """(x0, y0) int64 (h, w): the floors of the float64 sample positions of one (2, 3) transform, clipped to
    [-2, size] (everything outside reads nothing either way)."""
    t = np.asarray(t, np.float64)
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    with np.errstate(all='ignore'):
        sx, sy = t[0, 0] * j + t[0, 1] * i + t[0, 2], t[1, 0] * j + t[1, 1] * i + t[1, 2]
        x0 = np.clip(np.nan_to_num(np.floor(sx), nan=-2.0), -2, w).astype(np.int64)
        y0 = np.clip(np.nan_to_num(np.floor(sy), nan=-2.0), -2, h).astype(np.int64)
    return x0, y0


def taps(t, h, w):
    """The (i, j, qy, qx) of every (output pixel, tap inside the plane) pair of one transform, as four flat arrays."""
    x0, y0 = floors(t, h, w)
    j, i = np.meshgrid(np.arange(w), np.arange(h))
    out = [[], [], [], []]
    for dy in (0, 1):
        for dx in (0, 1):
            qx, qy = x0 + dx, y0 + dy
            m = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            for lst, a in zip(out, (i, j, qy, qx)):
                lst.append(a[m])
    return [np.concatenate(a) for a in out]


def readers(t, h, w):
    """(h, w) int: how many output pixels have source pixel (qy, qx) among their taps."""
    _, _, qy, qx = taps(t, h, w)
    count = np.zeros((h, w), np.int64)
    np.add.at(count, (qy, qx), 1)
    return count


def affine(h, w, angle=0.0, scale=1.0, flip_x=False, flip_y=False, shift=(0.0, 0.0)):
    """(2, 3) float32: rotation by ``angle`` times ``scale`` about the plane's centre, after optional flips, plus
    ``shift`` pixels."""
    a = scale * np.array([[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]])
    a = a @ np.diag([-1.0 if flip_x else 1.0, -1.0 if flip_y else 1.0])
    centre = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
    return np.concatenate([a, (centre - a @ centre + np.asarray(shift, np.float64))[:, None]], 1).astype(np.float32)


def seeded_transforms(h, w, count, seed):
    """Rotations by any angle, flips, scales 0.25 ... 3 (log-uniform) and shifts of up to a plane width."""
    rng = np.random.default_rng(seed)
    return [affine(h, w, angle=rng.uniform(0, 2 * np.pi), scale=float(np.exp(rng.uniform(np.log(0.25), np.log(3.0)))),
                   flip_x=bool(rng.integers(2)), flip_y=bool(rng.integers(2)), shift=rng.uniform(-w, w, 2))
            for _ in range(count)]


IDENTITY = np.array([[1, 0, 0], [0, 1, 0]], np.float32)


def integer_shift(dx, dy):
    return np.array([[1, 0, dx], [0, 1, dy]], np.float32)


def rot90_flip(h, w):
    """Source (x, y) = (i, w - 1 - j) needs a square plane or one that is read partly outside: a quarter turn with a
    flip, integer coefficients."""
    return np.array([[0, 1, 0], [-1, 0, w - 1]], np.float32)


def index_sample(x, t):
    """``x`` (c, h, w) sampled at an integer-valued transform by plain indexing (outside: 0), in x's dtype."""
    c, h, w = x.shape
    x0, y0 = floors(t, h, w)
    m = (x0 >= 0) & (x0 < w) & (y0 >= 0) & (y0 < h)
    out = np.zeros_like(x)
    out[:, m] = x[:, y0[m], x0[m]]
    return out
