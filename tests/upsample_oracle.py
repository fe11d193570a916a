"""The sampling rule of ``ocrf_upsample_cat_forward`` / ``_backward`` (include/ocrf_hip.h) in numpy float64, written as
loops over the output pixels: independent of torch's ``interpolate`` and of the kernel's tables.

For output index d of ``out = in * scale`` points on an axis: ``n = d (in - 1)``, ``i0 = n // (out - 1)``,
``lambda = (n % (out - 1)) / (out - 1)``, ``i1 = min(i0 + 1, in - 1)``; with ``in = 1`` every lambda is 0.  The value is
``(1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11)``.  The planes (batch, channel) are the only vectorised
axes.
"""
import numpy as np


def taps(n_in, scale):
    """[(i0, i1, lambda)] for every output index of an axis."""
    n_out = n_in * scale
    out = []
    for d in range(n_out):
        if n_in == 1:
            out.append((0, 0, 0.0))
            continue
        n = d * (n_in - 1)
        i0 = n // (n_out - 1)
        out.append((i0, min(i0 + 1, n_in - 1), (n % (n_out - 1)) / (n_out - 1)))
    return out


def upsample(x1, scale):
    """(B, C, H, W) -> float64 (B, C, H * scale, W * scale)."""
    x1 = np.asarray(x1, np.float64)
    B, C, H, W = x1.shape
    ty, tx = taps(H, scale), taps(W, scale)
    out = np.empty((B, C, H * scale, W * scale), np.float64)
    for oy, (y0, y1, ly) in enumerate(ty):
        for ox, (x0, x1_, lx) in enumerate(tx):
            top = (1.0 - lx) * x1[:, :, y0, x0] + lx * x1[:, :, y0, x1_]
            bot = (1.0 - lx) * x1[:, :, y1, x0] + lx * x1[:, :, y1, x1_]
            out[:, :, oy, ox] = (1.0 - ly) * top + ly * bot
    return out


def upsample_cat(x2, x1, scale):
    up = upsample(x1, scale)
    return up if x2 is None else np.concatenate([np.asarray(x2, np.float64), up], 1)


def upsample_transpose(grad_up, scale):
    """The transpose of ``upsample``: (B, C, H * scale, W * scale) -> float64 (B, C, H, W); every output pixel adds its
    gradient, times the weight it read with, to the four input pixels it read."""
    grad_up = np.asarray(grad_up, np.float64)
    B, C, Ho, Wo = grad_up.shape
    H, W = Ho // scale, Wo // scale
    ty, tx = taps(H, scale), taps(W, scale)
    g = np.zeros((B, C, H, W), np.float64)
    for oy, (y0, y1, ly) in enumerate(ty):
        for ox, (x0, x1_, lx) in enumerate(tx):
            v = grad_up[:, :, oy, ox]
            g[:, :, y0, x0] += (1.0 - ly) * (1.0 - lx) * v
            g[:, :, y0, x1_] += (1.0 - ly) * lx * v
            g[:, :, y1, x0] += ly * (1.0 - lx) * v
            g[:, :, y1, x1_] += ly * lx * v
    return g
