"""numpy float64 oracle for ``ocrfdet_amd.distill``: the group-wise correlation volume with both gradients, and the two
distillation losses with the gradient of the first operand.  Written from the sums in ``include/ocrf_hip.h``; shares no
code with the package.  Every result comes with what a float32 error bound needs: the number of addends ``n`` of each
output element and the sum of their magnitudes."""
import numpy as np

EPS = 1e-8
U = 2.0 ** -24                                  # unit roundoff of float32


def _shift_index(W, d):
    return np.maximum(np.arange(W) - d, 0)


def volume(left, right, G, D):
    """left, right (B, C, H, W) -> (out, n, mag): out[b, g, d, h, w] = sum_c left[b, g Cg + c, h, w] * right[b, g Cg + c,
    h, max(w - d, 0)] in float64, n = Cg addends each, mag the sum of their magnitudes."""
    L, R = np.asarray(left, np.float64), np.asarray(right, np.float64)
    B, C, H, W = L.shape
    Cg = C // G
    out = np.empty((B, G, D, H, W))
    mag = np.empty((B, G, D, H, W))
    for d in range(D):
        prod = (L * R[..., _shift_index(W, d)]).reshape(B, G, Cg, H, W)
        out[:, :, d] = prod.sum(2)
        mag[:, :, d] = np.abs(prod).sum(2)
    return out, Cg, mag


def volume_grads(left, right, grad_out, G, D):
    """-> (gL, nL, magL, gR, nR, magR).  gL[b, c, h, w] = sum_d g[b, g, d, h, w] * right[b, c, h, max(w - d, 0)] (D
    addends); gR[b, c, h, w'] = sum over (w, d) with max(w - d, 0) = w' of g[b, g, d, h, w] * left[b, c, h, w], whose
    number of addends nR (W,) depends on the column: column 0 collects every clamped read."""
    L, R, g = (np.asarray(a, np.float64) for a in (left, right, grad_out))
    B, C, H, W = L.shape
    Cg = C // G
    gc = np.repeat(g, Cg, axis=1).reshape(B, C, D, H, W)           # the group's gradient at every channel
    gL, magL = np.zeros_like(L), np.zeros_like(L)
    gR, magR = np.zeros_like(L), np.zeros_like(L)
    nR = np.zeros(W, np.int64)
    for d in range(D):
        idx = _shift_index(W, d)
        term = gc[:, :, d] * R[..., idx]
        gL += term
        magL += np.abs(term)
        back = gc[:, :, d] * L
        for w in range(W):                                         # scatter to the column that was read
            gR[..., idx[w]] += back[..., w]
            magR[..., idx[w]] += np.abs(back[..., w])
            nR[idx[w]] += 1
    return gL, D, magL, gR, nR, magR


def sum_bound(n, mag):
    """|float32 sum of n products in any order - exact| <= (n + 1) 2^-24 sum|addend| (inputs exact in float64)."""
    return (np.asarray(n, np.float64) + 1.0) * U * mag


def kd_losses(s, t):
    """s, t (B, n) -> (smooth, cos) in float64."""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    a = np.abs(s - t)
    smooth = 0.1 * np.where(a < 1.0, 0.5 * a * a, a - 0.5).mean()
    ns, nt = np.sqrt((s * s).sum(1)), np.sqrt((t * t).sum(1))
    cos = 1.0 - ((s * t).sum(1) / (np.maximum(ns, EPS) * np.maximum(nt, EPS))).mean()
    return smooth, cos


def kd_grad(s, t, g_smooth, g_cos):
    """-> (grad_s, mag): the gradient of ``g_smooth * smooth + g_cos * cos`` with respect to s, as torch's autograd
    gives it through the clamp of the norms, and the sum of the magnitudes of its three terms."""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    B, n = s.shape
    ns, nt = np.sqrt((s * s).sum(1, keepdims=True)), np.sqrt((t * t).sum(1, keepdims=True))
    hs, ht = np.maximum(ns, EPS), np.maximum(nt, EPS)
    st = (s * t).sum(1, keepdims=True)
    t1 = 0.1 * np.clip(s - t, -1.0, 1.0) / (B * n) * g_smooth
    t2 = -g_cos / B * t / (hs * ht)
    with np.errstate(divide='ignore', invalid='ignore'):
        t3 = np.where(ns > EPS, g_cos / B * st * s / (hs * hs * ht * ns), 0.0)
    return t1 + t2 + t3, np.abs(t1) + np.abs(t2) + np.abs(t3)


def loss_bound(want):
    """double accumulation and one float32 rounding, with fourfold slack"""
    return 2.0 ** -22 * max(1.0, abs(float(want)))


def grad_bound(mag):
    return 8.0 * U * mag
