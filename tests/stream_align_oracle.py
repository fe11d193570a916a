"""What the tests of the streaming alignment share (test_stream_align_host.py, test_stream_align_gpu.py): the selection
rule and the transform from raw poses in numpy float64, the concatenation they give (the warp itself is
``tests/bev_align_oracle.py``'s), the bound on a transform, and the seeded poses.

Nothing here imports the package: the transform is ``gen_grid``'s expression (bevdet.py:322-361) written out with 4 x 4
matrices, ``inv(feat2bev) . ((bda4_h . curr) . inv(bda4_s . adj))[rows, cols (0, 1, 3)] . feat2bev``, for
``curr = inv(E_h) E_h S_h`` and ``adj = inv(E_h) E_s S_s``.  The inverse of an affine map is formed from the inverse of its
3 x 3 block (well conditioned: a rotation, or a rotation times an augmentation) and ``-inv(R) t``, so that the 1e3 m of a
global translation do not enter a pivot.
"""
import math

import numpy as np
import torch

from tests import bev_align_oracle as bo


def affine_inverse(m):
    r = np.linalg.inv(m[:3, :3])
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = r, -r @ m[:3, 3]
    return out


def bda4(a):
    out = np.eye(4)
    out[:3, :3] = a
    return out


def select(age, valid, head, S):
    """(effective age, source slot) of a sample with ``valid`` real history frames."""
    e = min(age, max(int(valid), 0))
    return e, (head - e) % S


def transform(s2e_h, e2g_h, bda_h, s2e_s, e2g_s, bda_s, interval, lower):
    """(3, 3) float64: pixel of the head slot's plane -> pixel of the source slot's plane."""
    g2h = affine_inverse(np.asarray(e2g_h, np.float64))
    curr = g2h @ (np.asarray(e2g_h, np.float64) @ np.asarray(s2e_h, np.float64))
    adj = g2h @ (np.asarray(e2g_s, np.float64) @ np.asarray(s2e_s, np.float64))
    L = (bda4(np.asarray(bda_h, np.float64)) @ curr) @ affine_inverse(bda4(np.asarray(bda_s, np.float64)) @ adj)
    L = L[np.ix_([0, 1, 3], [0, 1, 3])]
    feat2bev = np.array([[interval[0], 0, lower[0]], [0, interval[1], lower[1]], [0, 0, 1]], np.float64)
    return np.linalg.inv(feat2bev) @ L @ feat2bev


def concat(ring, head, valid, s2e, e2g, bda, interval, lower, align=True):
    """The concatenation and what made it, float64:

    * ``out`` (B, S * C, H, W); ``tf`` (K, B, 3, 3), the identity for a copied group;
    * ``slot`` (S, B) int, the source slot of every group (the last row is ``head``); ``warped`` (S, B) bool."""
    ring = np.asarray(ring, np.float64)
    S, B, C, H, W = ring.shape
    K = S - 1
    out = np.zeros((B, S * C, H, W))
    tf = np.tile(np.eye(3), (K, B, 1, 1))
    slot = np.zeros((S, B), np.int64)
    warped = np.zeros((S, B), bool)
    for g in range(S):
        for b in range(B):
            e, s = select(K - g, valid[b], head, S)
            slot[g, b] = s
            if e == 0 or not align:
                out[b, g * C:(g + 1) * C] = ring[s, b]
                continue
            warped[g, b] = True
            tf[g, b] = transform(s2e[head, b], e2g[head, b], bda[head, b], s2e[s, b], e2g[s, b], bda[s, b], interval, lower)
            out[b, g * C:(g + 1) * C] = bo.sample(torch.from_numpy(ring[s, b][None]), tf[g, b][None])[0].numpy()
    return out, tf, slot, warped


def within_one_ulp(got, want):
    """|got - want| <= max(1 float32 ulp of want, 1e-9), elementwise.  Both sides evaluate in float64 and round once:
    they differ by one ulp where the float64 value lies next to a rounding boundary.  The floor: float64 products over
    translations of 1e3 m carry about 1e-12 of error, which matters only where the entry itself is near zero; 1e-9 sits
    well above that and far below a pixel."""
    want32 = np.asarray(want, np.float64).astype(np.float32)
    bound = np.maximum(np.spacing(np.abs(want32)).astype(np.float64), 1e-9)
    return np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) <= bound


# ------------------------------------------------------------------------------------------------ seeded operands
INTERVAL, LOWER = (0.8, 0.8, 8.0), (-4.8, -3.2, -5.0)          # a plane of up to 12 x 8 cells of 0.8 m


def _yaw(deg):
    a = math.radians(deg)
    return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])


def _rigid(rot, trans):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = rot, trans
    return m


def poses(S, B, seed=0):
    """float32 ``sensor2ego0``, ``ego2global0`` (S, B, 4, 4) and ``bda`` (S, B, 3, 3):

    * a nuScenes-like global pose (translations of about 1e3 m, yaw 35 degrees), per sample a little different;
    * per slot an ego motion of a few pixels (up to 2.5 m at 0.8 m per pixel) and a few degrees of yaw, with a little
      pitch and roll so that the full 3 x 3 blocks are exercised;
    * slot 1 (where there is one) has exactly slot 0's ego pose: zero motion between them;
    * the last slot carries a non-identity ``bda`` (a flip, a rotation and a scale), the others the identity;
    * camera 0's mount is not axis-aligned and moves by a few millimetres between the slots."""
    rng = np.random.default_rng(1000 + seed)
    s2e = np.zeros((S, B, 4, 4))
    e2g = np.zeros((S, B, 4, 4))
    bda = np.tile(np.eye(3), (S, B, 1, 1))
    for b in range(B):
        G = _rigid(_yaw(35.0 + b), [612.5 + 300 * b, -1104.25 - 50 * b, 2.5])
        base = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float64)
        mount = _rigid(_yaw(7.0 - 3 * b) @ base, [1.5, 0.1 * b, 1.6])
        for s in range(S):
            a, c = math.radians(rng.uniform(-0.5, 0.5)), math.radians(rng.uniform(-0.5, 0.5))
            tilt = (np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
                    @ np.array([[math.cos(c), 0, math.sin(c)], [0, 1, 0], [-math.sin(c), 0, math.cos(c)]]))
            step = _rigid(_yaw(rng.uniform(-4, 4)) @ tilt, [rng.uniform(-2.5, 2.5), rng.uniform(-1.5, 1.5),
                                                            rng.uniform(-0.05, 0.05)])
            e2g[s, b] = G @ step
            s2e[s, b] = mount @ _rigid(np.eye(3), rng.uniform(-0.003, 0.003, 3))
        if S > 1:
            e2g[1, b] = e2g[0, b]
        bda[S - 1, b] = 1.05 * _yaw(11.0) @ np.diag([1.0, -1.0, 1.0])
    return s2e.astype(np.float32), e2g.astype(np.float32), bda.astype(np.float32)


def ring(S, B, C, H, W, seed=0):
    return np.random.default_rng(2000 + seed).standard_normal((S, B, C, H, W)).astype(np.float32)
