"""CPU: ``temporal.stream_align_torch`` (and ``stream_align``, which dispatches to it here) against the numpy float64
oracle of ``tests/stream_align_oracle.py``: the selection rule at every ``head`` and at ``valid`` = 0, 1, K and above K,
the transform against ``feature_transform(frame_poses_torch(...))`` on the same poses, and the argument refusals."""
import numpy as np
import pytest
import torch

from ocrfdet_amd import detector as det_mod
from ocrfdet_amd import temporal
from tests import bev_align_oracle as bo
from tests import stream_align_oracle as so

C, H, W = 3, 8, 12


def operands(S, B, seed=0, dtype=torch.float32):
    s2e, e2g, bda = (torch.from_numpy(a) for a in so.poses(S, B, seed))
    return torch.from_numpy(so.ring(S, B, C, H, W, seed)).to(dtype), s2e, e2g, bda


def run(ring, head, valid, s2e, e2g, bda, **kw):
    return temporal.stream_align_torch(ring, head, torch.tensor(valid, dtype=torch.int32), s2e, e2g, bda, so.INTERVAL,
                                       so.LOWER, **kw)


@pytest.mark.parametrize('S', [1, 2, 4])
def test_selection_rule_and_values_at_every_head(S):
    """``valid`` = (0, 1, K, K + 2) per sample.  A float64 ring separates the rule from the rounding: the torch formulation
    then agrees with the oracle to 1e-10; with the float32 ring it keeps the forward bound of the warp."""
    K, B = S - 1, 4
    valid = [0, 1, K, K + 2]
    ring, s2e, e2g, bda = operands(S, B, seed=S)
    for head in range(S):
        want, want_tf, slot, warped = so.concat(ring.numpy(), head, valid, s2e.numpy(), e2g.numpy(), bda.numpy(),
                                                so.INTERVAL, so.LOWER)
        # the rule itself, spelled out: a sample with v real frames repeats its oldest one
        for g in range(S):
            for b, v in enumerate(valid):
                e = min(K - g, v)
                assert slot[g, b] == (head - e) % S and warped[g, b] == (e > 0)
        got64, tf = run(ring.double(), head, valid, s2e, e2g, bda)
        assert got64.shape == (B, S * C, H, W) and got64.dtype == torch.float64
        assert tf.shape == (K, B, 3, 3) and tf.dtype == torch.float32
        assert np.abs(got64.numpy() - want).max() <= 1e-10
        assert so.within_one_ulp(tf.numpy(), want_tf).all()
        got, _ = run(ring, head, valid, s2e, e2g, bda)
        assert got.dtype == torch.float32
        for g in range(S):
            for b in range(B):
                block = got[b, g * C:(g + 1) * C]
                if not warped[g, b]:
                    assert torch.equal(block, ring[slot[g, b], b]), (head, g, b)
                    if g < K:
                        assert torch.equal(tf[g, b], torch.eye(3))
                else:
                    bound = bo.forward_bound(want_tf[g, b][None], H, W, float(ring[slot[g, b], b].abs().max()))
                    assert np.abs(block.numpy() - want[b, g * C:(g + 1) * C]).max() <= bound, (head, g, b)
        # the dispatching op is the same function on the CPU
        again, tf_again = temporal.stream_align(ring, head, torch.tensor(valid, dtype=torch.int32), s2e, e2g, bda,
                                                so.INTERVAL, so.LOWER)
        assert torch.equal(again, got) and torch.equal(tf_again, tf)


def test_zero_motion_and_align_off_copy():
    S, B = 3, 2
    ring, s2e, e2g, bda = operands(S, B, seed=5)
    # slots 0 and 1 share an ego pose (so.poses): with head = 1 the age-1 transform is the identity up to the mount's
    # millimetres, and with the mounts made equal it is the identity to rounding
    s2e[1] = s2e[0]
    _, tf = run(ring, 1, [2, 2], s2e, e2g, bda)
    assert np.abs(tf[1].numpy() - np.eye(3)).max() <= 1e-6
    out, tf = run(ring, 2, [2, 1], s2e, e2g, bda, align=False)
    assert torch.equal(tf, torch.eye(3).expand(2, B, 3, 3))
    assert torch.equal(out[0], torch.cat([ring[0, 0], ring[1, 0], ring[2, 0]]))
    assert torch.equal(out[1], torch.cat([ring[1, 1], ring[1, 1], ring[2, 1]]))


def test_transform_matches_feature_transform_of_the_frame_poses():
    """The same poses through the batch forward's own chain: ``frame_poses_torch`` on the (B, F, 1) stack [head, source]
    (in float64, so that its result is not rounded on the way) and ``feature_transform`` with the slot's ``bda`` as
    ``bda_adj``."""
    S, B, head = 4, 3, 2
    ring, s2e, e2g, bda = operands(S, B, seed=9)
    _, tf = run(ring, head, [3, 3, 3], s2e, e2g, bda)
    for g in range(S - 1):
        slot = (head - (S - 1 - g)) % S
        stack = lambda t: torch.stack([t[head], t[slot]], 1)[:, :, None].double()      # noqa: E731
        unused3 = torch.zeros(B, 2, 1, 3, 3, dtype=torch.float64)
        s2k, _, _ = det_mod.frame_poses_torch(stack(s2e), stack(e2g), unused3, unused3[..., 0], unused3, unused3,
                                              unused3[..., 0], bda[head].double(), 0)
        want = temporal.feature_transform([s2k[:, 0], s2k[:, 1]], bda[head], so.INTERVAL, so.LOWER, bda_adj=bda[slot])
        assert want.dtype == torch.float64
        assert so.within_one_ulp(tf[g].numpy(), want.numpy()).all(), g


def test_out_view_and_refusals():
    S, B = 2, 2
    ring, s2e, e2g, bda = operands(S, B, seed=3)
    valid = torch.tensor([1, 0], dtype=torch.int32)
    want, _ = temporal.stream_align_torch(ring, 0, valid, s2e, e2g, bda, so.INTERVAL, so.LOWER)
    wide = torch.full((B, S * C + 4, H, W), -7.5)
    ret, _ = temporal.stream_align_torch(ring, 0, valid, s2e, e2g, bda, so.INTERVAL, so.LOWER, out=wide[:, 2:2 + S * C])
    assert ret.data_ptr() == wide[:, 2:].data_ptr() and torch.equal(ret, want)
    assert (wide[:, :2] == -7.5).all() and (wide[:, 2 + S * C:] == -7.5).all()
    args = (s2e, e2g, bda, so.INTERVAL, so.LOWER)
    for op in (temporal.stream_align_torch, temporal.stream_align):
        with pytest.raises(ValueError, match='head'):
            op(ring, S, valid, *args)
        with pytest.raises(ValueError, match='head'):
            op(ring, -1, valid, *args)
        with pytest.raises(ValueError, match='ring'):
            op(ring[0], 0, valid, *args)
        with pytest.raises(ValueError, match='valid'):
            op(ring, 0, valid[:1], *args)
        with pytest.raises(ValueError, match='valid'):
            op(ring, 0, valid.float(), *args)
        with pytest.raises(ValueError, match='sensor2ego0'):
            op(ring, 0, valid, s2e[:1], e2g, bda, so.INTERVAL, so.LOWER)
        with pytest.raises(ValueError, match='bda'):
            op(ring, 0, valid, s2e, e2g, bda[0], so.INTERVAL, so.LOWER)
        with pytest.raises(ValueError, match='out'):
            op(ring, 0, valid, *args, out=wide[:, :S * C + 1])
    # nothing here records a gradient
    out, _ = temporal.stream_align(ring.clone().requires_grad_(True), 0, valid, *args)
    assert not out.requires_grad


def c_boundary_refusals():
    """Argument validation of ``ocrf_bev_stream_align`` alone (nothing is launched, no memory is touched): non-positive
    sizes, ``head`` out of range, a stride below a row, null operands, operands of 2 GiB and intervals that are not
    positive return hipErrorInvalidValue.  ``tests/test_stream_align_gpu.py`` runs it where a launch would be possible."""
    import ctypes
    from ocrfdet_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)
    invalid = 1

    def call(S=2, B=3, C=2, h=8, w=12, head=0, stride=None, interval=(0.8, 0.8), tf_out=p, **ptrs):
        q = dict(ring=p, valid=p, sensor2ego0=p, ego2global0=p, bda=p, out=p)
        q.update(ptrs)
        stride = S * C * h * w if stride is None else stride
        return L.ocrf_bev_stream_align(S, B, C, h, w, q['ring'], head, q['valid'], q['sensor2ego0'], q['ego2global0'],
                                       q['bda'], interval[0], interval[1], -4.8, -3.2, 1, q['out'],
                                       ctypes.c_longlong(stride), tf_out, None)
    for size in ('S', 'B', 'C', 'h', 'w'):
        assert call(**{size: 0}) == invalid and call(**{size: -2}) == invalid, size
    assert call(head=2) == invalid and call(head=-1) == invalid and call(S=1, head=1) == invalid
    assert call(stride=2 * 2 * 8 * 12 - 1) == invalid                             # samples would overlap
    for name in ('ring', 'valid', 'sensor2ego0', 'ego2global0', 'bda', 'out'):
        assert call(**{name: None}) == invalid, name
    assert call(S=8, B=1, C=1 << 12, h=128, w=128) == invalid                      # the ring is exactly 2 GiB
    assert call(S=1 << 15, B=1 << 15, C=1 << 15, h=1 << 15, w=1 << 15, stride=1 << 60) == invalid
    assert call(S=2, B=2, C=80, h=128, w=128, stride=1 << 29) == invalid           # the strided operand reaches 2 GiB
    assert call(interval=(0.0, 0.8)) == invalid and call(interval=(0.8, float('nan'))) == invalid


def test_c_boundary_refuses_bad_arguments():
    c_boundary_refusals()
