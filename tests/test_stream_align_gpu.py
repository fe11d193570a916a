"""GPU: ``ocrf_bev_stream_align`` (csrc/bev_stream_align.hip) through ``temporal.stream_align`` against the numpy float64
oracle of ``tests/stream_align_oracle.py`` and, bit for bit, against the existing warp kernel fed the kernel's own
transforms.

All cases run B = 3 samples with ``valid`` = (0, 1, K): a sample right after a reset (every group a copy of the key
frame), one with a single real history frame (repeated for every older age) and one with a full history.  The poses are
``so.poses``: a nuScenes-like global pose, a few pixels and degrees of ego motion per slot, two slots with the same ego
pose, a non-identity ``bda`` in the last slot.  The oracle of a case is computed once and shared by its checks.
"""
import functools

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib
from ocrfdet_amd import temporal
from tests import bev_align_oracle as bo
from tests import stream_align_oracle as so
from tests import test_stream_align_host as host

pytestmark = pytest.mark.gpu
B = 3

# (K, C, H, W): 5 x 7 is no multiple of 4 (4-byte stores) and C = 3 leaves the second channel block half empty;
# 8 x 12 takes the 16-byte stores
NARROW, WIDE = (1, 3, 5, 7), (3, 2, 8, 12)


@functools.lru_cache(maxsize=None)
def case(K, C, H, W, head, align=True):
    S = K + 1
    valid = [0, min(1, K), K]
    ring = so.ring(S, B, C, H, W, seed=S + head)
    s2e, e2g, bda = so.poses(S, B, seed=S)
    want = so.concat(ring, head, valid, s2e, e2g, bda, so.INTERVAL, so.LOWER, align=align)
    return ring, valid, s2e, e2g, bda, want


def run(cuda, K, C, H, W, head, align=True, out=None):
    ring, valid, s2e, e2g, bda, _ = case(K, C, H, W, head, align)
    t = lambda a: torch.from_numpy(a).to(cuda)                    # noqa: E731
    ring_d = t(ring)
    got, tf = temporal.stream_align(ring_d, head, torch.tensor(valid, dtype=torch.int32, device=cuda), t(s2e), t(e2g),
                                    t(bda), so.INTERVAL, so.LOWER, align=align, out=out)
    return ring_d, got, tf


def check(cuda, K, C, H, W, head, got, tf, ring_d, align=True):
    """Checks 1 to 3 of a result against the shared oracle of its case."""
    ring, valid, _, _, _, (want, want_tf, slot, warped) = case(K, C, H, W, head, align)
    S = K + 1
    assert got.shape == (B, S * C, H, W) and got.dtype == torch.float32
    assert tf.shape == (K, B, 3, 3) and tf.dtype == torch.float32 and tf.is_contiguous()
    # 1. the transforms: one float32 ulp of the oracle's, floor 1e-9 (so.within_one_ulp)
    ok = so.within_one_ulp(tf.cpu().numpy(), want_tf)
    assert ok.all(), np.abs(tf.cpu().numpy() - want_tf)[~ok]
    for g in range(S):
        dst = got[:, g * C:(g + 1) * C]
        copied = [b for b in range(B) if not warped[g, b]]
        for b in copied:
            # 2. a copied group is its source, and its transform the identity
            assert torch.equal(dst[b], ring_d[slot[g, b], b]), (g, b)
            if g < K:
                assert torch.equal(tf[g, b].cpu(), torch.eye(3)), (g, b)
        if len(copied) == B:
            continue
        # 2. a warped group is bit-equal to the existing kernel fed the kernel's own transform
        src = torch.stack([ring_d[slot[g, b], b] for b in range(B)])
        ref = temporal.shift_feature(src, tf[g], out=torch.empty_like(src))
        for b in range(B):
            if warped[g, b]:
                assert torch.equal(dst[b], ref[b]), (g, b)
                # 3. and within the forward's bound of the float64 oracle's warp (tests/test_bev_align_gpu.py)
                bound = bo.forward_bound(want_tf[g, b][None], H, W, float(np.abs(ring[slot[g, b], b]).max()))
                err = float(np.abs(dst[b].cpu().numpy() - want[b, g * C:(g + 1) * C]).max())
                print(f'K={K} head={head} group {g} sample {b}: kernel - oracle {err:.3e} (bound {bound:.3e})')
                assert err <= bound, (g, b, err, bound)
    assert warped[:K].any() == (K > 0 and align)                  # the case does warp something


def test_narrow_plane_with_a_ragged_channel_block(cuda):
    ring_d, got, tf = run(cuda, *NARROW, head=1)
    check(cuda, *NARROW, 1, got, tf, ring_d)


@pytest.mark.parametrize('head', [0, 1, 2, 3])
def test_wide_plane_at_every_head(cuda, head):
    ring_d, got, tf = run(cuda, *WIDE, head=head)
    check(cuda, *WIDE, head, got, tf, ring_d)


def test_out_as_a_channel_slice_and_with_an_odd_stride(cuda):
    K, C, H, W = WIDE
    S, P, sentinel = K + 1, H * W, -12345.5
    _, want, want_tf = run(cuda, *WIDE, head=2)
    # a channel slice of a wider buffer: the stride stays a multiple of 4 floats, the 16-byte stores
    wide = torch.full((B, S * C + 6, H, W), sentinel, device=cuda)
    view = wide[:, 4:4 + S * C]
    assert view.data_ptr() % 16 == 0 and view.stride(0) % 4 == 0
    ring_d, got, tf = run(cuda, *WIDE, head=2, out=view)
    assert got.data_ptr() == view.data_ptr() and torch.equal(got, want) and torch.equal(tf, want_tf)
    assert (wide[:, :4] == sentinel).all() and (wide[:, 4 + S * C:] == sentinel).all()
    check(cuda, *WIDE, 2, got, tf, ring_d)
    # samples S * C * P + 3 floats apart: no multiple of 4, the 4-byte stores; the gaps stay untouched
    stride = S * C * P + 3
    flat = torch.full((B * stride,), sentinel, device=cuda)
    odd = flat.as_strided((B, S * C, H, W), (stride, P, W, 1))
    _, got, tf = run(cuda, *WIDE, head=2, out=odd)
    assert torch.equal(got, want) and torch.equal(tf, want_tf)
    assert (flat.view(B, stride)[:, S * C * P:] == sentinel).all()


def test_align_off_copies_every_group(cuda):
    ring_d, got, tf = run(cuda, *WIDE, head=1, align=False)
    check(cuda, *WIDE, 1, got, tf, ring_d, align=False)
    assert torch.equal(tf.cpu(), torch.eye(3).expand(WIDE[0], B, 3, 3))


def test_no_history_is_a_copy_of_the_key_frame(cuda):
    ring_d, got, tf = run(cuda, 0, 3, 5, 7, head=0)
    assert tf.shape == (0, B, 3, 3) and torch.equal(got, ring_d[0])
    ring_d, got, tf = run(cuda, 0, 2, 8, 12, head=0)
    assert torch.equal(got, ring_d[0])


def test_one_launch_and_two_runs_are_bit_identical(cuda, monkeypatch):
    calls = []
    real = _lib.launch
    monkeypatch.setattr(temporal._lib, 'launch', lambda name, *a, **k: calls.append(name) or real(name, *a, **k))
    first = run(cuda, *WIDE, head=3)
    assert calls == ['ocrf_bev_stream_align']
    second = run(cuda, *WIDE, head=3)
    assert calls == ['ocrf_bev_stream_align'] * 2
    assert torch.equal(first[1], second[1]) and torch.equal(first[2], second[2])
    narrow = run(cuda, *NARROW, head=0), run(cuda, *NARROW, head=0)
    assert torch.equal(narrow[0][1], narrow[1][1]) and torch.equal(narrow[0][2], narrow[1][2])
    assert _lib.lib().ocrf_kernel_name(_lib.K_BEV_STREAM_ALIGN) == b'bev_stream_align_kernel<*>'


def test_no_host_synchronisation(cuda):
    run(cuda, *WIDE, head=0)                                      # warm-up: the library's first call
    ring, valid, s2e, e2g, bda, _ = case(*WIDE, 0)
    args = [torch.from_numpy(a).to(cuda) for a in (ring, s2e, e2g, bda)]
    valid = torch.tensor(valid, dtype=torch.int32, device=cuda)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out, _ = temporal.stream_align(args[0], 0, valid, *args[1:], so.INTERVAL, so.LOWER)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


def test_dispatch_and_c_boundary(cuda, monkeypatch):
    """What the kernel does not take goes to the torch formulation (no launch); the entry point refuses bad arguments."""
    host.c_boundary_refusals()
    ring, valid, s2e, e2g, bda, _ = case(*WIDE, 0)
    t = lambda a: torch.from_numpy(a).to(cuda)                    # noqa: E731
    args = (t(s2e), t(e2g), t(bda), so.INTERVAL, so.LOWER)
    v = torch.tensor(valid, dtype=torch.int32, device=cuda)
    want, want_tf = temporal.stream_align(t(ring), 0, v, *args)
    calls = []
    real = _lib.launch
    monkeypatch.setattr(temporal._lib, 'launch', lambda name, *a, **k: calls.append(name) or real(name, *a, **k))
    for other in (dict(ring=t(ring).double()), dict(valid=v.long()), dict(fused=False)):
        got, tf = temporal.stream_align(other.get('ring', t(ring)), 0, other.get('valid', v), *args,
                                        fused=other.get('fused'))
        assert calls == [] and got.dtype == other.get('ring', t(ring)).dtype
        # both sides keep the forward's bound of the truth, and both round a float64 transform once
        bound = 2 * bo.forward_bound(want_tf.cpu().numpy().reshape(-1, 3, 3), 8, 12, float(np.abs(ring).max()))
        assert float((got.float() - want).abs().max()) <= bound
        assert so.within_one_ulp(tf.cpu().numpy(), want_tf.cpu().numpy()).all()
    with pytest.raises(_lib.OcrfHipError):                       # the entry point itself: head out of range
        _lib.launch('ocrf_bev_stream_align', cuda, 4, B, 2, 8, 12, t(ring), 4, v, *args[:3], 0.8, 0.8, -4.8, -3.2, 1,
                    want, want.stride(0), want_tf)
