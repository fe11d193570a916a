"""GPU: ``ocrf_bev_stream_align_bf16`` (csrc/bev_stream_align.hip) through ``temporal.stream_align(keep_bf16=True)``.

The contracts are bit equalities, so nothing here has a tolerance: a copied group is its source plane, a warped group is
``shift_feature(src, tf[g], keep_bf16=True)`` (``ocrf_bev_align_forward_bf16``) on the same bfloat16 planes, ``tf`` is the
float32 kernel's for the same poses, and the whole result is the float32 kernel's on ``ring.float()`` rounded once.  The
float32 kernel is held to the float64 oracle by ``tests/test_stream_align_gpu.py``.

Shapes, poses and the B = 3 / ``valid`` = (0, min(1, K), K) arrangement are that file's: NARROW has P = 35 (2-byte stores,
a ragged channel block), WIDE P = 96 (16-byte stores of 8 pixels).  The float32 reference of a case is computed once and
shared by its checks; nothing writes to it."""
import functools

import pytest
import torch

from ocrfdet_amd import _lib
from ocrfdet_amd import temporal
from tests import stream_align_oracle as so
from tests.test_stream_align_gpu import B, NARROW, WIDE

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = 'cuda:0'


@functools.lru_cache(maxsize=None)
def case(K, C, H, W, head, align=True):
    """The bfloat16 operands on the device, the oracle's ``slot`` / ``warped`` maps, and the float32 kernel's result and
    transforms on the widened ring."""
    S = K + 1
    valid = [0, min(1, K), K]
    t = lambda a: torch.from_numpy(a).to(DEV)                     # noqa: E731
    ring = t(so.ring(S, B, C, H, W, seed=S + head)).to(BF16)
    s2e, e2g, bda = so.poses(S, B, seed=S)
    _, _, slot, warped = so.concat(ring.float().cpu().numpy(), head, valid, s2e, e2g, bda, so.INTERVAL, so.LOWER,
                                   align=align)
    ops = (torch.tensor(valid, dtype=torch.int32, device=DEV), t(s2e), t(e2g), t(bda), so.INTERVAL, so.LOWER)
    want32, want_tf = temporal.stream_align(ring.float(), head, *ops, align=align)
    return ring, ops, slot, warped, want32, want_tf


def run(K, C, H, W, head, align=True, out=None, ring=None):
    r, ops, *_ = case(K, C, H, W, head, align)
    return temporal.stream_align(r if ring is None else ring, head, *ops, align=align, out=out, keep_bf16=True)


def check(K, C, H, W, head, got, tf, align=True):
    ring, _, slot, warped, want32, want_tf = case(K, C, H, W, head, align)
    S = K + 1
    assert got.shape == (B, S * C, H, W) and got.dtype == BF16
    assert tf.shape == (K, B, 3, 3) and tf.dtype == torch.float32 and tf.is_contiguous()
    assert torch.equal(tf, want_tf)                               # the float32 kernel's transforms, bit for bit
    assert torch.equal(got, want32.bfloat16())                    # its result, rounded once
    for g in range(S):
        dst = got[:, g * C:(g + 1) * C]
        src = torch.stack([ring[slot[g, b], b] for b in range(B)])
        ref = temporal.shift_feature(src, tf[g], keep_bf16=True) if warped[g].any() else None
        for b in range(B):
            if warped[g, b]:
                assert ref.dtype == BF16 and torch.equal(dst[b], ref[b]), (g, b)
            else:
                assert torch.equal(dst[b], src[b]), (g, b)
    assert warped[:K].any() == (K > 0 and align)                  # the case warps something ...
    assert (~warped).any()                                        # ... and copies something


def test_narrow_plane_with_a_ragged_channel_block(cuda):
    got, tf = run(*NARROW, head=1)
    check(*NARROW, 1, got, tf)


@pytest.mark.parametrize('head', [0, 1, 2, 3])
def test_wide_plane_at_every_head(cuda, head):
    got, tf = run(*WIDE, head=head)
    check(*WIDE, head, got, tf)


def test_out_as_a_channel_slice_and_with_an_odd_stride(cuda):
    K, C, H, W = WIDE
    S, P, sentinel = K + 1, H * W, -12288.0          # a bfloat16 value
    want, want_tf = run(*WIDE, head=2)
    # a channel slice of a wider buffer: offset and stride multiples of 8 elements, the 16-byte stores
    wide = torch.full((B, S * C + 3, H, W), sentinel, dtype=BF16, device=cuda)
    view = wide[:, 1:1 + S * C]
    assert view.data_ptr() % 16 == 0 and view.stride(0) % 8 == 0 and P % 8 == 0
    got, tf = run(*WIDE, head=2, out=view)
    assert got.data_ptr() == view.data_ptr() and torch.equal(got, want) and torch.equal(tf, want_tf)
    assert (wide[:, :1] == sentinel).all() and (wide[:, 1 + S * C:] == sentinel).all()
    # samples S * C * P + 3 elements apart: the 2-byte stores; the gaps stay untouched
    stride = S * C * P + 3
    flat = torch.full((B * stride,), sentinel, dtype=BF16, device=cuda)
    odd = flat.as_strided((B, S * C, H, W), (stride, P, W, 1))
    got, tf = run(*WIDE, head=2, out=odd)
    assert torch.equal(got, want) and torch.equal(tf, want_tf)
    assert (flat.view(B, stride)[:, S * C * P:] == sentinel).all()


def test_a_ring_that_is_only_8_byte_aligned_gives_the_same_bits(cuda):
    """16-byte stores with element loads in the copied groups: the ``wide_source`` rule."""
    ring = case(*WIDE, 1)[0]
    flat = torch.empty(ring.numel() + 8, dtype=BF16, device=cuda)
    assert flat.data_ptr() % 16 == 0
    shifted = flat[4:4 + ring.numel()].view(ring.shape)
    shifted.copy_(ring)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 8
    want, want_tf = run(*WIDE, head=1)
    got, tf = run(*WIDE, head=1, ring=shifted)
    assert torch.equal(got, want) and torch.equal(tf, want_tf)
    check(*WIDE, 1, got, tf)


def test_align_off_copies_every_group(cuda):
    got, tf = run(*WIDE, head=1, align=False)
    check(*WIDE, 1, got, tf, align=False)
    assert torch.equal(tf.cpu(), torch.eye(3).expand(WIDE[0], B, 3, 3))


def test_no_history_is_a_copy_of_the_key_frame(cuda):
    for shape in ((0, 3, 5, 7), (0, 2, 8, 12)):
        got, tf = run(*shape, head=0)
        assert tf.shape == (0, B, 3, 3) and got.dtype == BF16 and torch.equal(got, case(*shape, 0)[0][0])


def test_one_launch_and_two_runs_are_bit_identical(cuda, monkeypatch):
    case(*WIDE, 3), case(*NARROW, 0)                              # the float32 references, outside the launch count
    calls = []
    real = _lib.launch
    monkeypatch.setattr(temporal._lib, 'launch', lambda name, *a, **k: calls.append(name) or real(name, *a, **k))
    first = run(*WIDE, head=3)
    assert calls == ['ocrf_bev_stream_align_bf16']
    second = run(*WIDE, head=3)
    assert calls == ['ocrf_bev_stream_align_bf16'] * 2
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    narrow = run(*NARROW, head=0), run(*NARROW, head=0)
    assert torch.equal(narrow[0][0], narrow[1][0]) and torch.equal(narrow[0][1], narrow[1][1])
    # without the keyword the bfloat16 ring goes where it went: the torch formulation, no launch
    del calls[:]
    ring, ops, *_ = case(*WIDE, 3)
    plain, _ = temporal.stream_align(ring, 3, *ops)
    assert calls == [] and plain.dtype == BF16


def test_no_host_synchronisation(cuda):
    run(*WIDE, head=0)                                            # warm-up: the library's first call
    ring, ops, *_ = case(*WIDE, 0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out, _ = temporal.stream_align(ring, 0, *ops, keep_bf16=True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()


def test_the_entry_point_refuses_a_head_out_of_range(cuda):
    ring, ops, _, _, _, want_tf = case(*WIDE, 0)
    out = torch.empty(B, 4 * 2, 8, 12, dtype=BF16, device=cuda)
    with pytest.raises(_lib.OcrfHipError, match='hipError_t 1$'):
        _lib.launch('ocrf_bev_stream_align_bf16', cuda, 4, B, 2, 8, 12, ring, 4, *ops[:4], 0.8, 0.8, -4.8, -3.2, 1, out,
                    out.stride(0), torch.empty_like(want_tf))
