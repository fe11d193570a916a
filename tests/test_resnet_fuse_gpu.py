"""GPU: the four entry points of ``csrc/resnet_fuse.hip`` through ``image_encoder.add_relu`` / ``upsample_add``.

* ``add_relu`` forward is ``torch.relu(a + b)`` bit for bit (one float32 addition and a select: nothing to round
  differently), with NaN in the same places; signed zeros count as equal.  The backward is
  ``torch.where(out <= 0, 0, grad_out)`` bit for bit.
* ``upsample_add`` forward is ``dst + F.interpolate(src, mode='nearest')`` bit for bit, and its index maps are the rule
  ``i = min(floor(d * (float(in) / float(out))), in - 1)`` evaluated in numpy float32 on the host.
* ``upsample_add`` backward sums, per source pixel, its k destination pixels sequentially in float32: against the
  float64 sum the error is at most (k - 1) 2^-24 sum|g| over those k values (Jeannerod and Rump, "Improved error bounds
  for inner products in floating-point arithmetic", 2013: the bound holds without higher-order terms); k = 1 is exact.

Sizes: the smallest at which a vector kernel can go wrong (below, at and above one 16-byte group, one wave row of 256
groups, one chunk of the kernel's ``kThreads * kGroups`` groups for both access widths) and one beyond ``kMaxBlocks``
chunks, where the grid-stride loop takes a second turn; the constants are read from the kernels' shared header.
"""
import copy
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ocrfdet_amd import _lib, blocks
from ocrfdet_amd import image_encoder as ie

pytestmark = pytest.mark.gpu

_SRC = os.path.join(os.path.dirname(os.path.abspath(ie.__file__)), 'csrc', 'plane_walk.h')
with open(_SRC) as _f:
    _K = {k: int(v) for k, v in re.findall(r'constexpr int (k\w+) = (\d+);', _f.read())}
GROUPS_PER_CHUNK = _K['kThreads'] * _K['kGroups']                 # 16-byte groups (or floats, unaligned) per chunk
CHUNK4 = 4 * GROUPS_PER_CHUNK
SECOND_TURN = _K['kMaxBlocks'] * CHUNK4 + 3 * CHUNK4 + 5           # vector kernel: > kMaxBlocks chunks; scalar: 4 x that
SIZES = [1, 3, 4, 5, 255, 256, 257, GROUPS_PER_CHUNK - 1, GROUPS_PER_CHUNK, GROUPS_PER_CHUNK + 1, CHUNK4 - 1, CHUNK4,
         CHUNK4 + 1, SECOND_TURN]
SPECIAL = [float('nan'), float('inf'), float('-inf'), 0.0, -0.0, 1e-40, -1e-40, 3e-45, 1.0, -1.0]


def test_constants_are_the_ones_the_sizes_assume():
    assert _K['kThreads'] == 256 and GROUPS_PER_CHUNK == 1024 and CHUNK4 == 4096 and _K['kMaxBlocks'] >= 1


def operand(n, seed, dev, unaligned):
    """n floats: random, with every pair of SPECIAL values meeting at the head (a[i], b[i] = SPECIAL[i // 10], [i % 10]:
    inf - inf, NaN + x, -0 + 0, denormal sums) and again at the tail, where the scalar lanes work."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    buf = torch.empty(n + 1, device=dev)
    t = buf[1:] if unaligned else buf[:n]
    t.normal_(generator=gen)
    sp = torch.tensor(SPECIAL, device=dev)
    pairs = sp.repeat_interleave(len(SPECIAL)) if seed % 2 == 0 else sp.repeat(len(SPECIAL))
    m = min(n, pairs.numel())
    t[:m] = pairs[:m]
    if n > 2 * pairs.numel():
        t[n - pairs.numel():] = pairs
    assert t.is_contiguous() and t.data_ptr() % 16 == (4 if unaligned else 0)
    return t


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def equal_with_nans(got, want):
    nan = want.isnan()
    return torch.equal(got.isnan(), nan) and torch.equal(got[~nan], want[~nan])


@pytest.mark.parametrize('unaligned', [False, True])
@pytest.mark.parametrize('n', SIZES)
def test_add_relu_forward_and_backward_are_torchs_bit_for_bit(cuda, n, unaligned):
    a, b = operand(n, 2, cuda, unaligned), operand(n, 3, cuda, unaligned)
    g = operand(n, 5, cuda, unaligned)
    assert bool(a[:100].isnan().any()) and (n < 100 or bool((a + b)[:100].isnan().sum() > a[:100].isnan().sum()))
    a.requires_grad_(True)
    b.requires_grad_(True)
    out = ie.add_relu(a, b)
    want = torch.relu(a.detach() + b.detach())
    assert out.shape == a.shape and equal_with_nans(out.detach(), want)
    ga, gb = torch.autograd.grad(out, [a, b], g)
    want_g = torch.where(out.detach() <= 0, torch.zeros_like(g), g)
    assert same_bits(ga, want_g) and same_bits(gb, want_g)
    # a NaN out passes the gradient, a zero out (of either sign) stops it
    nan = out.detach().isnan()
    assert bool(nan.any()) and same_bits(ga[nan], g[nan]) and not bool(ga[out.detach() == 0].ne(0).any())
    # the torch formulation under autograd gives the same input gradients
    a2, b2 = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    out2 = ie.add_relu_torch(a2, b2)
    ga2, gb2 = torch.autograd.grad(out2, [a2, b2], g)
    assert equal_with_nans(out.detach(), out2.detach()) and same_bits(ga, ga2) and same_bits(gb, gb2)


def test_add_relu_keeps_the_shape_and_two_runs_are_bit_identical(cuda):
    a, b = torch.randn(2, 5, 7, 9, device=cuda), torch.randn(2, 5, 7, 9, device=cuda)
    x, y = ie.add_relu(a, b), ie.add_relu(a, b)
    assert x.shape == a.shape and x.is_contiguous() and same_bits(x, y) and torch.equal(x, torch.relu(a + b))
    assert float(x.min()) == 0.0


# ------------------------------------------------------------------------------------------------ upsample + add
SHAPES = [((8, 22), (16, 44)), ((1, 1), (3, 5)), ((5, 7), (5, 7)), ((8, 11), (15, 21)), ((5, 3), (9, 7)),
          ((4, 6), (12, 18)), ((22, 8), (43, 15))]
BCS = [(1, 1), (2, 3), (1, 256)]


def rule(n_in, n_out):
    """Source index of every destination index: the kernel's rule in numpy float32."""
    d = np.arange(n_out, dtype=np.float32)
    return np.minimum(np.floor(d * (np.float32(n_in) / np.float32(n_out))).astype(np.int64), n_in - 1)


def interpolate_kwargs(hin, hout):
    """``scale_factor`` where the target is an integer multiple (both spellings reach the kernel), else ``size``."""
    if hout[0] % hin[0] == 0 and hout[1] % hin[1] == 0 and hout[0] // hin[0] == hout[1] // hin[1] > 1:
        return dict(scale_factor=hout[0] // hin[0])
    return dict(size=hout)


@functools.lru_cache(maxsize=None)
def backward_reference(hin, hout, B, C):
    """grad_out (float32, seeded) with, in float64, the sum and the sum of magnitudes of every source pixel's
    destinations and their count k."""
    rng = np.random.default_rng(hash((hin, hout, B, C)) % (1 << 32))
    g = rng.standard_normal((B, C, *hout)).astype(np.float32)
    iy, ix = rule(hin[0], hout[0]), rule(hin[1], hout[1])
    rows = np.zeros((hin[0], hout[0]))
    rows[iy, np.arange(hout[0])] = 1.0
    cols = np.zeros((hout[1], hin[1]))
    cols[np.arange(hout[1]), ix] = 1.0
    g64 = g.astype(np.float64)
    total, mags = rows @ g64 @ cols, rows @ np.abs(g64) @ cols
    k = np.outer(rows.sum(1), cols.sum(0))
    return g, total, mags, k


@pytest.mark.parametrize('bc', BCS)
@pytest.mark.parametrize('hin,hout', SHAPES)
def test_upsample_add_forward_and_backward(cuda, hin, hout, bc):
    B, C = bc
    gen = torch.Generator(device=cuda).manual_seed(B * 1000 + C)
    dst = torch.randn(B, C, *hout, device=cuda, generator=gen)
    src = torch.randn(B, C, *hin, device=cuda, generator=gen)
    kw = interpolate_kwargs(hin, hout)
    out = ie.upsample_add(dst, src, **kw)
    assert out.shape == dst.shape and out.is_contiguous()
    assert same_bits(out, dst + F.interpolate(src, mode='nearest', **kw))
    assert same_bits(out, ie.upsample_add(dst, src, size=hout))
    # the index maps: a source plane that holds its own flat index, added to zeros
    code = torch.arange(hin[0] * hin[1], dtype=torch.float32, device=cuda).view(1, 1, *hin).expand(B, C, *hin)
    maps = ie.upsample_add(torch.zeros_like(dst), code.contiguous(), size=hout).cpu().numpy()
    want = (rule(hin[0], hout[0])[:, None] * hin[1] + rule(hin[1], hout[1])[None, :]).astype(np.float32)
    assert np.array_equal(maps, np.broadcast_to(want, maps.shape))

    g_np, total, mags, k = backward_reference(hin, hout, B, C)
    g = torch.from_numpy(g_np).to(cuda)
    runs = []
    for _ in range(2):
        d, s = dst.clone().requires_grad_(True), src.clone().requires_grad_(True)
        gd, gs = torch.autograd.grad(ie.upsample_add(d, s, **kw), [d, s], g)
        assert gd.untyped_storage().data_ptr() == g.untyped_storage().data_ptr() and gd.shape == g.shape
        assert same_bits(gd, g)                    # the gradient of dst is grad_out itself: no launch, no copy
        runs.append(gs)
    assert same_bits(runs[0], runs[1])
    err = np.abs(runs[0].cpu().numpy().astype(np.float64) - total)
    bound = (k - 1) * 2.0 ** -24 * mags
    print(f'{hin} -> {hout} B={B} C={C}: k up to {int(k.max())}, max err {err.max():.3e}, max bound {bound.max():.3e}, '
          f'max err / bound {np.max(err[bound > 0] / bound[bound > 0]) if (bound > 0).any() else 0.0:.3f}')
    assert (err <= bound).all()
    # the torch formulation under autograd: the same gradients, within the same bound
    d, s = dst.clone().requires_grad_(True), src.clone().requires_grad_(True)
    gd2, gs2 = torch.autograd.grad(ie.upsample_add_torch(d, s, **kw), [d, s], g)
    assert same_bits(gd2, g)
    assert (np.abs((runs[0] - gs2).cpu().numpy().astype(np.float64)) <= bound).all()


def test_upsample_add_on_unaligned_views(cuda):
    """Contiguous views that start 4 bytes into their storage take the 4-byte accesses: same results."""
    hin, hout = (8, 22), (16, 44)                  # a plane of 704 floats: the vector kernel when aligned
    dst, src = torch.randn(2, 3, *hout, device=cuda), torch.randn(2, 3, *hin, device=cuda)
    g = torch.randn(2, 3, *hout, device=cuda)
    off = lambda t: torch.empty(t.numel() + 1, device=cuda)[1:].view(t.shape).copy_(t)      # noqa: E731
    dst_o, src_o, g_o = off(dst), off(src), off(g)
    assert dst_o.data_ptr() % 16 == 4 and src_o.data_ptr() % 16 == 4 and dst_o.is_contiguous()
    want = ie.upsample_add(dst, src, size=hout)
    assert same_bits(ie.upsample_add(dst_o, src, size=hout), want)
    assert same_bits(ie.upsample_add(dst, src_o, size=hout), want)
    s1, s2 = src.clone().requires_grad_(True), src_o.requires_grad_(True)
    g1, = torch.autograd.grad(ie.upsample_add(dst, s1, size=hout), [s1], g)
    g2, = torch.autograd.grad(ie.upsample_add(dst_o, s2, size=hout), [s2], g_o)
    assert same_bits(g1, g2)


def test_no_host_synchronisation(cuda):
    a = torch.randn(3, 5, 16, 44, device=cuda, requires_grad=True)
    b = torch.randn(3, 5, 16, 44, device=cuda, requires_grad=True)
    s = torch.randn(3, 5, 8, 22, device=cuda, requires_grad=True)

    def step():
        ie.upsample_add(ie.add_relu(a, b), s, scale_factor=2).sum().backward()
    step()                                          # warm-up: library, code objects
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        a.grad = b.grad = s.grad = None
        step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.isfinite(a.grad).all() and torch.equal(a.grad, b.grad) and float(s.grad.min()) == 4.0


def test_other_inputs_raise_and_the_modules_take_the_torch_path(cuda, monkeypatch):
    a = torch.randn(2, 4, 6, 8, device=cuda)
    strided = torch.randn(2, 6, 8, 4, device=cuda).permute(0, 3, 1, 2)
    assert strided.shape == a.shape and not strided.is_contiguous()
    for args in [(a, strided), (a.half(), a.half()), (a, a[:, :2]), (a.double(), a.double()), (a, a.cpu()),
                 (a[:0], a[:0])]:
        with pytest.raises(_lib.OcrfHipError):
            ie.add_relu(*args)
    src = torch.randn(2, 4, 3, 4, device=cuda)
    for args, kw in [((a, src), dict()), ((a, src), dict(size=(6, 8), scale_factor=2)), ((a, src), dict(size=(6, 9))),
                     ((a, src), dict(scale_factor=1.5)), ((a, src), dict(scale_factor=3)),
                     ((strided, src), dict(size=(6, 8))), ((a.half(), src.half()), dict(size=(6, 8))),
                     ((a, src[:, :2]), dict(size=(6, 8))), ((src, a), dict(size=(3, 4)))]:
        with pytest.raises(_lib.OcrfHipError):
            ie.upsample_add(*args, **kw)

    calls = []
    real_tail, real_merge = ie.add_relu, ie.upsample_add
    monkeypatch.setattr(blocks, 'add_relu', lambda *x: calls.append('tail') or real_tail(*x))
    monkeypatch.setattr(ie, 'upsample_add', lambda *x, **k: calls.append('merge') or real_merge(*x, **k))
    block = ie.BasicBlock(4, 4).to(cuda).eval()
    fpn = ie.CustomFPN([4, 4], 4, num_outs=1, out_ids=[0]).to(cuda)
    maps = [a, src]
    # the fused ops are exact; the slack is for the convolution library's own choice of algorithm from call to call
    same = lambda x, y: torch.allclose(x, y, rtol=1e-5, atol=1e-6)      # noqa: E731
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    with torch.no_grad():
        block.fused_tail, fpn.fused_merge = True, True
        want_b, want_f = block(a), fpn(maps)
        assert calls == ['tail', 'merge']
        block.fused_tail, fpn.fused_merge = False, False
        assert same(block(a), want_b) and same(fpn(maps), want_f) and len(calls) == 2
        block.fused_tail, fpn.fused_merge = True, True
        got = copy.deepcopy(block).half()(a.half())  # other dtypes: the torch formulation, silently (copies: half()
        assert got.dtype == torch.float16 and len(calls) == 2       # rounds the weights)
        assert copy.deepcopy(fpn).half()([a.half(), src.half()]).dtype == torch.float16 and len(calls) == 2
        fpn.upsample_cfg = dict(mode='bilinear', align_corners=False)
        assert fpn(maps).shape == want_f.shape and len(calls) == 2
        fpn.upsample_cfg = dict(mode='nearest', scale_factor=2.0)
        assert same(fpn(maps), want_f) and calls[2:] == ['merge']
