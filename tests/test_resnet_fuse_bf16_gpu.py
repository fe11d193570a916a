"""GPU: the four bfloat16 entry points of ``csrc/resnet_fuse.hip`` through ``image_encoder.add_relu`` / ``upsample_add``.

torch's bf16 element-wise ops widen to float32, add once and round once to nearest even; the kernels do the same, so:

* ``add_relu`` forward is ``torch.relu(a + b)`` on bf16 tensors bit for bit, NaN in the same places (which NaN is not
  specified); the backward is ``torch.where(out <= 0, 0, grad_out)`` bit for bit, NaN gradients included (a select).
  The pairs below do not hold -0 + -0: the kernels' ``s < 0 ? 0 : s`` keeps the sum's -0, as the float32 kernels do,
  where torch's ``relu`` on this device returns +0 (the float32 test counts signed zeros as equal for the same reason).
  The kernel tests the float32 sum where torch tests the rounded one; the two have one sign, because a sum of two bf16
  values is a multiple of the smallest bf16 denormal, 2^-133, and so does not round to zero.  The denormal pairs below,
  (-1e-40, 3e-41) and (-2e-40, 1e-40) with their small negative sums among them, are the cases that would show otherwise.
* ``upsample_add`` forward is ``dst + F.interpolate(src, mode='nearest')`` on bf16 tensors bit for bit, with the index
  maps of the float32 kernel (``rule``); a bf16 plane holds the codes 0..256 exactly.
* ``upsample_add`` backward adds the k destinations of a source pixel sequentially in float32 and rounds once to bf16
  (unit roundoff 2^-8): against the float64 sum ``total``, with ``m`` the sum of magnitudes, the error is at most
  ``e32 + 2^-8 (|total| + e32)`` with ``e32 = (k - 1) 2^-24 m`` (the float32 accumulation, Jeannerod and Rump 2013, then
  one rounding of a value within e32 of ``total``).

Sizes: around one 16-byte group of 8 elements, around one chunk of ``kThreads * kGroups`` groups of 8 (8192 elements),
and several chunks with a tail.  Views that start 2 and 8 bytes into their storage take the 2-byte accesses.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ocrfdet_amd import _lib
from ocrfdet_amd import image_encoder as ie

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SIZES = [1, 7, 8, 9, 8191, 8192, 8193, 3 * 8192 + 5]
OFFSETS = [0, 1, 4]                                # elements: aligned, 2 bytes in, 8 bytes in
NAN, INF = float('nan'), float('inf')
# (a, b): inf + (-inf); NaN + x; -0 + 0; sums of float32 denormals (exact, and bf16 denormals themselves); overflow to
# inf of either sign; the ties 1 + 2^-8 (to even: stays 1) and (1 + 2^-7) + 2^-8 (to even: up to 1 + 2^-6), both signs
PAIRS = [(INF, -INF), (-INF, INF), (NAN, 1.0), (1.0, NAN), (NAN, INF), (-0.0, 0.0), (0.0, -0.0), (1e-40, 1e-40),
         (-1e-40, 3e-41), (1e-40, -1e-40), (-2e-40, 1e-40), (3e38, 3e38), (-3e38, -3e38), (3e38, -3e38),
         (1.0, 2.0 ** -8), (1.0 + 2.0 ** -7, 2.0 ** -8), (-1.0, -2.0 ** -8), (-1.0 - 2.0 ** -7, -2.0 ** -8),
         (1.0, -2.0 ** -9), (-1.0, 1.0)]
GRADS = [NAN, INF, -INF, 0.0, -0.0, 1e-40, -1.0, 2.5]


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype == BF16 and torch.equal(bits(a), bits(b))


def same_bits_but_nan_payload(got, want):
    nan = want.isnan()
    return torch.equal(got.isnan(), nan) and torch.equal(bits(got)[~nan], bits(want)[~nan])


def view_at(values, offset):
    """A contiguous bf16 copy of ``values`` that starts ``offset`` elements into its storage."""
    buf = torch.empty(values.numel() + 8, dtype=BF16, device=values.device)
    t = buf[offset:offset + values.numel()].view(values.shape)
    t.copy_(values)
    assert t.is_contiguous() and t.data_ptr() % 16 == 2 * offset
    return t


def scaled_normals(shape, gen, dev):
    """Normals times 2^-20, 1 or 2^20 per element: in a + b the float32 sum itself rounds when the scales differ."""
    x = torch.randn(shape, device=dev, generator=gen)
    e = torch.randint(-1, 2, shape, device=dev, generator=gen).float() * 20
    return x * torch.exp2(e)


def operand(n, seed, dev, offset, column):
    """n bf16 values: scaled normals, with column ``column`` (0 | 1) of PAIRS, or GRADS for column 2, at the head and
    again at the tail, where the tail lanes work."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    vals = scaled_normals((n,), gen, dev)
    sp = torch.tensor(GRADS if column == 2 else [p[column] for p in PAIRS], device=dev)
    m = min(n, sp.numel())
    vals[:m] = sp[:m]
    if n > 2 * sp.numel():
        vals[n - sp.numel():] = sp
    return view_at(vals, offset)


def test_the_special_pairs_survive_the_cast_to_bf16(cuda):
    a = torch.tensor([p[0] for p in PAIRS], device=cuda).bfloat16().float()
    b = torch.tensor([p[1] for p in PAIRS], device=cuda).bfloat16().float()
    s = a + b
    assert int(s.isnan().sum()) == 5 and bool((a[7:11] != 0).all()) and bool((a[7:11].abs() < 1e-38).all())
    assert s[11] == INF and s[12] == -INF
    assert s[14].bfloat16() == 1.0 and s[15].bfloat16() == 1.0 + 2.0 ** -6 and s[14] != 1.0      # the ties are ties


@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('n', SIZES)
def test_add_relu_forward_and_backward_are_torchs_bit_for_bit(cuda, n, offset):
    a, b = operand(n, 2, cuda, offset, 0), operand(n, 3, cuda, offset, 1)
    g = operand(n, 5, cuda, offset, 2)
    a.requires_grad_(True)
    b.requires_grad_(True)
    out = ie.add_relu(a, b)
    want = torch.relu(a.detach() + b.detach())
    assert out.dtype == BF16 and out.shape == a.shape and want.dtype == BF16
    assert same_bits_but_nan_payload(out.detach(), want)
    ga, gb = torch.autograd.grad(out, [a, b], g)
    want_g = torch.where(out.detach() <= 0, torch.zeros_like(g), g)
    assert same_bits(ga, want_g) and same_bits(gb, want_g)
    if n >= len(PAIRS):                            # a NaN out passes the gradient, a zero out stops it
        nan = out.detach().isnan()
        assert bool(nan.any()) and same_bits(ga[nan], g[nan]) and not bool(bits(ga)[out.detach() == 0].ne(0).any())


def test_add_relu_keeps_the_shape_and_two_runs_are_bit_identical(cuda):
    a = torch.randn(2, 5, 7, 9, device=cuda).bfloat16()
    b = torch.randn(2, 5, 7, 9, device=cuda).bfloat16()
    x, y = ie.add_relu(a, b), ie.add_relu(a, b)
    assert x.shape == a.shape and x.is_contiguous() and same_bits(x, y) and same_bits(x, torch.relu(a + b))
    assert float(x.min()) == 0.0


# ------------------------------------------------------------------------------------------------ upsample + add
# (3, 2) -> (6, 4): P = 24, the 16-byte path; (3, 2) -> (3, 4): P = 12, wide for float32 but not for bf16;
# (8, 22) -> (16, 44): P = 704 with W no multiple of 8, groups straddle rows; (48, 88) -> (96, 176): 16896 elements, more
# than one chunk of 8192 per plane
SHAPES = [((1, 1), (3, 5)), ((5, 7), (5, 7)), ((3, 2), (6, 4)), ((3, 2), (3, 4)), ((8, 11), (15, 21)),
          ((8, 22), (16, 44)), ((48, 88), (96, 176))]
BCS = [(1, 1), (2, 3)]


def rule(n_in, n_out):
    """Source index of every destination index: the float32 kernel's rule in numpy float32."""
    d = np.arange(n_out, dtype=np.float32)
    return np.minimum(np.floor(d * (np.float32(n_in) / np.float32(n_out))).astype(np.int64), n_in - 1)


@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('bc', BCS)
@pytest.mark.parametrize('hin,hout', SHAPES)
def test_upsample_add_forward_is_torchs_bit_for_bit(cuda, hin, hout, bc, offset):
    B, C = bc
    gen = torch.Generator(device=cuda).manual_seed(B * 1000 + C)
    dst = view_at(scaled_normals((B, C, *hout), gen, cuda), offset)
    src = view_at(scaled_normals((B, C, *hin), gen, cuda), offset)
    out = ie.upsample_add(dst, src, size=hout)
    assert out.dtype == BF16 and out.shape == dst.shape and out.is_contiguous()
    want = dst + F.interpolate(src, size=hout, mode='nearest')
    assert want.dtype == BF16 and same_bits(out, want)
    if offset:                                     # one operand off a 16-byte boundary is enough for the narrow path
        aligned = view_at(dst, 0)
        assert same_bits(ie.upsample_add(aligned, src, size=hout), want)
    if hout[0] % hin[0] == 0 and hout[1] % hin[1] == 0 and hout[0] // hin[0] == hout[1] // hin[1] > 1:
        assert same_bits(ie.upsample_add(dst, src, scale_factor=hout[0] // hin[0]), want)
    if hin[0] * hin[1] <= 256:                     # the index maps: a source plane that holds its own flat index
        code = torch.arange(hin[0] * hin[1], dtype=torch.float32, device=cuda).view(1, 1, *hin).expand(B, C, *hin)
        maps = ie.upsample_add(view_at(torch.zeros_like(dst), offset), view_at(code, offset), size=hout)
        want_map = (rule(hin[0], hout[0])[:, None] * hin[1] + rule(hin[1], hout[1])[None, :]).astype(np.float32)
        assert np.array_equal(maps.float().cpu().numpy(), np.broadcast_to(want_map, maps.shape))


@functools.lru_cache(maxsize=None)
def backward_reference(hin, hout, B, C):
    """grad_out (bf16 values as float32, seeded) with, in float64, the sum and the sum of magnitudes of every source
    pixel's destinations and their count k."""
    gen = torch.Generator().manual_seed(hash((hin, hout, B, C)) % (1 << 31))
    g = torch.randn(B, C, *hout, generator=gen).bfloat16().float().numpy()
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
def test_upsample_add_backward(cuda, hin, hout, bc):
    B, C = bc
    g_np, total, mags, k = backward_reference(hin, hout, B, C)
    g = torch.from_numpy(g_np).to(cuda).bfloat16()
    gen = torch.Generator(device=cuda).manual_seed(7)
    dst = torch.randn(B, C, *hout, device=cuda, generator=gen).bfloat16()
    src = torch.randn(B, C, *hin, device=cuda, generator=gen).bfloat16()
    runs = []
    for _ in range(2):
        d, s = dst.clone().requires_grad_(True), src.clone().requires_grad_(True)
        gd, gs = torch.autograd.grad(ie.upsample_add(d, s, size=hout), [d, s], g)
        assert gd.untyped_storage().data_ptr() == g.untyped_storage().data_ptr() and gd.shape == g.shape
        assert same_bits(gd, g)                    # the gradient of dst is grad_out itself: no launch, no copy
        assert gs.dtype == BF16 and gs.shape == src.shape
        runs.append(gs)
    assert same_bits(runs[0], runs[1])
    e32 = (k - 1) * 2.0 ** -24 * mags
    bound = e32 + 2.0 ** -8 * (np.abs(total) + e32)
    err = np.abs(runs[0].float().cpu().numpy().astype(np.float64) - total)
    print(f'{hin} -> {hout} B={B} C={C}: k up to {int(k.max())}, max err {err.max():.3e}, max bound {bound.max():.3e}, '
          f'max err / bound {np.max(err[bound > 0] / bound[bound > 0]) if (bound > 0).any() else 0.0:.3f}')
    assert (err <= bound).all()
    # an offset grad_out and grad_src: the same bits
    d, s = dst.clone().requires_grad_(True), src.clone().requires_grad_(True)
    gs_o, = torch.autograd.grad(ie.upsample_add(d, s, size=hout), [s], view_at(g, 1))
    assert same_bits(gs_o, runs[0])
    # the torch formulation under autograd: the same gradients, within the same bound
    d, s = dst.clone().requires_grad_(True), src.clone().requires_grad_(True)
    gd2, gs2 = torch.autograd.grad(ie.upsample_add_torch(d, s, size=hout), [d, s], g)
    assert same_bits(gd2, g)
    diff = np.abs((runs[0].float() - gs2.float()).cpu().numpy().astype(np.float64))
    print(f'    against upsample_add_torch: max diff {diff.max():.3e}')
    assert (diff <= bound).all()


def test_no_host_synchronisation(cuda):
    a = torch.randn(3, 5, 16, 44, device=cuda).bfloat16().requires_grad_(True)
    b = torch.randn(3, 5, 16, 44, device=cuda).bfloat16().requires_grad_(True)
    s = torch.randn(3, 5, 8, 22, device=cuda).bfloat16().requires_grad_(True)

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
    assert a.grad.dtype == BF16 and torch.isfinite(a.grad).all() and same_bits(a.grad, b.grad)
    assert s.grad.dtype == BF16 and float(s.grad.min()) == 4.0


def test_what_still_raises(cuda):
    a = torch.randn(2, 4, 6, 8, device=cuda).bfloat16()
    src = torch.randn(2, 4, 3, 4, device=cuda).bfloat16()
    strided = torch.randn(2, 6, 8, 4, device=cuda).bfloat16().permute(0, 3, 1, 2)
    assert strided.shape == a.shape and not strided.is_contiguous()
    for args in [(a.half(), a.half()), (a.double(), a.double()), (a, a.float()), (a.float(), a), (a, strided),
                 (a.cpu(), a.cpu()), (a, a.cpu()), (a[:0], a[:0]), (a, a[:, :2])]:
        with pytest.raises(_lib.OcrfHipError):
            ie.add_relu(*args)
    for args in [(a.half(), src.half()), (a.double(), src.double()), (a, src.float()), (a.float(), src),
                 (strided, src), (a.cpu(), src.cpu()), (a[:0], src[:0]), (src, a)]:
        with pytest.raises(_lib.OcrfHipError):
            ie.upsample_add(*args, size=tuple(args[0].shape[2:]))
    assert ie.add_relu(a, a).dtype == BF16 and ie.upsample_add(a, src, size=(6, 8)).dtype == BF16
