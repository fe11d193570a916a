"""GPU: the bfloat16 forms of ``upsample_cat`` (csrc/upsample_cat.hip) and of the temporal alignment (csrc/bev_align.hip),
and the two opt-in switches that use them (``keep_bf16``, ``BEVEncoder.autocast_bf16``).

The contract: a ``*_bf16`` kernel returns, bit for bit, what the float32 kernel returns on the same operands widened to
float32, rounded once to bfloat16 to nearest even: ``op(x.float(), ...).bfloat16()``, and the same for the backwards
with ``grad_out.float()``.  The float32 kernels have their own tests against float64 oracles
(test_upsample_cat_gpu.py, test_bev_align_gpu.py); here the bf16 kernels are held to the same oracles directly as well,
at the float32 bound plus half a bf16 ulp of the result: ``|got - want| <= b + 2^-8 (|want| + b)``.

Inputs are seeded normals rounded to bf16 with a few -0.0, +-1e-30, zeros and +-3e38 among them.  The 3e38 stand in one
(sample, channel) plane of a tensor, of opposite signs and far apart, so that no float32 sum overflows and no NaN arises
(which NaN a kernel returns is not specified); the oracle bounds are taken per plane from that plane's own largest
magnitude, so every other plane is held to the bound of ordinary values.
"""
import functools
import json

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib, bev_encoder, center_head, plane_ops, temporal
from tests import bev_align_oracle as bo
from tests import upsample_oracle as uo

from .test_bev_align_gpu import frames, poses
from .test_center_head_host import boxes, make_head

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
HALF_ULP = 2.0 ** -8                               # half a bf16 ulp of v is at most 2^-8 |v|


def autocast():
    return torch.autocast('cuda', dtype=BF16)


def special(shape, seed):
    """A bf16 CPU tensor (B, C, H, W): seeded normals with -0.0, +-1e-30 and zeros sprinkled in, and a +3e38 and a
    -3e38 in ONE of its planes, placed so that they never meet in one sum (the first and the last element of the plane
    where it has four elements or more, else one of them alone)."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape).astype(np.float32)
    flat = a.reshape(-1)
    n = flat.size
    for value in (-0.0, 0.0, 1e-30, -1e-30):
        flat[rng.choice(n, size=min(3, max(1, n // 16)), replace=False)] = value
    planes = a.reshape(shape[0] * shape[1], -1)
    p = int(rng.integers(len(planes)))
    planes[p, 0] = 3e38
    if planes.shape[1] >= 4:
        planes[p, -1] = -3e38
    t = torch.from_numpy(a).to(BF16)
    assert torch.isfinite(t).all()
    return t


def same_bits(a, b):
    return (a.dtype == b.dtype == BF16 and a.shape == b.shape
            and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)))


def plane_max(t):
    """max|t| of every (sample, channel) plane as a float64 (B, C, 1, 1) array."""
    return t.detach().abs().double().amax((2, 3), keepdim=True).cpu().numpy()


def within(got, want, bound, what):
    """``|got - want| <= bound + 2^-8 (|want| + bound)`` elementwise, ``bound`` broadcastable."""
    got = got.detach().double().cpu().numpy()
    err, lim = np.abs(got - want), bound + HALF_ULP * (np.abs(want) + bound)
    worst = float((err / np.maximum(lim, 1e-300)).max())
    print(f'{what}: largest |got - want| / bound = {worst:.3f}')
    assert (err <= lim).all(), f'{what}: |got - want| reaches {worst:.3f} of its bound'


@pytest.fixture
def launches(monkeypatch):
    """The names of the library's entry points as they are launched."""
    names = []
    real = _lib.launch
    monkeypatch.setattr(_lib, 'launch', lambda name, *a, **k: names.append(name) or real(name, *a, **k))
    return names


# ------------------------------------------------------------------------------------------------ upsample_cat
UPSAMPLE_CASES = {                                 # (B, C2, C1, Hin, Win, scale)
    'a: V = 8, width 12': (2, 3, 5, 3, 3, 4),
    'b: P = 135, V = 1': (2, 2, 3, 3, 5, 3),
    'c: C2 = 0, two chunks': (1, 0, 4, 48, 48, 2),
    'd: one input pixel': (1, 1, 2, 1, 1, 8),
    'd: one input row': (1, 1, 2, 1, 4, 2),
    'e: scale 1': (2, 2, 3, 4, 6, 1),
    'g: 4096 units on 2048 workgroups': (2, 1024, 1024, 2, 2, 2),
}


@functools.lru_cache(maxsize=None)
def upsample_operands(name):
    """(x2 | None, x1, grad_out) of a case as bf16 CPU tensors."""
    B, C2, C1, Hin, Win, scale = UPSAMPLE_CASES[name]
    seed = sum(ord(ch) for ch in name)
    x2 = special((B, C2, Hin * scale, Win * scale), seed) if C2 else None
    return x2, special((B, C1, Hin, Win), seed + 1), special((B, C2 + C1, Hin * scale, Win * scale), seed + 2)


def run_upsample(x2, x1, g, scale):
    """(out, grad_x2 | None, grad_x1) of ``upsample_cat`` in the dtype of the operands."""
    x1 = x1.clone().requires_grad_(True)
    x2 = None if x2 is None else x2.clone().requires_grad_(True)
    out = plane_ops.upsample_cat(x2, x1, scale)
    out.backward(g)
    return out.detach(), None if x2 is None else x2.grad, x1.grad


@pytest.mark.parametrize('name', list(UPSAMPLE_CASES))
def test_upsample_cat_is_the_float32_kernel_rounded_once(cuda, launches, name):
    scale = UPSAMPLE_CASES[name][5]
    C2 = UPSAMPLE_CASES[name][1]
    x2, x1, g = (None if t is None else t.to(cuda) for t in upsample_operands(name))
    out, g2, g1 = run_upsample(x2, x1, g, scale)
    assert launches == ['ocrf_upsample_cat_forward_bf16', 'ocrf_upsample_cat_backward_bf16']
    want, _, want1 = run_upsample(None if x2 is None else x2.float(), x1.float(), g.float(), scale)
    assert launches[2:] == ['ocrf_upsample_cat_forward', 'ocrf_upsample_cat_backward']
    assert out.is_contiguous() and same_bits(out, want.bfloat16())
    assert same_bits(g1, want1.bfloat16())
    if C2:
        assert same_bits(out[:, :C2], x2) and same_bits(g2, g[:, :C2])             # copied: the bits themselves
    # twice: the same bits
    again = run_upsample(x2, x1, g, scale)
    assert same_bits(again[0], out) and same_bits(again[2], g1)


def test_upsample_cat_views_at_an_odd_offset_take_the_narrow_accesses(cuda):
    """Case (a), an 8-divisible plane, with x2 and the output starting one element (2 bytes) into larger buffers: the
    entry point must take V = 1.  Same bits, and the elements around the output stay as they were."""
    name = 'a: V = 8, width 12'
    B, C2, C1, Hin, Win, scale = UPSAMPLE_CASES[name]
    x2, x1, _ = (t.to(cuda) for t in upsample_operands(name))
    want = plane_ops.upsample_cat(x2, x1, scale)
    sentinel = -12288.0
    x2_buf = torch.zeros(x2.numel() + 8, dtype=BF16, device=cuda)
    x2_off = x2_buf[1:1 + x2.numel()].view(x2.shape).copy_(x2)
    out_buf = torch.full((want.numel() + 8,), sentinel, dtype=BF16, device=cuda)
    out_off = out_buf[1:1 + want.numel()].view(want.shape)
    assert x2_off.data_ptr() % 16 == 2 and out_off.data_ptr() % 16 == 2 and want.shape[2] * want.shape[3] % 8 == 0
    _lib.launch('ocrf_upsample_cat_forward_bf16', cuda, B, C2, C1, Hin, Win, scale, x2_off, x1, out_off)
    assert same_bits(out_off, want)
    assert float(out_buf[0]) == sentinel and (out_buf[1 + want.numel():] == sentinel).all()
    # an aligned output with x2 alone off the boundary
    assert same_bits(plane_ops.upsample_cat(x2_off, x1, scale), want)


@pytest.mark.parametrize('name', ['a: V = 8, width 12', 'b: P = 135, V = 1', 'c: C2 = 0, two chunks', 'd: one input row'])
def test_upsample_cat_against_the_float64_oracle(cuda, name):
    """The float32 bounds of test_upsample_cat_gpu.py (1e-6 max|x1| forward, (2 scale + 1)^2 2^-23 max|grad_out|
    backward), per plane, plus half a bf16 ulp."""
    B, C2, C1, Hin, Win, scale = UPSAMPLE_CASES[name]
    x2, x1, g = upsample_operands(name)
    out, _, g1 = run_upsample(*(None if t is None else t.to(cuda) for t in (x2, x1, g)), scale)
    up = uo.upsample(x1.double().numpy(), scale)
    gt = uo.upsample_transpose(g[:, C2:].double().numpy(), scale)
    within(out[:, C2:], up, 1e-6 * plane_max(x1), f'{name} forward')
    within(g1, gt, (2 * scale + 1) ** 2 * 2.0 ** -23 * plane_max(g[:, C2:]), f'{name} backward')


# ------------------------------------------------------------------------------------------------ bev_align
ALIGN_SHAPES = [(2, 3, 12, 12), (1, 5, 9, 15), (2, 4, 16, 24)]


def align_transforms(h, w):
    """(name, (2, 3) float32): three seeded ones, an integer shift and a quarter turn (exact), one that maps everything
    outside the plane, and a scale of 0.5, under which a source pixel is read by four times as many output pixels."""
    out = [(f'seeded {k}', t) for k, t in enumerate(bo.seeded_transforms(h, w, 3, seed=h * w))]
    out += [('shift', bo.integer_shift(3, -2)), ('turn', bo.rot90_flip(h, w)),
            ('outside', bo.integer_shift(w + 5, 0)), ('scale 0.5', bo.affine(h, w, scale=0.5))]
    return out


@functools.lru_cache(maxsize=None)
def align_batches(shape):
    """[(names, tf (n, 3, 3) float32 CPU tensor, x, g bf16 CPU tensors)], the last batch filled up from the front."""
    n, c, h, w = shape
    ts = align_transforms(h, w)
    out = []
    for s in range(0, len(ts), n):
        part = (ts[s:s + n] + ts[:n])[:n]
        tf = np.zeros((n, 3, 3), np.float32)
        tf[:, 2, 2] = 1
        tf[:, :2] = np.stack([t for _, t in part])
        out.append(([name for name, _ in part], torch.from_numpy(tf), special(shape, 7 * s + h), special(shape, 7 * s + w + 1)))
    return out


def run_align(x, tf, g, **kw):
    x = x.clone().requires_grad_(True)
    out = temporal.shift_feature(x, tf, **kw)
    out.backward(g)
    return out.detach(), x.grad


@pytest.mark.parametrize('shape', ALIGN_SHAPES)
def test_bev_align_is_the_float32_kernel_rounded_once(cuda, launches, shape):
    n, c, h, w = shape
    seen = set()
    for names, tf, x, g in align_batches(shape):
        tf, x, g = tf.to(cuda), x.to(cuda), g.to(cuda)
        del launches[:]
        out, gx = run_align(x, tf, g, keep_bf16=True)
        assert launches == ['ocrf_bev_align_forward_bf16', 'ocrf_bev_align_backward_bf16']
        want, want_g = run_align(x.float(), tf, g.float())
        assert launches[2:] == ['ocrf_bev_align_forward', 'ocrf_bev_align_backward']
        assert same_bits(out, want.bfloat16()), names
        assert same_bits(gx, want_g.bfloat16()), names
        again = run_align(x, tf, g, keep_bf16=True)
        assert same_bits(again[0], out) and same_bits(again[1], gx)                # twice: the same bits
        for b, name in enumerate(names):
            if name in ('shift', 'turn'):         # exact: the contract and plain indexing agree
                indexed = bo.index_sample(x[b].float().cpu().numpy(), tf[b, :2].cpu().numpy())
                assert np.array_equal(out[b].float().cpu().numpy(), indexed), name
            if name == 'outside':
                assert not out[b].float().any() and not gx[b].float().any()
            seen.add(name)
    assert {'shift', 'turn', 'outside', 'scale 0.5', 'seeded 0', 'seeded 1', 'seeded 2'} <= seen


def test_bev_align_into_a_channel_slice_of_a_bf16_concatenation(cuda):
    """(2, 3, 12, 12) into channels 3..6 of a (2, 9, 12, 12) concatenation, forward and backward through the strided
    operand, both against the contract; the bytes outside the written channels stay as they were."""
    shape = ALIGN_SHAPES[0]
    names, tf, x, g = align_batches(shape)[0]
    tf, x = tf.to(cuda), x.to(cuda)
    wide = special((2, 9, 12, 12), 99).to(cuda)
    before = wide.clone()
    ret = temporal.shift_feature(x, tf, out=wide[:, 3:6], keep_bf16=True)
    assert ret.data_ptr() == wide[:, 3:6].data_ptr()
    assert same_bits(wide[:, 3:6], temporal.shift_feature(x.float(), tf).bfloat16())
    assert same_bits(wide[:, :3], before[:, :3]) and same_bits(wide[:, 6:], before[:, 6:])
    # one element off a 16-byte boundary: the 2-byte stores, the same bits, the neighbours untouched
    buf = torch.full((x.numel() + 2,), -12288.0, dtype=BF16, device=cuda)
    off = buf[1:-1].view(x.shape)
    assert off.data_ptr() % 16 == 2
    temporal.shift_feature(x, tf, out=off, keep_bf16=True)
    assert same_bits(off, wide[:, 3:6]) and float(buf[0]) == -12288.0 and float(buf[-1]) == -12288.0
    # the backward reads its gradient through the same stride
    tf32 = temporal._tf32(tf, x)
    gwide = special((2, 9, 12, 12), 100).to(cuda)
    got = temporal._gather_from(gwide[:, 3:6], tf32, shape)
    want = temporal._gather_from(gwide.float()[:, 3:6], tf32, shape)
    assert got.dtype == BF16 and same_bits(got, want.bfloat16())
    assert same_bits(got, temporal._gather_from(gwide[:, 3:6].contiguous(), tf32, shape))


@pytest.mark.parametrize('shape', ALIGN_SHAPES)
def test_bev_align_against_the_float64_oracle(cuda, shape):
    """``forward_bound`` / ``backward_bound`` of tests/bev_align_oracle.py, per plane, plus half a bf16 ulp."""
    n, c, h, w = shape
    for names, tf, x, g in align_batches(shape):
        out, gx = run_align(x.to(cuda), tf.to(cuda), g.to(cuda), keep_bf16=True)
        want, want_g = bo.oracle(x.double().numpy(), tf.numpy(), g.double().numpy())
        xmax, gmax = plane_max(x), plane_max(g)
        for b, name in enumerate(names):
            t = tf[b:b + 1].numpy()
            fb = bo.forward_bound(t, h, w, 1.0) * xmax[b]                           # both are linear in the magnitude
            bb = bo.backward_bound(t, h, w, 1.0) * gmax[b]
            within(out[b], want[b], fb, f'{shape} {name} forward')
            within(gx[b], want_g[b], bb, f'{shape} {name} backward')


# ------------------------------------------------------------------------------------------------ dispatch
def test_align_and_cat_keeps_bf16_maps_only_on_request(cuda, launches):
    s2k, extra = poses(cuda)
    maps = [f.detach().bfloat16().requires_grad_(r) for f, r in zip(frames(cuda), (True, True, False))]
    kept = temporal.align_and_cat(maps, [0, 1, 2], s2k, *extra, fused=True, keep_bf16=True)
    assert launches == ['ocrf_bev_align_forward_bf16'] * 2 and kept.dtype == BF16 and kept.is_contiguous()
    assert same_bits(kept[:, :5].detach(), maps[0].detach())                       # the key frame: a bf16 copy
    wide = temporal.align_and_cat([m.detach().float() for m in maps], [0, 1, 2], s2k, *extra, fused=True)
    assert same_bits(kept.detach(), wide.bfloat16())
    del launches[:]
    r = special(tuple(kept.shape), 5).to(cuda)
    kept.backward(r)
    assert launches == ['ocrf_bev_align_backward_bf16']                            # the frame without a gradient: none
    assert maps[0].grad.dtype == maps[1].grad.dtype == BF16 and maps[2].grad is None
    assert same_bits(maps[0].grad, r[:, :5])
    # under autocast the same
    del launches[:]
    with autocast():
        again = temporal.align_and_cat(maps, [0, 1, 2], s2k, *extra, fused=True, keep_bf16=True)
    assert launches == ['ocrf_bev_align_forward_bf16'] * 2 and same_bits(again.detach(), kept.detach())
    # without the keyword: as it was
    del launches[:]
    plain = temporal.align_and_cat(maps, [0, 1, 2], s2k, *extra, fused=True)
    assert launches == ['ocrf_bev_align_forward'] * 2 and plain.dtype == torch.float32
    assert torch.equal(plain.detach(), wide)
    # one float32 map in the list, or float16 maps: the float32 path
    del launches[:]
    mixed = temporal.align_and_cat([maps[0], maps[1].detach().float(), maps[2]], [0, 1, 2], s2k, *extra, fused=True,
                                   keep_bf16=True)
    assert launches == ['ocrf_bev_align_forward'] * 2 and mixed.dtype == torch.float32
    assert torch.equal(mixed.detach(), wide)
    halves = temporal.align_and_cat([m.detach().half() for m in maps], [0, 1, 2], s2k, *extra, fused=True, keep_bf16=True)
    assert launches == ['ocrf_bev_align_forward'] * 4 and halves.dtype == torch.float32
    # the torch formulation keeps bf16 too
    del launches[:]
    unfused = temporal.align_and_cat(maps, [0, 1, 2], s2k, *extra, fused=False, keep_bf16=True)
    assert not launches and unfused.dtype == BF16 and same_bits(unfused[:, :5].detach(), maps[0].detach())
    # ... and samples where the kernels sample: its grid is float32, so it differs from the float32 kernels' result by
    # the two float32 formulations' bounds (as test_bev_align_gpu.py has it) and one rounding to bf16
    for k in (1, 2):
        tf = temporal.feature_transform([s2k[0], s2k[k]], *extra).cpu().numpy()
        bound = 2 * bo.forward_bound(tf, 16, 24, float(maps[k].detach().float().abs().max()))
        within(unfused[:, 5 * k:5 * k + 5], wide[:, 5 * k:5 * k + 5].double().cpu().numpy(), bound,
               f'torch formulation under keep_bf16, frame {k}')


def test_shift_feature_with_out_writes_bf16_in_place(cuda, launches):
    s2k, extra = poses(cuda)
    tf = temporal.feature_transform([s2k[0], s2k[1]], *extra)
    x = frames(cuda, grads=(False,))[0].bfloat16()
    wide = torch.zeros(3, 15, 16, 24, dtype=BF16, device=cuda)
    ret = temporal.shift_feature(x, tf, out=wide[:, 5:10], keep_bf16=True)
    assert launches == ['ocrf_bev_align_forward_bf16'] and ret.data_ptr() == wide[:, 5:10].data_ptr()
    assert same_bits(wide[:, 5:10], temporal.shift_feature(x, tf, keep_bf16=True))
    assert not wide[:, :5].float().any() and not wide[:, 10:].float().any()
    with pytest.raises(_lib.OcrfHipError):
        temporal.shift_feature(x, tf, out=torch.zeros(3, 15, 16, 24, device=cuda)[:, 5:10], keep_bf16=True)
    with pytest.raises(_lib.OcrfHipError):
        temporal.shift_feature(x, tf, out=wide[:, 5:10])                           # cast to float32: a float32 out
    # the detector's method reads align_keep_bf16
    det = type('Detector', (), dict(shift_feature=temporal.shift_feature_method))()
    det.img_view_transformer = type('VT', (), dict(grid_interval=extra[1], grid_lower_bound=extra[2]))()
    assert det.shift_feature(x, [s2k[0], s2k[1]], extra[0]).dtype == torch.float32
    det.align_keep_bf16 = True
    assert same_bits(det.shift_feature(x, [s2k[0], s2k[1]], extra[0]), wide[:, 5:10])
    assert det.shift_feature(x.float(), [s2k[0], s2k[1]], extra[0]).dtype == torch.float32


# ------------------------------------------------------------------------------------------------ the encoder
def small_encoder(c_in, c_out, cuda, **kw):
    torch.manual_seed(3)
    return bev_encoder.BEVEncoder(dict(type='CustomResNet', numC_input=c_in, num_channels=[8, 16, 32]),
                                  dict(type='FPN_LSS', in_channels=8 + 32, out_channels=c_out, scale_factor=4,
                                       extra_upsample=2), **kw).to(cuda)


def rms(a, b):
    return float((a.double() - b.double()).square().mean().sqrt())


def test_encoder_under_bf16_autocast(cuda, launches):
    enc = small_encoder(16, 8, cuda, autocast_bf16=True).train()
    neck = enc.img_bev_encoder_neck
    neck.fused_upsample = neck.fused_upsample_bf16 = True
    x = torch.randn(2, 16, 16, 16, generator=torch.Generator().manual_seed(4)).to(cuda).bfloat16().requires_grad_(True)
    with autocast():
        out = enc(x)
    assert out.dtype == BF16 and out.shape == (2, 8, 16, 16) and torch.isfinite(out).all()
    assert launches == ['ocrf_upsample_cat_forward_bf16'] * 2
    del launches[:]
    out.float().square().mean().backward()
    assert launches == ['ocrf_upsample_cat_backward_bf16'] * 2
    params = list(enc.parameters())
    assert all(p.dtype == torch.float32 and p.grad is not None and p.grad.dtype == torch.float32
               and torch.isfinite(p.grad).all() for p in params)
    assert any(float(p.grad.abs().max()) > 0 for p in params)
    assert x.grad.dtype == BF16 and torch.isfinite(x.grad).all() and float(x.grad.float().abs().max()) > 0

    enc.eval()
    with torch.no_grad():
        del launches[:]
        want = enc(x)                                                              # outside autocast: float32, as ever
        assert want.dtype == torch.float32 and launches == ['ocrf_upsample_cat_forward'] * 2
        with autocast():
            del launches[:]
            enc.autocast_bf16 = False                                              # today's: float32 under autocast too
            off = enc(x)
            assert off.dtype == torch.float32 and launches == ['ocrf_upsample_cat_forward'] * 2
            # (the convolution library may choose another algorithm from one call to the next: no bits compared)
            assert rms(off, want) <= 1e-4 * float(want.abs().max())
            enc.autocast_bf16 = True
            del launches[:]
            fused = enc(x.detach().float())                                        # a float32 input is narrowed once
            assert fused.dtype == BF16 and launches == ['ocrf_upsample_cat_forward_bf16'] * 2
            neck.fused_upsample_bf16 = False                                       # the torch formulation on bf16
            del launches[:]
            unfused = enc(x)
            assert unfused.dtype == BF16 and not launches
            neck.fused_upsample_bf16, neck.fused_upsample = True, False            # the module flag switches all off
            assert enc(x).dtype == BF16 and not launches
    # the two bf16 arms differ in the last bits of the interpolation weights only: their errors against the float32
    # encoder are draws from one distribution, dominated by the convolutions' rounding
    e_fused, e_torch = rms(fused, want), rms(unfused, want)
    print(f'RMS error against the float32 encoder: fused bf16 {e_fused:.4e}, torch bf16 {e_torch:.4e}, '
          f'ratio {e_fused / e_torch:.3f}; RMS of the output {rms(want, torch.zeros_like(want)):.4e}')
    assert e_fused <= 1.5 * e_torch


def test_chain_from_pre_process_to_the_loss_stays_bf16(cuda, golden, launches):
    """bf16 ``pre_process`` output -> ``align_and_cat(keep_bf16=True)`` -> ``BEVEncoder(autocast_bf16=True)`` ->
    ``CenterHead`` -> loss, under autocast: bf16 at the three seams, and the gradient reaches the key frame's map."""
    g = golden('center_head.npz')
    torch.manual_seed(6)
    head = make_head(g).to(cuda).train()
    assert isinstance(head, center_head.CenterHead)
    bx, lab = boxes(g, cuda)
    cfg = head.train_cfg
    W, H = (int(s) // int(cfg['out_size_factor']) for s in cfg['grid_size'][:2])
    B, C = len(lab), 4
    pre = bev_encoder.build_pre_process(dict(type='CustomResNet', numC_input=C, num_layer=[1], num_channels=[C],
                                             stride=[1], backbone_output_ids=[0])).to(cuda).train()
    enc = small_encoder(3 * C, json.loads(str(g['cfg']))['in_ch'], cuda, autocast_bf16=True).train()
    enc.img_bev_encoder_neck.fused_upsample = enc.img_bev_encoder_neck.fused_upsample_bf16 = True
    s2k, extra = poses(cuda)
    assert s2k[0].shape[0] == B
    raw = [torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(20 + k)).to(cuda) for k in range(3)]
    with autocast():
        key = pre(raw[0])[0]
        key.retain_grad()
        with torch.no_grad():                      # the reference computes adjacent frames under no_grad
            adjacent = [pre(r)[0] for r in raw[1:]]
        assert all(m.dtype == BF16 for m in [key] + adjacent)                      # seam 1
        cat = temporal.align_and_cat([key] + adjacent, [0, 1, 2], s2k, *extra, fused=True, keep_bf16=True)
        assert cat.dtype == BF16 and cat.shape == (B, 3 * C, H, W)                 # seam 2
        bev = enc(cat)
        assert bev.dtype == BF16 and bev.shape[2:] == (H, W)                       # seam 3
        preds = head([bev])
        assert all(v.dtype == BF16 for p in preds for v in p[0].values())
        losses = head.loss(bx, lab, preds)
    assert launches.count('ocrf_bev_align_forward_bf16') == 2 and 'ocrf_bev_align_forward' not in launches
    assert launches.count('ocrf_upsample_cat_forward_bf16') == 2 and 'ocrf_upsample_cat_forward' not in launches
    sum(losses.values()).backward()
    assert launches.count('ocrf_upsample_cat_backward_bf16') == 2
    assert 'ocrf_bev_align_backward_bf16' not in launches and 'ocrf_bev_align_backward' not in launches
    assert key.grad is not None and key.grad.dtype == BF16 and torch.isfinite(key.grad).all()
    assert float(key.grad.float().abs().max()) > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in pre.parameters())
