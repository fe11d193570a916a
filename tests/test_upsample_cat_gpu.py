"""GPU: ``ocrf_upsample_cat_forward`` / ``_backward`` (csrc/upsample_cat.hip) through ``bev_encoder.upsample_cat``
against the numpy float64 statement of the sampling rule (tests/upsample_oracle.py).

Bounds, each a fraction of the operand's largest magnitude:

* forward: a convex combination of four inputs with singly rounded weights; six roundings give 8 * 2^-24 = 4.8e-7;
  tested at 1e-6 max|x1|.  The copied channels are compared bit for bit.
* backward: a gather sums at most (2 scale + 1)^2 terms: (2 scale + 1)^2 * 2^-23 max|grad_out|.
* against ``upsample_cat_torch``: torch's float lambda is off by up to in * 2^-23: (in * 2^-22 + 2^-20) max|x1|, ``in``
  the larger input side.

The oracle is computed once per (input size, scale) for B = 2 and the most channels; the smaller cases are slices of the
same operands.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib
from ocrfdet_amd import bev_encoder as be
from tests import upsample_oracle as uo

SIZES = [(1, 1), (1, 5), (2, 3), (3, 2), (5, 7), (16, 16), (16, 44)]
SCALES = [2, 4]
C2S, C1S, BS = (0, 1, 3), (1, 5, 65), (1, 2)


@functools.lru_cache(maxsize=None)
def operands(hw, scale):
    """x1 (2, 65, H, W), x2 (2, 3, Ho, Wo), grad_out halves g2 (2, 3, Ho, Wo) and g1 (2, 65, Ho, Wo), with the oracle's
    upsampling of x1 and transpose of g1."""
    rng = np.random.default_rng(1000 * hw[0] + 10 * hw[1] + scale)
    Ho, Wo = hw[0] * scale, hw[1] * scale
    x1 = rng.standard_normal((2, 65, *hw)).astype(np.float32)
    x2 = rng.standard_normal((2, 3, Ho, Wo)).astype(np.float32)
    g2 = rng.standard_normal((2, 3, Ho, Wo)).astype(np.float32)
    g1 = rng.standard_normal((2, 65, Ho, Wo)).astype(np.float32)
    return x1, x2, g2, g1, uo.upsample(x1, scale), uo.upsample_transpose(g1, scale)


def case(hw, scale, B, C2, C1, dev):
    x1, x2, g2, g1, up, gt = operands(hw, scale)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)    # noqa: E731
    return (t(x2[:B, :C2]) if C2 else None, t(x1[:B, :C1]), t(np.concatenate([g2[:B, :C2], g1[:B, :C1]], 1)),
            up[:B, :C1], gt[:B, :C1])


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('hw', SIZES)
def test_forward_and_backward_against_the_float64_oracle(cuda, hw, scale):
    fails = []
    for B in BS:
        for C2 in C2S:
            for C1 in C1S:
                x2, x1, g, up, gt = case(hw, scale, B, C2, C1, cuda)
                x1.requires_grad_(True)
                if x2 is not None:
                    x2.requires_grad_(True)
                out = be.upsample_cat(x2, x1, scale)
                assert out.shape == (B, C2 + C1, hw[0] * scale, hw[1] * scale) and out.is_contiguous()
                out.backward(g)
                tag = f'B={B} C2={C2} C1={C1}'
                if C2:
                    if not torch.equal(out[:, :C2], x2) or not torch.equal(x2.grad, g[:, :C2]):
                        fails.append(f'{tag}: copied channels differ')
                xmax, gmax = float(x1.detach().abs().max()), float(g.abs().max())
                e_f = float(np.abs(out[:, C2:].detach().cpu().numpy().astype(np.float64) - up).max())
                e_b = float(np.abs(x1.grad.cpu().numpy().astype(np.float64) - gt).max())
                b_f, b_b = 1e-6 * xmax, (2 * scale + 1) ** 2 * 2.0 ** -23 * gmax
                print(f'{hw} x{scale} {tag}: forward {e_f:.3e} (bound {b_f:.3e}), backward {e_b:.3e} (bound {b_b:.3e})')
                if not e_f <= b_f:
                    fails.append(f'{tag}: forward {e_f:.3e} > {b_f:.3e}')
                if not e_b <= b_b:
                    fails.append(f'{tag}: backward {e_b:.3e} > {b_b:.3e}')
    assert not fails, fails


@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('hw', SIZES)
def test_against_the_torch_formulation(cuda, hw, scale):
    x2, x1, g, _, _ = case(hw, scale, 2, 3, 65, cuda)
    got, want = be.upsample_cat(x2, x1, scale), be.upsample_cat_torch(x2, x1, scale)
    assert torch.equal(got[:, :3], want[:, :3])
    err = float((got - want).abs().max())
    bound = (max(hw) * 2.0 ** -22 + 2.0 ** -20) * float(x1.abs().max())
    print(f'{hw} x{scale}: fused - torch {err:.3e} (bound {bound:.3e})')
    assert err <= bound
    up = be.upsample_cat(None, x1, scale)
    assert torch.equal(up, got[:, 3:])           # C2 = 0 is the same upsampling


@pytest.mark.parametrize('hw,scale', [((5, 7), 2), ((16, 44), 4), ((3, 2), 4)])
def test_two_runs_are_bit_identical(cuda, hw, scale):
    x2, x1, g, _, _ = case(hw, scale, 2, 3, 65, cuda)
    runs = []
    for _ in range(2):
        a = x1.clone().requires_grad_(True)
        out = be.upsample_cat(x2, a, scale)
        out.backward(g)
        runs.append((out.detach(), a.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_unaligned_operands_take_the_scalar_accesses(cuda):
    """A contiguous view that starts 4 bytes into its storage is not 16-byte aligned: same results."""
    x2, x1, g, up, _ = case((5, 7), 2, 2, 3, 5, cuda)
    buf = torch.empty(x2.numel() + 1, device=cuda)
    x2o = buf[1:].view(x2.shape).copy_(x2)
    assert x2o.data_ptr() % 16 == 4 and x2o.is_contiguous()
    assert torch.equal(be.upsample_cat(x2o, x1, 2), be.upsample_cat(x2, x1, 2))


def test_no_host_synchronisation(cuda):
    x2, x1, g, _, _ = case((16, 16), 4, 2, 3, 65, cuda)
    x1.requires_grad_(True)
    be.upsample_cat(x2, x1, 4).backward(g)          # warm-up: library, code object
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        x1.grad = None
        be.upsample_cat(x2, x1, 4).backward(g)
        be.upsample_cat(None, x1.detach(), 4)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.isfinite(x1.grad).all()


def test_other_inputs_take_the_torch_path(cuda, monkeypatch):
    """FPN_LSS's dispatch: a non-contiguous or non-float32 map goes through ``upsample_cat_torch`` without error, and
    ``upsample_cat`` itself refuses it rather than falling back."""
    neck = be.FPN_LSS(in_channels=8 + 4, out_channels=4, extra_upsample=None).to(cuda).eval()
    f0, f2 = torch.randn(2, 4, 8, 8, device=cuda), torch.randn(2, 8, 2, 2, device=cuda)
    strided = torch.randn(2, 2, 2, 8, device=cuda).permute(0, 3, 1, 2).copy_(f2)
    assert not strided.is_contiguous()
    real = be.upsample_cat
    with pytest.raises(_lib.OcrfHipError):
        real(None, strided, 4)
    with pytest.raises(_lib.OcrfHipError):
        real(None, f2.half(), 4)
    with pytest.raises(_lib.OcrfHipError):
        real(f0, f2, 2)                              # x2 is not scale times x1
    calls = []
    monkeypatch.setattr(be, 'upsample_cat', lambda *a: calls.append(1) or real(*a))
    with torch.no_grad():
        want = neck([f0, None, f2])
        assert calls == [1]
        got = neck([f0, None, strided])
        assert calls == [1]
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-5)
        half = copy.deepcopy(neck).half()           # a copy: half() rounds the weights
        assert half([f0.half(), None, f2.half()]).dtype == torch.float16
        assert calls == [1]
        neck.fused_upsample = False
        assert torch.allclose(neck([f0, None, f2]), want, rtol=1e-4, atol=1e-5)
        assert calls == [1]


def test_c_boundary_refuses_two_gib_operands():
    """Argument validation alone (nothing is launched, no memory is touched): an output of 2 GiB or more, and an axis sum
    beyond the LDS tables, return hipErrorInvalidValue; so does a missing x2."""
    L = _lib.lib()
    p = ctypes.c_void_p(4096)
    invalid = 1
    # 16 x (160 + 640) x 256 x 256 floats = 3.1 GiB of output; 8 x ... = 1.56 GiB would pass the size check
    assert L.ocrf_upsample_cat_forward(16, 160, 640, 64, 64, 4, p, p, p, None) == invalid
    assert L.ocrf_upsample_cat_backward(16, 160, 640, 64, 64, 4, p, p, None) == invalid
    assert L.ocrf_upsample_cat_forward(1, 0, 1 << 29, 1, 1, 1, None, p, p, None) == invalid        # exactly 2 GiB
    assert L.ocrf_upsample_cat_forward(1 << 20, 1 << 20, 1 << 20, 1, 1, 2, p, p, p, None) == invalid
    assert L.ocrf_upsample_cat_forward(1, 0, 1, 4096, 4096, 2, None, p, p, None) == invalid        # (H + W) scale > 8192
    assert L.ocrf_upsample_cat_forward(1, 2, 1, 4, 4, 2, None, p, p, None) == invalid              # C2 > 0 without x2
    assert L.ocrf_upsample_cat_forward(1, 0, 1, 4, 4, 0, None, p, p, None) == invalid
    assert L.ocrf_upsample_cat_backward(1, 0, 1, 4, 4, 2, None, p, None) == invalid
