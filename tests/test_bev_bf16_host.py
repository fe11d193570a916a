"""Host: the bfloat16 forms of ``upsample_cat`` and of the temporal alignment, without a GPU: the four ``*_bf16``
prototypes as ``_lib`` reads them from the header, their kernel ids, the argument validation of the entry points
themselves (nothing is launched), the predicates the modules dispatch with, and the two opt-in switches
(``BEVEncoder.autocast_bf16``, ``keep_bf16``) on the CPU, where everything takes the torch formulation."""
import ctypes
import inspect

import pytest
import torch

from ocrfdet_amd import _lib, plane_ops, temporal
from ocrfdet_amd import bev_encoder as be

UP_FWD, UP_BWD = 'ocrf_upsample_cat_forward_bf16', 'ocrf_upsample_cat_backward_bf16'
AL_FWD, AL_BWD = 'ocrf_bev_align_forward_bf16', 'ocrf_bev_align_backward_bf16'
NAMES = [UP_FWD, UP_BWD, AL_FWD, AL_BWD]
BF16 = torch.bfloat16


def test_prototypes_parse_from_the_header():
    protos = _lib.prototypes()
    enqueueing = _lib.parse_enqueueing(_lib._header_text())
    V, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    want = {UP_FWD: [I] * 6 + [V, V, V, V], UP_BWD: [I] * 6 + [V, V, V],
            AL_FWD: [I] * 4 + [V, V, V, LL, V], AL_BWD: [I] * 4 + [V, LL, V, V, V]}
    for name in NAMES:
        restype, argtypes = protos[name]
        assert restype is ctypes.c_int and argtypes == want[name], name
        assert name in enqueueing                                                  # the stream is the last parameter
        fn = getattr(_lib.lib(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[name]
        # the arguments are those of the float32 entry point
        assert protos[name[:-len('_bf16')]] == protos[name]
    text = _lib._header_text()

    def declaration(name):
        decl = text[text.index(name + '('):]
        return decl[:decl.index(';')]
    for name in (UP_FWD, UP_BWD):                                                  # bf16 travels as unsigned short
        decl = declaration(name)
        assert decl.count('unsigned short *') == want[name].count(V) - 1 and 'float' not in decl
    for name in (AL_FWD, AL_BWD):                                                  # and tf stays float
        decl = declaration(name)
        assert decl.count('unsigned short *') == 2 and decl.count('float *') == 1 and 'const float *tf' in decl


def test_kernel_ids_continue_and_none_moved():
    ids = [_lib.K_UPSAMPLE_CAT_BF16, _lib.K_UPSAMPLE_CAT_BWD_BF16, _lib.K_BEV_ALIGN_BF16, _lib.K_BEV_ALIGN_BWD_BF16]
    assert ids == [117, 118, 119, 120]
    L = _lib.lib()
    assert [L.ocrf_kernel_name(i) for i in ids] == [
        b'upsample_cat_kernel<unsigned short, *>', b'upsample_cat_backward_kernel<unsigned short>',
        b'bev_align_kernel<unsigned short, *>', b'bev_align_backward_kernel<unsigned short>']    # as a trace spells them
    old = ['ADD_RELU', 'ADD_RELU_BWD', 'UPSAMPLE_ADD', 'UPSAMPLE_ADD_BWD', 'BEV_ALIGN', 'BEV_ALIGN_BWD', 'OPTIM_SQNORM',
           'OPTIM_NORM_FINAL', 'OPTIM_STEP', 'ADD_RELU_BF16', 'ADD_RELU_BWD_BF16', 'UPSAMPLE_ADD_BF16',
           'UPSAMPLE_ADD_BWD_BF16']
    assert [getattr(_lib, 'K_' + k) for k in old] == list(range(104, 117))
    assert _lib.K_UPSAMPLE_CAT == 102 and _lib.K_UPSAMPLE_CAT_BWD == 103
    # the float32 kernels are instantiations of the same templates now, and are named as such
    assert [L.ocrf_kernel_name(i) for i in (102, 103, 108, 109)] == [
        b'upsample_cat_kernel<float, *>', b'upsample_cat_backward_kernel<float>', b'bev_align_kernel<float, *>',
        b'bev_align_backward_kernel<float>']
    assert L.ocrf_kernel_name(116) == b'upsample_add_backward_bf16_kernel'


def test_upsample_cat_c_boundary_refuses_bad_arguments():
    """Argument validation alone: the calls return before anything is launched, the pointers are never dereferenced."""
    L = _lib.lib()
    p = ctypes.c_void_p(4096)
    invalid = 1                                    # hipErrorInvalidValue
    fwd, bwd = getattr(L, UP_FWD), getattr(L, UP_BWD)
    assert fwd(1, 2, 1, 4, 4, 2, None, p, p, None) == invalid                      # C2 > 0 without x2
    assert fwd(1, 0, 1, 4, 4, 2, None, None, p, None) == invalid and fwd(1, 0, 1, 4, 4, 2, None, p, None, None) == invalid
    assert bwd(1, 0, 1, 4, 4, 2, None, p, None) == invalid and bwd(1, 0, 1, 4, 4, 2, p, None, None) == invalid
    for bad in ((0, 1, 1, 4, 4, 2), (1, -1, 1, 4, 4, 2), (1, 1, 0, 4, 4, 2), (1, 1, 1, 0, 4, 2), (1, 1, 1, 4, -4, 2),
                (1, 1, 1, 4, 4, 0), (1, 1, 1, 4, 4, -2)):
        assert fwd(*bad, p, p, p, None) == invalid and bwd(*bad, p, p, None) == invalid
    assert fwd(1, 0, 1, 4096, 4096, 2, None, p, p, None) == invalid               # Hout + Wout = 16384
    assert fwd(1, 0, 1, 4096, 4097, 1, None, p, p, None) == invalid               # Hout + Wout = 8193
    assert bwd(1, 0, 1, 4096, 4097, 1, p, p, None) == invalid
    # a destination of exactly 2 GiB of bf16 (2^30 elements), of more, and products that overflow
    for shape in [(1, 0, 1 << 30, 1, 1, 1), (1, 0, 1 << 20, 16, 16, 2), (32, 160, 640, 64, 64, 4),
                  (1 << 20, 1 << 20, 1 << 20, 1, 1, 2)]:
        assert fwd(*shape, p, p, p, None) == invalid, shape
        assert bwd(*shape, p, p, None) == invalid, shape


def test_bev_align_c_boundary_refuses_bad_arguments():
    L = _lib.lib()
    p = ctypes.c_void_p(4096)
    invalid = 1
    fwd, bwd = getattr(L, AL_FWD), getattr(L, AL_BWD)
    ok = (2, 3, 4, 5)
    row = 3 * 4 * 5
    for k in range(3):                                                             # each pointer in turn
        ptrs = [p, p, p]
        ptrs[k] = None
        assert fwd(*ok, ptrs[0], ptrs[1], ptrs[2], row, None) == invalid
        assert bwd(*ok, ptrs[0], row, ptrs[1], ptrs[2], None) == invalid
    for bad in ((0, 3, 4, 5), (2, 0, 4, 5), (2, 3, -4, 5), (2, 3, 4, 0)):
        assert fwd(*bad, p, p, p, 1 << 20, None) == invalid and bwd(*bad, p, 1 << 20, p, p, None) == invalid
    for stride in (row - 1, 0, -row):                                              # a stride smaller than c h w
        assert fwd(*ok, p, p, p, stride, None) == invalid and bwd(*ok, p, stride, p, p, None) == invalid
    # exactly 2 GiB of bf16: 2^30 elements in the contiguous operand, or in the strided one
    big = (1, 1 << 10, 1 << 10, 1 << 10)
    assert fwd(*big, p, p, p, 1 << 30, None) == invalid and bwd(*big, p, 1 << 30, p, p, None) == invalid
    assert fwd(2, 1, 4, 4, p, p, p, (1 << 30) - 16, None) == invalid               # (n - 1) stride + c h w = 2^30
    assert bwd(2, 1, 4, 4, p, (1 << 30) - 16, p, p, None) == invalid
    assert fwd(1 << 16, 1 << 16, 1 << 8, 1 << 8, p, p, p, 1 << 40, None) == invalid


class _OnGpu:
    """A tensor's metadata as the predicates read it, claiming to be on a GPU: the dtype logic without a device."""

    def __init__(self, t, device='cuda:0'):
        self._t, self.is_cuda, self.device = t, True, torch.device(device)

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_the_bf16_predicate_takes_all_bf16_operands_only():
    x1, x2 = torch.randn(2, 4, 3, 4), torch.randn(2, 3, 6, 8)
    on = _OnGpu
    take, f32 = plane_ops.upsample_cat_bf16_fusable, plane_ops.upsample_cat_fusable
    assert take(on(x2.bfloat16()), on(x1.bfloat16()), 2) and take(None, on(x1.bfloat16()), 2)
    assert take(None, on(x1.bfloat16()), 2.0) and not take(None, on(x1.bfloat16()), 1.5)
    for a, b in ((torch.float32, BF16), (BF16, torch.float32), (torch.float16, BF16), (BF16, torch.float16),
                 (torch.float16, torch.float16), (torch.float32, torch.float32), (torch.float64, torch.float64)):
        assert not take(on(x2.to(a)), on(x1.to(b)), 2), (a, b)
    assert not take(None, on(x1.half()), 2) and not take(None, on(x1), 2)
    assert not take(x2.bfloat16(), x1.bfloat16(), 2) and not take(None, x1.bfloat16(), 2)      # the CPU
    assert not take(on(x2.bfloat16()), on(x1.bfloat16()), 4)                                  # x2 is not 4 x x1
    assert not take(None, on(x1.bfloat16().permute(0, 1, 3, 2)), 2)
    # the float32 predicate keeps refusing bf16, and takes what it took
    assert not f32(None, on(x1.bfloat16()), 2) and not f32(on(x2.bfloat16()), on(x1.bfloat16()), 2)
    assert f32(on(x2), on(x1), 2) and f32(None, on(x1), 2) and not f32(on(x2), on(x1.bfloat16()), 2)
    # the op itself raises on a mixed pair and off the GPU rather than falling back
    for a, b in ((x2.bfloat16(), x1.bfloat16()), (x2, x1.bfloat16())):
        with pytest.raises(_lib.OcrfHipError):
            plane_ops.upsample_cat(a, b, 2)


def test_a_gradient_of_another_dtype_is_refused():
    plane_ops._check_grad(torch.zeros(3).bfloat16(), BF16, 'upsample_cat')
    for g, dtype in ((torch.zeros(3), BF16), (torch.zeros(3).bfloat16(), torch.float32)):
        with pytest.raises(_lib.OcrfHipError):
            plane_ops._check_grad(g, dtype, 'upsample_cat')
    with pytest.raises(_lib.OcrfHipError):
        temporal._check_bf16_grad(torch.zeros(3))


def small_encoder(**kw):
    return be.BEVEncoder(dict(type='CustomResNet', numC_input=8, num_channels=[8, 16, 32]),
                         dict(type='FPN_LSS', in_channels=8 + 32, out_channels=8), **kw)


def test_flags_and_their_defaults():
    assert isinstance(plane_ops.FUSED_UPSAMPLE_BF16_DEFAULT, bool)
    enc = small_encoder()
    assert enc.autocast_bf16 is False
    assert enc.img_bev_encoder_neck.fused_upsample_bf16 is plane_ops.FUSED_UPSAMPLE_BF16_DEFAULT
    assert enc.img_bev_encoder_neck.fused_upsample is True
    assert small_encoder(autocast_bf16=True).autocast_bf16 is True
    # neither flag is state: the keys and the parameter dtypes are the encoder's own
    on = small_encoder(autocast_bf16=True)
    assert list(on.state_dict()) == list(enc.state_dict())
    assert all(p.dtype == torch.float32 for p in on.parameters())
    assert inspect.signature(temporal.align_and_cat).parameters['keep_bf16'].default is False
    assert inspect.signature(temporal.shift_feature).parameters['keep_bf16'].default is False


def test_encoder_on_the_cpu_is_bf16_only_with_the_flag_and_under_bf16_autocast():
    torch.manual_seed(0)
    enc = small_encoder().eval()
    x = torch.randn(1, 8, 16, 16)
    with torch.no_grad():
        want = enc(x)
        with torch.autocast('cpu', dtype=BF16):
            kept = enc(x)                                                          # the flag is off: float32 as before
            assert kept.dtype == torch.float32 and torch.equal(kept, want)
            enc.autocast_bf16 = True
            got = enc(x)
            assert got.dtype == BF16 and got.shape == want.shape
            assert torch.equal(enc(x.bfloat16()), got)                             # a bf16 input is taken as it is
        assert torch.equal(enc(x), want)                                           # outside autocast the flag does nothing
        with torch.autocast('cpu', dtype=torch.float16):
            assert enc(x).dtype == torch.float32                                   # nor under float16 autocast
    err = float((got.float() - want).abs().max())
    assert err <= 0.1 * float(want.abs().max())                                    # bf16 convolutions, not noise
    assert all(p.dtype == torch.float32 for p in enc.parameters())


def test_align_and_cat_on_the_cpu_keeps_bf16_maps_only_on_request():
    torch.manual_seed(1)
    eye = torch.eye(4).repeat(2, 1, 1, 1)
    moved = eye.clone()
    moved[..., 0, 3] = 0.8
    args = ([eye, moved], torch.eye(3).repeat(2, 1, 1), (0.4, 0.4, 1.0), (-2.0, -2.0, 0.0))
    maps = [torch.randn(2, 3, 8, 8).bfloat16() for _ in range(2)]
    kept = temporal.align_and_cat(maps, [0, 1], *args, keep_bf16=True)
    assert kept.dtype == BF16 and kept.shape == (2, 6, 8, 8) and torch.equal(kept[:, :3], maps[0])
    assert temporal.align_and_cat(maps, [0, 1], *args).dtype == torch.float32
    mixed = [maps[0], maps[1].float()]
    assert temporal.align_and_cat(mixed, [0, 1], *args, keep_bf16=True).dtype == torch.float32
    halves = [m.half() for m in maps]
    with_kw, without = (temporal.align_and_cat(halves, [0, 1], *args, keep_bf16=k) for k in (True, False))
    assert with_kw.dtype == torch.float32 and torch.equal(with_kw, without)
    with torch.autocast('cpu', dtype=BF16):
        assert temporal.align_and_cat(maps, [0, 1], *args, keep_bf16=True).dtype == BF16
    with pytest.raises(_lib.OcrfHipError):
        temporal.shift_feature(maps[0], torch.eye(3).repeat(2, 1, 1), keep_bf16=True)          # the op: GPU only
