"""Host: what ``add_relu`` / ``upsample_add`` accept since they take bfloat16 (the predicates the modules dispatch
with), the four ``*_bf16`` prototypes as ``_lib`` reads them from the header, and the argument validation of the entry
points themselves (nothing is launched: no GPU needed)."""
import ctypes

import pytest
import torch

from ocrfdet_amd import _lib, blocks, plane_ops
from ocrfdet_amd import image_encoder as ie

NAMES = ['ocrf_add_relu_forward_bf16', 'ocrf_add_relu_backward_bf16', 'ocrf_upsample_add_forward_bf16',
         'ocrf_upsample_add_backward_bf16']


def test_predicates_refuse_what_is_not_on_the_gpu_or_not_of_one_kernel_dtype():
    a = torch.randn(2, 4, 6, 8)
    src = torch.randn(2, 4, 3, 4)
    for cast in (torch.Tensor.bfloat16, torch.Tensor.half, torch.Tensor.float):
        assert not plane_ops.add_relu_fusable(cast(a), cast(a))                    # the CPU
        assert not plane_ops.upsample_add_fusable(cast(a), cast(src), (6, 8), None)
    assert not plane_ops.add_relu_fusable(a.bfloat16(), a) and not plane_ops.add_relu_fusable(a, a.bfloat16())
    for t in (a.bfloat16(), a):
        with pytest.raises(_lib.OcrfHipError):
            plane_ops.add_relu(t, t)
        with pytest.raises(_lib.OcrfHipError):
            plane_ops.upsample_add(t, src.to(t.dtype), size=(6, 8))


class _OnGpu:
    """A tensor's metadata as the predicates read it, claiming to be on a GPU: the dtype logic without a device."""

    def __init__(self, t, device='cuda:0'):
        self._t, self.is_cuda, self.device = t, True, torch.device(device)

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_predicates_take_one_dtype_of_float32_and_bfloat16():
    a, src = torch.randn(2, 4, 6, 8), torch.randn(2, 4, 3, 4)
    on = _OnGpu
    for dtype, ok in ((torch.float32, True), (torch.bfloat16, True), (torch.float16, False), (torch.float64, False)):
        assert plane_ops.add_relu_fusable(on(a.to(dtype)), on(a.to(dtype))) is ok
        assert plane_ops.upsample_add_fusable(on(a.to(dtype)), on(src.to(dtype)), (6, 8), None) is ok
        assert plane_ops.upsample_add_fusable(on(a.to(dtype)), on(src.to(dtype)), None, 2) is ok
    for x, y in ((torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.float16)):
        assert not plane_ops.add_relu_fusable(on(a.to(x)), on(a.to(y)))
        assert not plane_ops.upsample_add_fusable(on(a.to(x)), on(src.to(y)), (6, 8), None)
    b16 = a.bfloat16()
    assert not plane_ops.add_relu_fusable(on(b16), on(b16, 'cuda:1'))               # two devices
    assert not plane_ops.add_relu_fusable(on(b16.permute(0, 1, 3, 2)), on(b16.permute(0, 1, 3, 2)))
    assert not plane_ops.add_relu_fusable(on(b16), on(b16[:, :2])) and not plane_ops.add_relu_fusable(on(b16[:0]), on(b16[:0]))
    assert not plane_ops.upsample_add_fusable(on(src.bfloat16()), on(b16), (3, 4), None)      # a smaller target
    # upsample_cat stays float32: BEVEncoder runs with autocast disabled
    assert plane_ops.upsample_cat_fusable(None, on(a), 2) and not plane_ops.upsample_cat_fusable(None, on(b16), 2)


def test_a_gradient_of_another_dtype_is_refused():
    plane_ops._check_grad(torch.zeros(3).bfloat16(), torch.bfloat16, 'add_relu')
    for g, dtype in ((torch.zeros(3), torch.bfloat16), (torch.zeros(3).bfloat16(), torch.float32),
                     (torch.zeros(3).half(), torch.bfloat16)):
        with pytest.raises(_lib.OcrfHipError):
            plane_ops._check_grad(g, dtype, 'add_relu')


def test_flags_and_their_defaults():
    assert isinstance(plane_ops.FUSED_TAIL_BF16_DEFAULT, bool) and isinstance(plane_ops.FUSED_MERGE_BF16_DEFAULT, bool)
    assert ie.FUSED_TAIL_BF16_DEFAULT is plane_ops.FUSED_TAIL_BF16_DEFAULT
    net = ie.ResNet(depth=18, base_channels=4)
    fpn = ie.CustomFPN([4, 4], 4, num_outs=1, out_ids=[0])
    assert net.fused_tail_bf16 is plane_ops.FUSED_TAIL_BF16_DEFAULT and net.fused_tail is plane_ops.FUSED_TAIL_DEFAULT
    assert fpn.fused_merge_bf16 is plane_ops.FUSED_MERGE_BF16_DEFAULT
    net.fused_tail_bf16 = not plane_ops.FUSED_TAIL_BF16_DEFAULT
    assert all(m.fused_tail_bf16 is (not plane_ops.FUSED_TAIL_BF16_DEFAULT) for m in net.modules()
               if isinstance(m, blocks._Block))
    assert net.fused_tail is plane_ops.FUSED_TAIL_DEFAULT                          # the float32 flag is its own
    # a CPU bf16 forward takes the torch formulation whatever the flags say
    net.fused_tail_bf16 = True
    with torch.no_grad():
        outs = net.bfloat16().eval()(torch.randn(1, 3, 32, 32).bfloat16())
    assert all(o.dtype == torch.bfloat16 for o in outs)


def test_prototypes_parse_from_the_header():
    protos = _lib.prototypes()
    enqueueing = _lib.parse_enqueueing(_lib._header_text())
    V, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    want = {NAMES[0]: [LL, V, V, V, V], NAMES[1]: [LL, V, V, V, V], NAMES[2]: [I] * 6 + [V, V, V, V],
            NAMES[3]: [I] * 6 + [V, V, V]}
    for name in NAMES:
        restype, argtypes = protos[name]
        assert restype is ctypes.c_int and argtypes == want[name], name
        assert name in enqueueing                                                  # the stream is the last parameter
        fn = getattr(_lib.lib(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[name]
    text = _lib._header_text()
    for name in NAMES:                                                             # bf16 travels as unsigned short
        decl = text[text.index(name):]
        decl = decl[:decl.index(';')]
        assert decl.count('unsigned short *') == want[name].count(V) - 1 and 'float' not in decl
    ids = [_lib.K_ADD_RELU_BF16, _lib.K_ADD_RELU_BWD_BF16, _lib.K_UPSAMPLE_ADD_BF16, _lib.K_UPSAMPLE_ADD_BWD_BF16]
    assert ids == [113, 114, 115, 116] and _lib.K_OPTIM_STEP == 112 and _lib.K_ADD_RELU == 104
    L = _lib.lib()
    assert L.ocrf_kernel_name(ids[0]) == b'binary_bf16_kernel<*, AddRelu>'
    assert L.ocrf_kernel_name(ids[3]) == b'upsample_add_backward_bf16_kernel'


def test_c_boundary_refuses_bad_arguments():
    """Argument validation alone: the calls return before anything is launched, the pointers are never dereferenced."""
    L = _lib.lib()
    p = ctypes.c_void_p(4096)
    invalid = 1                                    # hipErrorInvalidValue
    for fn in (L.ocrf_add_relu_forward_bf16, L.ocrf_add_relu_backward_bf16):
        assert fn(0, p, p, p, None) == invalid and fn(-8, p, p, p, None) == invalid
        assert fn(1 << 30, p, p, p, None) == invalid                      # exactly 2 GiB of bf16
        assert fn(1 << 31, p, p, p, None) == invalid and fn(1 << 40, p, p, p, None) == invalid
        assert fn(16, None, p, p, None) == invalid and fn(16, p, None, p, None) == invalid
        assert fn(16, p, p, None, None) == invalid
    fwd, bwd = L.ocrf_upsample_add_forward_bf16, L.ocrf_upsample_add_backward_bf16
    # 48 x 256 x 256 x 704 elements = 4.1 GiB of destination; 1 x 4096 x 512 x 512 = exactly 2 GiB; products that overflow
    for shape in [(48, 256, 128, 352, 256, 704), (1, 4096, 256, 256, 512, 512), (1 << 16, 1 << 16, 1, 1, 1, 1),
                  (1 << 20, 1 << 20, 1, 1, 2, 2)]:
        assert fwd(*shape, p, p, p, None) == invalid
        assert bwd(*shape, p, p, None) == invalid
    assert fwd(1, 1, 8, 8, 4, 16, p, p, p, None) == invalid and fwd(1, 1, 8, 8, 16, 4, p, p, p, None) == invalid
    assert bwd(1, 1, 8, 8, 4, 16, p, p, None) == invalid and bwd(1, 1, 8, 8, 16, 4, p, p, None) == invalid
    assert fwd(1, 1, 8, 8, 4096, 4097, p, p, p, None) == invalid          # Hout + Wout > 8192
    assert bwd(1, 1, 8, 8, 4096, 4097, p, p, None) == invalid
    for bad in ((0, 1, 8, 8, 16, 16), (1, 0, 8, 8, 16, 16), (1, 1, 0, 8, 16, 16), (1, 1, 8, -8, 16, 16)):
        assert fwd(*bad, p, p, p, None) == invalid and bwd(*bad, p, p, None) == invalid
    assert fwd(1, 1, 8, 8, 16, 16, None, p, p, None) == invalid and fwd(1, 1, 8, 8, 16, 16, p, None, p, None) == invalid
    assert fwd(1, 1, 8, 8, 16, 16, p, p, None, None) == invalid
    assert bwd(1, 1, 8, 8, 16, 16, None, p, None) == invalid and bwd(1, 1, 8, 8, 16, 16, p, None, None) == invalid
