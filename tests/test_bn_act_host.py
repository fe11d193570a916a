"""Host: the ``fused_norm`` flag of the blocks and ``ConvModule`` (off by default, ``fuse_norms`` sets and clears it, a CPU
model is bit for bit the same with it on), what ``norm_ops.bn_act_fusable`` refuses, ``bn_act`` on the CPU, and the
argument validation of the ``ocrf_bn_*`` entry points (nothing is launched: no GPU needed)."""
import copy
import ctypes

import pytest
import torch
from torch import nn

from ocrfdet_amd import _lib, blocks, norm_ops

ENTRY_POINTS = ['ocrf_bn_chunks', 'ocrf_bn_stats', 'ocrf_bn_finalize', 'ocrf_bn_act_forward',
                'ocrf_bn_act_backward_reduce', 'ocrf_bn_act_backward', 'ocrf_bn_stats_bf16', 'ocrf_bn_act_forward_bf16',
                'ocrf_bn_act_backward_reduce_bf16', 'ocrf_bn_act_backward_bf16']


def stack(with_cp=False):
    """A Bottleneck with a downsample, a Bottleneck, a BasicBlock and a ConvModule with norm and ReLU."""
    down = nn.Sequential(nn.Conv2d(8, 16, 1, stride=2, bias=False), nn.BatchNorm2d(16))
    return nn.Sequential(blocks.Bottleneck(8, 4, stride=2, downsample=down, with_cp=with_cp),
                         blocks.Bottleneck(16, 4, with_cp=with_cp), blocks.BasicBlock(16, 16, with_cp=with_cp),
                         blocks.ConvModule(16, 8, 3, padding=1, norm_cfg=dict(type='BN'), act_cfg=dict(type='ReLU')))


def flags(model):
    return [m.fused_norm for m in model.modules() if isinstance(m, (blocks._Block, blocks.ConvModule))]


def test_the_flag_is_off_by_default_and_fuse_norms_sets_and_clears_it():
    assert blocks._Block.fused_norm is False and blocks.ConvModule.fused_norm is False
    model = stack()
    assert flags(model) == [False] * 4
    blocks.fuse_norms(model)
    assert flags(model) == [True] * 4
    blocks.fuse_norms(model, False)
    assert flags(model) == [False] * 4
    blocks.fuse_norms(model[1])
    assert flags(model) == [False, True, False, False]


@pytest.mark.parametrize('training', [True, False])
def test_a_cpu_model_is_bit_for_bit_the_same_with_the_flag_on(training):
    torch.manual_seed(0)
    model = stack().train(training)
    x = torch.randn(3, 8, 10, 12)
    results = []
    for flag in (False, True):
        m = copy.deepcopy(model)
        blocks.fuse_norms(m, flag)
        xi = x.clone().requires_grad_()
        out = m(xi)
        out.square().sum().backward()
        results.append([out.detach(), xi.grad] + [p.grad for p in m.parameters()]
                       + [b for b in m.buffers()])
    assert len(results[0]) == len(results[1])
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_state_dict_keys_do_not_depend_on_the_flag():
    model = stack()
    keys = list(model.state_dict())
    blocks.fuse_norms(model)
    assert list(model.state_dict()) == keys
    assert 'fused_norm' not in ''.join(keys)


class _OnGpu:
    """A tensor's metadata as the predicate reads it, claiming to be on a GPU: the logic without a device."""

    def __init__(self, t, device='cuda:0'):
        self._t, self.is_cuda, self.device = t, True, torch.device(device)

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_bn_act_fusable_takes_and_refuses():
    on = _OnGpu
    x = torch.randn(2, 4, 6, 8)
    one = x[:1, :, :1, :1].contiguous()            # one value per channel
    fusable = norm_ops.bn_act_fusable

    def bn(cls=nn.BatchNorm2d, channels=4, **kw):
        return cls(channels, **kw)

    def ok(m, x, residual=None):
        """The predicate on a norm whose vectors claim the GPU of ``x`` as well."""
        for held in (m._parameters, m._buffers):
            for name, v in held.items():
                if v is not None and name != 'num_batches_tracked':
                    held[name] = on(v)
        return fusable(m, x, residual)

    # the CPU is refused whatever the rest
    assert not fusable(bn(), x) and not fusable(bn(), x.bfloat16()) and not fusable(bn(), on(x))
    assert ok(bn(), on(x)) and ok(bn(), on(x.bfloat16())) and ok(bn(), on(x), on(x.clone()))
    assert ok(bn(track_running_stats=False), on(x)) and ok(bn(track_running_stats=False).eval(), on(x))
    assert ok(bn(momentum=None), on(x)) and ok(bn().eval(), on(one))
    assert not ok(nn.SyncBatchNorm(4), on(x))                                  # cross-rank statistics
    assert not ok(bn(affine=False), on(x))
    assert not ok(bn(), on(x.half())) and not ok(bn(), on(x.double()))
    assert not ok(bn(), on(x.permute(0, 1, 3, 2))) and not ok(bn(), on(x[:, :, ::2]))   # not contiguous
    assert not ok(bn(), on(x[0])) and not ok(bn(), on(x[:0]))                          # not 4-D, empty
    assert not ok(bn(), on(x), on(x[:, :, :3]))                                        # residual: another shape
    assert not ok(bn(), on(x), on(x.bfloat16())) and not ok(bn(), on(x.bfloat16()), on(x))   # another dtype
    assert not ok(bn(), on(x), on(x, 'cuda:1'))                                        # another device
    assert not ok(bn(), on(x), on(x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)))
    assert not ok(bn().half(), on(x)) and not ok(bn().double(), on(x))                 # parameters not float32
    assert one.is_contiguous() and not ok(bn(), on(one))                                          # one value per channel, training
    assert not ok(bn(track_running_stats=False).eval(), on(one))          # batch statistics in eval too
    assert ok(bn(), on(x[:2, :, :1, :1].contiguous()))                                 # two values: the minimum
    assert not ok(bn(channels=5), on(x))                                            # another channel count


def test_bn_act_refuses_the_cpu_and_never_falls_back():
    x = torch.randn(2, 4, 6, 8)
    for t in (x, x.bfloat16()):
        with pytest.raises(_lib.OcrfHipError):
            norm_ops.bn_act(nn.BatchNorm2d(4), t)
        with pytest.raises(_lib.OcrfHipError):
            norm_ops.bn_act(nn.BatchNorm2d(4), t, residual=t, relu=False)


def test_bn_act_torch_is_the_blocks_formulation():
    torch.manual_seed(1)
    bn, x, r = nn.BatchNorm2d(4), torch.randn(2, 4, 6, 8), torch.randn(2, 4, 6, 8)
    want = torch.relu(nn.functional.batch_norm(x, None, None, bn.weight, bn.bias, True, 0.1, bn.eps) + r)
    assert torch.equal(norm_ops.bn_act_torch(bn, x, r), want)
    assert int(bn.num_batches_tracked) == 1
    bn.eval()
    assert torch.equal(norm_ops.bn_act_torch(bn, x, relu=False), bn(x))


def test_entry_points_are_declared_and_have_kernel_names():
    protos, L = _lib.prototypes(), _lib.lib()
    assert set(ENTRY_POINTS) <= set(protos)
    assert all(protos[n][1][-1] is ctypes.c_void_p for n in ENTRY_POINTS[1:])        # the stream comes last
    assert ENTRY_POINTS[0] not in _lib._ENQUEUEING and set(ENTRY_POINTS[1:]) <= _lib._ENQUEUEING
    ids = [_lib.K_BN_STATS, _lib.K_BN_FINALIZE, _lib.K_BN_ACT_FWD, _lib.K_BN_ACT_BWD_REDUCE, _lib.K_BN_ACT_BWD,
           _lib.K_BN_STATS_BF16, _lib.K_BN_ACT_FWD_BF16, _lib.K_BN_ACT_BWD_REDUCE_BF16, _lib.K_BN_ACT_BWD_BF16]
    assert ids == list(range(123, 132))
    assert L.ocrf_kernel_name(_lib.K_BN_ACT_FWD) == b'bn_act_forward_kernel<float, *>'
    assert L.ocrf_kernel_name(_lib.K_BN_ACT_BWD_BF16) == b'bn_act_backward_kernel<unsigned short, *>'


def test_the_number_of_chunks_follows_from_the_shape_alone():
    L = _lib.lib()
    assert L.ocrf_bn_chunks(3, 5, 7, 9) == 1 and L.ocrf_bn_chunks(2, 3, 1, 1) == 1
    assert L.ocrf_bn_chunks(1, 1, 64, 64) == 1 and L.ocrf_bn_chunks(1, 9, 64, 65) == 2
    assert L.ocrf_bn_chunks(48, 64, 64, 176) == 48 * 64 * 176 // 4096
    assert L.ocrf_bn_chunks(0, 1, 1, 1) == 0 and L.ocrf_bn_chunks(1, 1, 1, -1) == 0
    assert L.ocrf_bn_chunks(2, 1, 1 << 15, 1 << 15) == 0 and L.ocrf_bn_chunks(1, 2, 1 << 15, 1 << 15) == 0
    assert L.ocrf_bn_chunks(1, 1, (1 << 15) - 1, 1 << 16) == ((1 << 31) - (1 << 16)) // 4096


def test_entry_points_refuse_two_to_the_31_elements_and_null_operands_at_the_c_boundary():
    """Argument validation alone: the calls return before anything is launched."""
    L = _lib.lib()
    p, invalid = ctypes.c_void_p(4096), 1          # any non-null, 16-byte aligned value: never dereferenced
    big = (1, 2, 1 << 15, 1 << 15)                 # 2^31 elements
    for suffix in ('', '_bf16'):
        assert getattr(L, 'ocrf_bn_stats' + suffix)(*big, p, p, None) == invalid
        assert getattr(L, 'ocrf_bn_act_forward' + suffix)(*big, p, p, p, p, 1, p, None) == invalid
        assert getattr(L, 'ocrf_bn_act_backward_reduce' + suffix)(*big, p, p, p, p, p, p, None) == invalid
        assert getattr(L, 'ocrf_bn_act_backward' + suffix)(*big, p, p, p, p, p, p, p, 1, p, p, p, p, None) == invalid
        small = (2, 3, 4, 5)
        assert getattr(L, 'ocrf_bn_stats' + suffix)(*small, None, p, None) == invalid
        assert getattr(L, 'ocrf_bn_act_forward' + suffix)(*small, p, None, p, p, 1, None, None) == invalid
        assert getattr(L, 'ocrf_bn_act_backward_reduce' + suffix)(*small, p, p, None, p, p, None, None) == invalid
        # dx with the batch's statistics, or a parameter gradient, without the sums; and nothing to write at all
        assert getattr(L, 'ocrf_bn_act_backward' + suffix)(*small, p, p, p, p, p, p, None, 1, p, None, None, None,
                                                            None) == invalid
        assert getattr(L, 'ocrf_bn_act_backward' + suffix)(*small, p, p, p, p, p, p, None, 0, p, None, p, None,
                                                            None) == invalid
        assert getattr(L, 'ocrf_bn_act_backward' + suffix)(*small, p, p, p, p, p, p, p, 1, None, None, None, None,
                                                            None) == invalid
    f = ctypes.c_float
    assert L.ocrf_bn_finalize(*big, 0, p, p, p, p, p, None, f(0.1), f(1e-5), p, p, p, p, None) == invalid
    assert L.ocrf_bn_finalize(2, 3, 4, 5, 0, None, p, p, p, p, None, f(0.1), f(1e-5), p, p, p, p, None) == invalid
    assert L.ocrf_bn_finalize(2, 3, 4, 5, 1, p, p, p, None, None, None, f(0.1), f(1e-5), p, p, p, p, None) == invalid
    # momentum None (< 0) needs num_batches_tracked; one value per channel has no unbiased variance
    assert L.ocrf_bn_finalize(2, 3, 4, 5, 0, p, p, p, p, p, None, f(-1.0), f(1e-5), p, p, p, p, None) == invalid
    assert L.ocrf_bn_finalize(1, 3, 1, 1, 0, p, p, p, p, p, None, f(0.1), f(1e-5), p, p, p, p, None) == invalid
