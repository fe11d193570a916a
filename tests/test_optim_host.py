"""CPU: the host side of the fused training-step tail (ocrfdet_amd/optim.py, csrc/optim.hip) — table layout, chunk
planner, param groups, the EMA ramp, state_dict compatibility and every refusal.  Nothing here touches a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch
from torch import nn

import ocrfdet_amd
from ocrfdet_amd import _lib, optim
from ocrfdet_amd._lib import OcrfHipError

CHUNK = _lib.OCRF_OPTIM_CHUNK
SIZES = [0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7]
# configs/ocrfdet/ocrfdet.py:261-269
KEYS = ['img_view_transformer.S_MLP', 'img_view_transformer.R_MLP', 'img_view_transformer.A_MLP',
        'img_view_transformer.C_MLP', 'img_view_transformer.C_MLP_nerf', 'img_view_transformer.D_MLP_nerf',
        'img_view_transformer.sigma', 'img_feat_resize1', 'img_feat_resize2']


def test_names_are_exported_lazily():
    assert ocrfdet_amd.FusedAdamW is optim.FusedAdamW and ocrfdet_amd.ModelEMA is optim.ModelEMA
    assert ocrfdet_amd.paramwise_groups is optim.paramwise_groups


def test_table_layout_agrees_with_the_compiler():
    assert optim.numpy_layout() == optim.c_layout()
    assert (optim.TENSOR_DT.itemsize, optim.CHUNK_DT.itemsize, optim.REC_DT.itemsize) == (48, 8, 40)
    assert len(optim.c_layout()) == _lib.OCRF_OPTIM_LAYOUT_INTS
    assert CHUNK > 0 and CHUNK % 4 == 0
    assert (optim.ADAM_EMA, optim.ADAM, optim.EMA_ONLY) == (0, 1, 2)


def test_kernel_ids_have_names():
    L = _lib.lib()
    assert L.ocrf_kernel_name(_lib.K_OPTIM_SQNORM) == b'optim_grad_sqnorm_kernel'
    assert L.ocrf_kernel_name(_lib.K_OPTIM_NORM_FINAL) == b'optim_norm_final_kernel'
    assert L.ocrf_kernel_name(_lib.K_OPTIM_STEP) == b'optim_step_kernel'
    # the per-step record changes every step: the entry points are not replayable
    assert L.ocrf_step_fn_id(b'ocrf_optim_step') == -1 and L.ocrf_step_fn_id(b'ocrf_optim_grad_sqnorm') == -1
    assert {'ocrf_optim_step', 'ocrf_optim_grad_sqnorm'} <= _lib._ENQUEUEING and 'ocrf_optim_layout' not in _lib._ENQUEUEING


@pytest.mark.parametrize('sizes', [SIZES, SIZES[::-1], [0, 0], [], [3 * CHUNK]])
def test_chunk_planner_covers_every_element_once(sizes):
    chunks = optim.plan_chunks(sizes)
    assert chunks.dtype == optim.CHUNK_DT
    covered = [np.zeros(n, dtype=np.int32) for n in sizes]
    for t, off in zip(chunks['tensor'].tolist(), chunks['offset'].tolist()):
        assert 0 <= t < len(sizes) and off % CHUNK == 0 and 0 <= off < sizes[t]       # inside ONE tensor, never empty
        covered[t][off:min(off + CHUNK, sizes[t])] += 1
    assert all((c == 1).all() for c in covered)
    assert len(chunks) == sum(-(-n // CHUNK) for n in sizes)
    assert not set(chunks['tensor'].tolist()) & {i for i, n in enumerate(sizes) if n == 0}
    order = list(zip(chunks['tensor'].tolist(), chunks['offset'].tolist()))
    assert order == sorted(order)


class _Neck(nn.Module):
    def __init__(self):
        super().__init__()
        for name in ('S_MLP', 'R_MLP', 'A_MLP', 'C_MLP', 'C_MLP_nerf', 'D_MLP_nerf', 'depth_net'):
            setattr(self, name, nn.Linear(2, 2))
        self.sigma = nn.Parameter(torch.zeros(1))
        self.other = nn.Parameter(torch.zeros(1))


class _Toy(nn.Module):
    def __init__(self):
        super().__init__()
        self.img_backbone = nn.Sequential(nn.Conv2d(1, 1, 1), nn.BatchNorm2d(1))
        self.img_view_transformer = _Neck()
        self.img_feat_resize1 = nn.Conv2d(1, 1, 1)
        self.img_feat_resize2 = nn.Conv2d(1, 1, 1)
        self.pts_bbox_head = nn.Linear(2, 2)


def test_paramwise_groups_follow_the_custom_keys():
    model = _Toy()
    custom = {k: dict(lr_mult=2) for k in KEYS}
    groups = optim.paramwise_groups(model, 2e-4, 1e-2, custom)
    names = [n for n, _ in model.named_parameters()]
    assert [g['name'] for g in groups] == names and all(len(g['params']) == 1 for g in groups)
    assert all(g['params'][0] is p for g, (_, p) in zip(groups, model.named_parameters()))
    for g in groups:
        matched = any(k in g['name'] for k in KEYS)
        assert g['lr'] == (4e-4 if matched else 2e-4), g['name']
        assert g['weight_decay'] == 1e-2
    by_name = {g['name']: g for g in groups}
    assert by_name['img_view_transformer.sigma']['lr'] == 4e-4 and by_name['img_feat_resize2.bias']['lr'] == 4e-4
    assert by_name['img_view_transformer.depth_net.weight']['lr'] == 2e-4
    assert by_name['img_view_transformer.other']['lr'] == 2e-4 and by_name['pts_bbox_head.weight']['lr'] == 2e-4
    # the longest key wins: C_MLP_nerf matches both 'C_MLP' and 'C_MLP_nerf'
    custom = dict(custom)
    custom['img_view_transformer.C_MLP'] = dict(lr_mult=3, decay_mult=0.5)
    custom['img_view_transformer.C_MLP_nerf'] = dict(lr_mult=5, decay_mult=0.0)
    by_name = {g['name']: g for g in optim.paramwise_groups(model, 2e-4, 1e-2, custom)}
    assert by_name['img_view_transformer.C_MLP_nerf.weight']['lr'] == pytest.approx(1e-3)
    assert by_name['img_view_transformer.C_MLP_nerf.weight']['weight_decay'] == 0.0
    assert by_name['img_view_transformer.C_MLP.weight']['lr'] == pytest.approx(6e-4)
    assert by_name['img_view_transformer.C_MLP.weight']['weight_decay'] == pytest.approx(5e-3)
    # keys of one length: alphabetical, first match wins
    by_name = {g['name']: g for g in optim.paramwise_groups(model, 1.0, 1.0, {'S_MLP.w': dict(lr_mult=7),
                                                                                'MLP.wei': dict(lr_mult=9)})}
    assert by_name['img_view_transformer.S_MLP.weight']['lr'] == 9.0


def test_model_ema_ramp_and_copy():
    model = _Toy()
    ema = optim.ModelEMA(model, decay=0.9990, updates=10560)
    ref = lambda x: 0.9990 * (1 - math.exp(-x / 2000))  # noqa: E731  (mmdet3d/core/hook/ema.py:44)
    for updates in (1, 2000, 10561):
        assert ema.decay(updates) == ref(updates)
    assert optim.ModelEMA(model).decay(2000) == 0.9999 * (1 - math.exp(-1.0))
    assert ema.updates == 10560 and ema.ema is not model and not ema.ema.training and model.training
    assert all(not p.requires_grad for p in ema.ema.parameters())
    assert list(ema.ema.state_dict()) == list(model.state_dict())
    d, omd = ema.next_decay()
    assert ema.updates == 10561 and d == ref(10561) and omd == 1.0 - d
    wrapped = nn.DataParallel(model)
    assert optim.ModelEMA(wrapped).source is model


def test_state_dict_round_trip_with_torch_adamw():
    """Key names and shapes both ways (the values travel on the GPU: test_optim_gpu.py)."""
    model = nn.Sequential(nn.Linear(3, 5), nn.Linear(5, 2))
    groups = lambda: [dict(params=[p], lr=1e-3 * (i + 1)) for i, p in enumerate(model.parameters())]  # noqa: E731
    ref = torch.optim.AdamW(groups(), lr=2e-4, weight_decay=1e-2, foreach=False)
    model(torch.ones(2, 3)).sum().backward()
    ref.step()
    sd = ref.state_dict()
    fused = optim.FusedAdamW(groups(), lr=5.0)
    fused.load_state_dict(sd)
    back = fused.state_dict()
    assert set(back['state']) == set(sd['state'])
    for k, st in sd['state'].items():
        assert set(back['state'][k]) == set(st) == {'step', 'exp_avg', 'exp_avg_sq'}
        for name in st:
            assert back['state'][k][name].shape == st[name].shape
            assert torch.equal(back['state'][k][name], st[name])
    for a, b in zip(back['param_groups'], sd['param_groups']):
        assert a['lr'] == b['lr'] and a['params'] == b['params'] and set(b) <= set(a)
    again = torch.optim.AdamW(groups(), foreach=False)
    again.load_state_dict(back)
    again.step()                                              # torch accepts what came back
    assert float(again.state[next(model.parameters())]['step']) == 2.0
    # a fresh FusedAdamW's groups carry every key torch.optim.AdamW's do
    fresh = optim.FusedAdamW(groups())
    assert set(torch.optim.AdamW(groups()).state_dict()['param_groups'][0]) <= set(fresh.state_dict()['param_groups'][0])
    assert fresh.defaults['lr'] == 1e-3 and fresh.defaults['betas'] == (0.9, 0.999) and fresh.defaults['eps'] == 1e-8
    assert fresh.defaults['weight_decay'] == 1e-2 and fresh.max_grad_norm is None


def test_entry_points_refuse_null_tables_and_non_positive_counts():
    L = _lib.lib()
    p = ctypes.c_void_p(4096)                     # any non-null value: never dereferenced, nothing is launched
    invalid = 1                                   # hipErrorInvalidValue
    n = ctypes.c_longlong(100)
    assert L.ocrf_optim_layout(None) == invalid
    ok_step = [p, 1, p, 1, p, n, None, 5.0, 0.5, 0.5, None]
    ok_norm = [p, 1, p, 1, p, n, p, p, None]
    for fn, ok, nulls in ((L.ocrf_optim_step, ok_step, (0, 2, 4)), (L.ocrf_optim_grad_sqnorm, ok_norm, (0, 2, 4, 6, 7))):
        for k in nulls:
            args = list(ok)
            args[k] = None
            assert fn(*args) == invalid, (fn.__name__, k)
        for k in (1, 3):
            for bad in (0, -1):
                args = list(ok)
                args[k] = bad
                assert fn(*args) == invalid, (fn.__name__, k, bad)
        for bad in (0, -5, 1 << 29, 1 << 40):     # a tensor of 2 GiB or more: the kernels index with int
            args = list(ok)
            args[5] = ctypes.c_longlong(bad)
            assert fn(*args) == invalid, (fn.__name__, bad)


def _param(t):
    return nn.Parameter(t)


def test_unsupported_inputs_raise_naming_the_parameter():
    # CPU tensors
    w = _param(torch.zeros(4, 3))
    w.grad = torch.ones(4, 3)
    opt = optim.FusedAdamW([dict(params=[w], name='head.weight')])
    with pytest.raises(OcrfHipError, match=r'gradient of parameter 0 of group 0 \(head\.weight, shape \(4, 3\)\) is on cpu'):
        opt.step()
    w.grad = None
    with pytest.raises(OcrfHipError, match=r'parameter 0 of group 0 \(head\.weight.* is on cpu'):
        opt.step()
    # not float32: parameter, gradient
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        h = _param(torch.zeros(4, dtype=dtype))
        with pytest.raises(OcrfHipError, match=rf'parameter 0 of group 0 \(shape \(4,\)\) is {dtype}'):
            optim.FusedAdamW([dict(params=[h]), dict(params=[w])]).step()
        h.grad = torch.zeros(4, dtype=dtype)
        with pytest.raises(OcrfHipError, match=rf'gradient of parameter 0 of group 1 .* is {dtype}'):
            optim.FusedAdamW([dict(params=[w]), dict(params=[h])]).step()
    # not contiguous: parameter, gradient
    nc = _param(torch.zeros(6, 4).t())
    with pytest.raises(OcrfHipError, match=r'parameter 0 of group 0 \(shape \(4, 6\)\) is not contiguous'):
        optim.FusedAdamW([nc, w]).step()
    c = _param(torch.zeros(4, 6))
    c.grad = torch.zeros(6, 4).t()
    with pytest.raises(OcrfHipError, match=r'gradient of parameter 1 of group 0 .* is not contiguous'):
        optim.FusedAdamW([w, c]).step()
    # sparse gradient
    emb = nn.Embedding(5, 3, sparse=True)
    emb(torch.tensor([1, 2])).sum().backward()
    assert emb.weight.grad.is_sparse
    with pytest.raises(OcrfHipError, match=r'gradient of parameter 0 of group 0 \(shape \(5, 3\)\) is a torch\.sparse_coo'):
        optim.FusedAdamW(emb.parameters()).step()
    # flags of torch.optim.AdamW that are not implemented: at construction, and when they arrive later
    for flag in ('amsgrad', 'maximize', 'capturable'):
        with pytest.raises(OcrfHipError, match=rf'{flag}=True is not implemented.*head\.weight'):
            optim.FusedAdamW([dict(params=[w], name='head.weight')], **{flag: True})
        late = optim.FusedAdamW([dict(params=[w], name='head.weight')])
        late.param_groups[0][flag] = True
        with pytest.raises(OcrfHipError, match=rf'{flag}=True'):
            late.step()
    with pytest.raises(ValueError):
        optim.FusedAdamW([w], max_grad_norm=0.0)
    with pytest.raises(ValueError):
        optim.FusedAdamW([w], betas=(1.0, 0.9))
    # the EMA has the same rule, naming the entry
    bn = nn.BatchNorm1d(3)
    with pytest.raises(OcrfHipError, match=r'EMA entry weight is on cpu'):
        optim.ModelEMA(bn).update(bn)
    with pytest.raises(OcrfHipError, match=r'EMA entry weight is torch\.float64'):
        optim.ModelEMA(bn.double()).update(bn)
    assert int(optim.ModelEMA(bn).ema.num_batches_tracked) == 0
