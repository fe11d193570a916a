"""GPU: the fused CenterHead targets and losses (csrc/center_head.hip) against the plain oracle of
tests/center_head_oracle.py on its cases: more than 256 boxes per sample and filled slots past slot 256, maps that are
no multiple of a block, smaller than one and wider than 255 cells, 1 and 8 tasks with 64 planes, more than 256 loss
blocks per task with a ragged last block, labels outside the class table, ten distinct code weights, a NaN target code
and an infinite box dimension.  ``targets_fused``, ``HeatmapLoss`` and ``RegLoss`` are called directly; the losses run
on the oracle's targets, so that each part is held on its own.  Bounds: ``center_head_oracle.check_*``, the gradients by
region with the float32 torch formulation's own error (``e_torch``, CPU) printed beside the fused one.  Also:
bit-identical reruns, and the refusals at 9 tasks, 65 planes and max_objs 16385 that leave their outputs untouched."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib
from ocrfdet_amd import center_head as ch

from . import center_head_oracle as oracle
from .test_center_head_oracle_host import run_torch

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def torch_errors(name):
    """The float32 torch formulation (CPU) against the oracle: (heat-map regions, [regression heads per grad_out])."""
    c = oracle.build(name)
    got = run_torch(c)
    hm = oracle.check_heatmap_loss(*got.hm, c) if got.hm is not None else None
    return hm, [oracle.check_reg_loss(out, grads, c, i) for i, (out, grads) in enumerate(got.reg or ())]


def fused_targets(c, dev):
    got = ch.targets_fused(*(torch.from_numpy(a).to(dev) for a in (c.boxes, c.labels, c.offsets, c.table)), c.ncls,
                           c.cfg, c.with_velocity, c.norm_bbox)
    return tuple(a.cpu().numpy() for a in got)


def _counts(c, dev):
    return torch.tensor(np.concatenate([c.tg.ones, c.tg.msum]), dtype=torch.float32, device=dev)


def fused_heatmap_loss(c, dev):
    x = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in c.logits]
    out, *clipped = ch.HeatmapLoss.apply(torch.from_numpy(c.tg.flat).to(dev), _counts(c, dev), c.hm_weight, *x)
    out.backward(torch.from_numpy(c.hm_grad_out).to(dev))
    assert all(torch.equal(v.detach().cpu(), torch.from_numpy(a)) for v, a in zip(x, c.logits))     # inputs not written
    return out.detach().cpu().numpy(), [p.cpu().numpy() for p in clipped], [v.grad.cpu().numpy() for v in x]


def fused_reg_loss(c, dev, i):
    names = [n for n, _ in oracle.HEADS]
    heads = [{n: torch.from_numpy(a).to(dev).requires_grad_(True) for n, a in h.items()} for h in c.heads]
    flat = [h.get(n) for h in heads for n in names]                  # vel is None without velocity
    anno, ind, mask = (torch.from_numpy(a).to(dev) for a in (c.tg.anno, c.tg.ind, c.tg.mask))
    out = ch.RegLoss.apply(anno, ind, mask, _counts(c, dev), c.cfg['code_weights'], c.reg_weight, c.with_velocity, *flat)
    out.backward(torch.from_numpy(c.reg_grad_outs[i]).to(dev))
    return out.detach().cpu().numpy(), [{n: v.grad.cpu().numpy() for n, v in h.items()} for h in heads]


def _fmt(e):
    return ', '.join(f'{k} {v:.2e}' for k, v in e.items())


@pytest.mark.parametrize('name', oracle.cases_with('targets'))
def test_fused_targets_match_oracle(cuda, name):
    c = oracle.build(name)
    got = oracle.check_targets(fused_targets(c, cuda), c.tg)
    print(f'{name}: targets exact; heat map worst {got["heat_ulp"]:.0f} ulp ({got["heat_inexact"]} cells inexact), '
          f'anno 3:8 worst {got["anno_ulp"]:.0f} ulp')


@pytest.mark.parametrize('name', oracle.cases_with('hm'))
def test_fused_heatmap_loss_matches_oracle(cuda, name):
    c = oracle.build(name)
    e_torch = torch_errors(name)[0]
    out, clipped, grads = fused_heatmap_loss(c, cuda)
    print(f'{name}: heat-map loss {out} (oracle {c.hm.out})')
    e_fused = oracle.heatmap_errors(grads, c)
    print(f'{name}: heat-map gradient e_torch {_fmt(e_torch)}')
    print(f'{name}: heat-map gradient e_fused {_fmt(e_fused)}')
    oracle.check_heatmap_loss(out, clipped, grads, c, e_torch)


@pytest.mark.parametrize('name', oracle.cases_with('reg'))
def test_fused_reg_loss_matches_oracle(cuda, name):
    c = oracle.build(name)
    for i in range(len(c.reg_grad_outs)):
        e_torch = torch_errors(name)[1][i]
        out, grads = fused_reg_loss(c, cuda, i)
        e_fused = oracle.reg_errors(grads, c, i)
        print(f'{name}: regression gradient {i} e_torch {_fmt(e_torch)}')
        print(f'{name}: regression gradient {i} e_fused {_fmt(e_fused)}')
        oracle.check_reg_loss(out, grads, c, i, e_torch)


def test_nan_target_code_fused(cuda):
    """The loss of the NaN code's group and of the single sum is NaN; the gradient at that code is 0 and every other
    gradient finite (and the oracle's: test_fused_reg_loss_matches_oracle)."""
    c = oracle.build('nan_code')
    out, grads = fused_reg_loss(c, cuda, 0)
    assert np.isnan(out[0, 4]) and np.isnan(out[0, 5]) and np.isfinite(np.delete(out.reshape(-1), [4, 5])).all()
    cell = int(c.tg.ind[0, 0, 1])
    vel = grads[0]['vel'][0].reshape(2, -1)
    assert vel[0, cell] == 0 and vel[1, cell] != 0
    assert all(np.isfinite(v).all() for per in grads for v in per.values())


def test_infinite_dimension_fused(cuda):
    """A box with an infinite width is drawn with min_radius, as the torch formulation draws it."""
    c = oracle.build('inf_dim')
    heat = fused_targets(c, cuda)[0]
    H, W = c.tg.shape[4:]
    plane = heat[:H * W].reshape(H, W)
    iy, ix = divmod(int(c.tg.ind[0, 0, 1]), W)
    assert plane[iy, ix] == 1 and (plane == 0).any()   # a radius of 65536 would leave no cell of the plane at 0
    assert np.array_equal(plane == 0, c.tg.heat[0][0, 0] == 0)


@pytest.mark.parametrize('name', oracle.RERUN)
def test_reruns_bit_identical(cuda, name):
    c = oracle.build(name)
    runs = []
    for _ in range(2):
        arrays = list(fused_targets(c, cuda))
        out, clipped, grads = fused_heatmap_loss(c, cuda)
        arrays += [out, *clipped, *grads]
        if 'reg' in c.parts:
            out, grads = fused_reg_loss(c, cuda, 0)
            arrays += [out] + [v for per in grads for v in per.values()]
        runs.append(arrays)
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


# --------------------------------------------------------------------------------------------- refusals
SENTINEL = 7.0


def _target_buffers(dev, T, B, M, planes, HW):
    return (torch.full((B * planes * HW,), SENTINEL, device=dev), torch.full((T, B, M, 10), SENTINEL, device=dev),
            torch.full((T, B, M), 7, dtype=torch.int64, device=dev),
            torch.full((T, B, M), 7, dtype=torch.uint8, device=dev), torch.full((2 * T,), SENTINEL, device=dev))


def _untouched(*tensors):
    torch.cuda.synchronize()
    return all(bool((t == 7).all()) for t in tensors)


@pytest.mark.parametrize('ncls', [[1] * 9, [8] * 7 + [9]], ids=['9_tasks', '65_planes'])
def test_targets_refuse_too_many_tasks_or_planes(cuda, ncls):
    c = oracle.build('one_task')
    T, B, M, H, W = len(ncls), 1, 4, 5, 7
    assert T > _lib.OCRF_CH_MAX_TASKS or sum(ncls) > _lib.OCRF_CH_MAX_PLANES
    table = torch.from_numpy(oracle._table(ncls)).to(cuda)
    boxes, labels, offsets = (torch.from_numpy(a).to(cuda) for a in (c.boxes, c.labels, c.offsets))
    outs = _target_buffers(cuda, T, B, M, sum(ncls), H * W)
    ws = torch.empty(4096, dtype=torch.uint8, device=cuda)
    vs, pc = (ctypes.c_float * 2)(0.125, 0.125), (ctypes.c_float * 2)(-1.75, -1.25)
    with pytest.raises(_lib.OcrfHipError, match='hipError_t 1$'):
        _lib.launch('ocrf_center_head_targets', cuda, B, T, (ctypes.c_int * T)(*ncls), table.shape[0], table,
                    boxes.shape[0], boxes.shape[1], boxes, labels, offsets, H, W, M, 1, 1, vs, pc, 4, 0.1, 0, *outs, ws,
                    ws.numel())
    assert _untouched(*outs)


def test_losses_refuse_nine_tasks(cuda):
    T, B, HW, M = 9, 1, 35, 4
    ncls = (ctypes.c_int * T)(*[1] * T)
    x = [torch.zeros(B, 1, HW, device=cuda) for _ in range(T)]
    heat = torch.zeros(T * B * HW, device=cuda)
    counts = torch.ones(2 * T, device=cuda)
    outs = [torch.full((B, 1, HW), SENTINEL, device=cuda) for _ in range(T)]
    out, dens = torch.full((T,), SENTINEL, device=cuda), torch.full((T,), SENTINEL, device=cuda)
    ws = torch.empty(4096, dtype=torch.uint8, device=cuda)
    with pytest.raises(_lib.OcrfHipError, match='hipError_t 1$'):
        _lib.launch('ocrf_center_head_heatmap_loss', cuda, B, T, ncls, HW, ch._ptrs(x), heat, counts, 1.0, ch._ptrs(outs),
                    out, dens, ws, ws.numel())
    with pytest.raises(_lib.OcrfHipError, match='hipError_t 1$'):
        _lib.launch('ocrf_center_head_heatmap_loss_backward', cuda, B, T, ncls, HW, ch._ptrs(x), heat, counts[:T],
                    counts[:T], 1.0, ch._ptrs(outs))
    assert _untouched(out, dens, *outs)
    heads = [torch.zeros(B, k, HW, device=cuda) for _ in range(T) for _, k in oracle.HEADS]
    grads = [torch.full_like(h, SENTINEL) for h in heads]
    anno = torch.zeros(T, B, M, 10, device=cuda)
    ind = torch.zeros(T, B, M, dtype=torch.int64, device=cuda)
    mask = torch.ones(T, B, M, dtype=torch.uint8, device=cuda)
    cw = (ctypes.c_float * 10)(*oracle.CODE_WEIGHTS)
    out6, dens2 = torch.full((T, 6), SENTINEL, device=cuda), torch.full((T, 2), SENTINEL, device=cuda)
    with pytest.raises(_lib.OcrfHipError, match='hipError_t 1$'):
        _lib.launch('ocrf_center_head_reg_loss', cuda, B, T, HW, M, 1, ch._ptrs(heads), anno, ind, mask, cw, counts, 0.25,
                    out6, dens2, ws, ws.numel())
    with pytest.raises(_lib.OcrfHipError, match='hipError_t 1$'):
        _lib.launch('ocrf_center_head_reg_loss_backward', cuda, B, T, HW, M, 1, ch._ptrs(heads), anno, ind, mask, cw,
                    torch.ones(T, 2, device=cuda), torch.ones(T, 6, device=cuda), 0.25, ch._ptrs(grads))
    assert _untouched(out6, dens2, *grads)


def test_reg_loss_backward_refuses_max_objs_16385(cuda):
    """The backward keeps a sample's indices in LDS: 16384 slots are accepted (and written), 16385 refused."""
    T, B, HW = 1, 1, 35
    cw = (ctypes.c_float * 10)(*oracle.CODE_WEIGHTS)
    dens, go = torch.ones(T, 2, device=cuda), torch.ones(T, 6, device=cuda)
    heads = [torch.zeros(B, k, HW, device=cuda) for _, k in oracle.HEADS]
    for M, refused in ((16384, False), (16385, True)):
        anno = torch.ones(T, B, M, 10, device=cuda)
        ind = torch.full((T, B, M), 3, dtype=torch.int64, device=cuda)
        mask = torch.zeros(T, B, M, dtype=torch.uint8, device=cuda)
        mask[..., -1] = 1                              # the last slot alone is filled
        grads = [torch.full_like(h, SENTINEL) for h in heads]
        args = (B, T, HW, M, 1, ch._ptrs(heads), anno, ind, mask, cw, dens, go, 0.25, ch._ptrs(grads))
        if refused:
            with pytest.raises(_lib.OcrfHipError, match='hipError_t 1$'):
                _lib.launch('ocrf_center_head_reg_loss_backward', cuda, *args)
            assert _untouched(*grads)
        else:
            _lib.launch('ocrf_center_head_reg_loss_backward', cuda, *args)
            torch.cuda.synchronize()
            # only cell 3 is written: -(0.25 + 0.25) * code weight, the last slot's contribution
            for (name, k), gr in zip(oracle.HEADS, grads):
                assert bool((gr[0, :, [0, 1, 2] + list(range(4, HW))] == SENTINEL).all()), name
            want = -0.5 * np.array(oracle.CODE_WEIGHTS, np.float32)
            got = torch.cat([gr[0, :, 3] for gr in grads]).cpu().numpy()
            assert np.array_equal(got, want), (got, want)
