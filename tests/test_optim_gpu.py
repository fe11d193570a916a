"""GPU: the fused training-step tail (ocrfdet_amd/optim.py, csrc/optim.hip) against the sequence it replaces, run on
the CPU in float64: ``clip_grad_norm_`` + ``torch.optim.AdamW(foreach=False)`` + the two-line EMA loop of
mmdet3d/core/hook/ema.py:57-60.

Tolerance.  Nothing is hard-coded for p, exp_avg, exp_avg_sq and ema: the same torch sequence runs in float32 on the
CPU, its max absolute error against the float64 oracle is ``e_torch``, and the fused result must stay within
2 x e_torch per quantity (the norm is summed in another order, so coef and hence g may differ by an ulp, which can move
a result by one more rounding).  total_norm: 1e-5 relative to the float64 norm, the project's tolerance for fused
losses.

Recipe.  One tensor per size of SIZES (an empty one, sizes around the 4-element group and around the chunk), random
values; parameter VIEW is a view at a 4-byte offset into a larger allocation (4-byte accesses while its neighbours take
16-byte ones), parameter NOGRAD never has a gradient, lr alternates between 2e-4 and 4e-4, gradients are scaled x3 on
even steps (clipping active) and x0.01 on odd ones (inactive), fresh gradient tensors every step, the EMA starts away
from the weights with ``updates`` = 10560, BN running statistics move every step.
"""
import copy
import math

import numpy as np
import pytest
import torch
from torch import nn

from ocrfdet_amd import _lib, optim

pytestmark = pytest.mark.gpu

CHUNK = _lib.OCRF_OPTIM_CHUNK
SIZES = [0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7]
VIEW, NOGRAD = 7, 5
MAX_NORM, LR, WD, DECAY, UPDATES = 5.0, 2e-4, 1e-2, 0.9990, 10560
QUANTITIES = ('p', 'exp_avg', 'exp_avg_sq', 'ema')


class Bag(nn.Module):
    def __init__(self, values, dtype, device):
        super().__init__()
        self.ps = nn.ParameterList()
        for i, v in enumerate(values):
            t = torch.from_numpy(v).to(dtype, copy=True).to(device)          # the recipe's arrays stay as they are
            if i == VIEW:
                base = torch.zeros(t.numel() + 8, dtype=dtype, device=device)
                base[1:1 + t.numel()].copy_(t)
                t = base[1:1 + t.numel()]
            self.ps.append(nn.Parameter(t))
        self.bn = nn.BatchNorm1d(5).to(dtype).to(device)


def recipe(steps, seed=0):
    rng = np.random.default_rng(seed)
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    return dict(values=[f32(n) for n in SIZES], ema_shift=[0.5 * f32(n) for n in SIZES],
                grads=[[f32(n) * np.float32(3.0 if s % 2 == 0 else 0.01) for n in SIZES] for s in range(steps)],
                bn=[(0.1 * f32(5), np.abs(0.1 * f32(5))) for _ in range(steps)], steps=steps)


def groups(model):
    return [dict(params=[p], lr=LR * (1 + i % 2)) for i, p in enumerate(model.ps)]


def shifted_ema_copy(model, r, dtype, device):
    ema = copy.deepcopy(model).eval()
    with torch.no_grad():
        for p, s in zip(ema.ps, r['ema_shift']):
            p.add_(torch.from_numpy(s).to(dtype).to(device))
    return ema


def floating(module):
    return [v for v in module.state_dict().values() if v.dtype.is_floating_point]


def collect(model, opt, ema_module, norms):
    zeros = lambda p: torch.zeros_like(p)  # noqa: E731  (torch keeps no state for a parameter that never had a gradient)
    st = [opt.state.get(p, {}) for p in model.ps]
    out = dict(p=[p.detach().clone() for p in model.ps],
               exp_avg=[s['exp_avg'].clone() if s else zeros(p) for s, p in zip(st, model.ps)],
               exp_avg_sq=[s['exp_avg_sq'].clone() if s else zeros(p) for s, p in zip(st, model.ps)],
               ema=[v.clone() for v in floating(ema_module)] if ema_module is not None else [],
               step=[float(s['step']) if s else 0.0 for s in st], norm=norms)
    if ema_module is not None:
        out['tracked'] = int(ema_module.bn.num_batches_tracked)
    return out


def run_torch(r, dtype, state_after=None):
    """The reference's formulation on the CPU.  ``state_after``: also return (values, state_dict) after that many steps."""
    model = Bag(r['values'], dtype, 'cpu')
    opt = torch.optim.AdamW(groups(model), lr=LR, weight_decay=WD, foreach=False)
    ema = shifted_ema_copy(model, r, dtype, 'cpu')
    updates, norms, snapshot = UPDATES, [], None
    for s in range(r['steps']):
        if s == state_after:
            snapshot = ([p.detach().clone() for p in model.ps], copy.deepcopy(opt.state_dict()))
        for i, p in enumerate(model.ps):
            p.grad = None if i == NOGRAD else torch.from_numpy(r['grads'][s][i]).to(dtype, copy=True)   # clipped in place
        with torch.no_grad():
            model.bn.running_mean += torch.from_numpy(r['bn'][s][0]).to(dtype)
            model.bn.running_var += torch.from_numpy(r['bn'][s][1]).to(dtype)
            model.bn.num_batches_tracked += 1
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), MAX_NORM)))
        opt.step()
        with torch.no_grad():
            updates += 1
            d = DECAY * (1 - math.exp(-updates / 2000))
            msd = model.state_dict()
            for k, v in ema.state_dict().items():
                if v.dtype.is_floating_point:
                    v *= d
                    v += (1.0 - d) * msd[k].detach()
    out = collect(model, opt, ema, norms)
    return (out, snapshot) if state_after is not None else out


MOVED = (8, VIEW, 1)                                             # parameters that ``move_at`` gives a new storage


def run_fused(r, dev, attach=True, clip=True, sync_debug=False, with_ema=True, start=None, move_at=None):
    """``start``: (parameter values, a torch.optim.AdamW state_dict, first step) to continue from.  ``move_at``: before
    that step the parameters MOVED and BN's running mean get a new storage (``t.data = t.data.clone()``); the old
    storages are kept alive and returned with their values at that moment."""
    model = Bag(r['values'], torch.float32, dev)
    first = 0
    if start is not None:
        with torch.no_grad():
            for p, v in zip(model.ps, start[0]):
                p.copy_(v)
        first = start[2]
    opt = optim.FusedAdamW(groups(model), lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM if clip else None)
    if start is not None:
        opt.load_state_dict(start[1])
    ema = None
    if with_ema:
        ema = optim.ModelEMA(model, decay=DECAY, updates=UPDATES)
        with torch.no_grad():
            for p, s in zip(ema.ema.ps, r['ema_shift']):
                p.add_(torch.from_numpy(s).to(dev))
        if attach:
            opt.attach_ema(ema)
    # everything a step consumes is on the device before the first step (no blocking copy between steps)
    grads = [[torch.from_numpy(g).to(dev) for g in gs] for gs in r['grads']]
    bn = [(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)) for a, b in r['bn']]
    one = torch.ones((), dtype=torch.long, device=dev)
    norms, returned, left_behind = [], [], []
    torch.cuda.synchronize()
    if sync_debug:
        torch.cuda.set_sync_debug_mode('error')
    try:
        for s in range(first, r['steps']):
            opt.zero_grad(set_to_none=True)
            if s == move_at:
                for t in [model.ps[i] for i in MOVED] + [model.bn.running_mean]:
                    old = t.data
                    t.data = old.clone()
                    assert t.data_ptr() != old.data_ptr()
                    left_behind.append((old, old.clone()))
            for i, p in enumerate(model.ps):
                p.grad = None if i == NOGRAD else grads[s][i]
            with torch.no_grad():
                model.bn.running_mean += bn[s][0]
                model.bn.running_var += bn[s][1]
                model.bn.num_batches_tracked += one
            norm = opt.step()
            returned.append(norm)
            if clip:
                norms.append(norm.clone())
            if with_ema and not attach:
                ema.update(model)
    finally:
        if sync_debug:
            torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    out = collect(model, opt, ema.ema if ema is not None else None, [float(n) for n in norms])
    out.update(model=model, opt=opt, ema_obj=ema, returned=returned, grads=grads, left_behind=left_behind)
    return out


def max_err(got, want):
    return max([float((g.detach().cpu().double() - w.double()).abs().max()) for g, w in zip(got, want) if w.numel()] + [0.0])


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def check_against_oracle(got, r, steps_label):
    want, torch32 = run_torch(r, torch.float64), run_torch(r, torch.float32)
    for q in QUANTITIES:
        e_torch, e_fused = max_err(torch32[q], want[q]), max_err(got[q], want[q])
        print(f'{steps_label} {q}: e_torch {e_torch:.3e} e_fused {e_fused:.3e}')
        assert e_torch > 0
        assert e_fused <= 2 * e_torch, (q, e_fused, e_torch)
    assert len(got['norm']) == len(want['norm'])
    for s, (g, w) in enumerate(zip(got['norm'], want['norm'])):
        print(f'{steps_label} norm step {s}: fused {g!r} float64 {w!r}')
        assert abs(g - w) <= 1e-5 * w
    assert got['step'] == want['step']
    return want


@pytest.fixture(scope='module')
def r5():
    return recipe(5)


@pytest.fixture(scope='module')
def fused5(cuda, r5):
    return run_fused(r5, cuda)


def test_five_steps_match_the_float64_oracle(cuda, r5, fused5):
    model = fused5['model']
    assert model.ps[VIEW].data_ptr() % 16 == 4 and all(p.data_ptr() % 16 == 0 for i, p in enumerate(model.ps)
                                                         if i != VIEW and p.numel())
    want = check_against_oracle(fused5, r5, '5 steps')
    # clipping was active on the even steps and inactive on the odd ones
    assert [w > MAX_NORM for w in want['norm']] == [True, False, True, False, True]
    assert fused5['ema_obj'].updates == UPDATES + 5
    assert all(n.is_cuda and n.dim() == 0 and n.dtype is torch.float32 for n in fused5['returned'])
    # every step's record carried other gradient addresses (five tensors per parameter, all alive at once: the address
    # changes, not the allocator's free-and-reuse pattern behind a real backward())
    for i in (1, VIEW, 8):
        assert len({gs[i].data_ptr() for gs in fused5['grads']}) == 5


def test_buffers_are_averaged_and_counters_left_alone(cuda, r5, fused5):
    ema, model = fused5['ema_obj'].ema, fused5['model']
    assert fused5['tracked'] == 0 and int(model.bn.num_batches_tracked) == 5
    d = [DECAY * (1 - math.exp(-(UPDATES + k + 1) / 2000)) for k in range(5)]
    mean = np.zeros(5)
    var = np.ones(5)
    src_mean, src_var = np.zeros(5), np.ones(5)
    for k in range(5):
        src_mean, src_var = src_mean + r5['bn'][k][0], src_var + r5['bn'][k][1]
        mean, var = mean * d[k] + (1 - d[k]) * src_mean, var * d[k] + (1 - d[k]) * src_var
    assert np.abs(ema.bn.running_mean.cpu().numpy() - mean).max() < 1e-6
    assert np.abs(ema.bn.running_var.cpu().numpy() - var).max() < 1e-6
    assert np.abs(mean).max() > 1e-3                             # it did move


def test_a_tensor_without_gradient_keeps_its_bits(cuda, r5, fused5):
    p, opt = fused5['model'].ps[NOGRAD], fused5['opt']
    assert torch.equal(p.detach().cpu(), torch.from_numpy(r5['values'][NOGRAD]))
    assert fused5['step'][NOGRAD] == 0.0 and fused5['step'][NOGRAD + 1] == 5.0
    st = opt.state[p]
    assert not st or (float(st['step']) == 0.0 and not st['exp_avg'].any() and not st['exp_avg_sq'].any())
    # its EMA started 0.5 * N(0, 1) away from it and has moved towards it
    k = NOGRAD                                                   # state_dict order: ps.0 ... ps.8, then bn's entries
    start = torch.from_numpy(r5['values'][NOGRAD] + r5['ema_shift'][NOGRAD])
    now = fused5['ema'][k].cpu()
    assert not torch.equal(now, start)
    gap0, gap = (start - p.detach().cpu()).abs().max(), (now - p.detach().cpu()).abs().max()
    assert gap < gap0


def test_two_runs_give_the_same_bits(cuda, r5, fused5):
    again = run_fused(r5, cuda)
    for q in QUANTITIES:
        assert same_bits(again[q], fused5[q]), q
    assert again['norm'] == fused5['norm']


def test_attached_ema_equals_step_then_update(cuda, r5, fused5):
    apart = run_fused(r5, cuda, attach=False)
    for q in QUANTITIES:
        assert same_bits(apart[q], fused5[q]), q
    assert apart['ema_obj'].updates == UPDATES + 5 and apart['tracked'] == 0


def _count_launches(monkeypatch):
    names = []
    real = _lib.launch

    def counting(name, *args, **kwargs):
        names.append(name)
        return real(name, *args, **kwargs)
    monkeypatch.setattr(_lib, 'launch', counting)
    return names


def test_without_clipping_no_norm_kernel_is_launched(cuda, monkeypatch):
    names = _count_launches(monkeypatch)
    r = recipe(2)
    got = run_fused(r, cuda, clip=False, with_ema=False)
    assert names == ['ocrf_optim_step'] * 2
    assert got['returned'] == [None, None]
    assert not torch.equal(got['p'][8].cpu(), torch.from_numpy(r['values'][8]))


def test_a_step_with_ema_is_at_most_three_library_launches(cuda, monkeypatch):
    """Two entry-point calls; ``ocrf_optim_grad_sqnorm`` is two kernels, so three launches."""
    names = _count_launches(monkeypatch)
    r = recipe(1)
    run_fused(r, cuda)
    assert names == ['ocrf_optim_grad_sqnorm', 'ocrf_optim_step']
    del names[:]
    # ... whatever the tensor count: 40 more tensors
    model = nn.Sequential(*[nn.Linear(3, 3) for _ in range(20)]).to(cuda)
    opt = optim.FusedAdamW(model.parameters(), max_grad_norm=MAX_NORM)
    opt.attach_ema(optim.ModelEMA(model))
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    assert names == ['ocrf_optim_grad_sqnorm', 'ocrf_optim_step']
    del names[:]
    ema = optim.ModelEMA(model)
    ema.update(model)
    assert names == ['ocrf_optim_step'] and ema.updates == 1


@pytest.mark.parametrize('attach', [True, False])
def test_a_moved_tensor_is_followed(cuda, r5, fused5, attach):
    """``p.data = p.data.clone()`` (what ``module.to()`` does to a parameter) between two steps: the tables are rebuilt,
    the new storages are updated as if nothing had moved, and the old ones are not written again.  With ``attach``
    False the EMA's own table (``ModelEMA.update``) has to follow the moved sources as well."""
    got = run_fused(r5, cuda, attach=attach, move_at=2)
    assert len(got['left_behind']) == len(MOVED) + 1
    for q in QUANTITIES:
        assert same_bits(got[q], fused5[q]), q
    assert got['norm'] == fused5['norm'] and got['step'] == fused5['step']
    for old, then in got['left_behind']:
        assert torch.equal(old, then)
    assert got['model'].ps[VIEW].data_ptr() % 16 == 0           # the clone is no longer the unaligned view


def test_a_step_that_raises_leaves_the_counters(cuda, monkeypatch):
    r = recipe(2)
    got = run_fused(r, cuda)
    opt, ema, model = got['opt'], got['ema_obj'], got['model']
    real = _lib.launch

    def failing(name, *args, **kwargs):
        if name == 'ocrf_optim_step':
            raise _lib.OcrfHipError('ocrf_optim_step failed with hipError_t 1')
        return real(name, *args, **kwargs)
    monkeypatch.setattr(_lib, 'launch', failing)
    for p in model.ps:
        p.grad = None if p is model.ps[NOGRAD] else torch.ones_like(p)
    with pytest.raises(_lib.OcrfHipError):
        opt.step()
    with pytest.raises(_lib.OcrfHipError):
        ema.update(model)
    assert ema.updates == UPDATES + 2
    assert [float(opt.state[p]['step']) for p in model.ps] == got['step']
    monkeypatch.setattr(_lib, 'launch', real)
    opt.step()
    assert ema.updates == UPDATES + 3 and float(opt.state[model.ps[8]]['step']) == 3.0


def test_eight_steps_without_a_synchronisation(cuda):
    """More steps than the staging ring is deep, under ``set_sync_debug_mode('error')``: tables, staging buffers and
    state are built inside the first step, and no step reads the device or makes a blocking copy."""
    assert 8 > optim.RING_DEPTH
    r = recipe(8)
    got = run_fused(r, cuda, sync_debug=True)
    check_against_oracle(got, r, '8 steps')
    assert got['ema_obj'].updates == UPDATES + 8


def test_continues_from_a_torch_adamw_state_dict(cuda):
    """torch.optim.AdamW runs 2 steps, its state_dict is loaded into FusedAdamW, and the next fused step matches
    torch's next step."""
    r = recipe(3)
    want = run_torch(r, torch.float64)
    torch32, (values, sd) = run_torch(r, torch.float32, state_after=2)
    got = run_fused(r, cuda, with_ema=False, start=(values, sd, 2))
    for q in ('p', 'exp_avg', 'exp_avg_sq'):
        e_torch, e_fused = max_err(torch32[q], want[q]), max_err(got[q], want[q])
        print(f'after load_state_dict {q}: e_torch {e_torch:.3e} e_fused {e_fused:.3e}')
        assert 0 < e_torch and e_fused <= 2 * e_torch, (q, e_fused, e_torch)
    assert abs(got['norm'][0] - want['norm'][2]) <= 1e-5 * want['norm'][2]
    assert got['step'] == want['step'] == [0.0 if i == NOGRAD else 3.0 for i in range(len(SIZES))]
    # and back: torch loads what the fused optimizer saved
    back = torch.optim.AdamW(groups(got['model']), lr=LR, weight_decay=WD, foreach=False)
    back.load_state_dict(got['opt'].state_dict())
    assert float(back.state[got['model'].ps[8]]['step']) == 3.0
