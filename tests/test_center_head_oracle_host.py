"""Host: the plain oracle of the CenterHead targets and losses (tests/center_head_oracle.py) reproduces the reference's
own values (``tests/golden/center_head.npz``); its cases are what they claim to be (asserted by ``build``: box counts,
filled slots past 256, shared cells, labels outside the class table, block counts, clipped logits); and the torch
formulation (``targets_torch`` / ``heatmap_loss_torch`` / ``reg_loss_torch``, float32 on the CPU) is held to the
oracle on every case with the bounds of ``center_head_oracle.check_*``: the NaN target code and the infinite box
dimension among them."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ocrfdet_amd import center_head as ch

from . import center_head_oracle as oracle

T = 6
NAMES = ('xy', 'z', 'whl', 'yaw', 'vel')


def run_torch(c, dev='cpu'):
    """The case through ``targets_torch`` / ``heatmap_loss_torch`` / ``reg_loss_torch`` in float32 on ``dev`` ->
    namespace of tg (the five arrays, None without the part), hm (out, clipped, grads), reg (list of (out, grads))."""
    res = SimpleNamespace(tg=None, hm=None, reg=None)
    T, B, M, C, H, W = c.tg.shape
    if 'targets' in c.parts:
        got = ch.targets_torch(*(torch.from_numpy(a).to(dev) for a in (c.boxes, c.labels, c.offsets, c.table)),
                               c.ncls, c.cfg, c.with_velocity, c.norm_bbox)
        res.tg = tuple(a.cpu().numpy() for a in got)
    if 'hm' in c.parts:
        x = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in c.logits]
        heat = [torch.from_numpy(h).to(dev) for h in c.tg.heat]
        counts = torch.tensor(np.concatenate([c.tg.ones, c.tg.msum]), dtype=torch.float32, device=dev)
        clipped, out = ch.heatmap_loss_torch(x, heat, counts, c.hm_weight)
        out = torch.stack(out)
        out.backward(torch.tensor(c.hm_grad_out, dtype=torch.float32, device=dev))
        res.hm = (out.detach().cpu().numpy(), [p.detach().cpu().numpy() for p in clipped],
                  [v.grad.cpu().numpy() for v in x])
    if 'reg' in c.parts:
        res.reg, cw = [], c.cfg['code_weights']
        anno, ind, mask = (torch.from_numpy(a).to(dev) for a in (c.tg.anno, c.tg.ind, c.tg.mask))
        for go in c.reg_grad_outs:
            heads = [{n: torch.from_numpy(a).to(dev).requires_grad_(True) for n, a in h.items()} for h in c.heads]
            rows = []
            for t in range(T):
                num = torch.tensor(c.tg.msum[t], dtype=torch.float32, device=dev)
                five = ch.reg_loss_torch(heads[t], anno[t], ind[t], mask[t], num, cw, c.reg_weight, True)
                one = ch.reg_loss_torch(heads[t], anno[t], ind[t], mask[t], num, cw, c.reg_weight, False)
                rows.append(torch.stack(five + one))
            out = torch.stack(rows)
            out.backward(torch.tensor(go, dtype=torch.float32, device=dev))
            res.reg.append((out.detach().cpu().numpy(),
                            [{n: v.grad.cpu().numpy() for n, v in h.items()} for h in heads]))
    return res


@pytest.fixture(scope='module')
def g(golden):
    return golden('center_head.npz')


@pytest.fixture(scope='module')
def gold(g):
    """The oracle's targets on the golden's boxes."""
    c = json.loads(str(g['cfg']))
    ncls = [len(t['class_names']) for t in c['tasks']]
    n = sum(1 for k in g.files if k.startswith('boxes'))
    boxes = [g[f'boxes{b}'].reshape(-1, 9) for b in range(n)]
    offsets = np.concatenate([[0], np.cumsum([len(b) for b in boxes])])
    tg = oracle.targets(np.concatenate(boxes), np.concatenate([g[f'labels{b}'] for b in range(n)]), offsets,
                        oracle._table(ncls), ncls, c['train_cfg'], True, True)
    return tg, c['train_cfg']


def test_oracle_targets_reproduce_the_golden(g, gold):
    tg, _ = gold
    for t in range(T):
        assert np.array_equal(tg.heat[t], g[f'heatmap{t}']), t
        assert np.array_equal(tg.ind[t], g[f'ind{t}']) and np.array_equal(tg.mask[t], g[f'mask{t}']), t
        assert tg.ones[t] == g[f'num_pos{t}'] and tg.msum[t] == g[f'mask{t}'].sum(), t
        a, w = tg.anno[t], g[f'anno_box{t}']
        assert np.array_equal(a[..., [0, 1, 2, 8, 9]], w[..., [0, 1, 2, 8, 9]]), t
        assert oracle._ulps(a[..., 3:8], w[..., 3:8]).max() <= 2, t


@pytest.mark.parametrize('ts', [True, False])
def test_oracle_losses_reproduce_the_golden(g, gold, ts):
    tg, cfg = gold
    tag = 'ts' if ts else 'all'
    heads = [{n: g[f'fwd.t{t}.{n}'] for n, _ in oracle.HEADS} for t in range(T)]
    go = np.tile(np.array([1.0] * 5 + [0.0] if ts else [0.0] * 5 + [1.0]), (T, 1))
    hm = oracle.heatmap_loss([g[f'fwd.t{t}.heatmap'] for t in range(T)], tg.heat, tg.ones, 1.0, np.ones(T))
    reg = oracle.reg_loss(heads, tg.anno, tg.ind, tg.mask, tg.msum, cfg['code_weights'], 0.25, go)
    if ts:
        got = {f'task{t}.loss_{n}': reg.out[t, j] for t in range(T) for j, n in enumerate(NAMES)}
        got.update({f'task{t}.loss_heatmap': hm.out[t] for t in range(T)})
    else:
        got = {'loss': reg.out[:, 5].sum() + hm.out.sum()}
    keys = json.loads(str(g[f'loss_keys.{tag}']))
    assert sorted(got) == keys
    want = g[f'losses32.{tag}'].astype(np.float64)
    have = np.array([got[k] for k in keys])
    assert np.all(np.abs(have - want) <= 1e-6 * np.maximum(np.abs(want), 1e-30)), (have, want)
    for t in range(T):
        for n, grad in list(reg.grads[t].items()) + [('heatmap', hm.grads[t])]:
            w = g[f'grad.{tag}.t{t}.{n}'].astype(np.float64)
            assert np.abs(grad - w).max() <= 1e-6 * max(np.abs(w).max(), 1e-30), (t, n)


@pytest.mark.parametrize('name', list(oracle.CASES))
def test_case_is_what_it_claims(name):
    c = oracle.build(name)                             # ``_expect`` asserts the case's claims
    assert c.cfg['code_weights'] == oracle.CODE_WEIGHTS and len(set(oracle.CODE_WEIGHTS)) == 10
    if name == 'dense':
        assert (c.tg.mask[0, 0, 256:] == 1).sum() > 20 and c.tg.shape[2] == 300


@pytest.mark.parametrize('name', list(oracle.CASES))
def test_torch_formulation_matches_oracle(name):
    c = oracle.build(name)
    got = run_torch(c)
    if got.tg is not None:
        oracle.check_targets(got.tg, c.tg)
    if got.hm is not None:
        e = oracle.check_heatmap_loss(*got.hm, c)
        print(f'{name}: heat-map gradient e_torch ' + ', '.join(f'{k} {v:.2e}' for k, v in e.items()))
    for i, (out, grads) in enumerate(got.reg or ()):
        e = oracle.check_reg_loss(out, grads, c, i)
        print(f'{name}: regression gradient {i} e_torch ' + ', '.join(f'{k} {v:.2e}' for k, v in e.items()))


def test_nan_target_code_torch():
    """The loss of the NaN code's group and of the single sum is NaN, the gradient at that code is 0, every other
    gradient is finite (and equal to the oracle's: test_torch_formulation_matches_oracle)."""
    c = oracle.build('nan_code')
    out, grads = run_torch(c).reg[0]
    assert np.isnan(out[0, 4]) and np.isnan(out[0, 5]) and np.isfinite(np.delete(out.reshape(-1), [4, 5])).all()
    cell = int(c.tg.ind[0, 0, 1])
    vel = grads[0]['vel'][0].reshape(2, -1)
    assert vel[0, cell] == 0 and vel[1, cell] != 0
    assert all(np.isfinite(v).all() for per in grads for v in per.values())


def test_infinite_dimension_torch():
    """A box with an infinite width is drawn with min_radius."""
    c = oracle.build('inf_dim')
    heat = run_torch(c).tg[0]
    H, W = c.tg.shape[4:]
    plane = heat[:H * W].reshape(H, W)
    iy, ix = divmod(int(c.tg.ind[0, 0, 1]), W)
    assert plane[iy, ix] == 1 and (plane == 0).any()   # a radius of 65536 would leave no cell of the plane at 0
    assert np.array_equal(plane, c.tg.heat[0][0, 0])
