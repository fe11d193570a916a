"""Reads ``tests/golden/bev_encoder.npz`` (written by ``tests/golden/make_golden_bev_encoder.py``) for the host and the
GPU tests of ``ocrfdet_amd.bev_encoder``: builds this package's module for a case, loads the fixture's ``state_dict``
with ``strict=True``, runs it as the generator ran the reference and compares at the project's 1e-4 of the tensor's
largest magnitude.
"""
import json
import os

import numpy as np
import torch

from ocrfdet_amd import bev_encoder as be

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bev_encoder.npz')
TOL = 1e-4
_G = None


def golden():
    global _G
    if _G is None:
        with np.load(PATH) as g:
            _G = {k: g[k] for k in g.files}
    return _G


def cases():
    c = json.loads(str(golden()['cases']))
    return c['resnets'], c['fpns'], c['full']


def state_dict(tag):
    """The case's state_dict: the flat float16 array cut by ``.keys``; integer entries (num_batches_tracked) are 0."""
    g = golden()
    flat, at, state = g[f'{tag}.state'].astype(np.float32), 0, {}
    for key, shape, is_float in json.loads(str(g[f'{tag}.keys'])):
        if not is_float:
            state[key] = torch.zeros(shape, dtype=torch.int64)
            continue
        n = int(np.prod(shape, dtype=np.int64))
        state[key] = torch.from_numpy(flat[at:at + n].reshape(shape).copy())
        at += n
    assert at == flat.size
    return state


def build(tag):
    resnets, fpns, _ = cases()
    return be.CustomResNet(**resnets[tag]) if tag in resnets else be.FPN_LSS(**fpns[tag])


def inputs(tag):
    g = golden()
    resnets, _, _ = cases()
    names = ['x'] if tag in resnets else [f'resnet.eval.out{i}' for i in range(3)]
    return [torch.from_numpy(g[n].copy()) for n in names]


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, bound = float(np.abs(got - want).max()), TOL * float(np.abs(want).max())
    assert err <= bound, f'{what}: max|err| {err:.3e} > {bound:.3e}'


def check_case(tag, mode, device, fused=True):
    """Forward, input gradients, parameter gradients (sampled as the generator sampled them, and their norms) and, in
    train mode, the updated running statistics of case ``tag`` on ``device``."""
    g = golden()
    full = cases()[2]
    m = build(tag)
    m.load_state_dict(state_dict(tag), strict=True)
    m = m.to(device)
    m.train(mode == 'train')
    if isinstance(m, be.FPN_LSS):
        m.fused_upsample = fused
    leaves = [x.to(device).requires_grad_(True) for x in inputs(tag)]
    outs = m(leaves[0]) if isinstance(m, be.CustomResNet) else [m(leaves)]
    n_out = sum(1 for k in g if k.startswith(f'{tag}.R'))
    assert isinstance(outs, list) and len(outs) == n_out
    sum((o * torch.from_numpy(g[f'{tag}.R{i}']).to(device)).sum() for i, o in enumerate(outs)).backward()
    for i, o in enumerate(outs):
        close(o.detach().cpu().numpy(), g[f'{tag}.{mode}.out{i}'], f'{tag} {mode} out{i}')
    for i, x in enumerate(leaves):
        key = f'{tag}.{mode}.gx{i}'
        assert (x.grad is not None) == (key in g), key
        if x.grad is not None:
            close(x.grad.cpu().numpy(), g[key], f'{tag} {mode} gx{i}')
    grads, norms = [], []
    for k, p in m.named_parameters():
        gr = p.grad.detach().cpu().reshape(-1)
        norms.append(gr.double().norm().item())
        grads.append(gr[::-(-gr.numel() // full)].numpy())
    # per tensor, as the generator cut them: a tolerance relative to each tensor's own largest magnitude
    want, at = g[f'{tag}.{mode}.gp'], 0
    for (k, _), gr in zip(m.named_parameters(), grads):
        close(gr, want[at:at + gr.size], f'{tag} {mode} grad {k}')
        at += gr.size
    assert at == want.size
    assert np.allclose(norms, g[f'{tag}.{mode}.gnorm'], rtol=TOL, atol=0.0)
    if mode == 'train':
        stat = np.concatenate([v.cpu().numpy().reshape(-1) for k, v in m.state_dict().items() if 'running_' in k])
        close(stat, g[f'{tag}.train.stat'], f'{tag} running statistics')
    return m
