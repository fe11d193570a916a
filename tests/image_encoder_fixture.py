"""Shared by ``tests/golden/make_golden_image_encoder.py`` and the host and GPU tests of ``ocrfdet_amd.image_encoder``:
the ``CustomFPN`` cases of ``tests/golden/image_encoder.npz``, the seeded weights and inputs (rebuilt here from integers
of numpy's ``default_rng``, never stored), and ``check_case``, which builds this package's ``CustomFPN`` for a case, loads
the seeded ``state_dict`` with ``strict=True``, runs it as the generator ran the reference and compares at 1e-5 of each
tensor's largest magnitude.
"""
import json
import os

import numpy as np
import torch

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'image_encoder.npz')
TOL = 1e-5
FULL = 256                                         # elements stored of a parameter gradient
SEED = 20261018

# tag -> (constructor arguments, input shapes, modes).  ``start1``: the reference creates ``fpn_convs`` by absolute level
# (``i in out_ids`` for i from start_level) and indexes them and the laterals by ``out_ids`` directly, so with
# ``start_level=1`` this is the smallest argument set whose ``forward`` runs: outs[0] = fpn_convs[0](laterals[0]) after
# the top-down merge, the other two outputs (the stride-2 extra conv on laterals[1]) are computed and dropped.  ``bn``
# has no ``act_cfg``: the reference's in-place ``+=`` on the output of a ReLU cannot be differentiated.
CASES = dict(
    odd=(dict(in_channels=[8, 16], out_channels=4, num_outs=1, out_ids=[0]),
         [(2, 8, 15, 21), (2, 16, 8, 11)], ('eval',)),
    start1=(dict(in_channels=[6, 8, 16], out_channels=4, num_outs=3, start_level=1, out_ids=[0, 1, 1],
                 add_extra_convs='on_lateral'),
            [(2, 6, 18, 26), (2, 8, 9, 13), (2, 16, 5, 7)], ('eval',)),
    scale2=(dict(in_channels=[8, 16], out_channels=4, num_outs=1, out_ids=[0],
                 upsample_cfg=dict(mode='nearest', scale_factor=2)),
            [(2, 8, 10, 14), (2, 16, 5, 7)], ('eval',)),
    bn=(dict(in_channels=[8, 16], out_channels=4, num_outs=1, out_ids=[0], norm_cfg=dict(type='BN')),
        [(2, 8, 12, 20), (2, 16, 6, 10)], ('eval', 'train')),
    ref=(dict(in_channels=[1024, 2048], out_channels=256, num_outs=1, start_level=0, out_ids=[0]),
         [(2, 1024, 4, 6), (2, 2048, 2, 3)], ('eval',)),
)


# ``wiring``: a small encoder for the reference's own ``BEVDet.image_encoder`` / ``extract_stereo_ref_feat``; its two
# state_dicts are seeded under the tags ``wiring.backbone`` and ``wiring.neck``
WIRING = dict(img_backbone=dict(type='ResNet', depth=18, base_channels=8, out_indices=(0, 2, 3), norm_eval=False),
              img_neck=dict(type='CustomFPN', in_channels=[32, 64], out_channels=6, num_outs=1, start_level=0,
                            out_ids=[0]),
              img=(1, 2, 3, 64, 96))
TAGS = list(CASES) + ['wiring', 'wiring.backbone', 'wiring.neck']


def _rng(tag, what):
    return np.random.default_rng([SEED, TAGS.index(tag), what])


def seeded_state(module, tag):
    """Convolution weights = integers in [-8, 8] / 4 * 2^round(log2(fan_in^-1/2)); norm weights and running variances
    in [0.5, 1.5), biases and running means in [-0.5, 0.5), on a 1/64 grid: products of weights and inputs are exact."""
    rng, state = _rng(tag, 0), {}
    for k, v in module.state_dict().items():
        if not v.dtype.is_floating_point:
            state[k] = torch.zeros_like(v)
            continue
        if v.dim() == 4:
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]
            w = rng.integers(-8, 9, size=tuple(v.shape)) / 4.0 * 2.0 ** round(float(np.log2(fan_in ** -0.5)))
        else:
            u = rng.integers(0, 64, size=tuple(v.shape)) / 64.0
            w = u + 0.5 if k.endswith(('running_var', '.weight')) else u - 0.5
        state[k] = torch.from_numpy(np.asarray(w, np.float32))
    return state


def seeded_inputs(tag):
    """The case's feature maps (``wiring``: its images) on a 1/64 grid in [-2, 2]."""
    rng = _rng(tag, 1)
    shapes = [WIRING['img']] if tag == 'wiring' else CASES[tag][1]
    return [torch.from_numpy((rng.integers(-128, 129, size=s) / 64.0).astype(np.float32)) for s in shapes]


def seeded_weighting(tag, shape):
    """R of the scalar ``sum(out * R)`` whose gradients are stored: on a 1/4 grid in [-2, 2]."""
    return torch.from_numpy((_rng(tag, 2).integers(-8, 9, size=tuple(shape)) / 4.0).astype(np.float32))


def sampled_gradients(module):
    """Of every parameter's gradient (zeros where autograd left None: a conv whose output ``forward`` drops) every k-th
    element of the flattened tensor, k = ceil(numel / FULL), and its Euclidean norm."""
    grads, norms = [], []
    for _, p in module.named_parameters():
        g = (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().reshape(-1)
        norms.append(g.double().norm().item())
        grads.append(g[::-(-g.numel() // FULL)].numpy())
    return grads, np.array(norms, np.float64)


def run(module, tag, mode, device='cpu'):
    """Load the seeded state, run ``sum(module(inputs) * R)`` forward and backward in ``mode``; returns the output, the
    input leaves and the module."""
    module.load_state_dict(seeded_state(module, tag), strict=True)
    module = module.to(device)
    module.train(mode == 'train')
    module.zero_grad(set_to_none=True)
    leaves = [x.to(device).requires_grad_(True) for x in seeded_inputs(tag)]
    out = module(leaves)
    (out * seeded_weighting(tag, out.shape).to(device)).sum().backward()
    return out, leaves, module


# ------------------------------------------------------------------------------------------------ the tests' side
_G = None


def golden():
    global _G
    if _G is None:
        with np.load(PATH) as g:
            _G = {k: g[k] for k in g.files}
    return _G


def build(tag):
    from ocrfdet_amd import image_encoder as ie
    return ie.CustomFPN(**CASES[tag][0])


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, bound = float(np.abs(got - want).max()), TOL * float(np.abs(want).max())
    assert err <= bound, f'{what}: max|err| {err:.3e} > {bound:.3e}'


def check_case(tag, mode, device, fused=None):
    """Output, input gradients, parameter gradients (sampled as the generator sampled them, and their norms) and, in
    train mode, the updated running statistics of case ``tag`` on ``device``."""
    g = golden()
    m = build(tag)
    if fused is not None:
        m.fused_merge = fused
    out, leaves, m = run(m, tag, mode, device)
    close(out.detach().cpu().numpy(), g[f'{tag}.{mode}.out'], f'{tag} {mode} out')
    for i, x in enumerate(leaves):
        key = f'{tag}.{mode}.gx{i}'
        assert (x.grad is not None) == (key in g), key
        if x.grad is not None:
            close(x.grad.cpu().numpy(), g[key], f'{tag} {mode} gx{i}')
    grads, norms = sampled_gradients(m)
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


def reference_dicts():
    """``img_backbone`` and ``img_neck`` of configs/ocrfdet/ocrfdet.py:48-65 as the generator read them."""
    cfg = json.loads(str(golden()['ref_config']))
    cfg['img_backbone']['out_indices'] = tuple(cfg['img_backbone']['out_indices'])
    return cfg['img_backbone'], cfg['img_neck']
