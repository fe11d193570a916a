"""Float64 oracle for HOA-1 under autograd (``hoa.hoa1`` with ``fused_training=True``).

The oracle is the module itself: a ``.double()`` copy on the CPU run through ``hoa.hoa1``'s torch sequence under float64
autograd, dropout replaced by a fixed keep-mask.  That sequence is pinned to the reference by ``tests/golden/hoa.npz``
(``tests/test_hoa_modules.py``).

It also reports its AMBIGUOUS SET: where a float32 evaluation may legitimately take the other branch —

* CPB ReLU pre-activations with ``|x| < 1e-5`` (the float32 error of that tiny MLP on O(1) inputs is ~1e-6);
* sampling coordinates within 1e-3 of an integer (the bilinear cell edges and the zero-padding border);
* ``p == 0`` exactly in CPB's ``sign(p) log(|p| + 1)``.

The gradient tests assert that the set is empty for their inputs (``CASES`` holds input seeds found by ``search_seed``),
so nothing is masked or left out of a comparison.
"""
import copy
import functools

import torch

from ocrfdet_amd import hoa

# (B, Y, X) -> seed of the inputs: the first seed whose ambiguous set is empty (search_seed; the weights are fixed)
CASES = {
    (2, 36, 36): 0,
    (2, 36, 60): 2,
    (2, 60, 84): 0,
    (2, 128, 128): 3,
    (1, 200, 200): 16,
}
KEEP = 0.9                      # keep probability of the fixed dropout mask; the module's dropout.p = 1 - KEEP
MASK_SEED = 4321


def make_module():
    """The DeformableAttention2D OcRFDet instantiates, seeded, with the offset branch and CPB scaled up so that the
    sampling positions move by O(1) token and the positional bias has O(1) slopes: both get real gradients."""
    torch.manual_seed(1234)
    m = hoa.DeformableAttention2D(dim=13, dim_head=8, heads=1, dropout=1.0 - KEEP, downsample_factor=4, offset_scale=4,
                                  offset_groups=None, offset_kernel_size=6)
    with torch.no_grad():
        m.to_offsets[0].weight.mul_(2.0)
        m.to_offsets[2].weight.mul_(3.0)
        for layer in m.rel_pos_bias.mlp:
            lin = layer[0] if isinstance(layer, torch.nn.Sequential) else layer
            lin.weight.mul_(2.0)
            lin.bias.add_(0.25)
    return m.eval()


def token_counts(Y, X):
    hq, wq = Y // 6, X // 6
    return hq, wq, (hq - 4) // 4 + 1, (wq - 4) // 4 + 1


def make_inputs(shape, seed=None):
    """opacity, alpha (B,13,Y,X) in [0,1), the upstream gradient and the keep-mask (B, queries, keys) uint8."""
    B, Y, X = shape
    gen = torch.Generator().manual_seed(CASES[shape] if seed is None else seed)
    opacity = torch.rand(B, 13, Y, X, generator=gen)
    alpha = torch.rand(B, 13, Y, X, generator=gen)
    grad_out = torch.randn(B, 13, Y, X, generator=gen)
    hq, wq, hk, wk = token_counts(Y, X)
    mgen = torch.Generator().manual_seed(MASK_SEED + Y * 1000 + X)
    mask = (torch.rand(B, hq * wq, hk * wk, generator=mgen) < KEEP).to(torch.uint8)
    return opacity, alpha, grad_out, mask


def ambiguous(m64, opacity, alpha):
    """(size of the ambiguous set, kv samples with all four taps inside the map, kv samples with a tap outside, kv
    samples with at least one tap inside: those pass a gradient to alpha and to the offset branch) of the float64 forward of ``m64`` on float64 inputs."""
    B, _, Y, X = opacity.shape
    hq, wq, _, _ = token_counts(Y, X)
    with torch.no_grad():
        o_up = torch.nn.functional.interpolate(opacity, size=(hq, wq), mode='bilinear', align_corners=True)
        a_up = torch.nn.functional.interpolate(alpha, size=(hq, wq), mode='bilinear', align_corners=True)
        _, vgrid = m64(o_up, a_up, return_vgrid=True)                       # (B,2,hk,wk)
        vs = hoa._normalize_grid(vgrid)                                      # (B,hk,wk,2)
        fx = ((vs[..., 0] + 1) * wq - 1) / 2
        fy = ((vs[..., 1] + 1) * hq - 1) / 2
        n = int(((fx - fx.round()).abs() < 1e-3).sum() + ((fy - fy.round()).abs() < 1e-3).sum())
        x0, y0 = fx.floor(), fy.floor()
        inside = (x0 >= 0) & (x0 + 1 <= wq - 1) & (y0 >= 0) & (y0 + 1 <= hq - 1)
        gq = hoa._normalize_grid(hoa._grid_like(a_up), dim=0).reshape(1, -1, 2)           # (1, queries, 2)
        pos = gq[:, :, None, :] - vs.reshape(B, 1, -1, 2)                                 # (B, queries, keys, 2)
        n += int((pos == 0).sum())
        x = torch.sign(pos) * torch.log(pos.abs() + 1)
        mlp = m64.rel_pos_bias.mlp
        z0 = torch.nn.functional.linear(x, mlp[0][0].weight, mlp[0][0].bias)
        z1 = torch.nn.functional.linear(torch.relu(z0), mlp[1][0].weight, mlp[1][0].bias)
        n += int((z0.abs() < 1e-5).sum() + (z1.abs() < 1e-5).sum())
        touched = (x0 + 1 >= 0) & (x0 <= wq - 1) & (y0 + 1 >= 0) & (y0 <= hq - 1)       # at least one tap inside
    return n, int(inside.sum()), int((~inside).sum()), int(touched.sum())


def search_seed(shape, tries=200):
    """First input seed whose ambiguous set is empty and that has a kv sample touching the map."""
    m64 = copy.deepcopy(make_module()).double()
    for seed in range(tries):
        opacity, alpha, _, _ = make_inputs(shape, seed)
        n, _, _, touched = ambiguous(m64, opacity.double(), alpha.double())
        if n == 0 and touched > 0:
            return seed
    raise RuntimeError(f'no seed with an empty ambiguous set for {shape}')


def run(m, opacity, alpha, grad_out, mask, **kw):
    """out and the 16 gradients (opacity, alpha, the 14 parameters in the packed order) of ``hoa.hoa1`` on ``m``."""
    B, _, Y, X = opacity.shape
    o = opacity.detach().clone().requires_grad_(True)
    a = alpha.detach().clone().requires_grad_(True)
    params = hoa._hoa1_params(m)
    out = hoa.hoa1(m, o.reshape(-1, 1), a, 13, Y, X, dropout_mask=mask, **kw)
    grads = torch.autograd.grad(out, [o, a] + params, grad_out)
    return out.detach(), [g.detach() for g in grads]


@functools.lru_cache(maxsize=None)
def oracle(shape, masked):
    """dict(out, grads, ambiguous, inside, outside, touched) of the float64 oracle on the case ``shape``; computed once and
    shared: treat it as read-only."""
    m64 = copy.deepcopy(make_module()).double()
    opacity, alpha, grad_out, mask = make_inputs(shape)
    n, inside, outside, touched = ambiguous(m64, opacity.double(), alpha.double())
    out, grads = run(m64, opacity.double(), alpha.double(), grad_out.double(), mask if masked else None)
    return dict(out=out, grads=grads, ambiguous=n, inside=inside, outside=outside, touched=touched)


GRAD_NAMES = ['opacity', 'alpha', 'to_q.weight', 'to_offsets.0.weight', 'to_offsets.0.bias', 'to_offsets.2.weight',
              'to_k.weight', 'to_v.weight', 'to_out.weight', 'to_out.bias', 'cpb.0.weight', 'cpb.0.bias', 'cpb.1.weight',
              'cpb.1.bias', 'cpb.2.weight', 'cpb.2.bias']
