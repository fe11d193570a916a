"""HOA-1 on the fused training kernels (csrc/hoa1_train.hip through ``hoa.hoa1(..., fused_training=True)``) against the
float64 oracle of ``tests/hoa1_train_oracle.py``: forward, the 16 gradients with and without a dropout mask, dropped
pairs, determinism, launch and sync counts, the neck's switch and the fallbacks.

Bound per gradient tensor: ``max|g - g64| <= max(1e-4 * max|g64|, 4 * e32)``, e32 = the error of torch's own float32
autograd through the torch sequence on the GPU on the same inputs against the same oracle (a factor 4 for a different
summation order).  Every gradient test first asserts that the oracle's ambiguous set is empty for its inputs.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib, hoa
from tests import hoa1_train_oracle as O

pytestmark = pytest.mark.gpu
SHAPES = list(O.CASES)
DEV = 'cuda:0'


@functools.lru_cache(maxsize=None)
def module():
    return O.make_module().to(DEV)


@functools.lru_cache(maxsize=None)
def inputs(shape):
    return tuple(t.to(DEV) for t in O.make_inputs(shape))


@functools.lru_cache(maxsize=None)
def arms(shape, masked):
    """(fused out, fused grads, torch out, torch grads) in float32 on the GPU; computed once, read-only."""
    op, al, go, mask = inputs(shape)
    mask = mask if masked else None
    fo, fg = O.run(module(), op, al, go, mask, fused_training=True)
    to, tg = O.run(module(), op, al, go, mask)
    return fo, fg, to, tg


def err(a, b64):
    return float((a.double().cpu() - b64).abs().max())


def test_the_fused_path_is_taken(cuda):
    op, al, _, mask = inputs((2, 36, 36))
    o = op.clone().requires_grad_(True)
    out = hoa.hoa1(module(), o.reshape(-1, 1), al, 13, 36, 36, fused_training=True, dropout_mask=mask)
    assert type(out.grad_fn).__name__ == '_Hoa1TrainBackward'
    out = hoa.hoa1(module(), o.reshape(-1, 1), al, 13, 36, 36, dropout_mask=mask)
    assert type(out.grad_fn).__name__ != '_Hoa1TrainBackward'


@pytest.mark.parametrize('shape', SHAPES)
def test_forward(cuda, shape):
    """No mask, eval(): the eval kernels' output bit for bit.  With a mask: the oracle within the HOA-1 tolerance."""
    op, al, _, mask = inputs(shape)
    B, Y, X = shape
    with torch.no_grad():
        want = hoa.hoa1(module(), op.reshape(-1, 1), al, 13, Y, X)                  # the two eval kernels
        got = hoa.hoa1(module(), op.reshape(-1, 1), al, 13, Y, X, fused_training=True)
    assert torch.equal(got, want)
    assert torch.equal(arms(shape, False)[0], want)                                  # and under autograd
    np.testing.assert_allclose(arms(shape, True)[0].cpu().numpy(), O.oracle(shape, True)['out'].numpy(),
                               rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(want.cpu().numpy(), O.oracle(shape, False)['out'].numpy(), rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('shape', SHAPES)
def test_gradients(cuda, shape, masked):
    """grad_opacity, grad_alpha and the 14 parameter gradients against the float64 oracle, the upstream gradient random;
    the measured errors of both arms are printed per tensor (``-s``; recorded in profiles/hoa1_train_time.txt)."""
    ref = O.oracle(shape, masked)
    assert ref['ambiguous'] == 0
    _, fg, _, tg = arms(shape, masked)
    bad = []
    for name, g, t, g64 in zip(O.GRAD_NAMES, fg, tg, ref['grads']):
        assert g.shape == g64.shape and g.dtype == torch.float32
        e, e32, top = err(g, g64), err(t, g64), float(g64.abs().max())
        bound = max(1e-4 * top, 4 * e32)
        print(f'hoa1-grad {shape} {"mask" if masked else "nomask"} {name:22s} max|g64| {top:.3e}  fused {e:.3e}  '
              f'torch-f32 {e32:.3e}  bound {bound:.3e}')
        if not e <= bound:
            bad.append((name, e, bound))
    assert not bad, bad


def test_inputs_cover_samples_inside_and_outside_the_map(cuda):
    assert any(O.oracle(s, False)['inside'] > 0 and O.oracle(s, False)['outside'] > 0 for s in SHAPES)
    assert all(O.oracle(s, False)['touched'] > 0 for s in SHAPES)


def test_offset_tap_that_is_always_outside_has_zero_gradient(cuda):
    """(36,36): one offset window, rows -1 .. 4 of the 6 x 6 query map: the taps of window row 0 (and column 0) never
    see the map, so their weights' gradient is exactly 0 in every arm."""
    shape = (2, 36, 36)
    i = O.GRAD_NAMES.index('to_offsets.0.weight')
    for masked in (False, True):
        _, fg, _, tg = arms(shape, masked)
        for g in (fg[i], tg[i], O.oracle(shape, masked)['grads'][i]):
            assert float(g[:, 0, 0, :].abs().max()) == 0.0 and float(g[:, 0, :, 0].abs().max()) == 0.0
        assert float(fg[i].abs().max()) > 0.0


def test_dropped_pairs_contribute_nothing(cuda):
    """Everything dropped: the attention passes nothing on (out = upsample(to_out.bias) + opacity) and every gradient but
    grad_opacity = grad_out and to_out.bias is exactly 0.  All kept with scale 1: the no-mask result bit for bit."""
    shape = (2, 60, 84)
    op, al, go, mask = inputs(shape)
    m = copy.deepcopy(module())
    out, grads = O.run(m, op, al, go, torch.zeros_like(mask), fused_training=True)
    for name, g in zip(O.GRAD_NAMES, grads):
        if name == 'opacity':
            assert torch.equal(g, go)
        elif name != 'to_out.bias':
            assert float(g.abs().max()) == 0.0, name
    m64 = copy.deepcopy(O.make_module()).double()
    _, g64 = O.run(m64, op.double().cpu(), al.double().cpu(), go.double().cpu(), torch.zeros_like(mask).cpu())
    i = O.GRAD_NAMES.index('to_out.bias')
    assert err(grads[i], g64[i]) <= 1e-4 * float(g64[i].abs().max())
    m.dropout.p = 0.0                                               # scale 1 / (1 - p) = 1
    out1, grads1 = O.run(m, op, al, go, torch.ones_like(mask), fused_training=True)
    out0, grads0 = arms(shape, False)[:2]
    assert torch.equal(out1, out0)
    for name, a, b in zip(O.GRAD_NAMES, grads1, grads0):
        assert torch.equal(a, b), name


def test_reruns_and_single_samples_are_bit_identical(cuda):
    shape = (2, 128, 128)
    op, al, go, mask = inputs(shape)
    out0, grads0 = arms(shape, True)[:2]
    out1, grads1 = O.run(module(), op, al, go, mask, fused_training=True)
    assert torch.equal(out0, out1)
    for name, a, b in zip(O.GRAD_NAMES, grads0, grads1):
        assert torch.equal(a, b), name
    for b in range(shape[0]):
        out_b, grads_b = O.run(module(), op[b:b + 1], al[b:b + 1], go[b:b + 1], mask[b:b + 1], fused_training=True)
        assert torch.equal(out_b, out0[b:b + 1])
        assert torch.equal(grads_b[0], grads0[0][b:b + 1]) and torch.equal(grads_b[1], grads0[1][b:b + 1])


def test_launch_count_and_no_synchronisation(cuda):
    """(2,128,128), train() with dropout: from the hoa1 call to the end of autograd.grad w.r.t. all 16 inputs at most 12
    kernels (torch's mask draw and the weight pack included) and no synchronisation."""
    from torch.profiler import ProfilerActivity, profile
    shape = (2, 128, 128)
    op, al, go, _ = inputs(shape)
    m = copy.deepcopy(module()).train()
    assert m.dropout.p > 0

    def step(fused):
        o, a = op.clone().requires_grad_(True), al.clone().requires_grad_(True)
        m._hoa1_key = None                                          # a weight update since the last pack
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            out = hoa.hoa1(m, o.reshape(-1, 1), a, 13, 128, 128, fused_training=fused)
            torch.autograd.grad(out, [o, a] + hoa._hoa1_params(m), go)
            torch.cuda.synchronize()
        return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    step(True), step(False)                                         # warm-up
    names_torch = step(False)
    torch.cuda.set_sync_debug_mode('error')
    try:
        o, a = op.clone().requires_grad_(True), al.clone().requires_grad_(True)
        out = hoa.hoa1(m, o.reshape(-1, 1), a, 13, 128, 128, fused_training=True)
        torch.autograd.grad(out, [o, a] + hoa._hoa1_params(m), go)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    names = step(True)
    print(f'hoa1-launches (2,128,128) fused {len(names)} torch sequence {len(names_torch)}')
    print('hoa1-launches fused:', sorted(names))
    assert len(names) <= 12, names
    assert sum('hoa1_' in n for n in names) == 8, names


def test_dropout_mask_is_drawn_from_torchs_generator(cuda):
    shape = (2, 60, 84)
    op, al, _, _ = inputs(shape)
    m = copy.deepcopy(module()).train()
    outs = []
    with torch.no_grad():
        for seed in (7, 7, 8):
            torch.manual_seed(seed)
            outs.append(hoa.hoa1(m, op.reshape(-1, 1), al, 13, 60, 84, fused_training=True))
        m.eval()
        plain = hoa.hoa1(m, op.reshape(-1, 1), al, 13, 60, 84, fused_training=True)
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], plain)


@pytest.fixture(scope='module')
def neck():
    from ocrfdet_amd import view_transformer_ocrf as vto
    from tests import helpers
    cfg, g, state = helpers.core_fixture()
    pre = torch.from_numpy(g['pre']).cuda()

    class DepthNetStub(torch.nn.Module):
        def forward(self, x, mlp_input, stereo_metas=None):
            return pre
    m = vto.OcRFViewTransformerFull(
        pc_range=list(cfg.pc_range), bev_h=48, bev_w=48, num_height=13, grid_config=cfg.grid,
        input_size=cfg.input_size, downsample=16, in_channels=256, out_channels=80, depth_net=DepthNetStub())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    m.cuda().eval()
    B = int(g['batch'])
    voxel, pix, mask, rig = helpers.core_geometry(cfg, B)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    raw = t(g['raw'].astype(np.float32))
    inp = [t(g['x'].astype(np.float32))] + [t(rig[k]) for k in ('rots', 'trans', 'intrins', 'post_rots', 'post_trans', 'bda')]
    inp += [torch.zeros(B, 6, 27).cuda(), raw.clone(), raw, raw.clone(), t(rig['c2w'])]
    return dict(cfg=cfg, pre=pre, m=m, inp=inp)


def test_neck_switch_on_against_off(neck):
    """``OcRFViewTransformerFull.fused_hoa1_training``: train() with dropout.p = 0, on against off — the outputs within the
    forward tolerance, the gradients of the attention's parameters and of A_MLP within 1e-4 of the off arm's largest
    entry."""
    assert type(neck['m']).fused_hoa1_training is False
    cfg, pre = neck['cfg'], neck['pre']
    got = {}
    for fused in (True, False):
        m = copy.deepcopy(neck['m']).train()
        m.defor_cross_attention.dropout.p = 0.0
        m.fused_hoa1_training = fused
        depth = pre[:, :cfg.D].softmax(1).requires_grad_(True)
        feat = pre[:, cfg.D + 2:].clone().requires_grad_(True)
        torch.manual_seed(0)
        bev, _, logit, lst = m.view_transform_core(neck['inp'], depth, feat, cam_idx_list=[1, 4])
        loss = bev.square().mean() + logit.square().mean() + lst[0].mean() + lst[6].mean() + lst[4].square().mean()
        loss.backward()
        grads = {n: p.grad for n, p in m.named_parameters()
                 if p.grad is not None and n.startswith(('defor_cross_attention.', 'A_MLP.'))}
        got[fused] = (bev.detach(), logit.detach(), grads)
    for i in (0, 1):
        np.testing.assert_allclose(got[True][i].cpu().numpy(), got[False][i].cpu().numpy(), rtol=1e-4, atol=2e-5)
    assert set(got[True][2]) == set(got[False][2]) and any(n.startswith('A_MLP.') for n in got[False][2])
    assert sum(n.startswith('defor_cross_attention.') for n in got[False][2]) == 14
    # the last CPB bias adds one constant to every score of a softmax row: its gradient is 0 analytically and a residue of
    # cancelling sums of the size of the last CPB weight's gradient in either arm, which is the scale it is held to (as
    # tests/test_neck_gpu.py holds a convolution in front of a training-mode BatchNorm to the BatchNorm weight's scale)
    last_w = float(got[False][2]['defor_cross_attention.rel_pos_bias.mlp.2.weight'].abs().max())
    for n, want in got[False][2].items():
        e, top = float((got[True][2][n] - want).abs().max()), float(want.abs().max())
        print(f'hoa1-neck {n:50s} max|off| {top:.3e}  on-off {e:.3e}')
        scale = last_w if n == 'defor_cross_attention.rel_pos_bias.mlp.2.bias' else top
        assert e <= 1e-4 * scale, f'{n}: |err| {e:.3e} vs 1e-4 x {scale:.3e}'


def test_fallbacks_take_the_torch_sequence(cuda):
    """Y = 30, half precision, heads = 2 and a CPU tensor with fused_training=True: the torch sequence and its result."""
    def both(m, op, al, Y, X):
        o = op.clone().requires_grad_(True)
        with_switch = hoa.hoa1(m, o.reshape(-1, 1), al, 13, Y, X, fused_training=True)
        assert type(with_switch.grad_fn).__name__ != '_Hoa1TrainBackward'
        without = hoa.hoa1(m, o.reshape(-1, 1), al, 13, Y, X)
        assert torch.equal(with_switch, without)
    gen = torch.Generator().manual_seed(5)
    small = [torch.rand(1, 13, 30, 36, generator=gen).to(DEV) for _ in range(2)]
    both(module(), small[0], small[1], 30, 36)                                       # hq = 5 < 6
    op, al, _, _ = inputs((2, 36, 36))
    both(copy.deepcopy(module()).half(), op.half(), al.half(), 36, 36)
    torch.manual_seed(3)
    heads2 = hoa.DeformableAttention2D(dim=13, dim_head=4, heads=2, dropout=0.0, downsample_factor=4, offset_scale=4,
                                       offset_groups=1, offset_kernel_size=6).to(DEV).eval()
    both(heads2, op, al, 36, 36)
    both(copy.deepcopy(module()).cpu(), op.cpu(), al.cpu(), 36, 36)


def test_the_library_refuses_what_it_does_not_take(cuda):
    L = _lib.lib()
    assert L.ocrf_hoa1_train_workspace_floats(1, 30, 36) == 0 and L.ocrf_hoa1_train_workspace_floats(1, 246, 246) == 0
    x = torch.zeros(13 * 36 * 36, device=DEV)
    w = torch.zeros(L.ocrf_hoa1_weights_len(), device=DEV)
    with pytest.raises(_lib.OcrfHipError):
        _lib.launch('ocrf_hoa1_forward_train', x.device, x, x, w, 1, 30, 36, 4.0, None, 1.0, x, x)
    with pytest.raises(_lib.OcrfHipError):
        _lib.launch('ocrf_hoa1_backward', x.device, x, x, x, w, 1, 36, 36, 4.0, None, 1.0, None, x, x, w)
