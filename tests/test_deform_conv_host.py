"""CPU: the deformable convolution's torch formulation (``deform_conv.deform_conv2d_torch``) against the float64 oracle
(tests/dcn_oracle.py), its conventions pinned by constructions that need no oracle, the kernels' coordinate function
through the host-only ``ocrf_deform_taps``, and the modules and opt-in wiring built on the operator.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ocrfdet_amd import center_head as ch
from ocrfdet_amd import deform_conv as dc
from ocrfdet_amd import depthnet
from tests import dcn_oracle as do

CASES, problem, oracle = do.CASES, do.problem, do.oracle


@pytest.mark.parametrize('name', list(CASES))
def test_generator_delivers_its_classes(name):
    C, Cout, H, W, kernel, stride, padding, dilation, groups, dg = CASES[name]
    _, offset, _, _, classes, _ = problem(name)
    do.check_classes(offset, classes, H, W, kernel, stride, padding, dilation, dg)


@pytest.mark.parametrize('name', list(CASES))
def test_torch_formulation_against_the_oracle_in_float64(name):
    x, offset, weight, grad_out, _, geo = problem(name)
    want = oracle(name)
    t = [torch.from_numpy(a).double().requires_grad_(True) for a in (x, offset, weight)]
    out = dc.deform_conv2d_torch(*t, *geo)
    assert out.dtype == torch.float64 and tuple(out.shape) == want[0].shape
    assert float(np.abs(out.detach().numpy() - want[0]).max()) <= 1e-12
    grads = torch.autograd.grad(out, t, torch.from_numpy(grad_out).double())
    for g, w, what in zip(grads, want[1:], ('grad_x', 'grad_offset', 'grad_weight')):
        assert torch.isfinite(g).all(), what
        assert float(np.abs(g.numpy() - w).max()) <= 1e-10, what
    # the CPU takes the torch formulation whatever ``fused`` says
    assert torch.equal(dc.deform_conv2d(*t, *geo, fused=True), out)


@pytest.mark.parametrize('name', list(CASES))
def test_zero_offsets_are_the_plain_convolution(name):
    x, offset, weight, _, _, (stride, padding, dilation, groups, dg) = problem(name)
    xt, wt = torch.from_numpy(x).double(), torch.from_numpy(weight).double()
    got = dc.deform_conv2d_torch(xt, torch.zeros(offset.shape, dtype=torch.float64), wt, stride, padding, dilation,
                                 groups, dg)
    want = F.conv2d(xt, wt, None, stride, padding, dilation, groups)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12
    assert float(np.abs(do.forward(x, np.zeros_like(offset), weight, stride, padding, dilation, groups, dg)
                        - want.numpy()).max()) <= 1e-12


def test_integer_offsets_are_the_convolution_of_the_shifted_input():
    """Every tap moved by (dy, dx): the plain convolution of x shifted by (-dy, -dx) with zeros moved in."""
    rng = np.random.default_rng(3)
    n, C, H, W, dy, dx = 2, 4, 6, 9, 2, -3
    x = torch.from_numpy(rng.standard_normal((n, C, H, W)))
    w = torch.from_numpy(rng.standard_normal((6, 2, 3, 3)))
    offset = torch.zeros(n, 18, H, W, dtype=torch.float64)
    offset[:, 0::2], offset[:, 1::2] = dy, dx
    m = 5                                                                  # zero margin: the shift plus the padding fit
    padded = F.pad(x, (m, m, m, m))
    # the padded-by-1 input as the taps see it: window[r, c] = x[r - 1 + dy, c - 1 + dx], 0 outside the map
    window = padded[:, :, m - 1 + dy:m - 1 + dy + H + 2, m - 1 + dx:m - 1 + dx + W + 2]
    got = dc.deform_conv2d_torch(x, offset, w, 1, 1, 1, 2, 1)
    assert float((got - F.conv2d(window, w, None, 1, 0, 1, 2)).abs().max()) <= 1e-12
    assert float(np.abs(do.forward(x.numpy(), offset.numpy(), w.numpy(), (1, 1), (1, 1), (1, 1), 2, 1)
                        - got.numpy()).max()) <= 1e-12


def test_channel_2k_moves_rows_and_2k_plus_1_moves_columns():
    """A 3 x 1 kernel on a 4 x 9 input whose value is 10 row + column: moving tap 1 by +1 through offset channel 2
    reads the next ROW, through channel 3 the next COLUMN."""
    H, W = 4, 9
    x = (10.0 * torch.arange(H).view(H, 1) + torch.arange(W).view(1, W)).double().view(1, 1, H, W)
    w = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64).view(1, 1, 3, 1)          # reads the centre tap only
    for channel, want in ((2, x[0, 0, 2, 3]), (3, x[0, 0, 1, 4])):
        offset = torch.zeros(1, 6, H, W, dtype=torch.float64)
        offset[0, channel] = 1.0
        got = dc.deform_conv2d_torch(x, offset, w, 1, (1, 0), 1, 1, 1)
        assert got.shape == (1, 1, H, W) and float(got[0, 0, 1, 3]) == float(want)
        assert float(do.forward(x.numpy(), offset.numpy(), w.numpy(), (1, 1), (1, 0), (1, 1), 1, 1)[0, 0, 1, 3]) == float(want)


def test_the_second_offset_block_moves_the_upper_half_of_the_channels():
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((1, 4, 5, 6)))
    w = torch.zeros(4, 4, 1, 1, dtype=torch.float64)
    w[range(4), range(4)] = 1.0                                            # out channel c = sample of channel c
    offset = torch.zeros(1, 4, 5, 6, dtype=torch.float64)
    offset[0, 3] = 1.0                                                     # group 1, tap 0, column offset
    got = dc.deform_conv2d_torch(x, offset, w, 1, 0, 1, 1, 2)
    assert torch.equal(got[:, :2], x[:, :2])
    assert torch.equal(got[:, 2:, :, :-1], x[:, 2:, :, 1:]) and float(got[:, 2:, :, -1].abs().max()) == 0.0
    assert np.array_equal(do.forward(x.numpy(), offset.numpy(), w.numpy(), (1, 1), (0, 0), (1, 1), 1, 2), got.numpy())


# --------------------------------------------------------------------------------------------- ocrf_deform_taps
def taps_reference(H, W, base_h, base_w, off_h, off_w):
    """The definition in float32 arithmetic: (weights[4], index[4] or None where the weight is 0)."""
    f = np.float32
    with np.errstate(invalid='ignore', over='ignore'):
        h, w = f(base_h) + f(off_h), f(base_w) + f(off_w)
    if not (h > -1 and w > -1 and h < H and w < W):
        return [0.0] * 4, [None] * 4
    hl, wl = np.floor(h), np.floor(w)
    lh, lw = f(h - hl), f(w - wl)
    wts, idx = [], []
    for a in (0, 1):
        for b in (0, 1):
            r, c = int(hl) + a, int(wl) + b
            ok = 0 <= r < H and 0 <= c < W
            wgt = f(lh if a else f(1) - lh) * f(lw if b else f(1) - lw)
            wts.append(float(wgt) if ok else 0.0)
            idx.append(r * W + c if ok else None)
    return wts, idx


@pytest.mark.parametrize('name', ['3x3 pad 1', 'stride 2', 'dilation 2', '3x1'])
def test_taps_over_the_generators_classes(name):
    """The kernels' own coordinate function for every class the generator places, the non-finite ones included: the
    weights and indices of the definition, and indices inside the map whatever the offset is."""
    C, Cout, H, W, kernel, stride, padding, dilation, groups, dg = CASES[name]
    _, offset, _, _, classes, _ = problem(name)
    K = kernel[0] * kernel[1]
    bh, bw = do.base_coordinates(H, W, kernel, stride, padding, dilation)
    off = offset.reshape(offset.shape[0], dg, K, 2, *offset.shape[2:])
    shape = off[:, :, :, 0].shape
    base_h, base_w = np.broadcast_to(bh, shape).reshape(-1), np.broadcast_to(bw, shape).reshape(-1)
    off_h, off_w = off[:, :, :, 0].reshape(-1), off[:, :, :, 1].reshape(-1)
    seen = 0
    for (cls, axis), where in classes.items():
        for u in where[:6]:
            args = (H, W, int(base_h[u]), int(base_w[u]), float(off_h[u]), float(off_w[u]))
            wts, idx, frac = dc.deform_taps(*args)
            want_w, want_i = taps_reference(*args)
            assert all(0 <= i < H * W for i in idx), (cls, args, idx)
            assert wts == want_w, (cls, args, wts, want_w)
            assert all(wi is None or wi == gi for wi, gi in zip(want_i, idx)), (cls, args, idx, want_i)
            assert 0.0 <= frac[0] < 1.0 and 0.0 <= frac[1] < 1.0
            if cls not in ('fractional', 'integer', 'just_inside_low', 'just_inside_high'):
                assert wts == [0.0] * 4 and frac == (0.0, 0.0), (cls, args)
            seen += 1
    assert seen >= 2 * len(do.CLASSES)                                    # every class on both axes


def test_taps_at_exact_coordinates_and_refusals():
    from ocrfdet_amd import _lib
    wts, idx, frac = dc.deform_taps(5, 7, 2, 3, 0.0, 0.0)                 # an integer coordinate: one corner, from the right
    assert wts == [1.0, 0.0, 0.0, 0.0] and idx[0] == 2 * 7 + 3 and frac == (0.0, 0.0)
    wts, idx, _ = dc.deform_taps(5, 7, 4, 6, 0.5, 0.5)                    # the last row and column: three corners outside
    assert wts == [0.25, 0.0, 0.0, 0.0] and idx == [34, 34, 34, 34]
    wts, idx, _ = dc.deform_taps(5, 7, -1, -1, 0.5, 0.5)                  # between -1 and 0: only the far corner
    assert wts == [0.0, 0.0, 0.0, 0.25] and idx == [0, 0, 0, 0]
    for bad in (float('nan'), float('inf'), -float('inf'), 1e30, -1e30, 3e38):
        for args in ((bad, 0.0), (0.0, bad), (bad, bad)):
            wts, idx, frac = dc.deform_taps(5, 7, 2, 3, *args)
            assert wts == [0.0] * 4 and all(0 <= i < 35 for i in idx) and frac == (0.0, 0.0)
    for args in ((0, 7, 0, 0), (5, 0, 0, 0), (5, 1 << 20, 0, 0), (5, 7, 1 << 22, 0)):
        with pytest.raises(_lib.OcrfHipError):
            dc.deform_taps(*args, 0.0, 0.0)


# --------------------------------------------------------------------------------------------- modules
def test_module_keys_shapes_and_zero_offsets():
    torch.manual_seed(0)
    m = dc.DeformConv2dPack(8, 12, 3, stride=2, padding=1, dilation=1, groups=4, deform_groups=2, im2col_step=128)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {
        'weight': (12, 2, 3, 3), 'conv_offset.weight': (36, 8, 3, 3), 'conv_offset.bias': (36,)}
    assert not m.conv_offset.weight.detach().any() and not m.conv_offset.bias.detach().any()
    assert m.conv_offset.stride == (2, 2) and m.conv_offset.padding == (1, 1)
    bound = (6.0 / (2 * 9)) ** 0.5                                          # kaiming_uniform_, relu, fan_in 18
    assert float(m.weight.detach().abs().max()) <= bound and float(m.weight.detach().std()) > 0.3 * bound
    x = torch.randn(2, 8, 9, 11)
    got = m(x)
    want = F.conv2d(x, m.weight, None, 2, 1, 1, 4)
    assert got.shape == want.shape and float((got - want).detach().abs().max()) <= 1e-5
    plain = dc.DeformConv2d(8, 12, 3, padding=1)
    assert list(plain.state_dict()) == ['weight']
    assert plain(x, torch.zeros(2, 18, 9, 11)).shape == (2, 12, 9, 11)
    built = dc.build_dcn(dict(type='DCN', in_channels=8, out_channels=8, kernel_size=3, padding=1, groups=4, im2col_step=128))
    assert isinstance(built, dc.DeformConv2dPack) and built.groups == 4


def test_module_refusals():
    with pytest.raises(NotImplementedError):
        dc.build_dcn(dict(type='DCNv2', in_channels=8, out_channels=8, kernel_size=3))
    with pytest.raises(NotImplementedError):
        dc.build_dcn(dict())
    with pytest.raises(NotImplementedError):
        dc.DeformConv2dPack(8, 8, 3, bias=True)
    m = dc.DeformConv2d(4, 4, 3)
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 4, 2, 2), torch.zeros(1, 18, 1, 1))


@pytest.fixture
def native_dcn():
    before = depthnet.NATIVE_DCN
    depthnet.NATIVE_DCN = True
    try:
        yield
    finally:
        depthnet.NATIVE_DCN = before


def test_depthnet_default_still_refuses_dcn():
    assert depthnet.NATIVE_DCN is False
    with pytest.raises(NotImplementedError):
        depthnet.DepthNet(8, 8, 4, 6)
    with pytest.raises(NotImplementedError):
        depthnet.DepthNet(8, 8, 4, 6, use_dcn=True)
    assert not depthnet.supports({}) and not depthnet.supports(dict(use_dcn=True)) and depthnet.supports(dict(use_dcn=False))


def test_depthnet_with_native_dcn(native_dcn):
    assert depthnet.supports({}) and depthnet.supports(dict(use_dcn=True)) and depthnet.supports(dict(use_dcn=False))
    torch.manual_seed(1)
    net = depthnet.DepthNet(8, 8, 4, 6)
    without = depthnet.DepthNet(8, 8, 4, 6, use_dcn=False)
    keys = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert keys['depth_conv.4.weight'] == (8, 2, 3, 3)
    assert keys['depth_conv.4.conv_offset.weight'] == (18, 8, 3, 3) and keys['depth_conv.4.conv_offset.bias'] == (18,)
    assert keys['depth_conv.5.weight'] == (6, 8, 1, 1) and keys['depth_conv.5.bias'] == (6,)
    assert set(keys) - set(without.state_dict()) == {'depth_conv.4.conv_offset.weight', 'depth_conv.4.conv_offset.bias',
                                                     'depth_conv.5.weight', 'depth_conv.5.bias'}
    assert set(without.state_dict()) - set(keys) == {'depth_conv.4.bias'}      # there, 4 is the final 1 x 1 convolution
    assert isinstance(net.depth_conv[4], dc.DeformConv2dPack) and net.depth_conv[4].groups == 4
    x, mlp = torch.randn(2, 8, 6, 10, requires_grad=True), torch.randn(2, 27)
    torch.nn.init.normal_(net.depth_conv[4].conv_offset.weight, std=0.1)                 # offsets that move
    out = net(x, mlp)
    assert out.shape == (2, 10, 6, 10)
    out.square().sum().backward()
    for p in (net.depth_conv[4].weight, net.depth_conv[4].conv_offset.weight, net.depth_conv[4].conv_offset.bias):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
    assert x.grad is not None and torch.isfinite(x.grad).all()
    # with_cp: the same values through a non-reentrant checkpoint (eval: no dropout, batch statistics fixed)
    net.eval()
    want = net(x, mlp)
    g_want = torch.autograd.grad(want.sum(), net.depth_conv[4].weight)[0]
    net.with_cp = True
    got = net(x, mlp)
    assert torch.equal(got, want)
    assert torch.equal(torch.autograd.grad(got.sum(), net.depth_conv[4].weight)[0], g_want)


def test_the_neck_builds_the_native_module_for_a_dcn_cfg(native_dcn):
    from ocrfdet_amd import view_transformer_ocrf as vto
    grid = dict(x=[-40.0, 40.0, 0.8], y=[-40.0, 40.0, 0.8], z=[-1.0, 5.4, 6.4], depth=[1.0, 45.0, 0.5])
    neck = vto.OcRFViewTransformerFull(pc_range=[-40.0, -40.0, -1.0, 40.0, 40.0, 5.4], grid_config=grid,
                                       input_size=(256, 704), downsample=16, in_channels=32, out_channels=16,
                                       depthnet_cfg=dict(aspp_mid_channels=8))
    assert isinstance(neck.depth_net, depthnet.DepthNet)
    assert isinstance(neck.depth_net.depth_conv[4], dc.DeformConv2dPack)


TASKS = [dict(num_class=1, class_names=['car']), dict(num_class=2, class_names=['truck', 'bus'])]
COMMON = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2))
DCN = dict(type='DCN', in_channels=16, out_channels=16, kernel_size=3, padding=1, groups=4)


def test_dcn_separate_head_shapes_and_keys():
    torch.manual_seed(2)
    head = ch.DCNSeparateHead(16, 2, dict(COMMON, heatmap=(2, 2)), DCN, head_conv=16, final_kernel=3)
    keys = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    for name in ('feature_adapt_cls', 'feature_adapt_reg'):
        assert keys[f'{name}.weight'] == (16, 4, 3, 3)
        assert keys[f'{name}.conv_offset.weight'] == (18, 16, 3, 3) and keys[f'{name}.conv_offset.bias'] == (18,)
    assert keys['cls_head.0.conv.weight'] == (16, 16, 3, 3) and 'cls_head.0.conv.bias' not in keys
    assert keys['cls_head.0.bn.weight'] == (16,)
    assert keys['cls_head.1.weight'] == (2, 16, 3, 3) and keys['cls_head.1.bias'] == (2,)
    assert keys['task_head.reg.0.conv.weight'] == (16, 16, 3, 3) and keys['task_head.reg.1.weight'] == (2, 16, 3, 3)
    assert not any(k.startswith('task_head.heatmap') for k in keys)
    head.init_weights()
    assert torch.all(head.cls_head[-1].bias == torch.tensor(-2.19))
    out = head(torch.randn(2, 16, 8, 12))
    assert {k: tuple(v.shape[1:]) for k, v in out.items()} == dict(
        reg=(2, 8, 12), height=(1, 8, 12), dim=(3, 8, 12), rot=(2, 8, 12), vel=(2, 8, 12), heatmap=(2, 8, 12))


def test_center_head_accepts_dcn_separate_head():
    head = ch.CenterHead(in_channels=8, tasks=TASKS, common_heads=COMMON, share_conv_channel=16,
                         separate_head=dict(type='DCNSeparateHead', dcn_config=DCN, head_conv=16, final_kernel=3))
    head.init_weights()
    assert all(isinstance(t, ch.DCNSeparateHead) for t in head.task_heads) and len(head.task_heads) == 2
    outs = head([torch.randn(2, 8, 8, 12, requires_grad=True)])
    assert len(outs) == 2 and outs[0][0]['heatmap'].shape == (2, 1, 8, 12) and outs[1][0]['heatmap'].shape == (2, 2, 8, 12)
    sum(v.sum() for t in outs for v in t[0].values()).backward()
    assert head.task_heads[1].feature_adapt_reg.weight.grad is not None
    for cfg in (dict(), dict(type='DCNv2', in_channels=16, out_channels=16, kernel_size=3)):
        with pytest.raises(NotImplementedError):
            ch.DCNSeparateHead(16, 2, dict(), cfg)
        with pytest.raises(NotImplementedError):
            ch.CenterHead(in_channels=8, tasks=TASKS, common_heads=COMMON, share_conv_channel=16,
                          separate_head=dict(type='DCNSeparateHead', dcn_config=cfg))
