"""GPU: ``ocrf_stereo_cost_volume`` (csrc/stereo.hip) against the reference's values (``tests/golden/stereo.npz``) and
against the torch formulation at the reference shape, its determinism, the stereo ``DepthNet`` without host
synchronisation, and ``OcRFViewTransformerFull.forward(input, stereo_metas)`` with the native depth net."""
import random

import numpy as np
import pytest
import torch

from ocrfdet_amd import depthnet, index_prep, synthetic
from tests import helpers
from tests import stereo_fixture as sf

pytestmark = pytest.mark.gpu

# Tolerances.  The raw cost is a sum of n = 4 floor(C / 4) terms |curr - warp|.  Two sources separate two formulations:
# * accumulation: the terms are non-negative and added in the same group order, so the rounding of the sums is at most
#   n * 2^-24 * |raw| (first order);
# * the sample position: the formulations' coordinates may differ by a few ulps (the torch formulation's 3x3 product is a
#   GEMM, the kernel's plain products; grid_sample's weights may be fused multiply-adds).  With delta feature pixels per
#   axis and post-ReLU features (corner differences bounded by the channel's maximum m_c), a warped value moves by at most
#   2 delta m_c, the cost by 2 delta sum_c m_c.  delta = 4 ulp of the largest coordinate (W).
# plus 1e-4 absolute for the bilinear products themselves.  The softmax of raw values that differ by at most d per cell
# differs by at most p * (exp(2 d) - 1).
def raw_tol(raw, n_terms, lipschitz=None):
    tol = n_terms * 2.0 ** -24 * raw.abs() + 1e-4
    return tol if lipschitz is None else tol + lipschitz.view(-1, 1, 1, 1)


def position_term(prev, W):
    G = prev.shape[1] // 4
    delta = 4 * W * 2.0 ** -24
    return 2 * delta * prev[:, :4 * G].flatten(2).amax(2).sum(1)


def check_softmax(got, want, raw, n_terms, keep, lipschitz=None):
    delta = raw_tol(raw, n_terms, lipschitz).amax(1, keepdim=True)           # per (camera, pixel) column
    bound = want * torch.expm1(2 * delta) + 1e-7
    bad = ((got - want).abs() > bound) & keep
    assert not bad.any(), f'{int(bad.sum())} softmax cells out of bound; max |err| {(got - want)[keep].abs().max():.3e}'


@pytest.fixture(scope='module')
def g():
    return sf.load()


def test_kernel_matches_reference_fixture(g, cuda):
    metas = sf.metas(g, cuda)
    H, W = g['cost_raw'].shape[-2:]
    amb = sf.ambiguity(g['grid'], H, W).to(cuda)
    bias = g['meta']['BIAS']
    raw = depthnet.stereo_cost_volume_hip(metas, bias, raw=True)
    want = torch.from_numpy(g['cost_raw']).to(cuda)
    ok = ~amb
    flips = ((raw - want).abs() > 1.0) & ok                     # a bias / validity decision that differs (bias = 5)
    assert not flips.any(), f'{int(flips.sum())} bias decisions differ outside the ambiguous cells'
    err = (raw - want).abs()
    assert (err <= raw_tol(want, 16))[ok].all(), f'raw max |err| {err[ok].max():.3e}'
    soft = depthnet.stereo_cost_volume_hip(metas, bias)
    cols = ~amb.any(1, keepdim=True).expand_as(amb)
    check_softmax(soft, torch.from_numpy(g['cost_volume']).to(cuda), want, 16, cols)
    print(f'fixture: {int(amb.sum())} ambiguous cells reported, not compared; raw max |err| {err[ok].max():.2e}')


def full_metas(dev, seed=0, B=2, N=6, C=256):
    """The reference shape: 256 x 704 input, stereo features at downsample 4 (64 x 176), depth [1, 60, 0.5] (D = 118),
    ReLU-sparse features, adjacent-frame poses from the synthetic rig."""
    r = synthetic.rig(N, (256, 704), batch=B)
    gen = torch.Generator(device='cpu').manual_seed(seed)
    feat = lambda: torch.relu(torch.randn(B * N, C, 64, 176, generator=gen)).to(dev)       # noqa: E731
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)           # noqa: E731
    return dict(k2s_sensor=t(synthetic.stereo_k2s(N, batch=B)), intrins=t(r['intrins']), post_rots=t(r['post_rots']),
                post_trans=t(r['post_trans']), frustum=index_prep.create_frustum([1.0, 60.0, 0.5], (256, 704), 4).to(dev),
                cv_downsample=4, downsample=16, grid_config=None, cv_feat_list=[feat(), feat()])


@pytest.fixture(scope='module')
def full(cuda):
    return full_metas(cuda)


def test_kernel_matches_torch_full_size(full):
    H, W = 64, 176
    with torch.no_grad():
        grid = depthnet.stereo_grid_torch(full, H, W)
        want_raw = depthnet.stereo_cost_volume_torch(full, 5.0, raw=True)
        raw = depthnet.stereo_cost_volume_hip(full, 5.0, raw=True)
    # both formulations take the same closed-form algebra in the same order (the torch one's 3x3 product by a GEMM):
    # their coordinates differ by a few ulps (~1e-5 feature pixels at W = 176), so a 1e-4 px band around the corner
    # lines holds every cell whose == 0 test can flip; in-map samples are spread evenly across it (~2e-4 of the cells)
    amb = sf.ambiguity(grid.reshape(12, -1, W, 2), H, W, tol=1e-4)
    frac = amb.float().mean().item()
    assert frac < 1e-3, f'ambiguous fraction {frac:.2e}'
    ok = ~amb
    flips = ((raw - want_raw).abs() > 1.0) & ok
    assert not flips.any(), f'{int(flips.sum())} bias / validity decisions differ outside ambiguous cells'
    err = (raw - want_raw).abs()
    lip = position_term(full['cv_feat_list'][0], W)
    assert (err <= raw_tol(want_raw, 256, lip))[ok].all(), f'raw max |err| {err[ok].max():.3e}'
    soft = depthnet.stereo_cost_volume_hip(full, 5.0)
    want = want_raw.softmax(1)
    cols = ~amb.any(1, keepdim=True).expand_as(amb)
    check_softmax(soft, want, want_raw, 256, cols, lip)
    assert torch.allclose(soft.sum(1), torch.ones_like(soft[:, 0]), atol=1e-5)
    print(f'full size: ambiguous fraction {frac:.2e}, raw max |err| {err[ok].max():.2e} (position term up to '
          f'{lip.max():.2e}), '
          f'softmax max |err| {(soft - want)[cols].abs().max():.2e}')


def test_kernel_deterministic(full):
    a = depthnet.stereo_cost_volume_hip(full, 5.0)
    b = depthnet.stereo_cost_volume_hip(full, 5.0)
    assert torch.equal(a, b)


def test_depthnet_forward_no_sync(full, cuda):
    net = depthnet.DepthNet(256, 256, 80, 120, use_dcn=False, stereo=True, bias=5.0, aspp_mid_channels=96).to(cuda).eval()
    x = torch.randn(12, 256, 16, 44, device=cuda)
    mlp = torch.randn(2, 6, 27, device=cuda)
    with torch.no_grad():
        net(x, mlp, full)                                          # warm-up: MIOpen's first calls may synchronise
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            out = net(x, mlp, full)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    assert out.shape == (12, 120 + 80, 16, 44) and torch.isfinite(out).all()


def _neck_and_inputs(dev):
    from ocrfdet_amd import view_transformer_ocrf as vto
    cfg, g, state = helpers.core_fixture()
    torch.manual_seed(0)
    m = vto.OcRFViewTransformerFull(pc_range=list(cfg.pc_range), bev_h=48, bev_w=48, num_height=13, grid_config=cfg.grid,
                                    input_size=cfg.input_size, downsample=16, in_channels=256, out_channels=80,
                                    depthnet_cfg=dict(use_dcn=False, aspp_mid_channels=96, stereo=True, bias=5.))
    assert isinstance(m.depth_net, depthnet.DepthNet)
    m.to(dev)
    B = int(g['batch'])
    _, _, _, rig = helpers.core_geometry(cfg, B)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)       # noqa: E731
    raw = t(g['raw'])
    x = t(g['x'])
    inp = [x] + [t(rig[k]) for k in ('rots', 'trans', 'intrins', 'post_rots', 'post_trans', 'bda')]
    inp += [torch.randn(B, cfg.n_cams, 27, device=dev), raw.clone(), raw, raw.clone(), t(rig['c2w'])]
    BN = B * cfg.n_cams
    Hs, Ws = cfg.input_size[0] // 4, cfg.input_size[1] // 4
    gen = torch.Generator(device='cpu').manual_seed(1)
    feat = lambda: torch.relu(torch.randn(BN, 64, Hs, Ws, generator=gen)).to(dev)    # noqa: E731
    metas = dict(k2s_sensor=t(synthetic.stereo_k2s(cfg.n_cams, batch=B)), intrins=inp[3], post_rots=inp[4],
                 post_trans=inp[5], frustum=m.cv_frustum.to(x), cv_downsample=4, downsample=m.downsample,
                 grid_config=m.grid_config, cv_feat_list=[feat(), feat()])
    return m, inp, metas


def test_neck_forward_eval_and_train(cuda):
    from torch.profiler import ProfilerActivity, profile
    m, inp, metas = _neck_and_inputs(cuda)
    assert metas['frustum'].data_ptr() == m.cv_frustum.data_ptr()          # on the device already: no copy
    m.eval()
    random.seed(0)
    with torch.no_grad(), profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = m(inp, metas)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    assert any('stereo_cost_volume_kernel' in n for n in names), 'the fused cost volume did not run'
    bev, depth = out[0], out[1]
    assert torch.isfinite(bev).all() and torch.isfinite(depth).all()
    # fused vs torch cost volume through the whole neck
    m.depth_net.fused_cost_volume = False
    random.seed(0)
    with torch.no_grad():
        ref = m(inp, metas)
    m.depth_net.fused_cost_volume = True
    assert torch.allclose(depth, ref[1], rtol=1e-3, atol=1e-4), (depth - ref[1]).abs().max()
    assert torch.allclose(bev, ref[0], rtol=1e-3, atol=1e-3), (bev - ref[0]).abs().max()
    # training: convolution gradients flow, the cost volume stays gradient-free
    m.train()
    out = m(inp, metas)
    (out[0].float().mean() + out[1].float().mean()).backward()
    dn = m.depth_net
    assert dn.reduce_conv[0].weight.grad is not None and dn.cost_volumn_net[0].weight.grad is not None
    assert torch.isfinite(dn.cost_volumn_net[0].weight.grad).all()
    assert not metas['cv_feat_list'][0].requires_grad
