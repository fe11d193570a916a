"""CPU: the native stereo ``DepthNet`` (ocrfdet_amd/depthnet.py) and its torch cost-volume formulation against the
reference's own values (``tests/golden/stereo.npz``, ``make_golden_stereo.py``), and the neck's ``cv_frustum`` /
``depth_net`` wiring."""
import numpy as np
import pytest
import torch

from ocrfdet_amd import depthnet, index_prep
from tests import stereo_fixture as sf


@pytest.fixture(scope='module')
def g():
    return sf.load()


def _shapes(module):
    return {k: list(v.shape) for k, v in module.state_dict().items()}


def test_state_dict_keys_small(g):
    m = g['meta']
    net = depthnet.DepthNet(m['IN'], m['MID'], m['CTX'], m['D'] + 2, use_dcn=False, stereo=True, bias=m['BIAS'],
                            aspp_mid_channels=m['ASPP_MID'])
    assert _shapes(net) == m['small_keys']
    assert list(net.state_dict()) == list(m['small_keys'])


def test_state_dict_keys_reference_config(g):
    net = depthnet.DepthNet(256, 256, 80, 120, use_dcn=False, stereo=True, bias=5.0, aspp_mid_channels=96)
    assert _shapes(net) == g['meta']['full_keys']


def test_strict_load(g):
    net = sf.build(g)
    for k, v in net.state_dict().items():
        assert torch.equal(v, sf.state_dict(g)[k]), k


def test_dcn_is_refused():
    with pytest.raises(NotImplementedError):
        depthnet.DepthNet(8, 8, 4, 6)
    assert not depthnet.supports({}) and depthnet.supports(dict(use_dcn=False))


def test_fixture_covers_the_cases(g):
    grid = torch.from_numpy(g['grid'])
    assert g['prev_q'].shape[1] % 4 == 2                      # two channels past the last whole group
    assert 0.3 < (g['prev_q'] == 0).mean() < 0.7               # ReLU-sparse: the bias quirk fires on valid samples
    behind = grid[..., 0] == -2
    assert behind.any() and not behind.all()
    assert behind.reshape(2, 3, -1)[1, 2].any()               # the z < 1e-3 camera
    valid = ~behind
    assert ((grid.abs() > 1).any(-1) & valid).any()           # samples that leave the image
    inside = ((grid.abs() <= 1).all(-1) & valid).reshape(g['cost_raw'].shape)
    # the bias channel (4 (C // 4 - 1) = 12) warped on the reference's grid: exactly 0 for some samples inside the map
    prev = torch.from_numpy(g['prev_q'][:, 12:13].astype(np.float32))
    BN, D, H, W = g['cost_raw'].shape
    warp = torch.nn.functional.grid_sample(prev, grid.reshape(BN, D * H, W, 2), align_corners=True)
    assert ((warp.reshape(BN, D, H, W) == 0) & inside).any()


def _ambiguous(g, metas):
    H, W = g['cost_raw'].shape[-2:]
    mine = depthnet.stereo_grid_torch(metas, H, W)
    return sf.ambiguity(g['grid'], H, W, other=mine)


def test_cost_volume_torch_matches_reference(g):
    metas = sf.metas(g)
    amb = _ambiguous(g, metas)
    assert amb.float().mean() < 1e-2, f'ambiguous fraction {amb.float().mean():.2e}'
    raw = depthnet.stereo_cost_volume_torch(metas, g['meta']['BIAS'], raw=True)
    want = torch.from_numpy(g['cost_raw'])
    ok = ~amb
    # 16 channels of k/16 values: a sum of 16 terms below ~16 in magnitude, fp32
    assert torch.allclose(raw[ok], want[ok], rtol=1e-5, atol=1e-4), (raw - want)[ok].abs().max()
    # the bias decisions agree exactly (they differ by 5 from anything else)
    assert torch.equal(((raw - want).abs() > 1.0)[ok], torch.zeros_like(want[ok], dtype=torch.bool))
    cols = ~amb.any(1, keepdim=True).expand_as(amb)
    soft = depthnet.stereo_cost_volume_torch(metas, g['meta']['BIAS'])
    assert torch.allclose(soft[cols], torch.from_numpy(g['cost_volume'])[cols], rtol=1e-4, atol=1e-6)
    print(f'ambiguous cells: {int(amb.sum())} of {amb.numel()}')


def test_cost_volume_ignores_partial_group(g):
    metas = sf.metas(g)
    base = depthnet.stereo_cost_volume_torch(metas, 5.0, raw=True)
    prev, curr = metas['cv_feat_list']
    prev2, curr2 = prev.clone(), curr.clone()
    prev2[:, 16:] += 3.0
    curr2[:, 16:] -= 1.0
    other = depthnet.stereo_cost_volume_torch(dict(metas, cv_feat_list=[prev2, curr2]), 5.0, raw=True)
    assert torch.equal(base, other)


def test_dispatch_on_cpu_is_torch(g):
    metas = sf.metas(g)
    assert torch.equal(depthnet.stereo_cost_volume(metas, 5.0, fused=True),
                       depthnet.stereo_cost_volume_torch(metas, 5.0))


def _close(got, want, what):
    err = (got - want).abs().max().item()
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-4), f'{what}: max |err| {err}'


def test_forward_eval(g):
    net = sf.build(g).eval()
    metas = sf.metas(g)
    x, mlp = torch.from_numpy(g['x']), torch.from_numpy(g['mlp_input'])
    with torch.no_grad():
        _close(net(x, mlp, metas), torch.from_numpy(g['out_eval']), 'stereo')
        _close(net(x, mlp, dict(metas, cv_feat_list=[None, metas['cv_feat_list'][1]])),
               torch.from_numpy(g['out_none']), 'zeros branch')


def test_forward_train(g):
    net = sf.build(g).train()
    metas = sf.metas(g)
    x, mlp = torch.from_numpy(g['x']), torch.from_numpy(g['mlp_input'])
    torch.manual_seed(7)
    out = net(x, mlp, metas)
    _close(out.detach(), torch.from_numpy(g['out_train']), 'train')
    out.square().mean().backward()
    assert net.depth_conv[0].conv1.weight.grad is not None
    assert net.cost_volumn_net[0].weight.grad is not None


def test_with_cp_same_values(g):
    net = sf.build(g).eval()
    metas = sf.metas(g)
    x, mlp = torch.from_numpy(g['x']), torch.from_numpy(g['mlp_input'])
    with torch.no_grad():
        a = net(x, mlp, metas)
    net.with_cp = True
    b = net(x.requires_grad_(), mlp, metas)
    assert torch.equal(a, b.detach())


# --------------------------------------------------------------------------------------------- the neck
GRID = dict(x=[-40.0, 40.0, 0.8], y=[-40.0, 40.0, 0.8], z=[-1.0, 5.4, 6.4], depth=[1.0, 45.0, 0.5])
REF_DEPTHNET_CFG = dict(use_dcn=False, aspp_mid_channels=96, stereo=True, bias=5.)


def _neck(**kw):
    from ocrfdet_amd import view_transformer_ocrf as vto
    return vto.OcRFViewTransformerFull(pc_range=[-40.0, -40.0, -1.0, 40.0, 40.0, 5.4], grid_config=GRID,
                                       input_size=(256, 704), downsample=16, in_channels=256, out_channels=80, **kw)


def test_neck_cv_frustum():
    neck = _neck(depthnet_cfg=REF_DEPTHNET_CFG)
    want = index_prep.create_frustum(GRID['depth'], (256, 704), 4)
    assert neck.cv_frustum.shape == (88, 64, 176, 3) and neck.cv_frustum.dtype == torch.float32
    assert torch.equal(neck.cv_frustum, want)
    assert 'cv_frustum' not in neck.state_dict()
    assert 'cv_frustum' in dict(neck.named_buffers())


def test_neck_builds_native_depth_net():
    neck = _neck(depthnet_cfg=REF_DEPTHNET_CFG)
    assert isinstance(neck.depth_net, depthnet.DepthNet)
    assert neck.depth_net.depth_channels == neck.D + 2
    assert neck.depth_net.cost_volumn_net[0].in_channels == neck.D
    assert neck.depth_net.reduce_conv[0].in_channels == 256 and neck.depth_net.context_conv.out_channels == 80


def test_neck_default_cfg_unchanged():
    assert _neck().depth_net is None                   # DCN on: the reference's DepthNet when importable, else none
    ident = torch.nn.Identity()
    assert _neck(depthnet_cfg=REF_DEPTHNET_CFG, depth_net=ident).depth_net is ident
