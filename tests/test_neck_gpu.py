"""GPU parity of csrc/neck.hip and of the assembled ``OcRFViewTransformerFull`` against the oracle and
the vectors dumped from the reference's own forward (tests/golden/core_small.npz).  Tolerances: 1e-4
on network outputs (BASELINE.json north_star), exact on masks / integer decisions."""
import numpy as np
import pytest
import torch

from oracle import core as oc
from oracle.hoa import conv2d, conv_transpose2d_k2s2
from tests import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def core():
    from ocrfdet_amd import view_transformer_ocrf as vto
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
    return dict(cfg=cfg, g=g, p=state, m=m, B=B, voxel=voxel, pix=pix, mask=mask, inp=inp, t=t)


def close(got, want, tol, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    err = float(np.abs(got.astype(np.float64) - np.asarray(want, np.float64)).max())
    assert err <= tol, f'{what}: max|err| {err:.3e} > {tol}'


def test_prefilter(core):
    from ocrfdet_amd import neck_ops
    cfg, g = core['cfg'], core['g']
    thr = 1.0 / cfg.D
    depth, fdepth, sem, feat = neck_ops.prefilter(core['t'](g['pre']), cfg.D, cfg.channels, thr, 0.25)
    want_d, want_fd, want_s, want_f = oc.prefilter(g['pre'], cfg.D, cfg.channels, thr, 0.25)
    close(depth, g['depth'], 1e-6, 'depth vs reference'), close(sem, g['semantic'], 1e-6, 'semantic vs reference')
    d = depth.cpu().numpy()
    fd = fdepth.cpu().numpy()
    assert ((fd == 0) | (fd == d)).all()
    flips = ((fd == 0) != (want_fd == 0)) & (np.abs(want_d - np.float32(thr)) > 1e-6)   # only ties at the threshold may differ
    assert not flips.any()
    s1 = sem.cpu().numpy()[:, 1]
    keep = (s1 >= np.float32(0.25))[:, None]
    tf = g['pre'][:, cfg.D + 2:]
    assert np.array_equal(feat.cpu().numpy(), np.ascontiguousarray((keep * tf).transpose(0, 2, 3, 1)))
    sure = np.abs(want_s[:, 1] - 0.25) > 1e-6
    assert np.array_equal((feat.cpu().numpy() != 0).any(-1)[sure], (want_f != 0).any(1)[sure])


def test_prefilter_ragged_width(core):
    """HW not a multiple of the 64-pixel tile, C not a multiple of 4."""
    from ocrfdet_amd import neck_ops
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 7 + 2 + 9, 5, 15)).astype(np.float32)
    depth, fdepth, sem, feat = neck_ops.prefilter(torch.from_numpy(x).cuda(), 7, 9, 0.1, 0.4)
    wd, wfd, ws, wf = oc.prefilter(x, 7, 9, 0.1, 0.4)
    close(depth, wd, 1e-6, 'depth'), close(sem, ws, 1e-6, 'semantic')
    ok = (np.abs(wd - 0.1) > 1e-6)
    assert np.array_equal(fdepth.cpu().numpy()[ok] == 0, wfd[ok] == 0)
    close(fdepth.cpu().numpy()[ok], wfd[ok], 1e-6, 'filter_depth')
    sure = np.abs(ws[:, 1] - 0.4) > 1e-6
    assert np.array_equal(feat.cpu().numpy()[sure], np.ascontiguousarray(wf.transpose(0, 2, 3, 1))[sure])


def test_pillar_sample_mean(core):
    from ocrfdet_amd import neck_ops
    g, t = core['g'], core['t']
    raw = g['raw'].astype(np.float32)
    got = neck_ops.pillar_sample_mean(t(raw), t(core['pix']), t(core['mask']))
    want = oc.color_voxels_avg(oc.lidar_points_to_image_values(core['pix'], raw, core['mask']), core['mask'])
    close(got, want, 2e-4, 'avg colour vs oracle (0..255 scale)')
    close(got / 255.0, g['colored_avg'] / 255.0, 2e-4, 'avg colour vs reference (0..1 scale)')
    # empty mask -> zeros; single channel with the swapped view
    none = np.zeros_like(core['mask'])
    assert float(neck_ops.pillar_sample_mean(t(raw), t(core['pix']), t(none)).abs().max()) == 0.0
    H, W = core['cfg'].input_size
    a = np.random.default_rng(1).random((core['B'], 6, 1, H, W), dtype=np.float32)
    got = neck_ops.pillar_sample_mean(t(a), t(core['pix']), t(core['mask']), view_hw=(W, H))
    want = oc.color_voxels_avg(oc.lidar_points_to_image_values(core['pix'], a.reshape(core['B'], 6, 1, W, H), core['mask']),
                               core['mask'])
    close(got, want, 1e-5, 'swapped-view alpha sampling')


def test_retain_valid_pixels(core):
    from ocrfdet_amd import neck_ops
    g, t = core['g'], core['t']
    raw = g['raw'].astype(np.float32)
    want = oc.retain_valid_pixels(raw, core['pix'], core['mask'])
    got = neck_ops.retain_valid_pixels(t(raw), t(core['pix']), t(core['mask']))
    assert np.array_equal(got.cpu().numpy(), want)
    cams = g['cam_idx_list'].astype(np.int32)
    sel = neck_ops.retain_valid_pixels(t(raw), t(core['pix']), t(core['mask']), torch.from_numpy(cams).cuda())
    for b, c in enumerate(cams):
        assert np.array_equal(sel[b].cpu().numpy(), want[b, c])
        assert np.array_equal(sel[b].cpu().numpy().astype(np.uint8), g['sparse_sel'][b])


def test_gauss_heads(core):
    from ocrfdet_amd import neck_ops
    cfg, g, p, m, t = core['cfg'], core['g'], core['p'], core['m'], core['t']
    op, sc, rot, col = neck_ops.gauss_heads(t(g['ht_feat']), t(g['colored_avg']), m._head_params(), cfg.num_height)
    lift = oc.voxel_lift(g['ht_feat'], p)
    for b in range(core['B']):
        want = oc.gauss_heads(lift[b].reshape(-1, cfg.channels), g['colored_avg'][b].reshape(-1, 3) / np.float32(255.0), p)
        for got, ref, name in zip((op, sc, rot, col), want, ('opacity', 'scales', 'rotations', 'colour')):
            close(got[b], ref, 5e-6, name + ' vs oracle')       # hardware exp / log / rcp in the activations
        close(op[b, ::5], g[f'gauss_opacity{b}'], 1e-5, 'opacity vs reference')
        close(sc[b, ::5], g[f'gauss_scales{b}'], 1e-5, 'scales vs reference')
        close(rot[b, ::5], g[f'gauss_rot{b}'], 1e-5, 'rotations vs reference')
        close(col[b, ::5], g[f'gauss_rgb{b}'], 1e-5, 'colour vs reference')


def test_nerf_branch(core):
    from ocrfdet_amd import neck_ops
    cfg, g, p, m, t = core['cfg'], core['g'], core['p'], core['m'], core['t']
    B = core['B']
    H, W = cfg.input_size
    x = g['x'].astype(np.float32)
    w_s, c_s, block = m._nerf_params()
    with torch.no_grad():
        z = m.image_feat_resize.stem(t(x).reshape(B * 6, 256, *cfg.feat_hw))
    zr = np.stack([conv2d(conv_transpose2d_k2s2(conv2d(x[b], p['image_feat_resize.conv1.weight'], p['image_feat_resize.conv1.bias'], padding=1),
                                                p['image_feat_resize.upsample1.weight'], p['image_feat_resize.upsample1.bias']),
                          p['image_feat_resize.conv2.weight'], p['image_feat_resize.conv2.bias'], padding=1) for b in range(B)])
    close(z, zr.reshape(B * 6, 32, *z.shape[2:]), 1e-4, 'ResizeNetwork stem (MIOpen) vs oracle')
    alpha = neck_ops.nerf_alpha(z, w_s, c_s)
    cams = torch.from_numpy(g['cam_idx_list'].astype(np.int32)).cuda()
    sparse = t(g['sparse_sel'].astype(np.float32))
    img_n, dep_n = neck_ops.nerf_render(z, cams, alpha, sparse, block, 6)
    close(img_n, g['render_N'], 1e-5, 'render_N vs reference'), close(dep_n, g['render_depth_N'], 1e-5, 'render_depth_N vs reference')
    for b in range(B):
        feat = oc.resize_network(x[b], p)
        close(alpha.view(B, 6, H, W)[b], oc.nerf_alpha(feat, p), 1e-5, 'alpha vs oracle')
    a_l = neck_ops.pillar_sample_mean(alpha.view(B, 6, 1, H, W), t(core['pix']), t(core['mask']), view_hw=(W, H))
    close(a_l, g['alpha_lidar'], 1e-4, 'alpha_lidar vs reference')


def _check_outputs(core, out, tol=1e-4):
    g = core['g']
    bev, depth, (bev_mask, sem), lst = out
    close(depth, g['depth'], 1e-6, 'depth'), close(sem, g['semantic'], 1e-6, 'semantic')
    close(bev_mask, g['bev_mask_logit'], tol, 'bev_mask_logit')
    close(lst[4], g['opacity_alpha_view'], tol, 'opacity_alpha_view')
    close(bev, g['bev_feat'], tol, 'bev_feat')
    assert list(lst[5]) == [int(c) for c in g['cam_idx_list']]
    close(lst[1], g['gt_images'], 1e-6, 'gt_images')
    close(lst[3], g['render_N'], 1e-5, 'render_N'), close(lst[8], g['render_depth_N'], 1e-5, 'render_depth_N')
    # the reference-side render was the C oracle (the CUDA rasteriser cannot run in the build container)
    for name, got, want in (('render_G', lst[2], g['render_G']), ('render_depth_G', lst[7], g['render_depth_G']),
                            ('render_imgs', lst[0], g['render_imgs']), ('render_depth', lst[6], g['render_depth'])):
        d = np.abs(got.detach().cpu().numpy() - want)
        assert (d > tol).mean() < 1e-3 and d.max() < 5e-2, f'{name}: {d.max():.3e}, {(d > tol).mean():.2e} of pixels off'


def test_module_forward_vs_reference(core):
    m, g = core['m'], core['g']
    cams = [int(c) for c in g['cam_idx_list']]
    with torch.no_grad():
        x = core['inp'][0]
        B, N, C, H, W = x.shape
        y = m.depth_net(x.view(B * N, C, H, W), core['inp'][7], None)
        from ocrfdet_amd import neck_ops
        depth, fdepth, sem, feat_cl = neck_ops.prefilter(y, m.D, m.out_channels, m.depth_threshold, m.semantic_threshold)
        bev, _, bev_mask, lst = m.view_transform_core(core['inp'], fdepth, None, feat_cl, cam_idx_list=cams)
    _check_outputs(core, (bev, depth, (bev_mask, sem), lst))


def test_module_forward_entry_point_and_accelerate(core):
    """``forward`` end to end with Python's RNG seeded like the fixture's generator, then the cached
    (``accelerate=True``) geometry gives the same result."""
    import random
    m = core['m']
    random.seed(3)
    with torch.no_grad():
        out = m(core['inp'])
    _check_outputs(core, out)
    m.accelerate, m.initial_flag = True, True
    try:
        random.seed(3)
        with torch.no_grad():
            m(core['inp'])
            random.seed(3)
            out2 = m(core['inp'])
        # MIOpen may pick another convolution algorithm on a later call: compare to 1e-5, not bitwise
        close(out2[0], out[0].cpu().numpy(), 1e-5, 'bev_feat with cached geometry')
        close(out2[3][4], out[3][4].cpu().numpy(), 1e-5, 'opacity view with cached geometry')
    finally:
        m.accelerate, m._geo = False, None


def test_training_path_matches_fused_path(core):
    """The differentiable torch formulation used in training mode (BatchNorm / dropout kept in eval
    so both paths see the same statistics) agrees with the fused kernels, and gradients reach the
    heads through the rasteriser's and the pooling's HIP backwards."""
    m, g = core['m'], core['g']
    cams = [int(c) for c in g['cam_idx_list']]
    cfg = core['cfg']
    pre = torch.from_numpy(g['pre']).cuda()
    depth = pre[:, :cfg.D].softmax(1)
    feat = pre[:, cfg.D + 2:].clone().requires_grad_(True)
    m.training = True               # top level only: sub-modules stay in eval mode
    try:
        bev, _, bev_mask, lst = m.view_transform_core(core['inp'], depth, feat, cam_idx_list=cams)
        (lst[0].sum() + bev.sum() + lst[4].sum()).backward()
    finally:
        m.training = False
    assert feat.grad is not None and torch.isfinite(feat.grad).all() and float(feat.grad.abs().sum()) > 0
    for name in ('S_MLP', 'R_MLP', 'A_MLP', 'C_MLP', 'sigma', 'img_feat_resize1'):
        gr = getattr(m, name)
        gr = (gr.fc1 if hasattr(gr, 'fc1') else gr[0]).weight.grad
        assert gr is not None and torch.isfinite(gr).all(), name
    m.zero_grad()
    with torch.no_grad():
        bev2, _, bev_mask2, lst2 = m.view_transform_core(core['inp'], depth, feat.detach(), cam_idx_list=cams)
    close(bev, bev2.cpu().numpy(), 1e-4, 'bev_feat train vs fused')
    close(bev_mask, bev_mask2.cpu().numpy(), 1e-4, 'bev_mask train vs fused')
    close(lst[4], lst2[4].cpu().numpy(), 1e-4, 'opacity view train vs fused')
    close(lst[3], lst2[3].cpu().numpy(), 1e-5, 'render_N train vs fused')
    close(lst[8], lst2[8].cpu().numpy(), 1e-5, 'render_depth_N train vs fused')


def test_second_forward_does_not_disturb_saved_ranks(core):
    """A forward of the same module BEFORE the backward of an earlier one (adjacent frame, second view, eval
    hook) must not change that backward: the rank vectors an autograd Function saved may not alias the
    module's persistent rank buffers (which only the forward-only sync=False path may use)."""
    m, g = core['m'], core['g']
    cams = [int(c) for c in g['cam_idx_list']]
    cfg = core['cfg']
    pre = torch.from_numpy(g['pre']).cuda()
    depth = pre[:, :cfg.D].softmax(1)

    def run(disturb):
        feat = pre[:, cfg.D + 2:].clone().requires_grad_(True)
        m.training = True
        try:
            bev, _, _, _ = m.view_transform_core(core['inp'], depth, feat, cam_idx_list=cams)
            if disturb:
                # another calibration (cameras rolled by one): different rank vectors of different lengths
                inp2 = list(core['inp'])
                for i in (1, 2, 3, 4, 5, 11):
                    inp2[i] = torch.roll(inp2[i], 1, 1) * (1.0 if i != 2 else 1.1)
                with torch.no_grad():
                    m.view_transform_core(inp2, depth, feat.detach(), cam_idx_list=cams)
                m.training = False
                with torch.no_grad():                      # and an eval forward, which does use the buffers
                    m.view_transform_core(inp2, depth, feat.detach(), cam_idx_list=cams)
            bev.sum().backward()
        finally:
            m.training = False
        m.zero_grad()
        return feat.grad.clone()

    a, b = run(False), run(True)
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def test_ht_project_bit_exact(core):
    """ocrf_ht_project vs the numpy oracle of get_sampling_point (itself pinned bit-exactly to the
    reference's vectors): mask identical, pixel coordinates of valid samples bit-identical."""
    from ocrfdet_amd import index_prep
    from oracle import index_prep as oip
    from ocrfdet_amd import synthetic
    cfg, B = core['cfg'], core['B']
    X, Y, _ = cfg.bev_xyz
    r = synthetic.rig(cfg.n_cams, cfg.input_size, B)
    calib = [torch.from_numpy(r[k]) for k in ('rots', 'trans', 'intrins', 'post_rots', 'post_trans', 'bda')]
    l2i, aug, _, _ = index_prep.get_projection(*calib)
    block = index_prep.ht_camera_block(l2i, aug).cuda()
    tmpl = index_prep.get_reference_points_3d(Y, X, bs=1, num_points_in_pillar=cfg.num_height, device='cpu')[0].cuda()
    pix, mask, voxel = index_prep.ht_project_hip(tmpl, block, B, cfg.n_cams, list(cfg.pc_range), cfg.input_size,
                                                 cfg.grid['depth'])
    # torch formulation with the SAME lidar2img / img_aug (the 3x3 inverses are LAPACK's on both sides)
    ref = tmpl.cpu()[None].repeat(B, 1, 1, 1)
    coor, tmask, _ = index_prep.get_sampling_point(ref, list(cfg.pc_range), cfg.grid['depth'], l2i, aug, cfg.input_size)
    want_pix = coor[..., :2].clone()
    want_pix[..., 0] *= cfg.input_size[1]
    want_pix[..., 1] *= cfg.input_size[0]
    m = tmask.squeeze(-1)
    assert torch.equal(mask.cpu(), m)
    assert torch.equal(pix.cpu()[m], want_pix[m])
    assert torch.equal(voxel.cpu(), ref)
    # and the numpy oracle's mask (pinned to the reference's sha256 in tests/test_index_prep.py)
    assert np.array_equal(mask.cpu().numpy(), core['mask'][..., 0])
    ok = core['mask'][..., 0]
    assert np.abs(pix.cpu().numpy()[ok] - core['pix'][ok]).max() < 1e-4


def test_gauss_heads_ragged_plane(core):
    """Y*X not a multiple of the 64-pillar wave tile: against the module's own torch layers."""
    from ocrfdet_amd import neck_ops
    m, cfg = core['m'], core['cfg']
    g = torch.Generator().manual_seed(3)
    bev = torch.randn(2, cfg.channels, 10, 7, generator=g).cuda()
    rgb = (torch.rand(2, cfg.num_height, 70, 3, generator=g) * 255).cuda()
    op, sc, rot, col = neck_ops.gauss_heads(bev, rgb, m._head_params(), cfg.num_height)
    with torch.no_grad():
        vf = m.ObtainVoxelFeature(bev.permute(0, 2, 3, 1).unsqueeze(1)).reshape(2, cfg.num_height * 70, -1)
        want = (m.A_MLP(vf), m.S_MLP(vf), m.R_MLP(vf), m.C_MLP(torch.cat((vf, rgb.reshape(2, -1, 3) / 255.0), -1)))
    for got, ref, name in zip((op, sc, rot, col), want, ('opacity', 'scales', 'rotations', 'colour')):
        close(got, ref.cpu().numpy(), 1e-5, name)


def test_dual_feat_fusion(core):
    """ocrf_dual_feat_fusion vs the numpy oracle, the reference fixture and the module's torch path
    (also a ragged plane)."""
    g, p, m, t = core['g'], core['p'], core['m'], core['t']
    with torch.no_grad():
        got = m.fuser(t(g['lss_feat']), t(g['ht_feat']))
    close(got, g['channel_feat'], 1e-5, 'fuser vs reference')
    close(got, oc.dual_feat_fusion(g['lss_feat'], g['ht_feat'], p), 1e-5, 'fuser vs oracle')
    gen = torch.Generator().manual_seed(9)
    a, b = torch.randn(3, 80, 9, 13, generator=gen).cuda(), torch.randn(3, 80, 9, 13, generator=gen).cuda()
    with torch.no_grad():
        fused = m.fuser(a, b)
        cf = m.fuser.ca(torch.cat((a, b), 1))
        want = cf * a + (1 - cf) * b
    close(fused, want.cpu().numpy(), 1e-5, 'fuser ragged vs torch ops')


@pytest.mark.parametrize('shape', [(2, 50, 70), (1, 33, 35), (3, 8, 130)])
def test_probnet_fused_matches_torch_layers(shape):
    """ProbNet in eval mode (three MIOpen convolutions with folded BatchNorms + ocrf_plane_bias_act_stats /
    ocrf_channel_mlp / ocrf_scaled_channel_stats / ocrf_cbam_tail) against the same module's torch layers
    (taken with autograd enabled); planes that are not multiples of the 64x4 tile or of 4 floats."""
    from ocrfdet_amd import view_transformer_ocrf as vto
    B, Y, X = shape
    torch.manual_seed(B * 100 + Y)
    dev = torch.device('cuda:0')
    prob = vto.ProbNet(in_channels=80).to(dev).eval()
    for mod in prob.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.3), mod.running_var.uniform_(0.5, 1.5)
            mod.weight.data.uniform_(0.5, 1.5), mod.bias.data.normal_(0, 0.2)
    x = torch.randn(B, 80, Y, X, device=dev)
    with torch.no_grad():
        got = prob(x)
    with torch.enable_grad():
        want = prob(x).detach()
    assert got.shape == want.shape == (B, 1, Y, X)
    close(got, want.cpu().numpy(), 2e-5 * float(want.abs().max()) + 2e-5, 'ProbNet fused vs torch layers')
    # a parameter update must invalidate the folded pack
    with torch.no_grad():
        prob.mask_net.bias.add_(0.5)
        got2 = prob(x)
    close(got2, (want + 0.5).cpu().numpy(), 2e-5 * float(want.abs().max()) + 2e-5, 'ProbNet after a parameter update')


def test_global_att_vector_matches_torch_layers():
    """MS_CAM's global branch (ocrf_plane_bias_act_stats in statistics-only mode + ocrf_channel_mlp) vs the layers."""
    from ocrfdet_amd import neck_ops
    from ocrfdet_amd import view_transformer_ocrf as vto
    torch.manual_seed(5)
    dev = torch.device('cuda:0')
    fuser = vto.DualFeatFusion(160, 80).to(dev).eval()
    for mod in fuser.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.3), mod.running_var.uniform_(0.5, 1.5)
    a, b = torch.randn(2, 80, 21, 37, device=dev), torch.randn(2, 80, 21, 37, device=dev) + 0.3
    with torch.no_grad():
        g = neck_ops.global_att_vector(a, b, neck_ops.pack_global_att(fuser.ca))
        want = torch.cat((a, b), 1).mean((2, 3), keepdim=True)
        for layer in list(fuser.ca.global_att)[1:]:
            want = layer(want)
    close(g, want.reshape(2, 80).cpu().numpy(), 1e-5, 'global_att vector')
    with torch.no_grad():
        fused = fuser(a, b)
    with torch.enable_grad():
        ref = fuser(a, b).detach()
    close(fused, ref.cpu().numpy(), 1e-5, 'DualFeatFusion fused vs torch layers')


@pytest.mark.parametrize('zh', [1, 2, 4, 6, 8, 13])
def test_gauss_heads_every_supported_height_count(zh):
    """Every register-tile instantiation of ocrf_gauss_heads (heights per pillar) against torch layers."""
    from ocrfdet_amd import neck_ops
    from ocrfdet_amd import view_transformer_ocrf as vto
    torch.manual_seed(zh)
    dev = torch.device('cuda:0')
    vfe = vto.VoxelFeatureExtractor(1, zh).to(dev).eval()
    bn = vfe.conv[1]
    bn.running_mean.normal_(0, 0.2), bn.running_var.uniform_(0.5, 1.5)
    heads = [cls(80, 4, o).to(dev) for cls, o in ((vto.ScaleFactorMLP, 3), (vto.RotationFactorMLP, 4),
                                                   (vto.OpacityFactorMLP, 1), (vto.ColorFactorMLPGaussian, 3))]
    bev = torch.randn(1, 80, 5, 27, device=dev)
    rgb = torch.rand(1, zh, 135, 3, device=dev) * 255
    prm = neck_ops.pack_gauss_head_params(vfe, *heads)
    op, sc, rot, col = neck_ops.gauss_heads(bev, rgb, prm, zh)
    with torch.no_grad():
        vf = vfe(bev.permute(0, 2, 3, 1).unsqueeze(1)).reshape(1, zh * 135, -1)
        want = (heads[2](vf), heads[0](vf), heads[1](vf), heads[3](torch.cat((vf, rgb.reshape(1, -1, 3) / 255.0), -1)))
    for got, ref, name in zip((op, sc, rot, col), want, ('opacity', 'scales', 'rotations', 'colour')):
        close(got, ref.cpu().numpy(), 1e-5, f'{name} (Zh={zh})')


@pytest.mark.parametrize('D', [5, 40, 200])
def test_prefilter_every_depth_tile(D):
    """The three register-tile sizes of the pre-filter (D <= 32, <= 128, <= 512), 1-pixel-wide map."""
    from ocrfdet_amd import neck_ops
    rng = np.random.default_rng(D)
    x = (rng.standard_normal((2, D + 2 + 12, 3, 1)) * 2).astype(np.float32)
    depth, fdepth, sem, feat = neck_ops.prefilter(torch.from_numpy(x).cuda(), D, 12, 1.0 / D, 0.3)
    wd, wfd, ws, wf = oc.prefilter(x, D, 12, 1.0 / D, 0.3)
    close(depth, wd, 1e-6, 'depth'), close(sem, ws, 1e-6, 'semantic')
    ok = np.abs(wd - np.float32(1.0 / D)) > 1e-6
    assert np.array_equal(fdepth.cpu().numpy()[ok] == 0, wfd[ok] == 0)
    sure = np.abs(ws[:, 1] - 0.3) > 1e-6
    assert np.array_equal(feat.cpu().numpy()[sure], np.ascontiguousarray(wf.transpose(0, 2, 3, 1))[sure])


def test_sampling_and_retain_edge_cases():
    """One camera, coordinates far outside / non-finite, nothing valid, every point valid."""
    from ocrfdet_amd import neck_ops
    rng = np.random.default_rng(2)
    B, N, Zh, Q, H, W = 2, 1, 3, 50, 9, 14
    imgs = rng.uniform(0, 255, (B, N, 3, H, W)).astype(np.float32)
    pix = np.stack([rng.uniform(-3, W + 3, (B, N, Zh, Q)), rng.uniform(-3, H + 3, (B, N, Zh, Q))], -1).astype(np.float32)
    pix[0, 0, 0, 0] = (np.inf, 2.0)
    pix[0, 0, 0, 1] = (np.nan, np.nan)
    pix[0, 0, 0, 2] = (1e30, -1e30)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    for mask in (np.ones((B, N, Zh, Q, 1), bool), np.zeros((B, N, Zh, Q, 1), bool), rng.random((B, N, Zh, Q, 1)) < 0.5):
        got = neck_ops.pillar_sample_mean(t(imgs), t(pix), t(mask)).cpu().numpy()
        want = oc.color_voxels_avg(oc.lidar_points_to_image_values(pix, imgs, mask), mask)
        fin = np.isfinite(want)
        assert np.isfinite(got).all() or not fin.all()
        np.testing.assert_allclose(got[fin], want[fin], atol=2e-4)
        inside = mask.copy()
        inside[..., 0] &= (pix[..., 0] >= 0) & (pix[..., 0] < W) & (pix[..., 1] >= 0) & (pix[..., 1] < H)
        r_got = neck_ops.retain_valid_pixels(t(imgs), t(pix), t(inside)).cpu().numpy()
        assert np.array_equal(r_got, oc.retain_valid_pixels(imgs, pix, inside))


def test_full_size_neck_fused_vs_torch_formulation():
    """BASELINE configs[2] size (6 cams x 2 frames, 256x704, BEV 200x200, 520 000 Gaussians per sample):
    the fused HIP neck against the reference's op sequence run as plain torch ops on the same GPU
    (materialising the (B,13,Y,X,80) voxel feature and the 12 x (80,256,704) NeRF feature images), with
    random-init weights of the reference architecture.  Tolerance 1e-4 (north_star)."""
    from ocrfdet_amd import hotpath, synthetic
    cfg = synthetic.CONFIGS['cfg2_6cam_2frame_bev200x200_render_hoa']
    neck = hotpath.NeckPath(cfg, torch.device('cuda:0'), accelerate=True)
    m = neck.module
    cams = [2, 5]
    with torch.no_grad():
        d, fd, s, fcl = neck._ops.prefilter(neck.depthnet_out, m.D, m.out_channels, m.depth_threshold, m.semantic_threshold)
        want_d = neck.depthnet_out[:, :m.D].softmax(1)
        close(d, want_d.cpu().numpy(), 1e-6, 'depth softmax at full size')
        m.pre_compute(neck.inputs)
        fused = m.view_transform_core(neck.inputs, fd, None, fcl, cam_idx_list=cams)
        m.training = True                        # top level only: the torch formulation, BatchNorm still in eval
        try:
            tran = fcl.permute(0, 3, 1, 2).contiguous()
            plain = m.view_transform_core(neck.inputs, fd, tran, None, cam_idx_list=cams)
        finally:
            m.training = False
    close(fused[0], plain[0].cpu().numpy(), 1e-4, 'bev_feat')
    close(fused[2], plain[2].cpu().numpy(), 1e-4, 'bev_mask_logit')
    names = ['render_imgs', 'gt_images', 'render_G', 'render_N', 'opacity_alpha_view', None, 'render_depth',
             'render_depth_G', 'render_depth_N']
    for i, name in enumerate(names):
        if name is None:
            continue
        a, b = fused[3][i], plain[3][i]
        dlt = (a - b).abs()
        if name in ('render_imgs', 'render_G', 'render_depth', 'render_depth_G'):
            # the rasteriser blends ~100 Gaussians per pixel: parameters that differ by 1e-6 can move a
            # pixel's early-termination point; allow a vanishing share of such pixels
            assert float((dlt > 1e-4).float().mean()) < 1e-3 and float(dlt.max()) < 5e-2, name
        else:
            assert float(dlt.max()) <= 1e-4, f'{name}: {float(dlt.max()):.3e}'


def test_graph_captured_step_matches_eager():
    """hotpath.NeckPath: the whole neck step replayed as one hipGraph equals the eager step for the
    same camera choice, follows a changed camera choice through the static camera buffers, and
    survives many restaged replays (the library launches no memset inside a step: csrc/launch.h)."""
    import random
    from ocrfdet_amd import hotpath, synthetic
    cfg = synthetic.PathConfig(**{**helpers.CORE_CFG, 'n_frames': 2})
    neck = hotpath.NeckPath(cfg, torch.device('cuda:0'), accelerate=True)
    m = neck.module
    neck.capture()
    for cams in ([1, 4], [5, 0]):
        out_g = neck.step_graphed(cams)
        bev_g, view_g, img_g = out_g[0].clone(), out_g[3][4].clone(), out_g[3][0].clone()
        with torch.no_grad():
            d, fd, s, fcl = neck._ops.prefilter(neck.depthnet_out, m.D, m.out_channels, m.depth_threshold, m.semantic_threshold)
            out_e = m.view_transform_core(neck.inputs, fd, None, fcl, cam_idx_list=cams)
        close(bev_g, out_e[0].cpu().numpy(), 1e-5, 'bev_feat graph vs eager')
        close(view_g, out_e[3][4].cpu().numpy(), 1e-5, 'opacity view graph vs eager')
        close(img_g, out_e[3][0].cpu().numpy(), 1e-5, 'render graph vs eager')
        assert out_g[3][5] == cams
    for _ in range(40):
        neck.step_graphed([random.randint(0, 5), random.randint(0, 5)])
    torch.cuda.synchronize()
    # the captured graph was inspected: kernels only where it matters (a memset node would fault on replay)
    census = getattr(neck._graphed, 'census', None)
    if census is not None:
        assert census['memset'] == 0 and census['kernel'] > 20, census
        # ... and a graph that does hold one is refused by the same census
        from ocrfdet_amd import _lib
        g = torch.cuda.CUDAGraph(keep_graph=True)
        buf = torch.ones(1 << 16, device='cuda')
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(g, stream=s):
            buf.zero_()
            buf.add_(1.0)
        c2 = _lib.graph_census(g)
        assert c2['memset'] >= 1 or c2['kernel'] >= 2, c2      # torch may zero with a kernel: then nothing to refuse


def test_full_training_mode_forward_backward(core):
    """``module.train()`` for real (BatchNorm batch statistics, dropout in the deformable attention):
    forward + backward through the whole neck on the GPU; every trainable parameter of the path gets a
    finite gradient (a drop-in has to train, not only infer)."""
    import copy
    m = copy.deepcopy(core['m'])            # also: a module that has run its fused path must stay deep-copyable
    m.train()
    cfg, g = core['cfg'], core['g']
    pre = torch.from_numpy(g['pre']).cuda()
    depth = pre[:, :cfg.D].softmax(1).requires_grad_(True)
    feat = pre[:, cfg.D + 2:].clone().requires_grad_(True)
    torch.manual_seed(0)
    bev, _, logit, lst = m.view_transform_core(core['inp'], depth, feat, cam_idx_list=[1, 4])
    loss = bev.square().mean() + logit.square().mean() + lst[0].mean() + lst[6].mean() + lst[4].square().mean()
    loss.backward()
    assert torch.isfinite(loss)
    assert depth.grad is not None and feat.grad is not None
    assert torch.isfinite(depth.grad).all() and torch.isfinite(feat.grad).all()
    missing = [n for n, p in m.named_parameters()
               if p.requires_grad and not n.startswith(('depth_net.', 'D_MLP_nerf.', 'prob.ce_loss'))
               and (p.grad is None or not torch.isfinite(p.grad).all())]
    assert not missing, f'no / non-finite gradient for {missing[:8]}'


def test_fused_heads_training_matches_layer_formulation(core):
    """``module.train()``: the whole neck forward + backward with the voxel lift + four heads on the fused forward / backward
    kernels (csrc/neck_train.hip, the default) against the reference's layer formulation on the (B,13,Y,X,80) voxel
    feature (``fused_heads_training = False``) — loss, input gradients and every parameter gradient within 1e-4 of the
    largest entry, BatchNorm running statistics alike."""
    import copy
    cfg, g = core['cfg'], core['g']
    pre = torch.from_numpy(g['pre']).cuda()
    got = {}
    for fused in (True, False):
        m = copy.deepcopy(core['m']).train()
        m.fused_heads_training = fused
        depth = pre[:, :cfg.D].softmax(1).requires_grad_(True)
        feat = pre[:, cfg.D + 2:].clone().requires_grad_(True)
        torch.manual_seed(0)
        bev, _, logit, lst = m.view_transform_core(core['inp'], depth, feat, cam_idx_list=[1, 4])
        loss = bev.square().mean() + logit.square().mean() + lst[0].mean() + lst[6].mean() + lst[4].square().mean()
        loss.backward()
        grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
        grads['<depth>'], grads['<feat>'] = depth.grad, feat.grad
        bn = m.ObtainVoxelFeature.conv[1]
        got[fused] = (float(loss.detach()), grads, lst[2].detach(), (bn.running_mean.clone(), bn.running_var.clone()))
    assert abs(got[True][0] - got[False][0]) <= 1e-5 * abs(got[False][0])
    close(got[True][2], got[False][2].cpu().numpy(), 1e-5, 'Gaussian render, fused heads vs layers')
    assert set(got[True][1]) == set(got[False][1])
    # the convolution in front of a BatchNorm in training mode: its gradient is a residue of cancelling terms of the size
    # of the BatchNorm weight's gradient (tests/test_neck_train_gpu.py), which is the scale it is held to
    bn_scale = float(got[False][1]['ObtainVoxelFeature.conv.1.weight'].abs().max())
    for n, want in got[False][1].items():
        scale = bn_scale if n.startswith('ObtainVoxelFeature.conv.0') else float(want.abs().max())
        err = float((got[True][1][n] - want).abs().max())
        # (+ 1e-7: biases in front of a training-mode BatchNorm have gradients of ~1e-8 — rounding residue of sums that
        # cancel, in either formulation)
        assert err <= 1e-4 * scale + 1e-7, f'{n}: |err| {err:.3e} vs 1e-4 x {scale:.3e}'
    for a, b in zip(got[True][3], got[False][3]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def test_parallel_branches_match_single_stream(core):
    """The three strands of the fused step on side HIP streams give the single-stream result, call
    after call (buffers of one call are recycled by the next)."""
    m, g = core['m'], core['g']
    cams = [int(c) for c in g['cam_idx_list']]
    from ocrfdet_amd import neck_ops
    with torch.no_grad():
        y = m.depth_net(None, None, None)
        depth, fdepth, sem, feat_cl = neck_ops.prefilter(y, m.D, m.out_channels, m.depth_threshold, m.semantic_threshold)
        ref = m.view_transform_core(core['inp'], fdepth, None, feat_cl, cam_idx_list=cams)
        m.parallel_branches = True
        try:
            for _ in range(4):
                out = m.view_transform_core(core['inp'], fdepth, None, feat_cl, cam_idx_list=cams)
                torch.cuda.synchronize()
                close(out[0], ref[0].cpu().numpy(), 1e-5, 'bev_feat')
                close(out[2], ref[2].cpu().numpy(), 1e-5, 'bev_mask_logit')
                for i in (0, 1, 2, 3, 4, 6, 7, 8):
                    close(out[3][i], ref[3][i].cpu().numpy(), 1e-5, f'extras[{i}]')
        finally:
            m.parallel_branches = False
    _check_outputs(core, (out[0], depth, (out[2], sem), out[3]))


def test_graphed_neck_follows_new_inputs(core):
    """view_transformer_ocrf.GraphedNeck: new image features / raw images / DepthNet outputs are copied
    into the graph's static buffers; the replay matches the module's eager forward on them."""
    import copy
    from ocrfdet_amd import neck_ops
    from ocrfdet_amd.view_transformer_ocrf import GraphedNeck
    m = copy.deepcopy(core['m'])
    m.accelerate, m.initial_flag = True, True
    g = core['g']
    pre = torch.from_numpy(g['pre']).cuda()
    neck = GraphedNeck(m, core['inp'], pre)
    gen = torch.Generator().manual_seed(5)
    for trial in range(2):
        inp = list(core['inp'])
        inp[0] = torch.randn(inp[0].shape, generator=gen).cuda()
        raw = torch.randint(0, 256, inp[9].shape, generator=gen).float().cuda()
        inp[8], inp[9], inp[10] = raw.clone(), raw, raw.clone()
        y = (torch.randn(pre.shape, generator=gen) * 2).cuda()
        cams = [trial, 5 - trial]
        bev, depth, (bev_mask, sem), ex = neck(inp, y, cams)
        got = [bev.clone(), depth.clone(), bev_mask.clone(), ex[4].clone(), ex[0].clone(), ex[3].clone()]
        with torch.no_grad():
            d, fd, s, fcl = neck_ops.prefilter(y, m.D, m.out_channels, m.depth_threshold, m.semantic_threshold)
            want = m.view_transform_core(inp, fd, None, fcl, cam_idx_list=cams)
        close(got[0], want[0].cpu().numpy(), 1e-5, 'bev_feat')
        close(got[1], d.cpu().numpy(), 1e-6, 'depth')
        close(got[2], want[2].cpu().numpy(), 1e-5, 'bev_mask_logit')
        close(got[3], want[3][4].cpu().numpy(), 1e-5, 'opacity view')
        close(got[4], want[3][0].cpu().numpy(), 1e-5, 'render_imgs')
        close(got[5], want[3][3].cpu().numpy(), 1e-5, 'render_N')
        assert ex[5] == cams


def test_pinned_staging_outlasts_its_slots(core):
    """More refreshes in a row than the pinned rings have slots (four behind a staged camera dict, eight behind
    ``_small_h2d``): every refresh lands on the device with the host's values, and the module, which owns neither pinned
    memory nor events, stays deep-copyable."""
    import copy
    import math
    from ocrfdet_amd import gaussian_renderer
    from ocrfdet_amd.diff_gaussian_rasterization import pack_cameras
    m, inp = copy.deepcopy(core['m']), core['inp']
    dev, (H, W) = inp[0].device, m.input_size
    geo = m._geometry(inp)                       # host formulation: the rows are made on the host and staged
    K, c2w = inp[3].cpu(), inp[11].cpu()

    def row(b, c):
        cam = gaussian_renderer.camera_from_calibration(K[b, c].numpy(), c2w[b, c].numpy(), H, W, znear=m.znear, zfar=m.zfar)
        return pack_cameras(cam['world_view_transform'][None], cam['full_proj_transform'][None],
                            math.tan(float(cam['FovX']) * 0.5), math.tan(float(cam['FovY']) * 0.5), H, W, 'cpu')
    rng = np.random.default_rng(3)
    cams = m.stage_cameras(geo, [0, 0], dev)
    for _ in range(10):
        pick = [int(c) for c in rng.integers(0, 6, core['B'])]
        assert m.stage_cameras(geo, pick, dev, out=cams) is cams
        assert cams['cam_idx_list'] == pick and cams['cam_sel'].dtype == torch.int32
        assert cams['cam_sel'].cpu().tolist() == pick
        assert torch.equal(cams['packed'].cpu(), torch.cat([row(b, c) for b, c in enumerate(pick)]))
    for i in range(10):
        host = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, 1 + 7 * i, dtype=np.int64).astype(np.int32))
        got = m._small_h2d(host, dev)
        assert got.dtype == torch.int32 and got.device == dev and torch.equal(got.cpu(), host)
    m2 = copy.deepcopy(m)
    assert torch.equal(m2._small_h2d(host, dev).cpu(), host)


def test_cbam_entry_points_edge_cases_and_argument_errors():
    """Tiny planes (fewer elements than one chunk / one tile), K at the channel_mlp limit, and the C entry points'
    refusal of malformed calls (hipErrorInvalidValue = 1 instead of a launch)."""
    import ctypes
    from ocrfdet_amd import _lib, neck_ops
    dev = torch.device('cuda:0')
    torch.manual_seed(3)
    # 1 x 3 plane: every chunk but the first is empty
    y = torch.randn(2, 5, 1, 3, device=dev)
    bias = torch.randn(5, device=dev)
    psum, pmax = torch.empty(2, 5, 8, device=dev), torch.empty(2, 5, 8, device=dev)
    want = torch.relu(y + bias.view(1, 5, 1, 1))
    neck_ops.plane_bias_act_stats(y, bias, relu=True, stats=(psum, pmax))
    assert torch.equal(y, want)
    assert torch.allclose(psum.sum(2), want.sum((2, 3)), atol=1e-6) and torch.equal(pmax.amax(2), want.amax((2, 3)))
    # channel_mlp at K = 256, M = 64 against torch
    B, K, M, N, S = 3, 256, 64, 70, 4
    ps, pm = torch.randn(B, K, S, device=dev), torch.randn(B, K, S, device=dev)
    w1, b1 = torch.randn(M, K, device=dev) / 16, torch.randn(M, device=dev)
    w2, b2 = torch.randn(N, M, device=dev) / 8, torch.randn(N, device=dev)
    got = neck_ops.channel_mlp(ps, pm, 0.25, w1, b1, w2, b2, use_max=True, sigmoid=True)
    f = lambda v: torch.relu(v @ w1.t() + b1) @ w2.t() + b2
    ref = torch.sigmoid(f(ps.sum(2) * 0.25) + f(pm.amax(2)))
    close(got, ref.cpu().numpy(), 2e-5, 'channel_mlp at the size limits')
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    p = _lib.ptr
    assert L.ocrf_channel_mlp(p(ps), p(pm), B, 257, S, ctypes.c_float(1.0), p(w1), p(b1), p(w2), p(b2), M, N, 1, 1,
                              p(got), st) == 1                                    # K over the LDS budget
    assert L.ocrf_channel_mlp(p(ps), None, B, K, S, ctypes.c_float(1.0), p(w1), p(b1), p(w2), p(b2), M, N, 1, 1,
                              p(got), st) == 1                                    # use_max without maxima
    assert L.ocrf_plane_bias_act_stats(p(y), p(bias), 2, 5, 3, 1, 0, 8, 5, 0, None, None, st) == 1   # nothing to do
    assert L.ocrf_plane_bias_act_stats(p(y), p(bias), 2, 5, 3, 1, 1, 8, 4, 0, p(psum), p(pmax), st) == 1  # out_C < C
    x = torch.randn(1, 4, 2, 2, device=dev)
    sc, stt, w = torch.ones(1, 4, device=dev), torch.zeros(1, 2, 2, 2, device=dev), torch.zeros(2 * 16, device=dev)
    lg = torch.empty(1, 1, 2, 2, device=dev)
    assert L.ocrf_cbam_tail(p(x), p(sc), p(stt), p(w), 4, p(x), p(sc), ctypes.c_float(0.0), 1, 4, 2, 2, p(lg), None,
                            st) == 1                                              # even kernel size
    torch.cuda.synchronize()


@torch.no_grad()
def test_cached_geometry_renders_through_a_plan_and_matches_the_per_call_render(cuda):
    """accelerate=True: the fused forward renders through a static render plan (device-guarded); same images, bit for
    bit, as the per-call pipeline, for several random camera choices and after the scale head outgrows the plan's
    extent bound (the armed per-call chain then renders)."""
    from ocrfdet_amd import hotpath, synthetic
    cfg = synthetic.PathConfig(**{**synthetic.CONFIGS['cfg0_1cam_128x352_bev64x64x4'].__dict__, 'name': 'neck6', 'n_cams': 6,
                                  'n_frames': 2, 'input_size': (64, 176), 'grid': dict(x=[-19.2, 19.2, 0.8], y=[-19.2, 19.2, 0.8],
                                                                                      z=[-5.0, 3.0, 8.0], depth=[1.0, 60.0, 0.5]),
                                  'pc_range': (-19.2, -19.2, -5.0, 19.2, 19.2, 3.0)})
    a = hotpath.NeckPath(cfg, cuda, accelerate=True, seed=3)
    b = hotpath.NeckPath(cfg, cuda, accelerate=True, seed=3)
    b.module.render_plan = False
    for n in (a, b):
        n.module.pre_compute(n.inputs)
    # drive both modules through the same forwards
    for choice in ([0, 3], [5, 1], [2, 2]):
        outs = []
        for n in (a, b):
            m = n.module
            depth, fdepth, sem, feat_cl = n._ops.prefilter(n.depthnet_out, m.D, m.out_channels, m.depth_threshold,
                                                           m.semantic_threshold)
            outs.append(m.view_transform_core(n.inputs, fdepth, None, feat_cl, cam_idx_list=choice))
        torch.cuda.synchronize()
        assert a.module._geo.raster_plan and not b.module._geo.raster_plan
        ea, eb = outs[0][3], outs[1][3]
        assert torch.equal(ea[2], eb[2]) and torch.equal(ea[7], eb[7])          # render_image_G_all, render_depth_G_all
        assert torch.equal(outs[0][0], outs[1][0])
    plan = a.module._geo.raster_plan[0]
    assert not plan.exceeded()
    # the scale head outgrows the bound: still exact (device guard), and the plan says so
    for n in (a, b):
        with torch.no_grad():
            n.module.S_MLP.fc2.bias += 3.0
    outs = []
    for n in (a, b):
        m = n.module
        depth, fdepth, sem, feat_cl = n._ops.prefilter(n.depthnet_out, m.D, m.out_channels, m.depth_threshold, m.semantic_threshold)
        outs.append(m.view_transform_core(n.inputs, fdepth, None, feat_cl, cam_idx_list=[4, 0]))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][3][2], outs[1][3][2]) and torch.equal(outs[0][3][7], outs[1][3][7])
    assert plan.exceeded()
