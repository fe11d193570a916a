"""GPU: per-forward calibration algebra on the device (C ABI ``ocrf_geometry_blocks``) — the
camera blocks of both index preparations and the render-camera rows from the calibration tensors where they
already live, with no host read.  Double-precision cofactor inverses rounded once: ~1 ulp from the reference's
float32 LAPACK / matmul chain (which stays the default path and is pinned bit for bit elsewhere), so the bars here
are relative 3e-6 on the blocks and on the camera rows (of the row's largest entry), and identical rank vectors up to a 1e-5 fraction of
points that sit on a cell border."""
import math

import numpy as np
import pytest
import torch

from ocrfdet_amd import diff_gaussian_rasterization as dgr
from ocrfdet_amd import gaussian_renderer as gr
from ocrfdet_amd import index_prep as ip
from ocrfdet_amd import synthetic

pytestmark = pytest.mark.gpu


def _calib(cfg, B, cuda, jitter=0.0):
    r = synthetic.rig(cfg.n_cams, cfg.input_size, B)
    rng = np.random.default_rng(3)
    if jitter:
        # a non-trivial augmentation: in-plane rotation + scale of post_rots, a yawed bda, perturbed extrinsics
        for b in range(B):
            a = rng.uniform(-0.1, 0.1)
            R = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
            r['bda'][b] = (R * rng.uniform(0.95, 1.05)).astype(np.float32)
            for n in range(cfg.n_cams):
                t = rng.uniform(-jitter, jitter)
                Rz = np.array([[math.cos(t), -math.sin(t), 0], [math.sin(t), math.cos(t), 0], [0, 0, 1]])
                r['post_rots'][b, n] = (Rz @ r['post_rots'][b, n]).astype(np.float32)
                r['trans'][b, n] += rng.uniform(-0.05, 0.05, 3).astype(np.float32)
    host = [torch.from_numpy(r[k]) for k in ('rots', 'trans', 'intrins', 'post_rots', 'post_trans', 'bda')]
    return r, host, [t.to(cuda) for t in host], torch.from_numpy(r['c2w']).to(cuda)


@pytest.mark.parametrize('jitter', [0.0, 0.05])
def test_blocks_and_camera_rows_match_host_formulation(cuda, jitter):
    cfg = synthetic.CONFIGS['cfg2_6cam_2frame_bev200x200_render_hoa']
    B = 2
    r, host, dev, c2w = _calib(cfg, B, cuda, jitter)
    lss, ht, cam = ip.geometry_blocks_hip(*dev, c2w, cfg.input_size)
    want_lss = ip.lss_camera_block(*host)
    l2i, aug, _, _ = ip.get_projection(*host)
    want_ht = ip.ht_camera_block(l2i, aug)
    scale = lambda w: max(1.0, float(w.abs().max()))       # noqa: E731
    assert float((lss.cpu() - want_lss).abs().max()) <= 3e-6 * scale(want_lss)
    assert float((ht.cpu() - want_ht).abs().max()) <= 3e-6 * scale(want_ht)
    H, W = cfg.input_size
    for b in range(B):
        for n in range(cfg.n_cams):
            c = gr.camera_from_calibration(r['intrins'][b, n], r['c2w'][b, n], H, W)
            row = dgr.pack_cameras(c['world_view_transform'][None], c['full_proj_transform'][None],
                                   math.tan(float(c['FovX']) * 0.5), math.tan(float(c['FovY']) * 0.5), H, W, 'cpu')[0]
            got = cam[b, n].cpu()
            assert torch.equal(got[:16], row[:16])                               # the view matrix is a copy
            # full_proj = world_view @ projection in float32: a different accumulation order moves an element whose
            # terms cancel by a few ulp OF THE TERMS
            np.testing.assert_allclose(got.numpy(), row.numpy(), rtol=2e-6, atol=2e-6 * float(row.abs().max()))


def test_ranks_from_device_geometry_agree_with_the_host_path(cuda):
    cfg = synthetic.CONFIGS['cfg2_6cam_2frame_bev200x200_render_hoa']
    B = 2
    _, host, dev, c2w = _calib(cfg, B, cuda)
    lss_d, ht_d, _ = ip.geometry_blocks_hip(*dev, c2w, cfg.input_size)
    lss_h = ip.lss_camera_block(*host).to(cuda)
    l2i, aug, _, _ = ip.get_projection(*host)
    ht_h = ip.ht_camera_block(l2i, aug).to(cuda)
    frustum = ip.create_frustum(cfg.grid['depth'], cfg.input_size, cfg.downsample).to(cuda)
    lower, interval, size = ip.grid_infos(cfg.grid)
    X, Y, _ = cfg.bev_xyz
    Hf, Wf = cfg.feat_hw
    tmpl = ip.get_reference_points_3d(Y, X, bs=1, num_points_in_pillar=cfg.num_height, device='cpu')[0].to(cuda)
    for name, run in (('lss', lambda blk: ip.voxel_pooling_prepare_v2_hip(frustum, blk, B, cfg.n_cams, lower, interval, size)),
                      ('ht', lambda blk: ip.fast_sample_prepare_hip(tmpl, blk, B, cfg.n_cams, list(cfg.pc_range),
                                                                    cfg.input_size, cfg.grid['depth'], Wf, Hf, cfg.D))):
        a = run(lss_d if name == 'lss' else ht_d)
        b = run(lss_h if name == 'lss' else ht_h)
        ta = torch.stack([t.long() for t in a[:3]], 1).cpu().numpy()
        tb = torch.stack([t.long() for t in b[:3]], 1).cpu().numpy()
        sa = {tuple(x) for x in ta.tolist()}
        sb = {tuple(x) for x in tb.tolist()}
        moved = len(sa ^ sb)
        assert moved <= max(4, 2e-5 * len(sb)), f'{name}: {moved} of {len(sb)} rank triples differ'


def test_forward_with_device_geometry_does_not_synchronise(cuda):
    """The whole eval forward of the module with ``device_geometry`` and the calibration on the GPU: PyTorch's
    synchronisation checker sees no blocking call, and the outputs agree with the host-geometry forward."""
    from ocrfdet_amd import view_transformer_ocrf as vto
    from tests import helpers
    cfg, g, state = helpers.core_fixture()
    m = vto.OcRFViewTransformerFull(pc_range=list(cfg.pc_range), bev_h=48, bev_w=48, num_height=13, grid_config=cfg.grid,
                                    input_size=cfg.input_size, downsample=16, in_channels=256, out_channels=80,
                                    depth_net=torch.nn.Identity())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    m.cuda().eval()
    B = int(g['batch'])
    rig = synthetic.rig(cfg.n_cams, cfg.input_size, B)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    raw = t(g['raw'].astype(np.float32))
    inp = [t(g['x'].astype(np.float32))] + [t(rig[k]) for k in ('rots', 'trans', 'intrins', 'post_rots', 'post_trans', 'bda')]
    inp += [torch.zeros(B, 6, 27).cuda(), raw.clone(), raw, raw.clone(), t(rig['c2w'])]
    pre = t(g['pre'])
    depth = pre[:, :cfg.D].softmax(1)
    feat = pre[:, cfg.D + 2:].contiguous()
    cams = [int(c) for c in g['cam_idx_list']]
    with torch.no_grad():
        assert m.device_geometry is None                  # the default: on the device whenever the calibration is there
        m.device_geometry = False                         # ... opted out: the host formulation (bit-exact rank vectors)
        want = m.view_transform_core(inp, depth, feat, cam_idx_list=cams)
        m.device_geometry = None
        m.view_transform_core(inp, depth, feat, cam_idx_list=cams)            # warm-up: allocations, packs
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            got = m.view_transform_core(inp, depth, feat, cam_idx_list=cams)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    # a handful of border samples may change cell (module docstring): compare the bulk
    for a, b, what in ((got[0], want[0], 'bev_feat'), (got[3][0], want[3][0], 'render'), (got[3][4], want[3][4], 'opacity view')):
        d = (a - b).abs()
        frac = float((d > 1e-4).float().mean())
        assert frac <= 2e-3, f'{what}: {frac:.2e} of the elements differ by more than 1e-4'


def _setup(cuda):
    """The reference-shaped module on the core fixture's weights with every calibration tensor on the GPU."""
    from ocrfdet_amd import view_transformer_ocrf as vto
    from tests import helpers
    cfg, g, state = helpers.core_fixture()
    m = vto.OcRFViewTransformerFull(pc_range=list(cfg.pc_range), bev_h=48, bev_w=48, num_height=13, grid_config=cfg.grid,
                                    input_size=cfg.input_size, downsample=16, in_channels=256, out_channels=80,
                                    depth_net=torch.nn.Identity())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    m.cuda().eval()
    B = int(g['batch'])
    rig = synthetic.rig(cfg.n_cams, cfg.input_size, B)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    raw = t(g['raw'].astype(np.float32))
    inp = [t(g['x'].astype(np.float32))] + [t(rig[k]) for k in ('rots', 'trans', 'intrins', 'post_rots', 'post_trans', 'bda')]
    inp += [torch.zeros(B, 6, 27).cuda(), raw.clone(), raw, raw.clone(), t(rig['c2w'])]
    pre = t(g['pre'])
    return cfg, m, inp, pre[:, :cfg.D].softmax(1), pre[:, cfg.D + 2:].contiguous()


def test_training_forward_and_backward_read_nothing_back(cuda):
    """``module.train()`` with the calibration on the GPU (``device_geometry`` auto): the geometry stays on the device
    under autograd too — rank vectors at their capacity with device-side lengths in tensors of this forward, poolings
    differentiated by ``_FusedPool`` with counts, cameras staged from the device rows — so forward + backward run without a single
    synchronising call (the reference reads the calibration to the host once per forward, view_transformer_ocrf.py:1086-1088).
    Against the opted-out host formulation: same loss and gradients up to the handful of border samples that change cell."""
    cfg, m, inp, depth0, feat0 = _setup(cuda)
    cams = [1, 4]

    def run(mod):
        depth = depth0.clone().requires_grad_(True)
        feat = feat0.clone().requires_grad_(True)
        torch.manual_seed(0)
        bev, _, logit, lst = mod.view_transform_core(inp, depth, feat, cam_idx_list=cams)
        loss = bev.square().mean() + logit.square().mean() + lst[0].mean() + lst[6].mean() + lst[4].square().mean()
        loss.backward()
        return loss.detach(), depth.grad, feat.grad

    import copy
    host = copy.deepcopy(m).train()
    host.device_geometry = False
    want = run(host)
    dev = copy.deepcopy(m).train()
    run(dev)                                                   # warm-up: allocations, packs
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = run(dev)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert abs(float(got[0]) - float(want[0])) <= 2e-3 * abs(float(want[0]))
    for a, b, what in ((got[1], want[1], 'd depth'), (got[2], want[2], 'd feat')):
        d = (a - b).abs()
        frac = float((d > 1e-4 * float(b.abs().max())).float().mean())
        assert frac <= 2e-3, f'{what}: {frac:.2e} of the entries differ by more than 1e-4 of the largest'


def test_graph_with_the_geometry_inside_follows_the_calibration(cuda):
    """GraphedNeck on an ``accelerate=False`` module with ``device_geometry``: calibration algebra, both index
    preparations and the rest of the forward replay as ONE hipGraph launch, and the replay follows the calibration
    VALUES of each call (copied into the graph's static inputs) — equal to the eager per-forward path bit for bit."""
    from ocrfdet_amd import hotpath
    cfg = synthetic.CONFIGS['ref_6cam_256x704_bev128x128x1']
    neck = hotpath.NeckPath(cfg, cuda, accelerate=False)
    neck.module.device_geometry = True
    with torch.no_grad():
        neck.step()                                   # allocations, packs, MIOpen algorithms
        neck.capture()
        cams = [2] * neck.batch
        base = [t.clone() if torch.is_tensor(t) else t for t in neck.inputs]
        for trial in range(2):
            inp = [t.clone() if torch.is_tensor(t) else t for t in base]
            if trial == 1:                            # another rig pose: yaw the ego frame, move the cameras
                a = 0.07
                R = torch.tensor([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]], device=cuda)
                inp[6] = (R @ inp[6]).contiguous()
                inp[2] = inp[2] + 0.05
            m = neck.module
            depth, fdepth, sem, feat_cl = neck._ops.prefilter(neck.depthnet_out, m.D, m.out_channels, m.depth_threshold,
                                                              m.semantic_threshold)
            want = m.view_transform_core(inp, fdepth, None, feat_cl, cam_idx_list=cams)
            got = neck._graphed(inp, neck.depthnet_out, cam_idx_list=cams)
            torch.cuda.synchronize()
            assert torch.equal(got[0], want[0]), f'trial {trial}: BEV feature differs'
            assert torch.equal(got[3][0], want[3][0]), f'trial {trial}: rendered image differs'
            if trial == 1:
                assert not torch.equal(got[0], first), 'the replay ignored the new calibration'
            first = got[0].clone()
