"""GPU: the fused training losses of csrc/losses.hip (``ocrf_depth_labels``, ``ocrf_depth_semantic_loss``,
``ocrf_render_losses`` and their backwards) against the torch formulation and the reference's values
(``tests/golden/losses.npz``): labels bit for bit, losses within 1e-5 relative, gradients within 1e-5 of their largest
entry; deterministic; no host synchronisation; the module in training mode end to end."""
import copy

import numpy as np
import pytest
import torch

from ocrfdet_amd import losses

pytestmark = pytest.mark.gpu

CAMS = [1, 4]


def _module(g, dev):
    from ocrfdet_amd import view_transformer_ocrf as vto
    grid = dict(x=[-12.8, 12.8, 1.6], y=[-12.8, 12.8, 1.6], z=[-5.0, 3.0, 8.0], depth=list(g['depth_cfg']))
    return vto.OcRFViewTransformerFull(pc_range=[-12.8, -12.8, -5.0, 12.8, 12.8, 3.0], bev_h=16, bev_w=16, num_height=13,
                                       grid_config=grid, input_size=tuple(g['gt_depth'].shape[-2:]),
                                       downsample=int(g['ds']), in_channels=16, out_channels=16,
                                       depth_net=torch.nn.Identity()).to(dev)


def _boxes(g, dev=None):
    B, N = g['box_counts'].shape
    return [[torch.from_numpy(g['boxes'][b, n, :g['box_counts'][b, n]]).to(dev or 'cpu') for n in range(N)]
            for b in range(B)]


def _decode(g):
    """The fixture's float32 tensors: uint8 k -> k / 256 (images, render depths), int8 k -> k / 16 (logits), exact."""
    out = {}
    for k in g.files:
        v = g[k]
        if v.dtype == np.uint8:
            v = v.astype(np.float32) / np.float32(256)
        elif v.dtype == np.int8:
            v = v.astype(np.float32) / np.float32(16)
        out[k] = torch.from_numpy(np.ascontiguousarray(v))
    return out


def _want_grads(g, tag):
    """The stored reference gradients of one case (the label-loss ones are shared, see make_golden_losses.py)."""
    want = {'depth': g['grad_depth'], 'semantic': g['grad_semantic']}
    for k in ('render', 'render_G', 'render_N', 'render_depth', 'render_depth_N'):
        if f'grad_{tag}_{k}' in g.files:
            want[k] = g[f'grad_{tag}_{k}']
    return want


def _inputs(g, dev):
    """The fixture's tensors on ``dev`` (copied before any sync check is armed); the softmax on the host, so that the
    inputs are the fixture's to the bit."""
    t = _decode(g)
    t['depth'], t['semantic'] = t['depth_logits'].softmax(1), t['sem_logits'].softmax(1)
    return {k: v.to(dev) for k, v in t.items()}


def _run(m, g, tag, dev, device_boxes=False, t=None):
    t = _inputs(g, dev) if t is None else t
    m.loss_iteration = 3862 * 2 - 1 if tag == 'nomask' else 3862 * 2
    depth, sem = t['depth'].clone().requires_grad_(True), t['semantic'].clone().requires_grad_(True)
    rs = [t[k].clone().requires_grad_(True) for k in ('render', 'render_G', 'render_N')]
    rd, rdN = t['render_depth'].clone().requires_grad_(True), t['render_depth_N'].clone().requires_grad_(True)
    gd, gs = t['gt_depth'], t['gt_semantic']
    boxes = t['device_boxes'] if device_boxes else _boxes(g)
    ls = m.get_loss(depth, sem, gd, gs, boxes, CAMS, rs[0], t['gt_images'], rs[1], rs[2], rd, t['render_depth_G'], rdN)
    sum(ls).backward()
    grads = dict(depth=depth.grad, semantic=sem.grad, render=rs[0].grad, render_G=rs[1].grad, render_N=rs[2].grad,
                 render_depth=rd.grad, render_depth_N=rdN.grad)
    return [v.detach() for v in ls], grads, (gd, gs)


def _close_losses(got, want, tol=1e-5):
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = float(a), float(b)
        assert abs(a - b) <= tol * abs(b), f'loss {i}: {a} vs {b} (rel {abs(a - b) / abs(b):.2e})'


def _close_grads(got, want, tol=1e-5):
    for k, w in want.items():
        w = w.cpu().numpy() if torch.is_tensor(w) else w
        a = got[k].cpu().numpy()
        err = float(np.abs(a - w).max())
        assert err <= tol * float(np.abs(w).max()), f'd {k}: {err:.3e} vs max |g| {np.abs(w).max():.3e}'


def _same_labels(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(np.nan_to_num(a, nan=-1), np.nan_to_num(b, nan=-1))


def _lidar(B, N, H, W, seed):
    """Sparse synthetic lidar depth (about 4 % of the pixels, some outside [1, 60] and some at 60) with Bernoulli
    semantics."""
    gen = torch.Generator().manual_seed(seed)
    hit = torch.rand(B, N, H, W, generator=gen) < 0.04
    gd = torch.where(hit, torch.rand(B, N, H, W, generator=gen) * 66.0 + 0.3, torch.zeros(()))
    gd[..., ::97, ::89] = 60.0
    gs = (hit & (torch.rand(B, N, H, W, generator=gen) < 0.3)).float()
    return gd, gs


def test_depth_labels_bit_for_bit(golden, cuda):
    g = golden('losses.npz')
    cfg, D, ds = g['depth_cfg'], int(g['D']), int(g['ds'])
    gd, gs = torch.from_numpy(g['gt_depth']), torch.from_numpy(g['gt_semantic'])
    dl, sl = losses.depth_labels(gd.to(cuda), gs.to(cuda), cfg, D, ds)
    _same_labels(dl, torch.from_numpy(g['depth_labels']))
    assert torch.equal(sl.cpu(), torch.from_numpy(g['semantic_labels']))
    # cfg2 full size: B = 2, 6 x 256 x 704
    gd, gs = _lidar(2, 6, 256, 704, seed=1)
    want = losses.depth_labels_torch(gd, gs, cfg, D, ds)
    got = losses.depth_labels(gd.to(cuda), gs.to(cuda), cfg, D, ds)
    _same_labels(got[0], want[0])
    assert torch.equal(got[1].cpu(), want[1])
    assert (want[1][:, 1] > 0).any() and (want[1][:, 1] == 0).any()


@pytest.mark.parametrize('tag', ['nomask', 'mask'])
def test_get_loss_matches_reference_fixture(golden, cuda, tag):
    g = golden('losses.npz')
    m = _module(g, cuda)
    ls, grads, _ = _run(m, g, tag, cuda)
    _close_losses(ls, g[f'losses_{tag}'])
    _close_grads(grads, _want_grads(g, tag))
    # and against the torch formulation on the GPU
    m2 = _module(g, cuda)
    m2.fused_losses = False
    ls2, grads2, _ = _run(m2, g, tag, cuda)
    _close_losses(ls, ls2)
    _close_grads(grads, grads2)


def test_full_size_against_the_torch_formulation(cuda):
    """cfg2 size: B = 2, 6 cameras 256 x 704, D = 118, 30 random boxes per camera, box mask on."""
    from ocrfdet_amd import view_transformer_ocrf as vto
    B, N, H, W, D = 2, 6, 256, 704, 118
    gen = torch.Generator().manual_seed(5)
    gd, gs = _lidar(B, N, H, W, seed=2)
    x1 = torch.rand(B, N, 30, generator=gen) * 1700 - 100
    y1 = torch.rand(B, N, 30, generator=gen) * 800 + 200
    boxes = torch.stack((x1, y1, x1 + torch.rand(B, N, 30, generator=gen) * 400,
                         y1 + torch.rand(B, N, 30, generator=gen) * 300), -1)
    grid = dict(x=[-40.0, 40.0, 0.4], y=[-40.0, 40.0, 0.4], z=[-5.0, 3.0, 8.0], depth=[1.0, 60.0, 0.5])
    m = vto.OcRFViewTransformerFull(pc_range=[-40.0, -40.0, -5.0, 40.0, 40.0, 3.0], bev_h=16, bev_w=16, grid_config=grid,
                                    input_size=(H, W), downsample=16, in_channels=16, out_channels=16,
                                    depth_net=torch.nn.Identity()).to(cuda)
    inp = dict(depth=torch.randn(B * N, D, H // 16, W // 16, generator=gen).softmax(1),
               sem=torch.randn(B * N, 2, H // 16, W // 16, generator=gen).softmax(1),
               gt=torch.rand(B, 3, H, W, generator=gen))
    for k in ('r', 'G', 'N'):
        inp[k] = (inp['gt'] + 0.1 * torch.randn(B, 3, H, W, generator=gen)).clamp(0, 1)
    for k in ('rd', 'rdG', 'rdN'):
        inp[k] = torch.rand(B, 1, H, W, generator=gen)

    def run(fused):
        m.fused_losses, m.loss_iteration = fused, 10 ** 4
        v = {k: t.to(cuda).requires_grad_(k not in ('gt', 'rdG')) for k, t in inp.items()}
        ls = m.get_loss(v['depth'], v['sem'], gd.to(cuda), gs.to(cuda), boxes, [3, 0], v['r'], v['gt'], v['G'], v['N'],
                        v['rd'], v['rdG'], v['rdN'])
        sum(ls).backward()
        return [t.detach() for t in ls], {k: v[k].grad for k in ('depth', 'sem', 'r', 'G', 'N', 'rd', 'rdN')}
    got, want = run(True), run(False)
    _close_losses(got[0], want[0])
    _close_grads(got[1], want[1])


def test_two_runs_bit_identical(golden, cuda):
    g = golden('losses.npz')
    m = _module(g, cuda)
    a = _run(m, g, 'mask', cuda)
    b = _run(m, g, 'mask', cuda)
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


def test_no_host_synchronisation_and_inputs_untouched(golden, cuda):
    g = golden('losses.npz')
    m = _module(g, cuda)
    t = _inputs(g, cuda)
    t['device_boxes'] = _boxes(g, cuda)
    want = _run(m, g, 'mask', cuda, device_boxes=True, t=t)          # warm-up: library, workspaces, pinned pool
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = _run(m, g, 'mask', cuda, device_boxes=True, t=t)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    _close_losses(got[0], g['losses_mask'])
    for x, y in zip(got[0], want[0]):
        assert torch.equal(x, y)
    gd, gs = got[2]
    assert torch.equal(gd.cpu(), torch.from_numpy(g['gt_depth']))
    assert torch.equal(gs.cpu(), torch.from_numpy(g['gt_semantic']))


def test_ssim_module_fused(cuda):
    torch.manual_seed(0)
    a = torch.rand(2, 3, 70, 90, device=cuda)
    b = (a + 0.1 * torch.randn_like(a)).clamp(0, 1).requires_grad_(True)
    b2 = b.detach().clone().requires_grad_(True)
    s = losses.SSIM(window_size=11)(a, b)
    s2 = losses.ssim_torch(a, b2)
    assert abs(float(s) - float(s2)) <= 1e-5 * abs(float(s2))
    s.backward()
    s2.backward()
    assert float((b.grad - b2.grad).abs().max()) <= 1e-5 * float(b2.grad.abs().max())


def test_module_training_step_fused_against_torch(cuda):
    """The module in training mode at the core fixture's size: view_transform_core, get_loss and both ProbNet losses,
    backward; parameter gradients with fused_losses True and False agree to 1e-4 (relative, per parameter)."""
    from tests.test_device_geometry_gpu import _setup
    cfg, m, inp, depth0, feat0 = _setup(cuda)
    B, N = 2, cfg.n_cams
    H, W = cfg.input_size
    gd, gs = _lidar(B, N, H, W, seed=3)
    gd, gs = gd.to(cuda), gs.to(cuda)
    sem0 = torch.rand(B * N, 2, H // 16, W // 16, device=cuda).softmax(1)
    boxes = [[torch.tensor([[100.0, 1500.0, 900.0, 1800.0]], device=cuda)] * N for _ in range(B)]
    gt_bev = (torch.rand(B, 48, 48, device=cuda) < 0.3).float()

    def run(mod):
        torch.manual_seed(0)
        depth = depth0.clone().requires_grad_(True)
        bev, _, logit, lst = mod.view_transform_core(inp, depth, feat0, cam_idx_list=[1, 4])
        ls = mod.get_loss(depth, sem0, gd, gs, boxes, lst[5], lst[0], lst[1], lst[2], lst[3], lst[6], lst[7], lst[8])
        a = mod.prob.get_bev_mask_loss(gt_bev, logit)
        o = mod.prob.get_bev_opacity_loss(gt_bev, lst[4].squeeze(1))
        total = sum(ls) + sum(a.values()) + sum(o.values())
        total.backward()
        return total.detach(), {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}

    fused = copy.deepcopy(m).train()
    ref = copy.deepcopy(m).train()
    ref.fused_losses = False
    lf, gf = run(fused)
    lt, gt_ = run(ref)
    assert abs(float(lf) - float(lt)) <= 1e-4 * abs(float(lt))
    assert set(gf) == set(gt_) and len(gf) > 10
    for n in gt_:
        den = float(gt_[n].norm())
        if den > 0:
            assert float((gf[n] - gt_[n]).norm()) <= 1e-4 * den, n


def test_refusals(cuda):
    cfg = [1.0, 60.0, 0.5]
    with pytest.raises(ValueError):
        losses.depth_labels(torch.zeros(1, 2, 30, 32, device=cuda), torch.zeros(1, 2, 30, 32, device=cuda), cfg, 118, 16)
    with pytest.raises(ValueError):
        losses.depth_labels(torch.zeros(1, 2, 32, 32, device=cuda), torch.zeros(1, 2, 32, 16, device=cuda), cfg, 118, 16)
    with pytest.raises(ValueError):
        losses.depth_semantic_loss(torch.zeros(8, 118, device=cuda), torch.rand(2, 118, 2, 2, device=cuda),
                                   torch.zeros(8, 2, device=cuda), torch.rand(2, 2, 2, 3, device=cuda), 3.0, 25.0)
    img = torch.rand(2, 3, 32, 48, device=cuda)
    dep = torch.rand(2, 1, 32, 48, device=cuda)
    gtd = torch.rand(2, 6, 32, 48, device=cuda)
    boxes = [torch.zeros(0, 4)] * 2
    with pytest.raises(ValueError):
        losses.render_losses(img, (img, img, img[:, :, :16]), (dep, dep, dep), gtd, [0, 1], boxes, True, cfg)
    with pytest.raises(ValueError):
        losses.render_losses(img, (img, img, img), (dep, dep, dep[:, :, :16]), gtd, [0, 1], boxes, True, cfg)
    with pytest.raises(ValueError):
        losses.render_losses(img, (img, img, img), (dep, dep, dep), gtd, [0, 6], boxes, True, cfg)
