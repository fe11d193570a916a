"""CPU: the neck's training losses (``get_loss`` and its helpers, the ProbNet losses) in their torch formulation against
the reference's own values (``tests/golden/losses.npz``, ``make_golden_losses.py``), Box2dtoMask's slice rules, the
per-instance iteration counter and the untouched gt tensors."""
import numpy as np
import pytest
import torch

from ocrfdet_amd import losses

CAMS = [1, 4]


def _module(g):
    from ocrfdet_amd import view_transformer_ocrf as vto
    grid = dict(x=[-12.8, 12.8, 1.6], y=[-12.8, 12.8, 1.6], z=[-5.0, 3.0, 8.0], depth=list(g['depth_cfg']))
    return vto.OcRFViewTransformerFull(pc_range=[-12.8, -12.8, -5.0, 12.8, 12.8, 3.0], bev_h=16, bev_w=16, num_height=13,
                                       grid_config=grid, input_size=tuple(g['gt_depth'].shape[-2:]),
                                       downsample=int(g['ds']), in_channels=16, out_channels=16,
                                       depth_net=torch.nn.Identity())


def _boxes(g):
    B, N = g['box_counts'].shape
    return [[torch.from_numpy(g['boxes'][b, n, :g['box_counts'][b, n]]) for n in range(N)] for b in range(B)]


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


def _run(m, g, tag):
    t = _decode(g)
    m.loss_iteration = 3862 * 2 - 1 if tag == 'nomask' else 3862 * 2
    depth = t['depth_logits'].softmax(1).requires_grad_(True)
    sem = t['sem_logits'].softmax(1).requires_grad_(True)
    rs = [t[k].clone().requires_grad_(True) for k in ('render', 'render_G', 'render_N')]
    rd, rdN = t['render_depth'].clone().requires_grad_(True), t['render_depth_N'].clone().requires_grad_(True)
    gd, gs = t['gt_depth'].clone(), t['gt_semantic'].clone()
    ls = m.get_loss(depth, sem, gd, gs, _boxes(g), CAMS, rs[0], t['gt_images'], rs[1], rs[2], rd, t['render_depth_G'],
                    rdN)
    sum(ls).backward()
    grads = dict(depth=depth.grad, semantic=sem.grad, render=rs[0].grad, render_G=rs[1].grad, render_N=rs[2].grad,
                 render_depth=rd.grad, render_depth_N=rdN.grad)
    return ls, grads, (gd, gs)


@pytest.mark.parametrize('tag', ['nomask', 'mask'])
def test_get_loss_matches_reference_fixture(golden, tag):
    g = golden('losses.npz')
    m = _module(g)
    ls, grads, _ = _run(m, g, tag)
    want = g[f'losses_{tag}']
    assert len(ls) == 5
    for i, (a, b) in enumerate(zip(ls, want)):
        assert abs(float(a) - b) <= 1e-6 * abs(b), f'loss {i}: {float(a)} vs {b}'
    want_g = _want_grads(g, tag)
    assert len(want_g) == (7 if tag == 'mask' else 5)
    for k, w in want_g.items():
        v = grads[k]
        err = float(np.abs(v.numpy() - w).max())
        assert err <= 1e-6 * float(np.abs(w).max()), f'd {k}: {err} (max |g| {np.abs(w).max()})'


def test_labels_match_reference_bit_for_bit(golden):
    g = golden('losses.npz')
    m = _module(g)
    gd, gs = torch.from_numpy(g['gt_depth']), torch.from_numpy(g['gt_semantic'])
    dl, sl = m.get_downsampled_gt_depth_and_semantic(gd, gs)
    want = g['depth_labels']
    assert np.array_equal(np.isnan(dl.numpy()), np.isnan(want))
    assert np.isnan(want).any(), 'the fixture must hold a NaN row (semantic pixels only at d1)'
    assert np.array_equal(np.nan_to_num(dl.numpy(), nan=-1), np.nan_to_num(want, nan=-1))
    assert np.array_equal(sl.numpy(), g['semantic_labels'])
    # the fixture covers both label kinds and the range edges
    assert (g['semantic_labels'][:, 1] > 0).any() and (g['semantic_labels'][:, 1] == 0).any()
    assert (g['gt_depth'] == 60.0).any() and (g['gt_depth'] > 60.0).any() and ((g['gt_depth'] > 0) & (g['gt_depth'] < 1)).any()


def test_inputs_are_not_modified(golden):
    g = golden('losses.npz')
    m = _module(g)
    _, _, (gd, gs) = _run(m, g, 'mask')
    assert torch.equal(gd, torch.from_numpy(g['gt_depth']))
    assert torch.equal(gs, torch.from_numpy(g['gt_semantic']))


def test_box_mask_matches_reference_fixture(golden):
    g = golden('losses.npz')
    m = _module(g)
    H, W = g['gt_images'].shape[2:]
    for b, cam in enumerate(CAMS):
        got = m.Box2dtoMask(_boxes(g)[b][cam], W, H)
        assert got.shape == (1, 3, H, W)
        assert np.array_equal(got.numpy(), g[f'box_mask_{b}'])
    assert not g['box_mask_1'].any(), 'zero boxes give an all-zero mask'


def _slice_mask(boxes, W, H):
    """Box2dtoMask's loop restated with Python slices on a numpy array."""
    scale = np.float32(W / 1600)
    out = np.zeros((H, W), np.float32)
    for x1, y1, x2, y2 in boxes:
        x1, x2 = int(np.float32(x1) * scale), int(np.float32(x2) * scale)
        y1, y2 = int(np.float32(y1) * scale) - 158, int(np.float32(y2) * scale) - 158
        out[y1:y2, x1:x2] = 1.0
    return out


@pytest.mark.parametrize('box', [
    [100.0, 1500.0, 600.0, 1800.0],       # inside
    [1200.0, 1450.0, 2400.0, 1700.0],     # past W
    [0.0, 0.0, 300.0, 1600.0],            # negative start: y1 + H clamped to 0
    [300.0, 1255.0, 800.0, 1710.0],       # negative start after the shift, start >= stop: empty
    [50.0, 1255.0, 200.0, 1300.0],        # both negative: wrap around
    [-200.0, 1500.0, 100.0, 1600.0],      # x1 negative: wraps past x2, empty
    [400.0, 1600.0, 399.0, 1700.0],       # x1 > x2: empty
    [-20000.0, -9000.0, 20000.0, 9000.0], # everything clamped
])
def test_box2dtomask_slice_rules(box):
    for W, H in ((176, 64), (704, 256)):
        got = losses.box_mask(torch.tensor([box]), W, H)
        assert np.array_equal(got.numpy(), _slice_mask([box], W, H)), (box, W, H)
    # the issue's worked example at 704 x 256: y1 = -108, y2 = 42 after the shift selects nothing
    scale = 704 / 1600
    y1, y2 = (158 - 108 + 0.5) / scale, (158 + 42 + 0.5) / scale
    assert not losses.box_mask(torch.tensor([[0.0, y1, 1600.0, y2]]), 704, 256).any()


def test_zero_boxes_give_an_empty_mask():
    assert not losses.box_mask(torch.zeros(0, 4), 176, 64).any()


def test_iteration_counter_switches_the_mask_on(golden):
    g = golden('losses.npz')
    m = _module(g)
    assert m.loss_iteration == 0 and 'loss_iteration' not in m.state_dict()
    ls, _, _ = _run(m, g, 'nomask')
    assert m.loss_iteration == 3862 * 2
    assert abs(float(ls[2]) - g['losses_nomask'][2]) <= 1e-6 * g['losses_nomask'][2]
    ls, _, _ = _run(m, g, 'mask')
    assert m.loss_iteration == 3862 * 2 + 1
    assert abs(float(ls[2]) - g['losses_mask'][2]) <= 1e-6 * g['losses_mask'][2]
    assert g['losses_mask'][2] < 0.5 * g['losses_nomask'][2]
    other = _module(g)
    assert other.loss_iteration == 0, 'the counter is per instance'


def test_probnet_losses_match_reference_fixture(golden):
    g = golden('losses.npz')
    m = _module(g)
    t = _decode(g)
    bev, opa, gt = t['bev_logits'].requires_grad_(True), t['opa_logits'].requires_grad_(True), t['gt_bev']
    a = m.prob.get_bev_mask_loss(gt, bev)
    b = m.prob.get_bev_opacity_loss(gt, opa.squeeze(1))
    assert set(a) == {'mask_ce_loss', 'mask_dice_loss'}
    assert set(b) == {'mask_ce_opacity_loss', 'mask_dice_opacity_loss'}
    for k, v in list(a.items()) + list(b.items()):
        w = float(g[f'prob_{k}'])
        assert abs(float(v) - w) <= 1e-6 * abs(w), (k, float(v), w)
    (sum(a.values()) + sum(b.values())).backward()
    for got, k in ((bev.grad, 'grad_bev_logits'), (opa.grad, 'grad_opa_logits')):
        w = g[k]
        assert float(np.abs(got.numpy() - w).max()) <= 1e-6 * float(np.abs(w).max())
    assert m.prob.ce_loss.reduction == 'mean', 'the module state is left alone'


def test_ssim_module_matches_the_torch_formulation():
    torch.manual_seed(0)
    a, b = torch.rand(2, 3, 40, 50), torch.rand(2, 3, 40, 50)
    s = losses.SSIM(window_size=11)
    assert torch.equal(s(a, b), losses.ssim(a, b))
    assert losses.ssim(a, a).item() == pytest.approx(1.0, abs=1e-5)
    per_image = losses.ssim(a, b, size_average=False)
    assert per_image.shape == (2,)


def test_label_refusals():
    gd = torch.zeros(1, 2, 30, 32)
    with pytest.raises(ValueError):
        losses.depth_labels_torch(gd, gd, [1.0, 60.0, 0.5], 118, 16)
    with pytest.raises(ValueError):
        losses.depth_labels_torch(torch.zeros(1, 2, 32, 32), torch.zeros(1, 2, 32, 16), [1.0, 60.0, 0.5], 118, 16)
