"""GPU: the rasteriser's backward for the mean depth and final_T (``ocrf_rasterize_backward_depth``) through every
surface that offers it, against the composition tests/raster_depth_oracle.py makes of the C oracle's colour backward
(tests/test_raster_depth_grad_host.py pins that composition to autograd of a float64 restatement).

Metric and bars are those of tests/test_rasterize_backward_gpu.py for the same scenes: max error over the gradient's
scale, 1e-4 for the two small scenes, 2e-3 for random scenes (where single pixels may decide a threshold the other
way)."""
import copy

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib
from ocrfdet_amd import diff_gaussian_rasterization as dgr
from tests import helpers
from tests import raster_depth_oracle as rdo
from tests.test_neck_gpu import core  # noqa: F401  (the small neck configuration, as a fixture of this module too)
from tests.test_rasterize_backward_gpu import _check, _cov3d_of, _settings, _t, _two_view_scene

pytestmark = pytest.mark.gpu

_WANT = {}


def _want(oracle_lib, key, scene, views, grads, scale_modifier=1.0):
    """The composed oracle for ``grads`` = per view (gcol, gD, gT), summed over the views; computed once per ``key``."""
    if key not in _WANT:
        per_view = [rdo.expected_for(oracle_lib, scene, gD=gD, gT=gT, gcol=gcol, view=v, scale_modifier=scale_modifier)
                    for v, (gcol, gD, gT) in zip(views, grads)]
        _WANT[key] = {k: sum(w[k] for w in per_view) for k in per_view[0]}
    return _WANT[key]


def _functional(cuda, q, gcol, gD, gT):
    """rasterize_views (mean depth) + rasterize_views_backward on a one-view scene -> the dict of gradients."""
    a = [_t(q[k], cuda) for k in ('xyz', 'rgb', 'opac', 'sc', 'rot')]
    cam = (_t(q['view'], cuda).view(1, 4, 4), _t(q['full'], cuda).view(1, 4, 4), [q['tfx']], [q['tfy']], q['H'], q['W'],
           _t(q['bg'], cuda))
    fwd = dgr.rasterize_views(*a, *cam, depth_mode='mean')
    g = dgr.rasterize_views_backward(_t(gcol, cuda)[None] if gcol is not None else torch.zeros_like(fwd['color']), fwd, *a,
                                     *cam, want_means2D=True, grad_depth=None if gD is None else _t(gD, cuda)[None],
                                     grad_final_T=None if gT is None else _t(gT, cuda)[None])
    torch.cuda.synchronize()
    return {k: (v[0] if k == 'means2D' else v).cpu().numpy() for k, v in g.items()}


@pytest.mark.parametrize('which', ['depth', 'final_T', 'all'])
def test_single_gaussian_all_six_leaves(cuda, oracle_lib, which):
    q = rdo.single_gaussian_scene()
    gcol, gD, gT = rdo.image_gradients(q, 1)
    gcol, gD, gT = {'depth': (None, gD, None), 'final_T': (None, None, gT), 'all': (gcol, gD, gT)}[which]
    want = _want(oracle_lib, ('single', which), q, [0], [(gcol, gD, gT)])
    got = _functional(cuda, q, gcol, gD, gT)
    for name in rdo.LEAVES:
        _check(got[name], want[name], name, 1e-4)


def test_twelve_overlapping_gaussians(cuda, oracle_lib):
    q = rdo.twelve_gaussian_scene()
    grads = rdo.image_gradients(q, 2)
    want = _want(oracle_lib, 'twelve', q, [0], [grads])
    got = _functional(cuda, q, *grads)
    for name in rdo.LEAVES:
        _check(got[name], want[name], name, 1e-4)


def test_reference_shaped_surface_returns_a_differentiable_mean_depth(cuda, oracle_lib):
    """GaussianRasterizer(depth_mode='mean', depth_grad=True): colour + depth loss, means2D through autograd."""
    q = rdo.twelve_gaussian_scene()
    gcol, gD, _ = rdo.image_gradients(q, 2)
    want = _want(oracle_lib, 'twelve-rasterizer', q, [0], [(gcol, gD, None)])
    s = _settings(cuda, q['view'], q['full'], q['tfx'], q['tfy'], q['H'], q['W'], q['bg'])
    m3, m2 = _t(q['xyz'], cuda, True), torch.zeros(12, 3, device=cuda, requires_grad=True)
    c, o, sc, r = (_t(q[k], cuda, True) for k in ('rgb', 'opac', 'sc', 'rot'))
    color, _, depth = dgr.GaussianRasterizer(s, depth_mode='mean', depth_grad=True)(m3, m2, o, colors_precomp=c, scales=sc,
                                                                                     rotations=r)
    ((color * _t(gcol, cuda)).sum() + (depth[0] * _t(gD, cuda)).sum()).backward()
    torch.cuda.synchronize()
    for name, leaf in zip(rdo.LEAVES, (m3, m2, c, o, sc, r)):
        _check(leaf.grad.cpu().numpy(), want[name], name, 1e-4)


def _leaves(q, cuda, scales=None):
    return dict(means3D=_t(q['xyz'], cuda, True), colors=_t(q['rgb'], cuda, True), opacities=_t(q['opac'], cuda, True),
                scales=_t(q['sc'] if scales is None else scales, cuda, True), rotations=_t(q['rot'], cuda, True))


def _render_two_views(q, cuda, surface, leaves, scale_modifier=1.0, **kw):
    vms = torch.stack([_t(v, cuda) for v in q['views']])
    pms = torch.stack([_t(f, cuda) for f in q['fulls']])
    tfx, tfy, H, W = [q['tfx']] * 2, [q['tfy']] * 2, q['H'], q['W']
    if surface == 'packed':
        return dgr.rasterize_packed_autograd(*leaves.values(), dgr.pack_cameras(vms, pms, tfx, tfy, H, W, cuda), H, W,
                                             _t(q['bg'], cuda), **kw)
    return dgr.rasterize_views_autograd(*leaves.values(), vms, pms, tfx, tfy, H, W, _t(q['bg'], cuda), scale_modifier, **kw)


def _two_view_grads(q, seed):
    """Per view (gcol, gD, gT): the scene's own colour gradient and seeded depth / final_T gradients."""
    rng = np.random.default_rng(seed)
    return [(q['gcol'][v], rng.standard_normal((q['H'], q['W'])).astype(np.float32),
             rng.standard_normal((q['H'], q['W'])).astype(np.float32)) for v in range(2)]


def _check_two_views(q, cuda, oracle_lib, key, surface, scale_modifier=1.0, tol=2e-3):
    grads = _two_view_grads(q, 31)
    want = _want(oracle_lib, key, q, [0, 1], grads, scale_modifier)
    leaves = _leaves(q, cuda)
    color, depth, final_T, _ = _render_two_views(q, cuda, surface, leaves, scale_modifier, depth_mode='mean', depth_grad=True)
    gcol, gD, gT = (_t(np.stack([g[i] for g in grads]), cuda) for i in range(3))
    ((color * gcol).sum() + (depth[:, 0] * gD).sum() + (final_T * gT).sum()).backward()
    torch.cuda.synchronize()
    for name, leaf in leaves.items():
        _check(leaf.grad.cpu().numpy(), want[name], name, tol)


@pytest.mark.parametrize('surface', ['views', 'packed'])
def test_two_views_one_backward_is_the_sum_of_the_per_view_oracles(cuda, oracle_lib, surface):
    _check_two_views(_two_view_scene(oracle_lib), cuda, oracle_lib, 'two-view', surface)


def test_scale_modifier(cuda, oracle_lib):
    _check_two_views(_two_view_scene(oracle_lib, scale_modifier=0.75), cuda, oracle_lib, 'two-view-0.75', 'views', 0.75)


@pytest.mark.parametrize('n,W,H,seed', [(2100, 72, 40, 21), (5000, 176, 64, 1)])
def test_several_chunks_several_staged_batches_early_stops(cuda, oracle_lib, n, W, H, seed):
    """n = 2100 at 72 x 40: more than one preprocess chunk (1024) and scatter chunk (2048), no multiple of the 16 x 16 tile
    either way, a last tile pair without a second tile.  Both scenes walk more than one staged batch of 256 records per
    tile and have pixels that stop early (final_T at the 1e-4 floor): asserted from the oracle's forward."""
    q = _two_view_scene(oracle_lib, n=n, W=W, H=H, seed=seed)
    fwd = [oracle_lib.rasterize_forward(q['xyz'], q['rgb'], q['opac'], q['sc'], q['rot'], q['views'][v], q['fulls'][v],
                                        q['tfx'], q['tfy'], H, W, q['bg'], depth_mode='mean') for v in range(2)]
    assert max(int(f['n_contrib'].max()) for f in fwd) > 256
    assert min(float(f['final_T'].min()) for f in fwd) < 2e-4
    _check_two_views(q, cuda, oracle_lib, ('chunks', n), 'views')


def test_cov3d_precomp(cuda, oracle_lib):
    q = dict(rdo.twelve_gaussian_scene())
    q['rot'] = (q['rot'] / np.linalg.norm(q['rot'], axis=1, keepdims=True)).astype(np.float32)
    gcol, gD, _ = rdo.image_gradients(q, 4)
    want = _want(oracle_lib, 'twelve-cov', q, [0], [(gcol, gD, None)])
    s = _settings(cuda, q['view'], q['full'], q['tfx'], q['tfy'], q['H'], q['W'], q['bg'])
    m3, m2 = _t(q['xyz'], cuda, True), torch.zeros(12, 3, device=cuda, requires_grad=True)
    c, o, cov = _t(q['rgb'], cuda, True), _t(q['opac'], cuda, True), _t(_cov3d_of(q['sc'], q['rot']), cuda, True)
    color, _, depth = dgr.GaussianRasterizer(s, depth_mode='mean', depth_grad=True)(m3, m2, o, colors_precomp=c,
                                                                                     cov3D_precomp=cov)
    ((color * _t(gcol, cuda)).sum() + (depth[0] * _t(gD, cuda)).sum()).backward()
    torch.cuda.synchronize()
    for name, leaf in (('means3D', m3), ('means2D', m2), ('colors', c), ('opacities', o), ('cov3D', cov)):
        _check(leaf.grad.cpu().numpy(), want[name], name, 1e-4)


def test_empty_view_gives_exact_zeros(cuda):
    W, H = 32, 32
    view, full, tfx, tfy = helpers.simple_camera(W, H)
    leaves = [_t(np.float32(a), cuda, True) for a in ([[0, 0, -5.0], [100.0, 0, 5.0]], [[1, 1, 1], [1, 1, 1]], [[0.5], [0.5]],
                                                       [[0.1] * 3] * 2, [[1, 0, 0, 0]] * 2)]
    color, depth, final_T, _ = dgr.rasterize_views_autograd(*leaves, _t(view, cuda).view(1, 4, 4), _t(full, cuda).view(1, 4, 4),
                                                            [tfx], [tfy], H, W, torch.zeros(3, device=cuda),
                                                            depth_mode='mean', depth_grad=True)
    assert float(depth.detach().abs().max()) == 0.0 and float(final_T.detach().min()) == 1.0
    (color.sum() + (3.0 * depth).sum() + (2.0 * final_T).sum()).backward()
    for leaf in leaves:
        assert float(leaf.grad.abs().max()) == 0.0


def test_depth_grad_needs_the_mean_depth(cuda, oracle_lib):
    q = _two_view_scene(oracle_lib)
    for surface in ('views', 'packed'):
        with pytest.raises(ValueError, match="depth_mode='mean'"):
            _render_two_views(q, cuda, surface, _leaves(q, cuda), depth_grad=True)
    with pytest.raises(ValueError, match="depth_mode='mean'"):
        dgr.GaussianRasterizer(_settings(cuda, q['views'][0], q['fulls'][0], q['tfx'], q['tfy'], q['H'], q['W'], q['bg']),
                               depth_grad=True)
    # without depth_grad nothing changed: depth and final_T carry no graph
    _, depth, final_T, _ = _render_two_views(q, cuda, 'views', _leaves(q, cuda), depth_mode='mean')
    assert not depth.requires_grad and not final_T.requires_grad


@pytest.mark.parametrize('surface', ['views', 'packed'])
def test_in_place_edit_of_the_rendered_depth_raises(cuda, oracle_lib, surface):
    """The backward needs D - prefix_D from the saved forward depth: an edit of it must not silently change gradients."""
    q = _two_view_scene(oracle_lib)
    _, depth, _, _ = _render_two_views(q, cuda, surface, _leaves(q, cuda), depth_mode='mean', depth_grad=True)
    depth.clamp_(0, 10)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        depth.sum().backward()


def test_a_loss_on_the_colour_alone_launches_the_colour_only_backward(cuda, oracle_lib, monkeypatch):
    q = _two_view_scene(oracle_lib)
    names = []
    real = _lib.launch
    monkeypatch.setattr(_lib, 'launch', lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    leaves = _leaves(q, cuda)
    color, depth, final_T, _ = _render_two_views(q, cuda, 'views', leaves, depth_mode='mean', depth_grad=True)
    assert depth.requires_grad and final_T.requires_grad
    (color * _t(q['gcol'], cuda)).sum().backward()
    assert 'ocrf_rasterize_backward' in names and 'ocrf_rasterize_backward_depth' not in names
    # ... and it is the colour backward: the oracle's sum over the views
    for name, leaf in leaves.items():
        _check(leaf.grad.cpu().numpy(), q['want'][name], name, 2e-3)
    del names[:]
    leaves = _leaves(q, cuda)
    _, depth, _, _ = _render_two_views(q, cuda, 'views', leaves, depth_mode='mean', depth_grad=True)
    depth.sum().backward()                      # no colour gradient at all: zeros for it, the new entry
    assert 'ocrf_rasterize_backward_depth' in names and 'ocrf_rasterize_backward' not in names
    assert float(leaves['colors'].grad.abs().max()) == 0.0 and float(leaves['means3D'].grad.abs().max()) > 0.0


LINEARITY_TOL = 1e-5


def test_new_entry_agrees_with_the_colour_backward_of_the_depth_colours(cuda, oracle_lib):
    """Linearity on the GPU itself: backward(gD, gT) through the new entry against the existing colour backward of a render
    with colours (z_i, 1, 0) over a zero background for the image gradient (gD, -gT, 0), plus view[:3, 2] * dL/dz.  The
    two differ only by the order of float atomics.  Bar: the larger of 1e-5 of the gradient's scale and twice the spread
    of two reruns of the OLD path.  Measured on an MI355X: the reruns lie 9.7e-7 apart at most over the four
    leaves (scales), the new entry 9.0e-7 from them at most (rotations): so 1e-5."""
    q = _two_view_scene(oracle_lib)
    H, W = q['H'], q['W']
    for v in q['views']:
        assert np.array_equal(np.float32(v).reshape(4, 4)[:3, 2], np.float32([0, 0, 1]))      # z_i = mean_z + const, both views
    rng = np.random.default_rng(41)
    gD, gT = (_t(rng.standard_normal((2, H, W)).astype(np.float32), cuda) for _ in range(2))
    leaves = _leaves(q, cuda)
    _, depth, final_T, _ = _render_two_views(q, cuda, 'views', leaves, depth_mode='mean', depth_grad=True)
    ((depth[:, 0] * gD).sum() + (final_T * gT).sum()).backward()

    def old_path():
        # one view at a time: z_i is a per-view colour
        total = None
        for v in range(2):
            z = q['xyz'] @ np.float32(q['views'][v]).reshape(4, 4)[:3, 2] + np.float32(q['views'][v]).reshape(4, 4)[3, 2]
            lv = _leaves(q, cuda)
            lv['colors'] = _t(np.stack([z, np.ones_like(z), np.zeros_like(z)], 1).astype(np.float32), cuda, True)
            color, _, _, _ = dgr.rasterize_views_autograd(
                *lv.values(), _t(q['views'][v], cuda).view(1, 4, 4), _t(q['fulls'][v], cuda).view(1, 4, 4), [q['tfx']],
                [q['tfy']], H, W, torch.zeros(3, device=cuda))
            (color[0, 0] * gD[v] - color[0, 1] * gT[v]).sum().backward()
            g = {k: t.grad.clone() for k, t in lv.items()}
            g['means3D'][:, 2] += g['colors'][:, 0]
            total = g if total is None else {k: total[k] + g[k] for k in g}
        return total
    a, b = old_path(), old_path()
    for name in ('means3D', 'opacities', 'scales', 'rotations'):
        scale = float(a[name].abs().max())
        spread = float((a[name] - b[name]).abs().max()) / scale
        err = float((leaves[name].grad - a[name]).abs().max()) / scale
        print(f'linearity {name}: new vs old {err:.3e}, spread of two reruns of the old path {spread:.3e} (of {scale:.3e})')
        assert spread <= 0.5 * LINEARITY_TOL, f'{name}: the old path reruns {spread:.3e} apart'
        assert err <= LINEARITY_TOL, f'{name}: {err:.3e} of the gradient scale {scale:.3e}'


def _neck_render_depth_grads(core, depth_grad, fused_losses):  # noqa: F811
    """loss_render_depth.backward() on a copy of the small neck -> (rendered-depth gradient or None, head gradients)."""
    from tests.test_losses_gpu import _lidar
    m = copy.deepcopy(core['m'])
    m.training = True                                   # top level only: BatchNorm and dropout stay in eval mode
    m.render_depth_grad, m.fused_losses = depth_grad, fused_losses
    cfg, g, B = core['cfg'], core['g'], core['B']
    H, W = cfg.input_size
    pre = torch.from_numpy(g['pre']).cuda()
    depth, feat = pre[:, :cfg.D].softmax(1), pre[:, cfg.D + 2:].clone()
    sem = pre[:, cfg.D:cfg.D + 2].softmax(1)
    gd, gs = (t.cuda() for t in _lidar(B, cfg.n_cams, H, W, seed=3))
    boxes = [[torch.tensor([[100.0, 1500.0, 900.0, 1800.0]]).cuda()] * cfg.n_cams for _ in range(B)]
    cams = [int(c) for c in g['cam_idx_list']]
    _, _, _, lst = m.view_transform_core(core['inp'], depth, feat, cam_idx_list=cams)
    if lst[7].requires_grad:
        lst[7].retain_grad()
    ls = m.get_loss(depth, sem, gd, gs, boxes, lst[5], lst[0], lst[1], lst[2], lst[3], lst[6], lst[7], lst[8])
    ls[4].backward()
    torch.cuda.synchronize()
    heads = {n: getattr(m, n).fc1.weight.grad for n in ('A_MLP', 'S_MLP', 'R_MLP')}
    return lst[7].grad, heads


def test_neck_render_depth_loss_reaches_the_gaussians(core):  # noqa: F811
    """``render_depth_grad = True``: loss_render_depth gives the opacity, scale and rotation heads a gradient through the
    rasteriser; the fused loss kernels and ``fused_losses = False`` agree within 1e-5 (the bar of tests/test_losses_gpu.py:
    of the gradient's largest entry); with the attribute off those heads get nothing from that loss, as before."""
    rd_fused, fused = _neck_render_depth_grads(core, True, True)
    rd_torch, ref = _neck_render_depth_grads(core, True, False)
    assert rd_fused is not None and float(rd_fused.abs().max()) > 0
    assert float((rd_fused - rd_torch).abs().max()) <= 1e-5 * float(rd_torch.abs().max())
    for name in ('A_MLP', 'S_MLP', 'R_MLP'):
        assert fused[name] is not None and torch.isfinite(fused[name]).all() and float(fused[name].abs().max()) > 0, name
        err, scale = float((fused[name] - ref[name]).abs().max()), float(ref[name].abs().max())
        print(f'neck {name}: fused vs torch losses {err / scale:.3e} of {scale:.3e}')
        assert err <= 1e-5 * scale, f'{name}: {err / scale:.3e}'
    rd_off, off = _neck_render_depth_grads(core, False, True)
    assert rd_off is None
    for name, gr in off.items():
        assert gr is None or float(gr.abs().max()) == 0.0, name
