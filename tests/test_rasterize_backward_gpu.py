"""GPU parity: HIP rasteriser backward (C ABI ocrf_rasterize_backward through the reference-shaped
autograd surface) vs the C oracle's restatement of cuda_rasterizer/backward.cu.

Bar: float gradients within 1e-4 relative to the gradient scale of each output (north_star's float
tolerance; the reference itself is not bit-reproducible here — float atomics, backward.cu:509-541).
A pixel whose alpha sits within an ulp of a threshold can take a different branch than the oracle
(see test_rasterize_gpu.py); the scenes are sized so that such flips stay below the bar, and the
few-Gaussian cases below have none."""
import numpy as np
import pytest
import torch

from ocrfdet_amd import diff_gaussian_rasterization as dgr
from tests import helpers

pytestmark = pytest.mark.gpu


def _t(a, cuda, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda).requires_grad_(grad)


def _check(got, want, name, tol=1e-4):
    scale = max(float(np.abs(want).max()), 1e-6)
    err = float(np.abs(got - want).max()) / scale
    assert err <= tol, f'{name}: max err {err:.3e} of the gradient scale {scale:.3e}'


def _settings(cuda, view, full, tfx, tfy, H, W, bg, scale_modifier=1.0):
    return dgr.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=tfx, tanfovy=tfy, bg=_t(np.float32(bg), cuda),
        scale_modifier=scale_modifier, viewmatrix=_t(view, cuda), projmatrix=_t(full, cuda), sh_degree=0,
        campos=torch.zeros(3, device=cuda), prefiltered=False)


def _run(oracle_lib, cuda, xyz, rgb, opac, sc, rot, view, full, tfx, tfy, H, W, bg, seed=0, tol=1e-4,
         scale_modifier=1.0):
    rng = np.random.default_rng(seed)
    gcol = rng.standard_normal((3, H, W)).astype(np.float32)
    want = oracle_lib.rasterize_backward(gcol, xyz, rgb, opac, sc, rot, view, full, tfx, tfy, H, W, np.float32(bg),
                                         scale_modifier=scale_modifier)
    settings = _settings(cuda, view, full, tfx, tfy, H, W, bg, scale_modifier)
    m3, m2 = _t(xyz, cuda, True), torch.zeros(xyz.shape[0], 3, device=cuda, requires_grad=True)
    c, o, s, r = _t(rgb, cuda, True), _t(opac, cuda, True), _t(sc, cuda, True), _t(rot, cuda, True)
    color, radii, depth = dgr.GaussianRasterizer(settings)(m3, m2, o, colors_precomp=c, scales=s, rotations=r)
    (color * _t(gcol, cuda)).sum().backward()
    torch.cuda.synchronize()
    _check(c.grad.cpu().numpy(), want['colors'], 'dL_dcolors', tol)
    _check(o.grad.cpu().numpy(), want['opacities'], 'dL_dopacity', tol)
    _check(m2.grad.cpu().numpy(), want['means2D'], 'dL_dmeans2D', tol)
    _check(m3.grad.cpu().numpy(), want['means3D'], 'dL_dmeans3D', tol)
    _check(s.grad.cpu().numpy(), want['scales'], 'dL_dscales', tol)
    _check(r.grad.cpu().numpy(), want['rotations'], 'dL_drotations', tol)
    return want


def test_single_gaussian_backward(cuda, oracle_lib):
    W, H = 64, 48
    view, full, tfx, tfy = helpers.simple_camera(W, H)
    _run(oracle_lib, cuda, np.float32([[0.3, -0.2, 5.0]]), np.float32([[0.2, 0.5, 0.9]]), np.float32([[0.7]]),
         np.float32([[0.3, 0.2, 0.25]]), np.float32([[0.9, 0.1, -0.3, 0.2]]), view, full, tfx, tfy, H, W,
         (0.1, 0.2, 0.3))


def test_few_overlapping_gaussians_backward(cuda, oracle_lib):
    W, H = 80, 48
    view, full, tfx, tfy = helpers.simple_camera(W, H)
    rng = np.random.default_rng(3)
    n = 12
    xyz = np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.6, 0.6, n), rng.uniform(3, 9, n)], 1).astype(np.float32)
    _run(oracle_lib, cuda, xyz, rng.uniform(0, 1, (n, 3)).astype(np.float32),
         rng.uniform(0.2, 0.9, (n, 1)).astype(np.float32), rng.uniform(0.1, 0.5, (n, 3)).astype(np.float32),
         rng.standard_normal((n, 4)).astype(np.float32), view, full, tfx, tfy, H, W, (0.3, 0.1, 0.6))


@pytest.mark.parametrize('n,seed', [(300, 0), (5000, 1)])
def test_random_scene_backward(cuda, oracle_lib, n, seed):
    rng = np.random.default_rng(seed)
    W, H = 176, 64
    view, full, tfx, tfy = helpers.simple_camera(W, H)
    xyz, rgb, opac, sc, rot = helpers.random_gaussians(rng, n)
    _run(oracle_lib, cuda, xyz, rgb, opac, sc, rot, view, full, tfx, tfy, H, W, (0.2, 0.4, 0.1), seed, tol=2e-3)


_SCENES = {}


def _two_view_scene(oracle_lib, n=400, W=96, H=64, seed=5, scale_modifier=1.0):
    """Random Gaussians under two cameras, an image gradient per view and the oracle's backward summed over the views
    (computed once per scene, shared by the tests below, never written to)."""
    key = (n, W, H, seed, scale_modifier)
    if key not in _SCENES:
        rng = np.random.default_rng(seed)
        view, full, tfx, tfy = helpers.simple_camera(W, H)
        view2, full2, _, _ = helpers.simple_camera(W, H, cam_pos=(-0.4, 0.1, 0.0))
        xyz, rgb, opac, sc, rot = helpers.random_gaussians(rng, n)
        bg = np.float32([0.1, 0.1, 0.1])
        gcol = rng.standard_normal((2, 3, H, W)).astype(np.float32)
        per_view = [oracle_lib.rasterize_backward(gcol[i], xyz, rgb, opac, sc, rot, v, f, tfx, tfy, H, W, bg,
                                                  scale_modifier=scale_modifier)
                    for i, (v, f) in enumerate(((view, full), (view2, full2)))]
        want = {k: per_view[0][k] + per_view[1][k] for k in ('means3D', 'colors', 'opacities', 'scales', 'rotations')}
        _SCENES[key] = dict(xyz=xyz, rgb=rgb, opac=opac, sc=sc, rot=rot, bg=bg, gcol=gcol, views=(view, view2),
                            fulls=(full, full2), tfx=tfx, tfy=tfy, H=H, W=W, want=want)
    return _SCENES[key]


def _render_two_views(scene, cuda, surface, scale_modifier=1.0, scales=None):
    """-> (leaves that require grad, (color, depth, final_T, radii)) of the scene through one batched surface."""
    q = scene
    leaves = dict(means3D=_t(q['xyz'], cuda, True), colors=_t(q['rgb'], cuda, True), opacities=_t(q['opac'], cuda, True),
                  scales=_t(q['sc'] if scales is None else scales, cuda, True), rotations=_t(q['rot'], cuda, True))
    vms = torch.stack([_t(v, cuda) for v in q['views']])
    pms = torch.stack([_t(f, cuda) for f in q['fulls']])
    tfx, tfy, H, W = [q['tfx']] * 2, [q['tfy']] * 2, q['H'], q['W']
    if surface == 'packed':
        assert scale_modifier == 1.0
        out = dgr.rasterize_packed_autograd(*leaves.values(), dgr.pack_cameras(vms, pms, tfx, tfy, H, W, cuda), H, W,
                                            _t(q['bg'], cuda))
    else:
        out = dgr.rasterize_views_autograd(*leaves.values(), vms, pms, tfx, tfy, H, W, _t(q['bg'], cuda), scale_modifier)
    return leaves, out


def _check_two_view_grads(scene, cuda, leaves, color):
    (color * _t(scene['gcol'], cuda)).sum().backward()
    torch.cuda.synchronize()
    for name, leaf in leaves.items():
        _check(leaf.grad.cpu().numpy(), scene['want'][name], name, 2e-3)


@pytest.mark.parametrize('surface', ['views', 'packed'])
def test_multi_view_backward_sums_views(cuda, oracle_lib, surface):
    """rasterize_views_autograd / rasterize_packed_autograd (the rows pack_cameras makes for the same cameras): one
    backward over V cameras == the sum of the per-view oracle backwards."""
    scene = _two_view_scene(oracle_lib)
    leaves, out = _render_two_views(scene, cuda, surface)
    _check_two_view_grads(scene, cuda, leaves, out[0])


def test_packed_and_matrix_surfaces_render_the_same_bits(cuda, oracle_lib):
    """The forward has no atomics: colour, depth, final_T and radii of the two batched surfaces agree bit for bit."""
    scene = _two_view_scene(oracle_lib)
    _, a = _render_two_views(scene, cuda, 'views')
    _, b = _render_two_views(scene, cuda, 'packed')
    for name, x, y in zip(('color', 'depth', 'final_T', 'radii'), a, b):
        assert torch.equal(x, y), name


def test_scale_modifier_batched(cuda, oracle_lib):
    """rasterize_views_autograd with scale_modifier 0.75.  The kernel forms scale_modifier * scale first, as one float
    product, so the images are those of the pre-multiplied scales; the gradients are the oracle's at that modifier
    (the reference's backward applies no chain-rule factor to dL_dscales, backward.cu:346-396, nor does the kernel)."""
    scene = _two_view_scene(oracle_lib, scale_modifier=0.75)
    leaves, out = _render_two_views(scene, cuda, 'views', 0.75)
    with torch.no_grad():
        _, pre = _render_two_views(scene, cuda, 'views', 1.0, scales=scene['sc'] * np.float32(0.75))
    for name, x, y in zip(('color', 'depth', 'final_T', 'radii'), out, pre):
        assert torch.equal(x, y), name
    _check_two_view_grads(scene, cuda, leaves, out[0])


def test_scale_modifier_reference_shaped(cuda, oracle_lib):
    """GaussianRasterizer with raster_settings.scale_modifier 0.75: the first camera of the two-view scene."""
    q = _two_view_scene(oracle_lib, scale_modifier=0.75)
    cam = (q['views'][0], q['fulls'][0], q['tfx'], q['tfy'], q['H'], q['W'], q['bg'])
    _run(oracle_lib, cuda, q['xyz'], q['rgb'], q['opac'], q['sc'], q['rot'], *cam, seed=5, tol=2e-3, scale_modifier=0.75)
    images = []
    for mod, sc in ((0.75, q['sc']), (1.0, q['sc'] * np.float32(0.75))):
        with torch.no_grad():
            images.append(dgr.GaussianRasterizer(_settings(cuda, *cam, mod))(
                _t(q['xyz'], cuda), None, _t(q['opac'], cuda), colors_precomp=_t(q['rgb'], cuda), scales=_t(sc, cuda),
                rotations=_t(q['rot'], cuda)))
    for name, x, y in zip(('color', 'radii', 'depth'), *images):
        assert torch.equal(x, y), name


@pytest.mark.parametrize('surface', ['rasterizer', 'views', 'packed'])
def test_in_place_edit_of_the_rendered_colour_raises(cuda, oracle_lib, surface):
    """The backward rebuilds S = C_out - T_final * bg from the saved forward image, so an edit of that image must not
    silently change the gradients.  The batched surfaces return the saved tensor itself: the edit is caught in backward.
    GaussianRasterizer returns view [0] of the batch it rendered, and torch refuses an in-place edit of a view made
    inside a custom Function at the edit itself."""
    scene = _two_view_scene(oracle_lib)
    if surface == 'rasterizer':
        q = scene
        s = _settings(cuda, q['views'][0], q['fulls'][0], q['tfx'], q['tfy'], q['H'], q['W'], q['bg'])
        color, _, _ = dgr.GaussianRasterizer(s)(_t(q['xyz'], cuda, True), None, _t(q['opac'], cuda, True),
                                                colors_precomp=_t(q['rgb'], cuda, True), scales=_t(q['sc'], cuda, True),
                                                rotations=_t(q['rot'], cuda, True))
        with pytest.raises(RuntimeError, match='is a view and is being modified inplace'):
            color.clamp_(0, 1)
        return
    _, out = _render_two_views(scene, cuda, surface)
    color = out[0]
    color.clamp_(0, 1)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        color.sum().backward()


def test_smallest_shapes_that_split_the_front_end(cuda, oracle_lib):
    """P = 2100 is more than one preprocess chunk (1024) and more than one scatter chunk (2048); 72 x 40 is no multiple
    of the 16 x 16 tile either way, and its three tile rows leave the last vertical tile pair without a second tile.
    Two views.  Forward with the assertions of test_rasterize_gpu.py's random scenes, backward at the scene bar."""
    from tests.test_rasterize_gpu import AMBIGUITY, _compare
    q = _two_view_scene(oracle_lib, n=2100, W=72, H=40, seed=21)
    H, W = q['H'], q['W']
    args = [_t(q[k], cuda) for k in ('xyz', 'rgb', 'opac', 'sc', 'rot')]
    vms = torch.stack([_t(v, cuda) for v in q['views']])
    pms = torch.stack([_t(f, cuda) for f in q['fulls']])
    for mode in ('median', 'mean'):
        got = dgr.rasterize_views(*args, vms, pms, [q['tfx']] * 2, [q['tfy']] * 2, H, W, _t(q['bg'], cuda),
                                  depth_mode=mode, want_tiles_touched=True)
        torch.cuda.synchronize()
        assert int(got['status'].item()) & 1 == 0
        for v in range(2):
            want = oracle_lib.rasterize_forward(q['xyz'], q['rgb'], q['opac'], q['sc'], q['rot'], q['views'][v],
                                                q['fulls'][v], q['tfx'], q['tfy'], H, W, q['bg'], depth_mode=mode,
                                                ambiguity=AMBIGUITY)
            assert want['num_rendered'] > 100
            _compare(want, {k: t[v:v + 1].cpu().numpy() for k, t in got.items() if k != 'status'}, H, W,
                     label=f'72x40 view {v} {mode}')
    leaves, out = _render_two_views(q, cuda, 'views')
    _check_two_view_grads(q, cuda, leaves, out[0])


def test_backward_of_empty_view_is_zero(cuda):
    W, H = 32, 32
    view, full, tfx, tfy = helpers.simple_camera(W, H)
    xyz = np.float32([[0, 0, -5.0], [100.0, 0, 5.0]])       # behind the camera / far off screen
    m3 = _t(xyz, cuda, True)
    c = _t(np.float32([[1, 1, 1], [1, 1, 1]]), cuda, True)
    color, _, _, _ = dgr.rasterize_views_autograd(m3, c, _t(np.float32([[0.5], [0.5]]), cuda),
                                                  _t(np.float32([[0.1] * 3] * 2), cuda),
                                                  _t(np.float32([[1, 0, 0, 0]] * 2), cuda), _t(view, cuda).view(1, 4, 4),
                                                  _t(full, cuda).view(1, 4, 4), [tfx], [tfy], H, W,
                                                  torch.zeros(3, device=cuda))
    color.sum().backward()
    assert float(m3.grad.abs().max()) == 0.0 and float(c.grad.abs().max()) == 0.0


def _cov3d_of(sc, rot):
    """computeCov3D (forward.cu:118-121 layout xx xy xz yy yz zz) in float32, Sigma = (S R)^T (S R)."""
    r, x, y, z = (rot[:, i].astype(np.float32) for i in range(4))
    one, two = np.float32(1), np.float32(2)
    R = np.stack([np.stack([one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)], 1),
                  np.stack([two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)], 1),
                  np.stack([two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)], 1)], 1)   # (P,3,3)
    M = sc[:, :, None].astype(np.float32) * np.transpose(R, (0, 2, 1))     # M[k][i] = s_k R[i][k]
    S = np.einsum('pki,pkj->pij', M, M).astype(np.float32)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)


@pytest.mark.parametrize('n,seed,tol', [(12, 3, 1e-4), (2000, 7, 2e-3)])
def test_backward_with_cov3d_precomp(cuda, oracle_lib, n, seed, tol):
    """cov3D_precomp path (backward.cu:346-396 stops at dL/dcov3D): the oracle returns dL/dcov3D of the same scene
    built from (scales, rotations); the HIP op gets the covariance itself and must return that gradient, and the
    same gradients for everything upstream of the covariance."""
    rng = np.random.default_rng(seed)
    W, H = 112, 64
    view, full, tfx, tfy = helpers.simple_camera(W, H)
    xyz, rgb, opac, sc, rot = helpers.random_gaussians(rng, n)
    rot = (rot / np.linalg.norm(rot, axis=1, keepdims=True)).astype(np.float32)
    bg = np.float32([0.2, 0.1, 0.3])
    gcol = rng.standard_normal((3, H, W)).astype(np.float32)
    want = oracle_lib.rasterize_backward(gcol, xyz, rgb, opac, sc, rot, view, full, tfx, tfy, H, W, bg)
    settings = dgr.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=tfx, tanfovy=tfy, bg=_t(bg, cuda), scale_modifier=1.0,
        viewmatrix=_t(view, cuda), projmatrix=_t(full, cuda), sh_degree=0, campos=torch.zeros(3, device=cuda),
        prefiltered=False)
    m3, m2 = _t(xyz, cuda, True), torch.zeros(n, 3, device=cuda, requires_grad=True)
    c, o, cov = _t(rgb, cuda, True), _t(opac, cuda, True), _t(_cov3d_of(sc, rot), cuda, True)
    color, radii, depth = dgr.GaussianRasterizer(settings)(m3, m2, o, colors_precomp=c, cov3D_precomp=cov)
    (color * _t(gcol, cuda)).sum().backward()
    torch.cuda.synchronize()
    _check(c.grad.cpu().numpy(), want['colors'], 'dL_dcolors', tol)
    _check(o.grad.cpu().numpy(), want['opacities'], 'dL_dopacity', tol)
    _check(m2.grad.cpu().numpy(), want['means2D'], 'dL_dmeans2D', tol)
    _check(m3.grad.cpu().numpy(), want['means3D'], 'dL_dmeans3D', tol)
    _check(cov.grad.cpu().numpy(), want['cov3D'], 'dL_dcov3D', tol)
    # and the two forward paths render the same image
    s, r = _t(sc, cuda), _t(rot, cuda)
    with torch.no_grad():
        color2, _, _ = dgr.GaussianRasterizer(settings)(_t(xyz, cuda), None, _t(opac, cuda), colors_precomp=_t(rgb, cuda),
                                                        scales=s, rotations=r)
    assert float((color2 - color.detach()).abs().max()) <= 1e-4
