"""CPU: the composition tests/raster_depth_oracle.py makes of the C oracle's colour backward IS the gradient of the mean
depth and of final_T.

The forward is restated here densely in float64 torch (every Gaussian at every pixel; projection, conic with the 0.3
dilation, tile rectangle, the 1/255 cut, the 0.99 clamp, the 1e-4 stop, front-to-back blend) and differentiated by
autograd.  The two scenes are the small ones of tests/test_rasterize_backward_gpu.py: no decision lies near its
threshold there, so the float64 restatement takes the oracle's float32 branches, and the bar is the one that file holds
for them: 1e-4 of each gradient's scale."""
import numpy as np
import pytest
import torch

from tests import raster_depth_oracle as rdo


def _dense_forward(leaves, q):
    """-> (D (H,W), final_T (H,W)) in float64 from the leaves ``means3D, ndc_offset, opacities, scales, rotations``."""
    m3, m2, op, sc, rot = leaves
    H, W = q['H'], q['W']
    view = torch.from_numpy(np.asarray(q['view'], np.float64).reshape(4, 4))
    proj = torch.from_numpy(np.asarray(q['full'], np.float64).reshape(4, 4))
    fx, fy = W / (2.0 * q['tfx']), H / (2.0 * q['tfy'])
    hom = torch.cat((m3, torch.ones(m3.shape[0], 1, dtype=torch.float64)), 1)
    t = hom @ view
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    assert bool((tz > 0.2).all())
    # the reference clamps tx / tz to 1.3 tan(fov / 2) and differentiates as if it had not: not exercised here
    assert bool(((tx / tz).abs() < 1.3 * q['tfx']).all()) and bool(((ty / tz).abs() < 1.3 * q['tfy']).all())
    ph = hom @ proj
    p_w = 1.0 / (ph[:, 3] + 0.0000001)
    ndc = ph[:, :2] * p_w[:, None] + m2[:, :2]
    px = ((ndc[:, 0] + 1.0) * W - 1.0) * 0.5
    py = ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5
    r, x, y, z = rot[:, 0], rot[:, 1], rot[:, 2], rot[:, 3]
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], 1),
                     torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], 1),
                     torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    sigma = torch.einsum('pik,pk,pjk->pij', R, sc * sc, R)
    j00, j02 = fx / tz, -(fx * tx) / (tz * tz)
    j11, j12 = fy / tz, -(fy * ty) / (tz * tz)
    A = torch.stack([j00[:, None] * view[:3, 0][None] + j02[:, None] * view[:3, 2][None],
                     j11[:, None] * view[:3, 1][None] + j12[:, None] * view[:3, 2][None]], 1)      # (P,2,3)
    cov = A @ sigma @ A.transpose(1, 2)
    a, b, c = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = a * c - b * b
    cxx, cxy, cyy = c / det, -b / det, a / det
    with torch.no_grad():
        mid = 0.5 * (a + c)
        lam = mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
        radius = torch.ceil(3.0 * torch.sqrt(lam))
        gx, gy = (W + 15) // 16, (H + 15) // 16
        x0 = torch.clamp(((px - radius) / 16).long(), 0, gx)
        y0 = torch.clamp(((py - radius) / 16).long(), 0, gy)
        x1 = torch.clamp(((px + radius + 15) / 16).long(), 0, gx)
        y1 = torch.clamp(((py + radius + 15) / 16).long(), 0, gy)
        order = sorted(range(m3.shape[0]), key=lambda i: (float(tz[i]), i))
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    tile_x, tile_y = (xs / 16).long(), (ys / 16).long()
    T = torch.ones(H, W, dtype=torch.float64)
    D = torch.zeros(H, W, dtype=torch.float64)
    done = torch.zeros(H, W, dtype=torch.bool)
    for i in order:
        dx, dy = px[i] - xs, py[i] - ys
        power = -0.5 * (cxx[i] * dx * dx + cyy[i] * dy * dy) - cxy[i] * dx * dy
        alpha = torch.clamp(op[i, 0] * torch.exp(power), max=0.99)
        in_rect = (tile_x >= x0[i]) & (tile_x < x1[i]) & (tile_y >= y0[i]) & (tile_y < y1[i])
        valid = in_rect & ~(power > 0) & ~(alpha < 1.0 / 255.0) & ~done
        test_T = T * (1.0 - alpha)
        stop = valid & (test_T < 0.0001)
        done = done | stop
        valid = valid & ~stop
        D = D + torch.where(valid, alpha * T * tz[i], torch.zeros_like(T))
        T = torch.where(valid, test_T, T)
    return D, T


@pytest.mark.parametrize('scene', ['single', 'twelve'])
def test_composed_oracle_is_the_gradient_of_mean_depth_and_final_T(oracle_lib, scene):
    q = rdo.single_gaussian_scene() if scene == 'single' else rdo.twelve_gaussian_scene()
    _, gD, gT = rdo.image_gradients(q, 11)
    want = rdo.expected_for(oracle_lib, q, gD=gD, gT=gT)
    n = q['xyz'].shape[0]
    leaves = [torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True)
              for a in (q['xyz'], np.zeros((n, 3)), q['opac'], q['sc'], q['rot'])]
    D, T = _dense_forward(leaves, q)
    # the restatement renders what the oracle's forward renders
    fwd = oracle_lib.rasterize_forward(q['xyz'], q['rgb'], q['opac'], q['sc'], q['rot'], q['view'], q['full'], q['tfx'],
                                       q['tfy'], q['H'], q['W'], q['bg'], depth_mode='mean')
    assert float(np.abs(D.detach().numpy() - fwd['depth'][0]).max()) <= 1e-4 * max(float(fwd['depth'].max()), 1.0)
    assert float(np.abs(T.detach().numpy() - fwd['final_T']).max()) <= 1e-5
    (D * torch.from_numpy(gD.astype(np.float64))).sum().add((T * torch.from_numpy(gT.astype(np.float64))).sum()).backward()
    for name, leaf in zip(('means3D', 'means2D', 'opacities', 'scales', 'rotations'), leaves):
        got, w = leaf.grad.numpy(), want[name]
        scale = max(float(np.abs(w).max()), 1e-6)
        err = float(np.abs(got - w).max()) / scale
        print(f'{scene} {name}: max err {err:.3e} of the gradient scale {scale:.3e}')
        assert err <= 1e-4, f'{name}: max err {err:.3e} of the gradient scale {scale:.3e}'
    assert float(np.abs(want['colors']).max()) == 0.0


def test_the_depth_row_term_is_part_of_the_mean_gradient(oracle_lib):
    """Without ``view[:3, 2] * dL/dz`` the composition misses the bar by orders of magnitude: the test above would notice."""
    q = rdo.twelve_gaussian_scene()
    _, gD, _ = rdo.image_gradients(q, 11)
    want = rdo.expected_for(oracle_lib, q, gD=gD)
    zero3 = np.zeros(3, np.float32)
    z = oracle_lib.rasterize_forward(q['xyz'], q['rgb'], q['opac'], q['sc'], q['rot'], q['view'], q['full'], q['tfx'],
                                     q['tfy'], q['H'], q['W'], zero3, depth_mode='mean')['depths']
    g = np.zeros((3, q['H'], q['W']), np.float32)
    g[0] = gD
    bare = oracle_lib.rasterize_backward(g, q['xyz'], np.stack([z, np.ones_like(z), np.zeros_like(z)], 1), q['opac'],
                                         q['sc'], q['rot'], q['view'], q['full'], q['tfx'], q['tfy'], q['H'], q['W'], zero3)
    scale = float(np.abs(want['means3D']).max())
    assert float(np.abs(bare['means3D'][:, 2] - want['means3D'][:, 2]).max()) > 1e-2 * scale
    assert np.array_equal(bare['means3D'][:, :2], want['means3D'][:, :2])      # identity rotation: only z moves


def _depth_entry(**change):
    """ocrf_rasterize_backward_depth with arguments that pass every check except what ``change`` replaces.  Pointers are
    small integers: a refused call dereferences none of them."""
    import ctypes
    from ocrfdet_amd import _lib
    L = _lib.lib()
    P, V, H, W = 100, 2, 32, 48
    p = ctypes.c_void_p(4096)
    a = dict(W=W, H=H, scales=p, rotations=p, cov3D=None, fwd_depth=p, dL_ddepth=p, dL_dfinal_T=p, dL_dscales=p, dL_dcov3D=None,
             workspace=p, workspace_bytes=L.ocrf_rasterize_backward_depth_workspace_bytes(P, V))
    a.update(change)
    return L.ocrf_rasterize_backward_depth(P, V, a['H'], a['W'], p, p, p, a['scales'], ctypes.c_float(1.0), a['rotations'],
                                           a['cov3D'], p, p, p, a['fwd_depth'], p, p, p, a['dL_ddepth'], a['dL_dfinal_T'], p, p,
                                           p, a['dL_dscales'], p, a['dL_dcov3D'], None, a['workspace'],
                                           ctypes.c_size_t(a['workspace_bytes']), None)


def test_the_new_entry_refuses_bad_arguments_at_the_c_boundary():
    """Refused by the argument checks, before anything is enqueued (hipErrorInvalidValue without a device): what the
    colour-only entries refuse, no gradient of depth or final_T at all (their case), a depth gradient without the depth."""
    import ctypes
    from ocrfdet_amd import _lib
    L = _lib.lib()
    invalid = 1
    size = L.ocrf_rasterize_backward_depth_workspace_bytes(100, 2)
    assert _depth_entry(workspace=None) == invalid
    assert _depth_entry(workspace_bytes=size - 1) == invalid
    assert _depth_entry(W=16 * 65535 + 1, H=16) == invalid
    assert _depth_entry(rotations=None) == invalid
    assert _depth_entry(dL_dscales=None) == invalid
    assert _depth_entry(cov3D=ctypes.c_void_p(4096), dL_dcov3D=None) == invalid
    assert _depth_entry(dL_ddepth=None, dL_dfinal_T=None) == invalid
    assert _depth_entry(fwd_depth=None) == invalid
    # ten sums per (view, Gaussian) instead of nine, each accumulator rounded up to 256 bytes: 8192 against 7424
    assert size == L.ocrf_rasterize_backward_workspace_bytes(100, 2) + 768
    assert L.ocrf_rasterize_backward_depth_workspace_bytes(0, 2) == 0
    assert L.ocrf_kernel_name(_lib.K_RASTER_BLEND_BWD_DEPTH) == b'raster_blend_kernel<false, true, true, true, true>'
    assert L.ocrf_kernel_name(_lib.K_RASTER_PRE_BWD_DEPTH) == b'raster_preprocess_backward_kernel<true>'


def test_depth_grad_needs_the_mean_depth_on_every_surface():
    from ocrfdet_amd import diff_gaussian_rasterization as dgr
    from ocrfdet_amd import view_transformer_ocrf as vto
    with pytest.raises(ValueError, match="depth_mode='mean'"):
        dgr.GaussianRasterizer(None, depth_grad=True)
    with pytest.raises(ValueError, match="depth_mode='mean'"):
        dgr.rasterize_packed_autograd(*(torch.zeros(1, k) for k in (3, 3, 1, 3, 4)), torch.zeros(1, 36), 16, 16, torch.zeros(3),
                                      depth_grad=True)
    assert dgr.GaussianRasterizer(None, depth_mode='mean', depth_grad=True).depth_grad is True
    assert vto.OcRFViewTransformerFull.render_depth_grad is False
