"""What the rasteriser's depth / final_T backward must return, composed from the C oracle's COLOUR backward, and the
scenes the two test files of that backward share.

The mean depth ``D = sum_i alpha_i T_i z_i`` is colour channel 0 of a render whose colours are ``(z_i, 1, 0)`` over a zero
background, and ``1 - final_T`` is its channel 1.  So the gradient of ``sum gD * D + gT * final_T`` is the oracle's colour
backward of that render for the image gradient ``(gD, -gT, 0)``; what it returns for the colours' first channel is
``dL/dz_i``, and ``z_i = view[:, 2] . (mean_i, 1)`` carries it to the mean.  The backward is linear in the image gradients:
a colour gradient of the real render adds its own backward."""
import numpy as np

from tests import helpers

LEAVES = ('means3D', 'means2D', 'colors', 'opacities', 'scales', 'rotations')


def expected(oracle_lib, gD, gT, xyz, opac, sc, rot, view, full, tfx, tfy, H, W, scale_modifier=1.0, gcol=None, rgb=None,
             bg=None):
    """-> dict of the oracle's gradients (``LEAVES`` and ``cov3D``) of ``sum gD * D + gT * final_T [+ gcol * colour]`` for
    one view.  ``gD`` / ``gT``: (H,W) arrays or None (zeros); ``gcol`` (3,H,W) with the scene's ``rgb`` and ``bg``."""
    zero3 = np.zeros(3, np.float32)
    z = oracle_lib.rasterize_forward(xyz, np.zeros_like(xyz), opac, sc, rot, view, full, tfx, tfy, H, W, zero3,
                                     scale_modifier=scale_modifier, depth_mode='mean')['depths']
    cols = np.stack([z, np.ones_like(z), np.zeros_like(z)], 1).astype(np.float32)
    g = np.zeros((3, H, W), np.float32)
    if gD is not None:
        g[0] = gD
    if gT is not None:
        g[1] = -np.asarray(gT, np.float32)
    w = oracle_lib.rasterize_backward(g, xyz, cols, opac, sc, rot, view, full, tfx, tfy, H, W, zero3,
                                      scale_modifier=scale_modifier)
    out = {k: w[k].copy() for k in ('means2D', 'opacities', 'scales', 'rotations', 'cov3D')}
    out['means3D'] = w['means3D'] + np.asarray(view, np.float32).reshape(4, 4)[:3, 2][None, :] * w['colors'][:, :1]
    out['colors'] = np.zeros_like(w['colors'])
    if gcol is not None:
        c = oracle_lib.rasterize_backward(gcol, xyz, rgb, opac, sc, rot, view, full, tfx, tfy, H, W, np.float32(bg),
                                          scale_modifier=scale_modifier)
        out = {k: out[k] + c[k] for k in out}
    return out


def single_gaussian_scene():
    """The single-Gaussian scene of tests/test_rasterize_backward_gpu.py, 64 x 48."""
    W, H = 64, 48
    view, full, tfx, tfy = helpers.simple_camera(W, H)
    return dict(xyz=np.float32([[0.3, -0.2, 5.0]]), rgb=np.float32([[0.2, 0.5, 0.9]]), opac=np.float32([[0.7]]),
                sc=np.float32([[0.3, 0.2, 0.25]]), rot=np.float32([[0.9, 0.1, -0.3, 0.2]]), view=view, full=full, tfx=tfx,
                tfy=tfy, H=H, W=W, bg=np.float32([0.1, 0.2, 0.3]))


def twelve_gaussian_scene():
    """The twelve overlapping Gaussians of tests/test_rasterize_backward_gpu.py, 80 x 48."""
    W, H = 80, 48
    view, full, tfx, tfy = helpers.simple_camera(W, H)
    rng = np.random.default_rng(3)
    n = 12
    xyz = np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.6, 0.6, n), rng.uniform(3, 9, n)], 1).astype(np.float32)
    return dict(xyz=xyz, rgb=rng.uniform(0, 1, (n, 3)).astype(np.float32), opac=rng.uniform(0.2, 0.9, (n, 1)).astype(np.float32),
                sc=rng.uniform(0.1, 0.5, (n, 3)).astype(np.float32), rot=rng.standard_normal((n, 4)).astype(np.float32),
                view=view, full=full, tfx=tfx, tfy=tfy, H=H, W=W, bg=np.float32([0.3, 0.1, 0.6]))


def image_gradients(scene, seed):
    """Seeded (gcol (3,H,W), gD (H,W), gT (H,W)) for a scene."""
    rng = np.random.default_rng(seed)
    H, W = scene['H'], scene['W']
    return (rng.standard_normal((3, H, W)).astype(np.float32), rng.standard_normal((H, W)).astype(np.float32),
            rng.standard_normal((H, W)).astype(np.float32))


def expected_for(oracle_lib, scene, gD=None, gT=None, gcol=None, view=0, scale_modifier=1.0):
    """``expected`` for a scene dict (``view`` picks the camera of a multi-view scene: ``views`` / ``fulls``)."""
    q = scene
    vm, pm = (q['views'][view], q['fulls'][view]) if 'views' in q else (q['view'], q['full'])
    return expected(oracle_lib, gD, gT, q['xyz'], q['opac'], q['sc'], q['rot'], vm, pm, q['tfx'], q['tfy'], q['H'], q['W'],
                    scale_modifier=scale_modifier, gcol=gcol, rgb=q['rgb'], bg=q['bg'])
