"""Gaussian rasteriser with depth output — drop-in for the ``diff_gaussian_rasterization`` module
OcRFDet imports (the JonathonLuiten *w-depth* fork; call site
``mmdet3d/models/necks/MVSGaussian/lib/gaussian_renderer/__init__.py:14,39-70``).

Surface kept (names, argument order, return arity of the fork):

``GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg, scale_modifier,
viewmatrix, projmatrix, sh_degree, campos, prefiltered[, debug])``
    the fork's 11 fields; ``debug`` (the stock 12th field,
    ``.../diff_gaussian_rasterization/__init__.py:157-169``) is accepted and defaults to False.
``GaussianRasterizer(raster_settings)(means3D, means2D, opacities, shs=None, colors_precomp=None,
scales=None, rotations=None, cov3D_precomp=None) -> (color (3,H,W), radii (P,) int32,
depth (1,H,W))``
    exactly one of shs / colors_precomp and one of (scales, rotations) / cov3D_precomp, else the
    reference's ``Exception`` (``__init__.py:191-195``).  ``viewmatrix`` / ``projmatrix`` are the
    transposed (row-vector) 4x4 matrices.
``rasterize_gaussians(...)`` and ``GaussianRasterizer.markVisible``.

Beyond the reference: ``rasterize_views`` renders a batch of cameras over one Gaussian set in a
single launch sequence and also returns ``final_T`` (1 - accumulated opacity) and ``n_contrib``.

Compute: ``csrc/rasterize.hip`` through the C ABI (``ocrf_rasterize_forward`` /
``ocrf_rasterize_backward``).  The backward covers what the fork's does — the colour output w.r.t.
means3D, means2D (screen-space, for densification statistics), colours, opacities, scales, rotations.
Depth has no backward in the fork (diff-gaussian-rasterization-w-depth/README.md:13); here it is differentiable on
request: ``depth_mode='mean', depth_grad=True`` on ``GaussianRasterizer``, ``rasterize_views_autograd`` and
``rasterize_packed_autograd`` makes the mean depth ``D = sum_i alpha_i T_i z_i`` (and, on the batched surfaces,
``final_T``) differentiable outputs (``ocrf_rasterize_backward_depth``).  ``D`` is unnormalised; the normalised expected
depth is ``D / (1 - final_T).clamp_min(eps)``, differentiable in both.  The defaults are the fork's graph.
``cov3D_precomp`` has its own backward (gradient w.r.t. the six covariance entries).  SH colours (``shs`` (P,M,3) with
``raster_settings.sh_degree`` / ``campos``; OcRFDet itself passes ``shs=None``) are evaluated by ``ocrf_sh_to_rgb`` into the
(P,3) colours of the ordinary pipeline, forward and backward (``forward.cu:20-71``, ``backward.cu:20-140``).
"""
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _lib

__all__ = ['GaussianRasterizationSettings', 'GaussianRasterizer', 'rasterize_gaussians', 'rasterize_views', 'pack_cameras',
           'rasterize_views_backward', 'rasterize_views_autograd', 'rasterize_packed_autograd', 'sh_to_rgb',
           'sh_to_rgb_backward']


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool = False


def _f32c(t):
    return t.detach().contiguous().float()


def pack_cameras(viewmatrices, projmatrices, tanfovx, tanfovy, H, W, dev):
    """(V,36) float rows: view16 | proj16 | tanfovx | tanfovy | focal_x | focal_y — the camera block of
    the C ABI.  Costs a few small host->device copies: callers with a fixed rig build it once and pass it
    as ``packed_cameras=``."""
    vm = _f32c(viewmatrices).reshape(-1, 16)
    pm = _f32c(projmatrices).reshape(-1, 16)
    V = vm.size(0)
    tfx = torch.as_tensor(tanfovx, dtype=torch.float64).reshape(-1).expand(V) if not torch.is_tensor(tanfovx) \
        else tanfovx.detach().double().reshape(-1).cpu().expand(V)
    tfy = torch.as_tensor(tanfovy, dtype=torch.float64).reshape(-1).expand(V) if not torch.is_tensor(tanfovy) \
        else tanfovy.detach().double().reshape(-1).cpu().expand(V)
    # focal = size / (2 * tan) evaluated in float32 like rasterizer_impl.cu:222-223
    tf = torch.stack((tfx, tfy), 1).float()
    focal = torch.stack((torch.tensor(float(W)) / (2.0 * tf[:, 0]), torch.tensor(float(H)) / (2.0 * tf[:, 1])), 1)
    return torch.cat((vm, pm, tf.to(dev), focal.float().to(dev)), 1).contiguous()


def sh_to_rgb(means3D, campos, shs, degree):
    """View-dependent colours from spherical harmonics (``forward.cu:20-71``): means3D (P,3), campos (3,) the camera
    centre, shs (P,M,3), ``degree`` 0..3 with M >= (degree+1)^2 -> (colors (P,3) float32, clamped (P,3) uint8)."""
    _lib.require_cuda(means3D, campos, shs)
    if shs.dim() != 3 or shs.size(2) != 3 or shs.size(0) != means3D.size(0):
        raise RuntimeError('shs must have dimensions (num_points, num_coefficients, 3)')
    P, M, degree = means3D.size(0), shs.size(1), int(degree)
    if not 0 <= degree <= 3 or M < (degree + 1) ** 2:
        raise RuntimeError(f'sh_degree {degree} needs 0 <= degree <= 3 and at least {(degree + 1) ** 2} coefficients, got {M}')
    means3D, campos, shs = _f32c(means3D), _f32c(campos).reshape(3), _f32c(shs)
    dev = means3D.device
    colors = torch.empty(P, 3, device=dev)
    clamped = torch.empty(P, 3, dtype=torch.uint8, device=dev)
    _lib.launch('ocrf_sh_to_rgb', dev, P, degree, M, means3D, campos, shs, colors, clamped)
    return colors, clamped


def sh_to_rgb_backward(means3D, campos, shs, degree, clamped, dL_dcolors, dL_dmeans3D=None):
    """Backward of ``sh_to_rgb`` (``backward.cu:20-140``) -> (dL_dmeans3D (P,3), dL_dshs (P,M,3)).  The means' part (the
    view direction depends on the mean) is ADDED to ``dL_dmeans3D`` when one is given (in place), else returned alone."""
    _lib.require_cuda(means3D, campos, shs, clamped, dL_dcolors)
    P, M = means3D.size(0), shs.size(1)
    means3D, campos, shs, g = _f32c(means3D), _f32c(campos).reshape(3), _f32c(shs), _f32c(dL_dcolors).reshape(P, 3)
    dev = means3D.device
    if dL_dmeans3D is None:
        dL_dmeans3D = torch.zeros(P, 3, device=dev)
    elif not (dL_dmeans3D.is_contiguous() and dL_dmeans3D.dtype == torch.float32 and dL_dmeans3D.numel() == 3 * P):
        raise RuntimeError('dL_dmeans3D must be a contiguous float32 (P,3) tensor')
    d_sh = torch.empty(P, M, 3, device=dev)
    _lib.launch('ocrf_sh_to_rgb_backward', dev, P, int(degree), M, means3D, campos, shs, clamped.contiguous(), g,
                dL_dmeans3D, d_sh)
    return dL_dmeans3D, d_sh


def _camera_rows(packed_cameras, viewmatrices, projmatrices, tanfovx, tanfovy, H, W, dev):
    """The (V,36) camera rows of a call: the packed ones if given, else ``pack_cameras`` of the matrices."""
    if packed_cameras is not None:
        return packed_cameras
    return pack_cameras(viewmatrices, projmatrices, tanfovx, tanfovy, H, W, dev)


def rasterize_views_backward(grad_color, fwd, means3D, colors, opacities, scales, rotations, viewmatrices,
                             projmatrices, tanfovx, tanfovy, image_height, image_width, bg, scale_modifier=1.0,
                             want_means2D=False, packed_cameras=None, cov3D_precomp=None, grad_depth=None,
                             grad_final_T=None):
    """Backward of ``rasterize_views``' colour output, summed over the views.  ``fwd`` is the dict
    ``rasterize_views`` returned for the same inputs.  Returns a dict ``means3D`` (P,3), ``colors``
    (P,3), ``opacities`` (P,1), ``scales`` (P,3), ``rotations`` (P,4) [, ``means2D`` (V,P,3)]; with
    ``cov3D_precomp`` (P,6) (``scales`` / ``rotations`` None) ``cov3D`` (P,6) instead of the last two
    (backward.cu:346-396 without computeCov3D's backward).

    ``grad_depth`` (V,[1,]H,W) / ``grad_final_T`` (V,H,W): gradients of the MEAN depth (``fwd`` then rendered with
    ``depth_mode='mean'`` and holds ``'depth'``) and of ``final_T``.  With either one the call goes to
    ``ocrf_rasterize_backward_depth``, which adds them to the same sums; without, to the colour-only entries."""
    has_cov = cov3D_precomp is not None
    _lib.require_cuda(means3D, colors, opacities, *((cov3D_precomp,) if has_cov else (scales, rotations)), grad_color)
    dev = means3D.device
    P = means3D.size(0)
    H, W = int(image_height), int(image_width)
    cams = _camera_rows(packed_cameras, viewmatrices, projmatrices, tanfovx, tanfovy, H, W, dev)
    V = cams.size(0)
    g = _f32c(grad_color).reshape(V, 3, H, W)
    means3D, colors, opac, bg = _f32c(means3D), _f32c(colors), _f32c(opacities).reshape(-1), _f32c(bg).reshape(3)
    fc, ft, fn = fwd['color'].contiguous(), fwd['final_T'].contiguous(), fwd['n_contrib'].contiguous()
    if tuple(fc.shape) != (V, 3, H, W) or tuple(ft.shape) != (V, H, W) or tuple(fn.shape) != (V, H, W):
        raise RuntimeError('rasterize_views_backward: forward outputs do not match the view batch')
    out = dict(means3D=torch.empty(P, 3, device=dev), colors=torch.empty(P, 3, device=dev),
               opacities=torch.empty(P, 1, device=dev))
    if has_cov:
        out['cov3D'] = torch.empty(P, 6, device=dev)
    else:
        out['scales'], out['rotations'] = torch.empty(P, 3, device=dev), torch.empty(P, 4, device=dev)
    m2d = torch.empty(V, P, 3, device=dev) if want_means2D else None
    if m2d is not None:
        out['means2D'] = m2d
    gd = gt = fd = None
    if grad_depth is not None:
        if fwd.get('depth') is None:
            raise RuntimeError("rasterize_views_backward: grad_depth needs the forward's mean depth in fwd['depth']")
        _lib.require_cuda(grad_depth, fwd['depth'])
        if grad_depth.numel() != V * H * W or fwd['depth'].numel() != V * H * W:
            raise RuntimeError('rasterize_views_backward: depth and its gradient do not match the view batch')
        gd, fd = _f32c(grad_depth).reshape(V, H, W), _f32c(fwd['depth']).reshape(V, H, W)
    if grad_final_T is not None:
        _lib.require_cuda(grad_final_T)
        if grad_final_T.numel() != V * H * W:
            raise RuntimeError('rasterize_views_backward: grad_final_T does not match the view batch')
        gt = _f32c(grad_final_T).reshape(V, H, W)
    if P == 0:
        return out
    if gd is not None or gt is not None:
        ws = _lib.workspace.get(dev, _lib.lib().ocrf_rasterize_backward_depth_workspace_bytes(P, V), 'raster')
        _lib.launch('ocrf_rasterize_backward_depth', dev, P, V, H, W, means3D, colors, opac,
                    None if has_cov else _f32c(scales), float(scale_modifier), None if has_cov else _f32c(rotations),
                    _f32c(cov3D_precomp).reshape(P, 6) if has_cov else None, cams, bg, fc, fd, ft, fn, g, gd, gt,
                    out['means3D'], out['colors'], out['opacities'], out.get('scales'), out.get('rotations'),
                    out.get('cov3D'), m2d, ws, ws.numel())
        return out
    ws = _lib.workspace.get(dev, _lib.lib().ocrf_rasterize_backward_workspace_bytes(P, V), 'raster')
    shared = (cams, bg, fc, ft, fn, g, out['means3D'], out['colors'], out['opacities'])
    if has_cov:
        _lib.launch('ocrf_rasterize_backward_cov3d', dev, P, V, H, W, means3D, colors, opac,
                    _f32c(cov3D_precomp).reshape(P, 6), *shared, out['cov3D'], m2d, ws, ws.numel())
    else:
        _lib.launch('ocrf_rasterize_backward', dev, P, V, H, W, means3D, colors, opac, _f32c(scales), float(scale_modifier),
                    _f32c(rotations), *shared, out['scales'], out['rotations'], m2d, ws, ws.numel())
    return out


def _forward(entry, dims, means3D, colors, opac, sc, scale_modifier, rot, cov, cams, bg, H, W, depth_mode, want_n_contrib,
             want_tiles_touched, workspace_tag):
    """Outputs, status word, workspace and launch of a forward entry point whose leading arguments are ``dims`` =
    (P, [sets,] views): fresh tensors over the ``cams.size(0)`` rendered views."""
    dev, P, NV = means3D.device, dims[0], cams.size(0)
    out = dict(color=torch.empty(NV, 3, H, W, device=dev), depth=torch.empty(NV, 1, H, W, device=dev),
               final_T=torch.empty(NV, H, W, device=dev), radii=torch.empty(NV, P, dtype=torch.int32, device=dev))
    if want_n_contrib:
        out['n_contrib'] = torch.empty(NV, H, W, dtype=torch.int32, device=dev)
    tt = torch.empty(NV, P, dtype=torch.int32, device=dev) if want_tiles_touched else None
    status = torch.empty(1, dtype=torch.int32, device=dev)      # zeroed on the device by the bucket scan kernel
    ws = _lib.workspace.get(dev, _lib.lib().ocrf_rasterize_workspace_bytes(P, NV), workspace_tag)
    _lib.launch(entry, dev, *dims, H, W, means3D, colors, opac, sc, float(scale_modifier), rot, cov, cams, bg,
                {'median': 0, 'mean': 1}[depth_mode], out['color'], out['depth'], out['final_T'], out.get('n_contrib'),
                out['radii'], tt, status, ws, ws.numel())
    if tt is not None:
        out['tiles_touched'] = tt
    out['status'] = status     # device int, informational: 2 = the exact streaming path ran for some tile
    return out


def rasterize_views(means3D, colors, opacities, scales, rotations, viewmatrices, projmatrices,
                    tanfovx, tanfovy, image_height, image_width, bg, scale_modifier=1.0,
                    cov3D_precomp=None, depth_mode='median', want_tiles_touched=False, packed_cameras=None,
                    workspace_tag='raster', want_n_contrib=True):
    """Render ``V`` cameras over the same ``P`` Gaussians.

    ``viewmatrices`` / ``projmatrices``: (V,4,4) transposed matrices as the reference passes them;
    ``tanfovx`` / ``tanfovy``: length-V sequences (or scalars).  Returns a dict of fresh tensors:
    ``color`` (V,3,H,W), ``depth`` (V,1,H,W), ``final_T`` (V,H,W), ``n_contrib`` (V,H,W) int32,
    ``radii`` (V,P) int32 [, ``tiles_touched`` (V,P) int32].  Calls that may run concurrently on
    different streams must use different ``workspace_tag``s (the scratch buffer is per tag).
    ``want_n_contrib=False`` (inference: only the backward reads the per-pixel contributor index) drops
    ``n_contrib`` and the two selects per pixel-record that track it."""
    _lib.require_cuda(means3D, colors, opacities, bg)
    if means3D.dim() != 2 or means3D.size(1) != 3:
        raise RuntimeError('means3D must have dimensions (num_points, 3)')     # rasterize_points.cu:57-59
    H, W = int(image_height), int(image_width)
    cams = _camera_rows(packed_cameras, viewmatrices, projmatrices, tanfovx, tanfovy, H, W, means3D.device)   # (V,36)
    _lib.require_cuda(cams)
    if cov3D_precomp is not None and cov3D_precomp.numel() > 0:
        cov, sc, rot = _f32c(cov3D_precomp), None, None
    else:
        cov, sc, rot = None, _f32c(scales), _f32c(rotations)
    return _forward('ocrf_rasterize_forward', (means3D.size(0), cams.size(0)), _f32c(means3D), _f32c(colors),
                    _f32c(opacities).reshape(-1), sc, scale_modifier, rot, cov, cams, _f32c(bg).reshape(3), H, W, depth_mode,
                    want_n_contrib, want_tiles_touched, workspace_tag)


def rasterize_sets(means3D, colors, opacities, scales, rotations, packed_cameras, image_height, image_width, bg,
                   scale_modifier=1.0, depth_mode='median', workspace_tag='raster', want_n_contrib=False):
    """``S`` Gaussian sets x ``V`` views each in one set of launches (C ABI ``ocrf_rasterize_forward_sets``):
    means3D (S,P,3), colors (S,P,3), opacities (S,P[,1]), scales (S,P,3), rotations (S,P,4),
    ``packed_cameras`` (S*V,36) from ``pack_cameras`` (view v renders set v // V).  Forward only, so the
    contributor index is not tracked unless ``want_n_contrib``.
    -> dict like ``rasterize_views`` with a leading S*V view axis."""
    _lib.require_cuda(means3D, colors, opacities, scales, rotations, packed_cameras, bg)
    if means3D.dim() != 3 or means3D.size(2) != 3:
        raise RuntimeError('means3D must have dimensions (num_sets, num_points, 3)')
    S, P = means3D.size(0), means3D.size(1)
    NV = packed_cameras.size(0)
    if NV % S:
        raise RuntimeError('packed_cameras rows must be a multiple of the number of sets')
    return _forward('ocrf_rasterize_forward_sets', (P, S, NV // S), _f32c(means3D), _f32c(colors),
                    _f32c(opacities).reshape(S, P), _f32c(scales), scale_modifier, _f32c(rotations), None,
                    _f32c(packed_cameras), _f32c(bg).reshape(3), int(image_height), int(image_width), depth_mode,
                    want_n_contrib, False, workspace_tag)


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                cov3Ds_precomp, raster_settings, depth_mode='median', depth_grad=False):
        rs = raster_settings
        ctx.depth_grad = _check_depth_grad(depth_mode, depth_grad)
        ctx.set_materialize_grads(False)
        ctx.has_sh = sh is not None and sh.numel() > 0
        if ctx.has_sh:
            # colours of THIS view from the SH coefficients (forward.cu:240-247); everything after is the ordinary pipeline
            colors_precomp, sh_clamped = sh_to_rgb(means3D, rs.campos, sh, rs.sh_degree)
        ctx.has_cov = cov3Ds_precomp is not None and cov3Ds_precomp.numel() > 0
        out = rasterize_views(means3D, colors_precomp, opacities, scales, rotations,
                              rs.viewmatrix.reshape(1, 4, 4), rs.projmatrix.reshape(1, 4, 4),
                              float(rs.tanfovx), float(rs.tanfovy), rs.image_height, rs.image_width,
                              rs.bg, float(rs.scale_modifier), cov3Ds_precomp if ctx.has_cov else None,
                              depth_mode=depth_mode,
                              want_n_contrib=any(ctx.needs_input_grad))      # only the backward reads it
        color, radii, depth = out['color'][0], out['radii'][0], out['depth'][0]
        ctx.mark_non_differentiable(radii, *(() if ctx.depth_grad else (depth,)))
        ctx.raster_settings = rs
        # the forward's outputs are saved through autograd (not as plain attributes): the backward
        # rebuilds S = C_out - T_final * bg from them, so an in-place edit of the rendered image
        # (clamp_, mul_) must raise instead of silently changing the gradients.  The same holds for the SH
        # coefficients and their clamp mask, which the backward of the colours reads: last in the tuple.
        # The covariance is saved in the shape it came in: (cov3D,) or (scales, rotations).  depth_grad: the mean depth is
        # saved the same way (the backward needs D - prefix_D), in front of the SH pair.
        shape = (cov3Ds_precomp,) if ctx.has_cov else (scales, rotations)
        sh_saved = (sh, sh_clamped) if ctx.has_sh else ()
        ctx.save_for_backward(means3D, colors_precomp, opacities, *shape, color, out['final_T'], out.get('n_contrib'),
                              *((depth,) if ctx.depth_grad else ()), *sh_saved)
        return color, radii, depth

    @staticmethod
    def _sh_grads(ctx, means3D, g):
        """With SH colours: dL/dcolors goes on to the coefficients and, through the view direction, to the means."""
        if not ctx.has_sh:
            return g['means3D'], None, g['colors']
        sh, clamped = ctx.saved_tensors[-2:]
        rs = ctx.raster_settings
        d_means, d_sh = sh_to_rgb_backward(means3D, rs.campos, sh, rs.sh_degree, clamped, g['colors'], g['means3D'])
        return d_means, d_sh.to(sh.dtype), None

    @staticmethod
    def backward(ctx, grad_color, _r, grad_depth):
        """Gradient tuple in the reference's order (diff_gaussian_rasterization/__init__.py:96-149):
        means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings (and None for the
        two depth switches).  ``grad_depth`` is None unless the depth is differentiable and the loss reached it: the
        colour-only entry runs then."""
        rs = ctx.raster_settings
        n = 4 if ctx.has_cov else 5
        means3D, colors, opacities, *shape = ctx.saved_tensors[:n]
        scales, rotations, cov = (None, None, *shape) if ctx.has_cov else (*shape, None)
        fwd_color, fwd_T, fwd_n = ctx.saved_tensors[n:n + 3]
        fwd = dict(color=fwd_color.unsqueeze(0), final_T=fwd_T, n_contrib=fwd_n)
        if ctx.depth_grad and grad_depth is not None:
            fwd['depth'] = ctx.saved_tensors[n + 3]
        else:
            grad_depth = None
        if grad_color is None:
            grad_color = torch.zeros_like(fwd_color)
        g = rasterize_views_backward(grad_color.unsqueeze(0), fwd, means3D, colors, opacities, scales, rotations,
                                     rs.viewmatrix.reshape(1, 4, 4), rs.projmatrix.reshape(1, 4, 4),
                                     float(rs.tanfovx), float(rs.tanfovy), rs.image_height, rs.image_width, rs.bg,
                                     float(rs.scale_modifier), want_means2D=True, cov3D_precomp=cov,
                                     grad_depth=grad_depth)
        d_means, d_sh, d_col = _RasterizeGaussians._sh_grads(ctx, means3D, g)
        grads = (d_means, g['means2D'][0], d_sh, d_col, g['opacities'].reshape(opacities.shape),
                 g.get('scales'), g.get('rotations'), g['cov3D'].reshape(cov.shape) if ctx.has_cov else None, None)
        # inputs that were not tensors needing a gradient (means2D=None from render()) must get None
        return tuple(v if need else None for v, need in zip(grads, ctx.needs_input_grad)) + (None, None)


class _RasterizeViews(torch.autograd.Function):
    """Differentiable batched render over packed camera rows ((V,36) of ``pack_cameras``, on the device: nothing of the
    call or its backward touches the host's copy of the calibration): colour (V,3,H,W) w.r.t. the Gaussian
    parameters, gradients summed over the views in one backward launch sequence.  With ``depth_grad`` (mean depth
    only) the depth and ``final_T`` are differentiable too; a backward that neither of them reached is the colour-only
    one."""

    @staticmethod
    def forward(ctx, means3D, colors, opacities, scales, rotations, packed, H, W, bg, scale_modifier,
                depth_mode='median', depth_grad=False):
        ctx.depth_grad = _check_depth_grad(depth_mode, depth_grad)
        ctx.set_materialize_grads(False)
        out = rasterize_views(means3D, colors, opacities, scales, rotations, None, None, None, None, H, W, bg,
                              scale_modifier, depth_mode=depth_mode, packed_cameras=packed)
        ctx.cam = (packed, H, W, bg, scale_modifier)
        # the rendered depth is saved through autograd like the colour: an in-place edit raises in backward
        ctx.save_for_backward(means3D, colors, opacities, scales, rotations, out['color'], out['final_T'], out['n_contrib'],
                              *((out['depth'],) if ctx.depth_grad else ()))
        ctx.mark_non_differentiable(out['radii'], *(() if ctx.depth_grad else (out['depth'], out['final_T'])))
        return out['color'], out['depth'], out['final_T'], out['radii']

    @staticmethod
    def backward(ctx, grad_color, grad_depth, grad_T, _r):
        means3D, colors, opacities, scales, rotations, fwd_color, fwd_T, fwd_n = ctx.saved_tensors[:8]
        packed, H, W, bg, scale_modifier = ctx.cam
        fwd = dict(color=fwd_color, final_T=fwd_T, n_contrib=fwd_n)
        if not ctx.depth_grad:
            grad_depth = grad_T = None
        if grad_depth is not None:
            fwd['depth'] = ctx.saved_tensors[8]
        if grad_color is None:
            grad_color = torch.zeros_like(fwd_color)
        g = rasterize_views_backward(grad_color, fwd, means3D, colors, opacities, scales, rotations, None, None, None, None,
                                     H, W, bg, scale_modifier, packed_cameras=packed, grad_depth=grad_depth,
                                     grad_final_T=grad_T)
        grads = (g['means3D'], g['colors'], g['opacities'].reshape(opacities.shape), g['scales'], g['rotations'])
        return tuple(v if n else None for v, n in zip(grads, ctx.needs_input_grad)) + (None,) * 7


def _check_depth_grad(depth_mode, depth_grad):
    """``depth_grad`` as a bool; only the mean depth has a gradient (the median depth is piecewise constant)."""
    if depth_grad and depth_mode != 'mean':
        raise ValueError(f"depth_grad=True needs depth_mode='mean' (the median depth is piecewise constant), "
                         f'got depth_mode={depth_mode!r}')
    return bool(depth_grad)


def rasterize_views_autograd(means3D, colors, opacities, scales, rotations, viewmatrices, projmatrices, tanfovx,
                             tanfovy, image_height, image_width, bg, scale_modifier=1.0, depth_mode='median',
                             depth_grad=False):
    """``rasterize_views`` with autograd through the colour output: returns (color (V,3,H,W),
    depth (V,1,H,W), final_T (V,H,W), radii (V,P)).  ``depth_grad=True`` (needs ``depth_mode='mean'``, else
    ``ValueError``): the mean depth ``D = sum_i alpha_i T_i z_i`` and ``final_T`` are differentiable outputs too.  ``D`` is
    not normalised; a normalised expected depth is ``D / (1 - final_T).clamp_min(eps)``, differentiable in both."""
    H, W = int(image_height), int(image_width)
    packed = pack_cameras(viewmatrices, projmatrices, tanfovx, tanfovy, H, W, means3D.device)
    return _RasterizeViews.apply(means3D, colors, opacities, scales, rotations, packed, H, W, bg, scale_modifier,
                                 depth_mode, depth_grad)


def rasterize_packed_autograd(means3D, colors, opacities, scales, rotations, packed_cameras, image_height, image_width, bg,
                              depth_mode='median', depth_grad=False):
    """``rasterize_views_autograd`` with the cameras given as packed device rows (V,36):
    -> (color (V,3,H,W), depth (V,1,H,W), final_T (V,H,W), radii (V,P)), autograd through the colour and, with
    ``depth_grad=True`` (``depth_mode='mean'``), through the depth and ``final_T``."""
    return _RasterizeViews.apply(means3D, colors, opacities, scales, rotations, packed_cameras, int(image_height),
                                 int(image_width), bg, 1.0, depth_mode, depth_grad)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                        cov3Ds_precomp, raster_settings, depth_mode='median', depth_grad=False):
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales,
                                     rotations, cov3Ds_precomp, raster_settings, depth_mode, depth_grad)


class GaussianRasterizer(nn.Module):
    """``depth_mode`` / ``depth_grad`` are beyond the fork: with ``depth_mode='mean', depth_grad=True`` the third return
    is the differentiable mean depth (the fork's depth has no backward)."""

    def __init__(self, raster_settings, depth_mode='median', depth_grad=False):
        super().__init__()
        self.raster_settings = raster_settings
        self.depth_mode, self.depth_grad = depth_mode, _check_depth_grad(depth_mode, depth_grad)

    def markVisible(self, positions):
        """Near-plane test of ``in_frustum`` (auxiliary.h:139-164): view-space z > 0.2."""
        with torch.no_grad():
            vm = self.raster_settings.viewmatrix.reshape(4, 4).to(positions)
            z = positions[:, 0] * vm[0, 2] + positions[:, 1] * vm[1, 2] + positions[:, 2] * vm[2, 2] + vm[3, 2]
            return z > 0.2

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                rotations=None, cov3D_precomp=None):
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, self.raster_settings, self.depth_mode, self.depth_grad)
