"""Temporal BEV alignment: ``BEVDet4D.gen_grid`` / ``shift_feature`` (mmdet3d/models/detectors/bevdet.py:305-376) and the
``torch.cat`` of the aligned frames in front of the BEV encoder (bevdet.py:529-536, ocrfdet.py:267-274), the step between
``pre_process`` and ``BEVEncoder`` of ``BEVDet4D`` / ``BEVStereo4D`` / ``OcRFDet4D``.

* ``feature_transform``: ``gen_grid``'s ``tf``, the (n, 3, 3) map from a pixel of the key frame's BEV plane to the pixel
  of the adjacent frame's plane that shows the same place, in float64 and in closed form (torch only, no kernel);
* ``shift_feature_torch(input, tf)``: the reference's formulation, a grid and ``F.grid_sample``;
* ``shift_feature(input, tf, out=None, keep_bf16=False)``: the same warp as one HIP launch (``csrc/bev_align.hip``), its
  backward a gather launch without atomics: deterministic;
* ``align_and_cat``: every frame warped (the key frame copied) straight into its channels of one concatenation;
* ``stream_align`` / ``stream_align_torch``: the streaming step's concatenation from a ring of the last key-frame maps
  and the raw poses kept with them, the transforms included, as one HIP launch (``csrc/bev_stream_align.hip``);
  ``keep_bf16=True`` keeps a bfloat16 ring bfloat16 (``ocrf_bev_stream_align_bf16`` / ``stream_align_torch_bf16``);
* ``gen_grid`` / ``shift_feature_method``: the reference's method signatures, adopted by assignment.

Sampling rule of the kernels (include/ocrf_hip.h): with ``t`` the float32 rounding of rows 0 and 1 of ``tf``, output
pixel (row i, column j) samples its source plane at ``sx = fmaf(t00, j, fmaf(t01, i, t02))``,
``sy = fmaf(t10, j, fmaf(t11, i, t12))``, bilinearly, a tap outside the plane read as 0.  That is
``grid_sample(bilinear, zeros, align_corners=True)`` on the reference's normalised grid without the normalise /
unnormalise round trip; ``shift_feature_torch`` makes that round trip and differs by its rounding.

Precondition: the 4 x 4 matrices of ``sensor2keyegos`` have the last row (0, 0, 0, 1), as the dataset's always have.  It
is not checked: a check would synchronise.

The ops never fall back: ``shift_feature`` raises on an input the kernels do not take.  ``align_and_cat`` and
``shift_feature_method`` dispatch: CUDA float32 contiguous maps take the kernels (float16 and bfloat16 maps after
the cast to float32 that the reference's ``@force_fp32`` makes), everything else (the CPU, other dtypes,
non-contiguous maps, poses that require a gradient) the torch formulation.

``keep_bf16=True`` (opt-in; the reference casts) keeps maps that are all bfloat16 as they are: the ``*_bf16`` kernels
read and write bf16, the result and the gradients are bf16, and each is bit for bit the float32 kernel's result on the
widened maps rounded once to nearest even.  Maps that are not all bfloat16 are treated as without the keyword.
"""
import torch
import torch.nn.functional as F

from . import _lib
from .plane_ops import _SUFFIX                   # the suffix of the entry points by the dtype of the maps they take

# Default of the dispatch flag of align_and_cat / shift_feature_method, from the measurement in
# profiles/bev_align_time.txt (tools/time_bev_align.py; INTEGRATION 3g has the table): on (8, 80, 128, 128) maps with 1
# and with 8 warped frames, forward and forward + backward, the kernels are faster than the torch formulation in all four
# cases (1.7x to 2.8x by device time, 1.06x to 1.47x by wall time, the transforms included in both).
FUSED_ALIGN_DEFAULT = True


# ------------------------------------------------------------------------------------------------ the transform
def _affine(bda, pose):
    """``bda4 . pose`` for (n, 3, 3) ``bda`` and (n, 4, 4) ``pose`` with last row (0, 0, 0, 1): its 3 x 3 block and its
    translation."""
    return (torch.einsum('nij,njk->nik', bda, pose[:, :3, :3]), torch.einsum('nij,nj->ni', bda, pose[:, :3, 3]))


def _inverse3(m):
    """Inverse of (n, 3, 3) matrices as adjugate / determinant, elementwise: cofactor (i, j) is
    m[i+1][j+1] m[i+2][j+2] - m[i+1][j+2] m[i+2][j+1] with the indices taken modulo 3."""
    def shifted(di, dj):
        return torch.roll(m, shifts=(-di, -dj), dims=(1, 2))
    cof = shifted(1, 1) * shifted(2, 2) - shifted(1, 2) * shifted(2, 1)
    det = (m[:, 0] * cof[:, 0]).sum(-1)
    return cof.transpose(1, 2) / det[:, None, None]


def _affine_inverse(m):
    """Inverse of (..., 4, 4) float64 affine maps [R t; 0 0 0 1] in closed form: inv(R) from the adjugate, -inv(R) t."""
    lead = m.shape[:-2]
    rinv = _inverse3(m[..., :3, :3].reshape(-1, 3, 3)).view(*lead, 3, 3)
    t = -(rinv * m[..., None, :3, 3]).sum(-1)
    top = torch.cat([rinv, t[..., None]], -1)
    last = torch.zeros_like(m[..., 3:, :])
    last[..., 0, 3] = 1.0
    return torch.cat([top, last], -2)


def _pair(values, like):
    """The first two entries of ``grid_interval`` / ``grid_lower_bound`` as float64: Python floats from a sequence or
    a CPU tensor (the view transformer's attributes), 0-dim tensors of a device tensor (no host read)."""
    if isinstance(values, torch.Tensor) and values.device.type != 'cpu':
        v = values.detach().to(device=like.device, dtype=torch.float64)
        return v[0], v[1]
    return float(values[0]), float(values[1])


def feature_transform(sensor2keyegos, bda, grid_interval, grid_lower_bound, bda_adj=None):
    """``gen_grid``'s ``tf`` (bevdet.py:322-361) for ``sensor2keyegos = [curr (n, v, 4, 4), adj (n, v, 4, 4)]`` (camera 0
    of each is read), ``bda`` (n, 3, 3) and the view transformer's ``grid_interval`` / ``grid_lower_bound``:

        inv(feat2bev) . ((bda4 . curr) . inv(bda_adj4 . adj))[rows, cols (0, 1, 3)] . feat2bev        -> (n, 3, 3) float64

    in float64 and in closed form: the inverse of an affine map from the adjugate of its 3 x 3 block, the conjugation
    with ``feat2bev`` written out.  Elementwise and einsum ops on the device of the poses, no host read, differentiable.
    Precondition: the 4 x 4 matrices have the last row (0, 0, 0, 1).  The reference computes the same in float32 with
    two ``torch.inverse`` calls."""
    curr, adj = sensor2keyegos[0][:, 0].double(), sensor2keyegos[1][:, 0].double()
    bda = bda.to(device=curr.device, dtype=torch.float64)
    bda_adj = bda if bda_adj is None else bda_adj.to(device=curr.device, dtype=torch.float64)
    rc, tc = _affine(bda, curr)
    ra, ta = _affine(bda_adj, adj)
    rm = torch.einsum('nij,njk->nik', rc, _inverse3(ra))          # key ego <- adjacent ego: 3 x 3 block ...
    tm = tc - torch.einsum('nij,nj->ni', rm, ta)                  # ... and translation
    ix, iy = _pair(grid_interval, curr)
    lx, ly = _pair(grid_lower_bound, curr)
    zero, one = torch.zeros_like(tm[:, 0]), torch.ones_like(tm[:, 0])
    # inv(feat2bev) . L . feat2bev, row by row
    off0 = (rm[:, 0, 0] * lx + rm[:, 0, 1] * ly + tm[:, 0] - lx) / ix
    off1 = (rm[:, 1, 0] * lx + rm[:, 1, 1] * ly + tm[:, 1] - ly) / iy
    row0 = torch.stack([rm[:, 0, 0], rm[:, 0, 1] * iy / ix, off0], -1)
    row1 = torch.stack([rm[:, 1, 0] * ix / iy, rm[:, 1, 1], off1], -1)
    return torch.stack([row0, row1, torch.stack([zero, zero, one], -1)], -2)


# ------------------------------------------------------------------------------------------------ torch formulation
def _normalised_grid(tf, h, w, dtype):
    """``gen_grid``'s result from ``tf``: (n, h, w, 2) sample positions normalised to [-1, 1] over (w - 1, h - 1),
    computed in float64 and rounded once to ``dtype``."""
    t = tf.to(torch.float64)
    xs = torch.arange(w, dtype=torch.float64, device=t.device).view(1, 1, w)
    ys = torch.arange(h, dtype=torch.float64, device=t.device).view(1, h, 1)
    sx = t[:, 0, 0, None, None] * xs + t[:, 0, 1, None, None] * ys + t[:, 0, 2, None, None]
    sy = t[:, 1, 0, None, None] * xs + t[:, 1, 1, None, None] * ys + t[:, 1, 2, None, None]
    grid = torch.stack([sx / max(w - 1, 1) * 2.0 - 1.0, sy / max(h - 1, 1) * 2.0 - 1.0], -1)
    return grid.to(dtype)


def shift_feature_torch(input, tf):
    """``shift_feature`` as the reference runs it: the normalised grid of ``tf`` (n, 3, 3), then
    ``F.grid_sample(input, grid, align_corners=True)``.  Any device, any floating dtype, differentiable in both."""
    n, c, h, w = input.shape
    grid = _normalised_grid(tf.to(input.device), h, w, input.dtype)
    return F.grid_sample(input, grid, mode='bilinear', padding_mode='zeros', align_corners=True)


def _shift_feature_torch_bf16(input, tf):
    """``shift_feature_torch`` for a bfloat16 map with a bfloat16 result, as the bf16 kernels compute it: the map widened
    (exact), grid and ``grid_sample`` in float32, the result rounded once.  (A grid in the map's own dtype would round
    the sample positions to bf16: 2^-9 of a half plane, 0.12 pixel at a width of 128.)"""
    with torch.autocast(input.device.type if input.device.type in ('cuda', 'cpu') else 'cuda', enabled=False):
        return shift_feature_torch(input.float(), tf).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ the kernels
_HALVES = (torch.float16, torch.bfloat16)


def _plain(t):
    """A map the kernels take, after the cast of a float16 or bfloat16 one."""
    return (t.is_cuda and t.dtype in (torch.float32, *_HALVES) and t.is_contiguous() and t.dim() == 4
            and t.numel() > 0)


def _cast(t):
    """The reference's ``@force_fp32``: a float16 map, or a bfloat16 one of bf16 autocast, is computed in float32."""
    return t.float() if t.dtype in _HALVES else t


def _tf32(tf, like):
    """(n, 3, 3) float32 contiguous on the device of ``like``, without a gradient: what the kernels read."""
    if tf.dim() != 3 or tuple(tf.shape) != (like.shape[0], 3, 3) or tf.device != like.device:
        raise _lib.OcrfHipError(f'tf must be (n, 3, 3) = ({like.shape[0]}, 3, 3) on {like.device}, got '
                                f'{tuple(tf.shape)} on {tf.device}')
    return tf.detach().to(torch.float32).contiguous()


def _batch_stride(t):
    """Floats between the samples of an (n, c, h, w) view with contiguous (c, h, w) blocks (n = 1: torch's stride of a
    dimension of size 1 means nothing)."""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1] * t.shape[2] * t.shape[3]


def _warp_into(x, tf32, dst):
    """One forward launch: ``x`` (n, c, h, w), float32 or bfloat16, warped into ``dst``, an (n, c, h, w) view of the same
    dtype whose planes are contiguous and whose samples are ``dst.stride(0)`` elements apart."""
    n, c, h, w = x.shape
    _lib.launch('ocrf_bev_align_forward' + _SUFFIX[x.dtype], x.device, n, c, h, w, x, tf32, dst, _batch_stride(dst))


def _gather_from(grad, tf32, shape):
    """One backward launch: the gradient of the source of ``_warp_into`` from ``grad``, addressed like ``dst``, in the
    dtype of ``grad``."""
    n, c, h, w = shape
    grad_x = torch.empty(n, c, h, w, dtype=grad.dtype, device=grad.device)
    _lib.launch('ocrf_bev_align_backward' + _SUFFIX[grad.dtype], grad.device, n, c, h, w, grad, _batch_stride(grad),
                tf32, grad_x)
    return grad_x


def _sliceable(dst, shape, dtype, device):
    """The ``out=`` contract: ``dst`` is an (n, c, h, w) = ``shape`` view of ``dtype`` on ``device`` with contiguous
    (c, h, w) blocks, such as a channel slice of a wider concatenation."""
    n, c, h, w = shape
    return (tuple(dst.shape) == (n, c, h, w) and dst.dtype == dtype and dst.device == device
            and dst.stride()[1:] == (h * w, w, 1) and (n == 1 or dst.stride(0) >= c * h * w))


def _all_bf16(feats):
    return all(x.dtype == torch.bfloat16 for x in feats)


def _check_bf16_grad(grad_out):
    if grad_out.dtype != torch.bfloat16:
        raise _lib.OcrfHipError(f'bev_align backward: grad_out is {grad_out.dtype}, the forward ran in bfloat16')


class _ShiftFeature(torch.autograd.Function):
    """The warp of a float32 or bfloat16 map, the result and the gradient in the map's dtype.

    No ``custom_fwd`` / ``custom_bwd``: ``shift_feature`` is the only caller and hands over a map it has cast already
    (float32, or bfloat16 under ``keep_bf16``) and a float32 ``tf32``, so ``cast_inputs`` has nothing to cast; forward
    and backward consist of ``empty``, ``contiguous`` and the library's launches, none of which autocast changes."""

    @staticmethod
    def forward(ctx, input, tf32):
        out = torch.empty_like(input)
        _warp_into(input, tf32, out)
        ctx.save_for_backward(tf32)
        ctx.shape, ctx.dtype = tuple(input.shape), input.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        tf32, = ctx.saved_tensors
        if ctx.dtype == torch.bfloat16:
            _check_bf16_grad(grad_out)
        return _gather_from(grad_out.contiguous(), tf32, ctx.shape), None


def shift_feature(input, tf, out=None, keep_bf16=False):
    """``shift_feature_torch`` as one HIP launch (``ocrf_bev_align_forward``; backward ``ocrf_bev_align_backward``, a
    gather): ``input`` (n, c, h, w) sampled at ``tf`` (n, 3, 3, any floating dtype, on the device of ``input``; rounded
    to float32).  CUDA float32 contiguous input only, a float16 or bfloat16 one is cast to float32 first
    (``@force_fp32``); anything else raises.  ``tf`` gets no gradient.

    ``out``: an (n, c, h, w) float32 view with contiguous (c, h, w) blocks, such as a channel slice of a wider
    concatenation, to write into; it is returned.  This form records no gradient, so ``input`` must not require one.

    ``keep_bf16``: a bfloat16 ``input`` is not cast: ``ocrf_bev_align_forward_bf16`` / ``_backward_bf16`` read and write
    bf16, the result and the gradient are bf16, and ``out`` must then be a bfloat16 view.  Any other input is treated
    as without it."""
    _lib.require_cuda(input, tf)
    if not _plain(input):
        raise _lib.OcrfHipError('shift_feature takes a non-empty contiguous float32 (or float16 / bfloat16) NCHW map on the '
                                'GPU')
    keep = keep_bf16 and input.dtype == torch.bfloat16
    if not keep:
        input = _cast(input)
    tf32 = _tf32(tf, input)
    if out is None:
        return _ShiftFeature.apply(input, tf32)
    if torch.is_grad_enabled() and input.requires_grad:
        raise _lib.OcrfHipError('shift_feature(out=...) records no gradient: detach the input, or use align_and_cat')
    if not _sliceable(out, input.shape, input.dtype, input.device):
        raise _lib.OcrfHipError(f'out must be a {"bfloat16" if keep else "float32"} (n, c, h, w) view with contiguous '
                                '(c, h, w) blocks on the device of the input')
    _warp_into(input, tf32, out)
    return out


def _align_into(out, tfs, feats):
    """``feats[k]`` copied (``tfs[k]`` None) or warped into its channels of ``out``, all of one dtype."""
    C = feats[0].shape[1]
    for k, (x, tf32) in enumerate(zip(feats, tfs)):
        dst = out[:, k * C:(k + 1) * C]
        if tf32 is None:
            dst.copy_(x)
        else:
            _warp_into(x, tf32, dst)


def _align_grads(ctx, grad_out):
    """The backward of ``_align_into``: the gradients of the frames, in the dtype of ``grad_out``."""
    B, C, H, W = ctx.shape
    grad_out = grad_out.contiguous()
    grads = []
    for k, tf32 in enumerate(ctx.tfs):
        if not ctx.needs_input_grad[1 + k]:
            grads.append(None)                       # the reference computes adjacent frames under no_grad
        elif tf32 is None:
            grads.append(grad_out[:, k * C:(k + 1) * C])
        else:
            grads.append(_gather_from(grad_out[:, k * C:(k + 1) * C], tf32, ctx.shape))
    return (None, *grads)


class _AlignCat(torch.autograd.Function):
    """``tfs[k]`` None: ``feats[k]`` is copied; else warped with it.  One launch per warped frame, each into its channels
    of the result.  The maps are all float32 or all bfloat16; the concatenation and the gradients are of their dtype.

    No ``custom_fwd`` / ``custom_bwd``, for ``_ShiftFeature``'s reason: ``align_and_cat`` is the only caller and casts
    before ``apply``, and ``copy_``, slicing and the launches are not autocast's."""

    @staticmethod
    def forward(ctx, tfs, *feats):
        B, C, H, W = feats[0].shape
        out = torch.empty(B, len(feats) * C, H, W, dtype=feats[0].dtype, device=feats[0].device)
        _align_into(out, tfs, feats)
        ctx.tfs = tfs                                # float32 tensors without a gradient, none of them an input
        ctx.shape, ctx.dtype = (B, C, H, W), out.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.dtype == torch.bfloat16:
            _check_bf16_grad(grad_out)
        return _align_grads(ctx, grad_out)


def align_fusable(feats, tfs):
    """The kernels take these maps: CUDA float32 (or float16 / bfloat16) contiguous, of one shape on one device, and no
    transform that requires a gradient."""
    first = feats[0]
    for x in feats:
        if not (_plain(x) and x.shape == first.shape and x.device == first.device):
            return False
    return not any(tf is not None and tf.requires_grad and torch.is_grad_enabled() for tf in tfs)


def align_and_cat(feats, frame_ids, sensor2keyegos, bda, grid_interval, grid_lower_bound, bda_adj=None, fused=None,
                  keep_bf16=False):
    """The aligned concatenation in front of the BEV encoder: ``feats`` a list of (B, C, H, W) maps, ``frame_ids[k]`` the
    index into the per-frame list ``sensor2keyegos`` of the frame ``feats[k]`` came from.  Frame 0 is the key frame and
    is copied; every other map is warped with ``feature_transform([sensor2keyegos[0], sensor2keyegos[frame_ids[k]]],
    bda, ...)``.  Returns (B, len(feats) * C, H, W).

    ``BEVDet4D`` (bevdet.py:529-536): ``align_and_cat(bev_feat_list, range(num_frame), ...)``; ``OcRFDet4D``
    (ocrfdet.py:267-274), whose list runs from the oldest frame to the key frame:
    ``align_and_cat(bev_feat_list, [num_frame - 2 - k for k in range(num_frame - 2)] + [0], ...)``.

    ``fused`` (default ``FUSED_ALIGN_DEFAULT``): maps that ``align_fusable`` accepts are written by one HIP launch per
    warped frame straight into their channels of the result, without ``torch.cat``; the backward hands a copied frame a
    view of the incoming gradient, runs one gather launch per warped frame that requires a gradient and nothing for one
    that does not.  Everything else takes ``shift_feature_torch`` and ``torch.cat``.

    ``keep_bf16``: maps that are ALL bfloat16 are not cast to float32: the ``*_bf16`` kernels write a bfloat16
    concatenation (the key frame a bf16 copy), the gradients are bfloat16, and the torch formulation runs on the bf16 maps
    too.  Maps that are not all bfloat16 (float16, float32, a mixed list) are treated as without it."""
    frame_ids = [int(f) for f in frame_ids]
    if len(frame_ids) != len(feats) or not feats:
        raise ValueError('align_and_cat takes one frame id per feature map')
    tfs = [None if fid == 0 else feature_transform([sensor2keyegos[0], sensor2keyegos[fid]], bda, grid_interval,
                                                   grid_lower_bound, bda_adj=bda_adj) for fid in frame_ids]
    keep = keep_bf16 and _all_bf16(feats)
    if (FUSED_ALIGN_DEFAULT if fused is None else fused) and align_fusable(feats, tfs):
        if not keep:
            feats = [_cast(x) for x in feats]
        return _AlignCat.apply(tuple(None if tf is None else _tf32(tf, feats[0]) for tf in tfs), *feats)
    if keep:
        return torch.cat([x if tf is None else _shift_feature_torch_bf16(x, tf) for x, tf in zip(feats, tfs)], dim=1)
    return torch.cat([x if tf is None else shift_feature_torch(_cast(x), tf) for x, tf in zip(feats, tfs)], dim=1)


# ------------------------------------------------------------------------------------------------ streaming
def _check_stream_operands(ring, head, valid, sensor2ego0, ego2global0, bda, out):
    if ring.dim() != 5 or ring.numel() == 0:
        raise ValueError(f'ring must be a non-empty (S, B, C, H, W) tensor, got {tuple(ring.shape)}')
    S, B, C, H, W = ring.shape
    if not 0 <= int(head) < S:
        raise ValueError(f'head must be in [0, {S}), got {head}')
    want = dict(valid=(B,), sensor2ego0=(S, B, 4, 4), ego2global0=(S, B, 4, 4), bda=(S, B, 3, 3))
    got = dict(valid=valid, sensor2ego0=sensor2ego0, ego2global0=ego2global0, bda=bda)
    for name, shape in want.items():
        if tuple(got[name].shape) != shape:
            raise ValueError(f'{name} must be {shape}, got {tuple(got[name].shape)}')
        if got[name].device != ring.device:
            raise ValueError(f'{name} is on {got[name].device}, the ring on {ring.device}')
    if valid.dtype.is_floating_point or valid.dtype == torch.bool:
        raise ValueError(f'valid must be an integer tensor, got {valid.dtype}')
    if out is not None and not _sliceable(out, (B, S * C, H, W), ring.dtype, ring.device):
        raise ValueError(f'out must be a {ring.dtype} (B, S * C, H, W) = ({B}, {S * C}, {H}, {W}) view with contiguous '
                         '(S * C, H, W) blocks on the device of the ring')
    return S, B, C, H, W


def stream_align_torch(ring, head, valid, sensor2ego0, ego2global0, bda, grid_interval, grid_lower_bound, align=True,
                       out=None):
    """The streaming step's aligned concatenation in torch, on any device and for any floating dtype; forward only (it
    runs under ``no_grad``), no host read.

    ``ring`` (S, B, C, H, W) holds the last S = K + 1 key-frame BEV maps, slot ``head`` the current one; ``valid`` (B)
    integers, the number of real history frames of each sample; ``sensor2ego0`` / ``ego2global0`` (S, B, 4, 4) and
    ``bda`` (S, B, 3, 3) the raw poses of camera 0 and the BEV augmentation at each slot's time.

    Selection rule: channel group g = 0 .. K - 1 of the result holds age a = K - g, oldest first, group K the key frame.
    For sample b the effective age is ``e = min(a, valid[b])`` and the source slot ``(head - e) mod S``; ``e == 0`` or
    ``align`` false copies the source plane, otherwise it is warped (``shift_feature_torch``) under
    ``feature_transform`` for ``curr = inv(E_h) E_h S_h`` and ``adj = inv(E_h) E_s S_s`` (h the head slot, s the source
    slot) with ``bda[h]`` and ``bda_adj = bda[s]``, evaluated in float64.

    Returns ``(out (B, S * C, H, W), tf (K, B, 3, 3) float32)``: ``tf[g][b]`` is the transform group g of sample b was
    warped with, the identity for a copied group.  ``out``: a view to write into (``shift_feature``'s)."""
    S, B, C, H, W = _check_stream_operands(ring, head, valid, sensor2ego0, ego2global0, bda, out)
    K, head, dev = S - 1, int(head), ring.device
    with torch.no_grad():
        rows = torch.arange(B, device=dev)
        e2g, s2e = ego2global0.double(), sensor2ego0.double()
        # not _affine_inverse: its -(rinv * t).sum(-1) and this einsum differ in float64 bits on the GPU
        head2global = e2g[head]
        rinv = _inverse3(head2global[:, :3, :3])
        global2head = torch.zeros_like(head2global)
        global2head[:, :3, :3], global2head[:, 3, 3] = rinv, 1.0
        global2head[:, :3, 3] = -torch.einsum('nij,nj->ni', rinv, head2global[:, :3, 3])
        curr = global2head @ (head2global @ s2e[head])
        groups, tfs = [], []
        eye = torch.eye(3, dtype=torch.float64, device=dev).expand(B, 3, 3)
        for g in range(K):
            e = torch.clamp(valid.long(), min=0, max=K - g)
            slot = torch.remainder(head - e, S)
            src = ring[slot, rows]
            if not align:
                groups.append(src)
                tfs.append(eye)
                continue
            adj = global2head @ (e2g[slot, rows] @ s2e[slot, rows])
            tf = feature_transform([curr[:, None], adj[:, None]], bda[head], grid_interval, grid_lower_bound,
                                   bda_adj=bda[slot, rows])
            copied = e == 0
            groups.append(torch.where(copied.view(B, 1, 1, 1), src, shift_feature_torch(src, tf)))
            tfs.append(torch.where(copied.view(B, 1, 1), eye, tf))
        groups.append(ring[head])
        tf_out = torch.stack(tfs).float() if K else torch.zeros(0, B, 3, 3, dtype=torch.float32, device=dev)
        if out is None:
            return torch.cat(groups, dim=1), tf_out
        for g, x in enumerate(groups):
            out[:, g * C:(g + 1) * C].copy_(x)
        return out, tf_out


def stream_align_fusable(ring, valid, sensor2ego0, ego2global0, bda, grid_interval, grid_lower_bound,
                         dtype=torch.float32):
    """The kernel takes these: a CUDA contiguous ring of ``dtype`` (float32; bfloat16 for ``ocrf_bev_stream_align_bf16``),
    ``valid`` int32 and float32 contiguous poses on its device, and grid constants on the host (a sequence or a CPU
    tensor: reading a device tensor would synchronise)."""
    if not (ring.is_cuda and ring.dtype == dtype and ring.is_contiguous() and ring.dim() == 5
            and ring.numel() > 0):
        return False
    if not (valid.dtype == torch.int32 and valid.device == ring.device and valid.is_contiguous()):
        return False
    if any(isinstance(v, torch.Tensor) and v.device.type != 'cpu' for v in (grid_interval, grid_lower_bound)):
        return False
    return all(t.dtype == torch.float32 and t.device == ring.device and t.is_contiguous()
               for t in (sensor2ego0, ego2global0, bda))


def stream_align_torch_bf16(ring, head, valid, sensor2ego0, ego2global0, bda, grid_interval, grid_lower_bound,
                            align=True, out=None):
    """``stream_align_torch`` for a bfloat16 ring with a bfloat16 result, as ``ocrf_bev_stream_align_bf16`` computes it:
    the selection and the float64 transforms are ``stream_align_torch``'s, every warped group is
    ``_shift_feature_torch_bf16(src, tf)`` (the map widened, grid and ``grid_sample`` in float32 with autocast off, the
    result rounded once) and a copied group is the bfloat16 source itself.  Any device; forward only."""
    S, B, C, H, W = _check_stream_operands(ring, head, valid, sensor2ego0, ego2global0, bda, out)
    if ring.dtype != torch.bfloat16:
        raise ValueError(f'stream_align_torch_bf16 takes a bfloat16 ring, got {ring.dtype}')
    with torch.no_grad(), torch.autocast(ring.device.type if ring.device.type in ('cuda', 'cpu') else 'cuda',
                                         enabled=False):
        # the widening is exact, the float32 warp rounded once is _shift_feature_torch_bf16, and a widened copied
        # group rounds back to its own bits
        wide, tf_out = stream_align_torch(ring.float(), head, valid, sensor2ego0, ego2global0, bda, grid_interval,
                                          grid_lower_bound, align=align)
        if out is None:
            return wide.to(torch.bfloat16), tf_out
        out.copy_(wide)
        return out, tf_out


def stream_align(ring, head, valid, sensor2ego0, ego2global0, bda, grid_interval, grid_lower_bound, align=True,
                 out=None, fused=None, keep_bf16=False):
    """``stream_align_torch`` with the usual dispatch: operands that ``stream_align_fusable`` accepts take ONE launch of
    ``ocrf_bev_stream_align`` (``csrc/bev_stream_align.hip``), which evaluates the transforms itself and writes every
    group of the concatenation; everything else, the CPU included, the torch formulation.  ``fused`` (default
    ``FUSED_ALIGN_DEFAULT``) False forces the latter.  Forward only: nothing here records a gradient.

    A warped group of the kernel is bit-equal to ``shift_feature(ring[slot], tf[g], out=...)``, the existing kernel fed
    the returned ``tf``; ``tf`` agrees with the torch formulation's within one float32 ulp (both round a float64 value
    once).

    ``keep_bf16`` (opt-in): a bfloat16 ring stays bfloat16.  The result is bfloat16 (``out=`` must then be a bfloat16
    view); CUDA contiguous operands take ONE launch of ``ocrf_bev_stream_align_bf16``, everything else
    ``stream_align_torch_bf16``, which computes as the kernel does.  A warped group of the kernel is bit-equal to
    ``shift_feature(ring[slot], tf[g], keep_bf16=True)`` (the float32 kernel's value on the widened taps, rounded once),
    a copied group a bit copy, ``tf`` bit-equal to the float32 kernel's.  Without the keyword, or with a ring that is
    not bfloat16, the call goes exactly where it goes without it."""
    keep = keep_bf16 and ring.dtype == torch.bfloat16
    dtype = torch.bfloat16 if keep else torch.float32
    if not ((FUSED_ALIGN_DEFAULT if fused is None else fused)
            and stream_align_fusable(ring, valid, sensor2ego0, ego2global0, bda, grid_interval, grid_lower_bound,
                                     dtype=dtype)):
        return (stream_align_torch_bf16 if keep else stream_align_torch)(
            ring, head, valid, sensor2ego0, ego2global0, bda, grid_interval, grid_lower_bound, align=align, out=out)
    S, B, C, H, W = _check_stream_operands(ring, head, valid, sensor2ego0, ego2global0, bda, out)
    if out is None:
        out = torch.empty(B, S * C, H, W, dtype=dtype, device=ring.device)
    tf_out = torch.empty(S - 1, B, 3, 3, dtype=torch.float32, device=ring.device)
    ix, iy = _pair(grid_interval, ring)
    lx, ly = _pair(grid_lower_bound, ring)
    _lib.launch('ocrf_bev_stream_align' + _SUFFIX[dtype], ring.device, S, B, C, H, W, ring, int(head), valid, sensor2ego0, ego2global0,
                bda, ix, iy, lx, ly, 1 if align else 0, out, _batch_stride(out), tf_out)
    return out, tf_out


# ------------------------------------------------------------------------------------------------ drop-in methods
def _method_transform(self, sensor2keyegos, bda, bda_adj):
    vt = self.img_view_transformer
    return feature_transform(sensor2keyegos, bda, vt.grid_interval, vt.grid_lower_bound, bda_adj=bda_adj)


def gen_grid(self, input, sensor2keyegos, bda, bda_adj=None):
    """``BEVDet4D.gen_grid`` (bevdet.py:305-370): the normalised sampling grid (n, h, w, 2) of ``input`` (n, c, h, w),
    from ``feature_transform`` (float64, rounded once to the dtype of ``input``).  Reads
    ``self.img_view_transformer.grid_interval`` / ``grid_lower_bound``."""
    n, c, h, w = input.shape
    return _normalised_grid(_method_transform(self, sensor2keyegos, bda, bda_adj).to(input.device), h, w, input.dtype)


def shift_feature_method(self, input, sensor2keyegos, bda, bda_adj=None):
    """``BEVDet4D.shift_feature`` (bevdet.py:372-376), adopted with ``Detector.shift_feature = shift_feature_method``.
    With ``input`` (num_frame - 1, C, H, W) and poses repeated per frame it is the sequential test's alignment
    (bevdet.py:401-406).  ``self.fused_align`` (default ``FUSED_ALIGN_DEFAULT``) and ``align_fusable`` dispatch;
    ``self.align_keep_bf16`` (default False) is ``shift_feature``'s ``keep_bf16``."""
    tf = _method_transform(self, sensor2keyegos, bda, bda_adj)
    keep = getattr(self, 'align_keep_bf16', False) and input.dtype == torch.bfloat16
    if getattr(self, 'fused_align', FUSED_ALIGN_DEFAULT) and align_fusable([input], [tf]):
        return shift_feature(input, tf.to(input.device), keep_bf16=keep)
    return _shift_feature_torch_bf16(input, tf) if keep else shift_feature_torch(_cast(input), tf)
