"""The input stage: from decoded camera frames and projected lidar points to ``img_inputs``, ``gt_depth`` and
``gt_semantic`` — what ``PrepareImageInputs`` and ``LoadAnnotationsBEVDepth`` (mmdet3d/datasets/pipelines/loading.py:
796-1258) do on the host with Pillow, mmcv and numpy.

* ``sample_augmentation``, ``post_homography``, ``sample_bda_augmentation``, ``bev_transform``, ``assemble_img_inputs``:
  the small host side, in the reference's operations and order (a seeded run draws the reference's values).
* ``prepare_images``: resize (Pillow BICUBIC), crop, flip, rotate (Pillow NEAREST) and mmcv's normalisation of all
  ``M = B * N * F`` frames in three launches of ``csrc/image_prep.hip``; bit-equal to Pillow, because both resampling
  passes are Pillow's integer arithmetic over coefficient tables built here in float64 as Pillow builds them.
  ``prepare_images_torch``: the same arithmetic in numpy, for the CPU and ``fused=False``.
* ``point_label_maps``: ``point_label_transform`` of all cameras in two launches of ``csrc/point_labels.hip``;
  ``point_label_maps_torch``: the same in numpy.

Not here: JPEG decoding and file I/O, the assembly of poses from quaternions, ``GetBEVMask``,
``PointToMultiViewDepth``, the range and name filters, ``DataContainer`` and ``aug_test``.
"""
import collections
import functools
import math

import numpy as np
import torch

from . import _lib

MEAN = (123.675, 116.28, 103.53)        # loading.py:787-788
STD = (58.395, 57.12, 57.375)
MAX_SOURCE = _lib.OCRF_IMAGE_PREP_MAX_SOURCE
MAX_OUTPUT = _lib.OCRF_IMAGE_PREP_MAX_OUTPUT
_ROW = _lib.OCRF_IMAGE_PREP_ROW
_POINT_ROW = _lib.OCRF_POINT_LABELS_ROW
_ONE = 1 << 22                          # Pillow's PRECISION_BITS = 32 - 8 - 2


# ------------------------------------------------------------------------------------------------ host side
def sample_augmentation(data_config, H, W, is_train, rng=np.random, flip=None, scale=None):
    """``PrepareImageInputs.sample_augmentation`` (loading.py:904-930) for a source of ``H x W``: ``(resize, resize_dims,
    crop, flip, rotate)`` with ``resize_dims = (newW, newH)`` and ``crop = (x0, y0, x1, y1)``.  ``rng``: a
    ``numpy.random.RandomState`` or the ``numpy.random`` module; in training the draws are resize, crop_h, crop_w, flip,
    rotate, in that order."""
    fH, fW = data_config['input_size']
    resize = float(fW) / float(W)
    if is_train:
        resize += rng.uniform(*data_config['resize'])
        newW, newH = resize_dims = (int(W * resize), int(H * resize))
        crop_h = int((1 - rng.uniform(*data_config['crop_h'])) * newH) - fH
        crop_w = int(rng.uniform(0, max(0, newW - fW)))
        flip = data_config['flip'] and rng.choice([0, 1])
        rotate = rng.uniform(*data_config['rot'])
    else:
        resize += data_config.get('resize_test', 0.0)
        if scale is not None:
            resize = scale
        newW, newH = resize_dims = (int(W * resize), int(H * resize))
        crop_h = int((1 - np.mean(data_config['crop_h'])) * newH) - fH
        crop_w = int(max(0, newW - fW) / 2)
        flip = False if flip is None else flip
        rotate = 0
    return resize, resize_dims, (crop_w, crop_h, crop_w + fW, crop_h + fH), flip, rotate


def post_homography(resize, crop, flip, rotate):
    """``post_rot`` (3, 3) and ``post_tran`` (3,) of one camera, float32: the image-plane map of the augmentation as
    ``img_transform`` accumulates it (loading.py:828-847) and ``get_inputs`` embeds it (:1094-1097) — float32 torch
    operations in the reference's order."""
    post_rot = torch.eye(2)
    post_tran = torch.zeros(2)
    post_rot *= resize
    post_tran -= torch.Tensor(crop[:2])
    if flip:
        A = torch.Tensor([[-1, 0], [0, 1]])
        b = torch.Tensor([crop[2] - crop[0], 0])
        post_rot = A.matmul(post_rot)
        post_tran = A.matmul(post_tran) + b
    h = rotate / 180 * np.pi
    A = torch.Tensor([[np.cos(h), np.sin(h)], [-np.sin(h), np.cos(h)]])
    b = torch.Tensor([crop[2] - crop[0], crop[3] - crop[1]]) / 2
    b = A.matmul(-b) + b
    post_rot = A.matmul(post_rot)
    post_tran = A.matmul(post_tran) + b
    rot3, tran3 = torch.eye(3), torch.zeros(3)
    rot3[:2, :2] = post_rot
    tran3[:2] = post_tran
    return rot3, tran3


def sample_bda_augmentation(bda_aug_conf, is_train, rng=np.random):
    """``LoadAnnotationsBEVDepth.sample_bda_augmentation`` (loading.py:1214-1226): ``(rotate_bda, scale_bda, flip_dx,
    flip_dy)``; in training four draws in that order."""
    if not is_train:
        return 0, 1.0, False, False
    rotate_bda = rng.uniform(*bda_aug_conf['rot_lim'])
    scale_bda = rng.uniform(*bda_aug_conf['scale_lim'])
    flip_dx = rng.uniform() < bda_aug_conf['flip_dx_ratio']
    flip_dy = rng.uniform() < bda_aug_conf['flip_dy_ratio']
    return rotate_bda, scale_bda, flip_dx, flip_dy


def bev_transform(gt_boxes, rotate_angle, scale_ratio, flip_dx, flip_dy):
    """``LoadAnnotationsBEVDepth.bev_transform`` (loading.py:1228-1258): the boxes (n, 9) float32 (centre, size, yaw,
    velocity) under the BEV augmentation, and the 3 x 3 ``bda``.  The boxes are transformed in place and returned, as the
    reference does."""
    angle = torch.tensor(rotate_angle / 180 * np.pi)
    sin, cos = torch.sin(angle), torch.cos(angle)
    rot_mat = torch.Tensor([[cos, -sin, 0], [sin, cos, 0], [0, 0, 1]])
    scale_mat = torch.Tensor([[scale_ratio, 0, 0], [0, scale_ratio, 0], [0, 0, scale_ratio]])
    flip_mat = torch.Tensor([[1, 0, 0], [0, 1, 0], [0, 0, 1]])
    if flip_dx:
        flip_mat = flip_mat @ torch.Tensor([[-1, 0, 0], [0, 1, 0], [0, 0, 1]])
    if flip_dy:
        flip_mat = flip_mat @ torch.Tensor([[1, 0, 0], [0, -1, 0], [0, 0, 1]])
    bda = flip_mat @ (scale_mat @ rot_mat)
    if gt_boxes.shape[0] > 0:
        gt_boxes[:, :3] = (bda @ gt_boxes[:, :3].unsqueeze(-1)).squeeze(-1)
        gt_boxes[:, 3:6] *= scale_ratio
        gt_boxes[:, 6] += angle
        if flip_dx:
            gt_boxes[:, 6] = 2 * torch.asin(torch.tensor(1.0)) - gt_boxes[:, 6]
        if flip_dy:
            gt_boxes[:, 6] = -gt_boxes[:, 6]
        gt_boxes[:, 7:] = (bda[:2, :2] @ gt_boxes[:, 7:].unsqueeze(-1)).squeeze(-1)
    return gt_boxes, bda


def assemble_img_inputs(imgs, imgs_wo_norm, imgs_wo_aug, rots, trans, intrins, post_rots, post_trans, bda, sensor2egos,
                        ego2globals, c2w):
    """The 12-entry ``img_inputs`` in the order ``detector.prepare_inputs`` takes: ``[imgs, rots, trans, intrins,
    post_rots, post_trans, bda, sensor2egos, ego2globals, imgs_wo_norm, imgs_wo_aug, c2w]``.

    The images are what ``prepare_images`` returns, (B * N * F, 3, H, W) or already (B, N * F, 3, H, W): camera-major, a
    camera's key frame first and then its adjacent frames.  The poses arrive as matrices per frame and camera,
    frame-major: ``rots`` (B, F * N, 3, 3), ``trans`` (B, F * N, 3), ``sensor2egos``, ``ego2globals`` and ``c2w``
    (B, F * N, 4, 4).  ``intrins``, ``post_rots`` (B, N, 3, 3) and ``post_trans`` (B, N, 3) belong to the cameras and are
    repeated over the frames, as loading.py:1134-1138 does.  ``bda`` is (B, 3, 3)."""
    if bda.dim() != 3 or tuple(bda.shape[1:]) != (3, 3):
        raise ValueError(f'bda is (B, 3, 3), got {tuple(bda.shape)}')
    B = bda.shape[0]
    if intrins.dim() != 4 or intrins.shape[0] != B or tuple(intrins.shape[2:]) != (3, 3):
        raise ValueError(f'intrins is (B, N, 3, 3), got {tuple(intrins.shape)}')
    N = intrins.shape[1]
    if rots.dim() != 4 or rots.shape[0] != B or rots.shape[1] % N or tuple(rots.shape[2:]) != (3, 3):
        raise ValueError(f'rots is (B, F * N, 3, 3) with N = {N}, got {tuple(rots.shape)}')
    F = rots.shape[1] // N
    for name, t, shape in (('trans', trans, (B, F * N, 3)), ('post_rots', post_rots, (B, N, 3, 3)),
                           ('post_trans', post_trans, (B, N, 3)), ('sensor2egos', sensor2egos, (B, F * N, 4, 4)),
                           ('ego2globals', ego2globals, (B, F * N, 4, 4)), ('c2w', c2w, (B, F * N, 4, 4))):
        if tuple(t.shape) != shape:
            raise ValueError(f'{name} is {shape} for B = {B}, N = {N}, F = {F}, got {tuple(t.shape)}')
    images = []
    for name, t in (('imgs', imgs), ('imgs_wo_norm', imgs_wo_norm), ('imgs_wo_aug', imgs_wo_aug)):
        if t.dim() == 4 and t.shape[0] == B * N * F:
            t = t.reshape(B, N * F, *t.shape[1:])
        if t.dim() != 5 or t.shape[0] != B or t.shape[1] != N * F or t.shape[2] != 3 or t.shape[3:] != imgs.shape[-2:]:
            raise ValueError(f'{name} holds B * N * F = {B * N * F} images of 3 x H x W, got {tuple(t.shape)}')
        images.append(t)
    per_frame = lambda t: t.repeat(1, F, *([1] * (t.dim() - 2)))      # noqa: E731  (frame-major: all cameras, F times)
    return [images[0], rots, trans, per_frame(intrins), per_frame(post_rots), per_frame(post_trans), bda, sensor2egos,
            ego2globals, images[1], images[2], c2w]


# ------------------------------------------------------------------------------------------------ Pillow's tables
def _bicubic(t):
    """Pillow's ``bicubic_filter`` (a = -0.5) on a float64 array."""
    a = -0.5
    t = np.abs(t)
    near = ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    far = (((t - 5) * t + 8) * t - 4) * a
    return np.where(t < 1.0, near, np.where(t < 2.0, far, 0.0))


@functools.lru_cache(maxsize=256)
def resample_table(in_size, out_size):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for BICUBIC over one axis ``in_size -> out_size``:
    ``(ksize, bounds, kk)`` with ``bounds`` (out_size, 2) int32 = (first source index, tap count) and ``kk`` (out_size,
    ksize) int32 with 22 fractional bits, zero behind the tap count.  float64 throughout, the weights summed left to
    right.  An axis that keeps its size is not resampled by Pillow: the one-tap table with coefficient 2^22, which copies."""
    if in_size == out_size:
        bounds = np.stack([np.arange(out_size), np.ones(out_size, np.int64)], 1).astype(np.int32)
        return 1, bounds, np.full((out_size, 1), _ONE, np.int32)
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # the cast truncates, as (int) does
    n = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    ss = 1.0 / filterscale
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = _bicubic((x + xmin[:, None] - center[:, None] + 0.5) * ss)
    w = np.where(np.arange(ksize)[None, :] < n[:, None], w, 0.0)
    ww = np.zeros(out_size)
    for t in range(ksize):                                                   # left to right, not pairwise
        ww = ww + w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    kk = np.where(w < 0, -0.5 + w * _ONE, 0.5 + w * _ONE).astype(np.int64)   # toward zero
    return ksize, np.stack([xmin, n], 1).astype(np.int32), kk.astype(np.int32)


def rotate_coefficients(angle, w, h):
    """``Image.rotate(angle)`` (NEAREST, no expand) on a ``w x h`` image as Pillow's ``affine_fixed`` runs it: ``None``
    for a copy (``angle % 360 == 0``), else ``(a0, ..., a5)`` in 16.16 fixed point, the source of output (x, y) being
    ``((a2 + a1 y + a0 x) >> 16, (a5 + a4 y + a3 x) >> 16)``."""
    angle = angle % 360.0
    if angle == 0:
        return None
    an = -math.radians(angle)
    m = [round(math.cos(an), 15), round(math.sin(an), 15), 0.0, round(-math.sin(an), 15), round(math.cos(an), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + 0.0
    m[5] = m[3] * -cx + m[4] * -cy + 0.0
    m[2] += cx
    m[5] += cy
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))      # noqa: E731
    return (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]),
            fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def _aug4(aug):
    """``(resize_dims, crop, flip, rotate)`` of an augmentation given as that or as ``sample_augmentation``'s 5-tuple, in
    plain Python numbers."""
    aug = tuple(aug)
    if len(aug) == 5:
        aug = aug[1:]
    if len(aug) != 4:
        raise ValueError('an augmentation is (resize_dims, crop, flip, rotate) or (resize, resize_dims, crop, flip, rotate)')
    dims, crop, flip, rotate = aug
    dims, crop = tuple(int(v) for v in dims), tuple(int(v) for v in crop)
    if len(dims) != 2 or len(crop) != 4 or min(dims) <= 0:
        raise ValueError(f'resize_dims is (newW, newH) > 0 and crop (x0, y0, x1, y1), got {dims} and {crop}')
    rotate = float(rotate)
    if not abs(rotate) < 90:
        raise ValueError(f'|rotate| < 90 (Pillow transposes at 90, 180 and 270 instead of resampling), got {rotate}')
    return dims, crop, bool(flip), rotate


def _check_images(frames, augs, input_size):
    if frames.dtype != torch.uint8:
        raise TypeError(f'frames are uint8 (decoded RGB), got {frames.dtype}')
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] == 0:
        raise ValueError(f'frames are (M, Hs, Ws, 3), got {tuple(frames.shape)}')
    if not frames.is_contiguous():
        raise ValueError('frames are contiguous')
    M, Hs, Ws = frames.shape[:3]
    if max(Hs, Ws) > MAX_SOURCE:
        raise ValueError(f'a source side is at most {MAX_SOURCE} pixels, got {Hs} x {Ws}')
    fH, fW = (int(v) for v in input_size)
    if not (0 < fH <= MAX_OUTPUT and 0 < fW <= MAX_OUTPUT):
        raise ValueError(f'input_size sides are 1 ... {MAX_OUTPUT}, got {(fH, fW)}')
    augs = tuple(_aug4(a) for a in augs)
    if not augs or M % len(augs):
        raise ValueError(f'{M} frames are not the same number of frames for each of {len(augs)} augmentations')
    for dims, crop, _, _ in augs:
        if (crop[2] - crop[0], crop[3] - crop[1]) != (fW, fH):
            raise ValueError(f'crop {crop} is not input_size {(fH, fW)}')
        if max(dims) > MAX_SOURCE:
            raise ValueError(f'a resized side is at most {MAX_SOURCE} pixels, got {dims}')
    return augs, M, Hs, Ws, fH, fW


def _norm_constants(mean, std):
    """float32 ``mean`` and ``1 / float64(std)`` rounded to float32: what cv2.subtract / cv2.multiply receive from
    mmcv's ``imnormalize``."""
    mean = np.asarray(mean, np.float32)
    stdinv = (1 / np.float64(np.asarray(std, np.float32))).astype(np.float32)
    if mean.shape != (3,) or stdinv.shape != (3,):
        raise ValueError('mean and std have three entries')
    return mean, stdinv


# ------------------------------------------------------------------------------------------------ images, numpy
def _resample(img, table, axis):
    """One Pillow pass over ``axis`` of the uint8 image (H, W, 3) in int32."""
    ksize, bounds, kk = table
    size = img.shape[axis]
    acc = np.full((bounds.shape[0] if axis == 0 else img.shape[0], bounds.shape[0] if axis == 1 else img.shape[1], 3),
                  1 << 21, np.int32)
    src = img.astype(np.int32)
    for t in range(ksize):
        idx = np.minimum(bounds[:, 0] + t, size - 1)       # behind the tap count the coefficient is zero
        if axis == 1:
            acc += src[:, idx, :] * kk[None, :, t, None]
        else:
            acc += src[idx, :, :] * kk[:, t, None, None]
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def _crop_resized(src, dims, crop):
    """``Image.resize(dims).crop(crop)`` of the uint8 image ``src`` (Hs, Ws, 3)."""
    newW, newH = dims
    img = _resample(src, resample_table(src.shape[1], newW), 1)        # horizontal first, a uint8 intermediate
    img = _resample(img, resample_table(src.shape[0], newH), 0)
    x0, y0, x1, y1 = crop
    out = np.zeros((y1 - y0, x1 - x0, 3), np.uint8)
    xa, xb, ya, yb = max(x0, 0), min(x1, newW), max(y0, 0), min(y1, newH)
    if xa < xb and ya < yb:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = img[ya:yb, xa:xb]
    return out


def _rotate(img, rotate):
    coef = rotate_coefficients(rotate, img.shape[1], img.shape[0])
    if coef is None:
        return img
    a0, a1, a2, a3, a4, a5 = coef
    y, x = np.mgrid[0:img.shape[0], 0:img.shape[1]].astype(np.int64)
    xin, yin = (a2 + a1 * y + a0 * x) >> 16, (a5 + a4 * y + a3 * x) >> 16
    ok = (xin >= 0) & (xin < img.shape[1]) & (yin >= 0) & (yin < img.shape[0])
    out = np.zeros_like(img)
    out[ok] = img[yin[ok], xin[ok]]
    return out


def prepare_images_torch(frames, augs, input_size, mean=MEAN, std=STD):
    """``prepare_images`` in numpy, image by image: the same tables and the same integer passes.  Takes and returns
    tensors on ``frames.device``."""
    augs, M, _, _, fH, fW = _check_images(frames, augs, input_size)
    mean, stdinv = _norm_constants(mean, std)
    F = M // len(augs)
    host = frames.cpu().numpy()
    outs = np.empty((3, M, 3, fH, fW), np.float32)
    normalise = lambda a: ((a[:, :, ::-1].astype(np.float32) - mean) * stdinv).transpose(2, 0, 1)   # noqa: E731
    for m in range(M):
        dims, crop, flip, rotate = augs[m // F]
        plain = _crop_resized(host[m], dims, crop)
        flipped = plain[:, ::-1] if flip else plain
        outs[0, m] = normalise(_rotate(flipped, rotate))
        outs[1, m] = normalise(plain)
        outs[2, m] = flipped.astype(np.float32).transpose(2, 0, 1)
    return tuple(torch.from_numpy(o).to(frames.device) for o in outs)


# ------------------------------------------------------------------------------------------------ images, HIP
def _window(table, first, count, size):
    """The part of a resampling table the crop window ``[first, first + count)`` of an axis of ``size`` resized pixels
    reads: bounds (count, 2) and coefficients (count, ksize), entries outside the resized image with no taps."""
    ksize, bounds, kk = table
    pos = np.arange(first, first + count)
    ok = (pos >= 0) & (pos < size)
    idx = np.clip(pos, 0, size - 1)
    return np.where(ok[:, None], bounds[idx], 0).astype(np.int32), np.where(ok[:, None], kk[idx], 0).astype(np.int32)


@functools.lru_cache(maxsize=16)
def _image_table(augs, Hs, Ws, fH, fW):
    """The device table of one call (``include/ocrf_hip.h``: ``ocrf_image_prep``) as an int32 array, and the number of
    rows the intermediate needs."""
    rows, blocks, offset, r_max = [], [], len(augs) * _ROW, 1
    for (newW, newH), crop, flip, rotate in augs:
        h_table, v_table = resample_table(Ws, newW), resample_table(Hs, newH)
        hb, hk = _window(h_table, crop[0], fW, newW)
        vb, vk = _window(v_table, crop[1], fH, newH)
        used = vb[:, 1] > 0
        r0 = int(vb[used, 0].min()) if used.any() else 0
        r1 = int((vb[used, 0] + vb[used, 1]).max()) if used.any() else 0
        r_max = max(r_max, r1 - r0)
        coef = rotate_coefficients(rotate, fW, fH)
        row = [r0, r1 - r0]
        # the horizontal coefficients tap-major: the threads of a wave own adjacent columns
        for part, ksize in ((hb, None), (np.ascontiguousarray(hk.T), h_table[0]), (vb, None), (vk, v_table[0])):
            row.append(offset)
            if ksize is not None:
                row.append(ksize)
            blocks.append(part.reshape(-1))
            offset += part.size
        row += [int(flip), int(coef is None)] + list(coef or (0,) * 6)
        assert len(row) == _ROW
        rows.append(np.asarray(row, np.int64))
    return np.concatenate([np.concatenate(rows).astype(np.int32)] + blocks), r_max


@functools.lru_cache(maxsize=16)
def _pinned_image_table(augs, Hs, Ws, fH, fW):
    """``_image_table`` in pinned memory: an unchanged augmentation (testing) costs one copy per call."""
    table, r_max = _image_table(augs, Hs, Ws, fH, fW)
    pinned = torch.empty(table.size, dtype=torch.int32, pin_memory=True)
    pinned.copy_(torch.from_numpy(table))
    return pinned, r_max


def prepare_images(frames, augs, input_size, mean=MEAN, std=STD, fused=True):
    """The image stage of ``PrepareImageInputs`` (loading.py:1071-1123) for a whole batch.

    ``frames`` (M, Hs, Ws, 3) uint8 RGB, contiguous, ``M = B * N * F`` camera-major (a camera's key frame, then its
    adjacent frames).  ``augs``: one ``(resize_dims, crop, flip, rotate)`` per (b, n) — or ``sample_augmentation``'s
    5-tuple — shared by that camera's ``F`` frames.  ``input_size = (fH, fW)`` is the crop's size.  Returns ``imgs``,
    ``imgs_wo_aug``, ``imgs_wo_norm``, each (M, 3, fH, fW) float32:

    * ``imgs`` = normalise(rotate(flip(crop(resize(frame)))))
    * ``imgs_wo_aug`` = normalise(crop(resize(frame)))
    * ``imgs_wo_norm`` = float(flip(crop(resize(frame)))), RGB

    with Pillow's ``resize`` (BICUBIC), ``crop``, ``transpose(FLIP_LEFT_RIGHT)`` and ``rotate`` (NEAREST), bit for bit,
    and ``normalise`` = mmcv's ``imnormalize(to_rgb=True)`` on the RGB array: output channel c is ``(float32(rgb[2 - c])
    - float32(mean[c])) * float32(1 / float64(std[c]))``.

    CUDA frames with ``fused=True`` take ``ocrf_image_prep``: three launches whatever ``M`` is, no host read; the
    per-camera parameters and coefficient tables (built in float64 on the host, cached by size pair) go up as one
    non-blocking copy.  Anything else takes ``prepare_images_torch``.  Raises on a dtype other than uint8, non-contiguous
    frames, a side above 32767 pixels and ``|rotate| >= 90``."""
    if not (fused and frames.is_cuda):
        return prepare_images_torch(frames, augs, input_size, mean, std)
    augs, M, Hs, Ws, fH, fW = _check_images(frames, augs, input_size)
    if M > 65535:
        raise ValueError(f'at most 65535 frames per call, got {M}')
    mean, stdinv = _norm_constants(mean, std)
    dev = frames.device
    pinned, r_max = _pinned_image_table(augs, Hs, Ws, fH, fW)
    table = pinned.to(dev, non_blocking=True)
    scratch = _lib.workspace.get(dev, M * (r_max + fH) * fW * 3, 'image_prep')
    tmp, crop = scratch, scratch[M * r_max * fW * 3:]
    imgs, wo_aug, wo_norm = torch.empty(3, M, 3, fH, fW, dtype=torch.float32, device=dev).unbind(0)
    _lib.launch('ocrf_image_prep', dev, M, M // len(augs), Hs, Ws, fH, fW, r_max, frames, table, table.numel(), tmp, crop,
                *(float(v) for v in mean), *(float(v) for v in stdinv), imgs, wo_aug, wo_norm)
    return imgs, wo_aug, wo_norm


# ------------------------------------------------------------------------------------------------ point labels
def _point_rows(augs):
    """(cameras, 8) float64: resize, crop[0], crop[1], flip, cos, sin of ``rotate / 180 * pi`` (numpy's), 0, 0."""
    rows = np.zeros((len(augs), _POINT_ROW))
    for k, aug in enumerate(augs):
        if len(aug) != 5:
            raise ValueError('point labels take (resize, resize_dims, crop, flip, rotate) per camera')
        resize, _, crop, flip, rotate = aug
        h = rotate / 180 * np.pi
        rows[k, :6] = (resize, crop[0], crop[1], 1.0 if flip else 0.0, np.cos(h), np.sin(h))
    return rows


def _check_points(points, counts, augs, input_size):
    if points.dtype != torch.float64:
        raise TypeError(f'points are float64, as the reference transforms them, got {points.dtype}')
    if points.dim() != 3 or points.shape[2] != 4 or points.shape[0] != len(augs) or not len(augs):
        raise ValueError(f'points are (cameras, P, 4) with one augmentation per camera, got {tuple(points.shape)} and '
                         f'{len(augs)} augmentations')
    if counts.dtype != torch.int32 or tuple(counts.shape) != (points.shape[0],):
        raise ValueError(f'counts are int32 (cameras,), got {counts.dtype} {tuple(counts.shape)}')
    if not (points.is_contiguous() and counts.is_contiguous()):
        raise ValueError('points and counts are contiguous')
    H, W = (int(v) for v in input_size)
    if not (0 < H <= MAX_OUTPUT and 0 < W <= MAX_OUTPUT):
        raise ValueError(f'input_size sides are 1 ... {MAX_OUTPUT}, got {(H, W)}')
    return H, W


def point_label_maps_torch(points, counts, augs, input_size):
    """``point_label_maps`` in numpy, camera by camera.  Refuses a coordinate of magnitude 32768 or more."""
    H, W = _check_points(points, counts, augs, input_size)
    rows = _point_rows(augs)
    host, n = points.cpu().numpy(), counts.cpu().numpy()
    depth, semantic = np.zeros((2, len(augs), H, W))
    for k, (resize, cx, cy, flip, cos, sin) in enumerate(rows[:, :6]):
        pts = host[k, :min(int(n[k]), host.shape[1])]
        x, y = pts[:, 0] * resize - cx, pts[:, 1] * resize - cy
        if flip:
            x = W - x
        x, y = x - W / 2.0, y - H / 2.0
        u, v = (cos * x + sin * y) + W / 2.0, ((-sin) * x + cos * y) + H / 2.0
        if not (np.all(np.abs(u) < 32768) and np.all(np.abs(v) < 32768)):
            raise ValueError('a transformed coordinate is not inside (-32768, 32768), where astype(int16) truncates')
        u, v = u.astype(np.int64), v.astype(np.int64)            # toward zero
        ok = (v < H) & (u < W) & (v >= 0) & (u >= 0)
        for i in np.nonzero(ok)[0]:                              # in order: the last point on a pixel wins
            depth[k, v[i], u[i]] = pts[i, 2]
            semantic[k, v[i], u[i]] = pts[i, 3] >= 0
    return (torch.from_numpy(depth.astype(np.float32)).to(points.device),
            torch.from_numpy(semantic.astype(np.float32)).to(points.device))


_WINNERS = collections.OrderedDict()       # (device index, cameras, H, W) -> the int32 plane, all zero between calls


def point_label_maps(points, counts, augs, input_size, fused=True):
    """``PrepareImageInputs.point_label_transform`` (loading.py:858-891) for all cameras: ``gt_depth`` and
    ``gt_semantic``, each (B * N, H, W) float32 with ``(H, W) = input_size``.

    ``points`` (B * N, P, 4) float64: (u, v, depth, label) in source pixels, padded to ``P``; ``counts`` (B * N,) int32:
    the real length of each row.  ``augs``: ``sample_augmentation``'s ``(resize, resize_dims, crop, flip, rotate)`` per
    camera.  float64 arithmetic in the reference's order; the flip mirrors about ``input_size[1]``, as the reference's
    ``resize_dims[1] - x`` does when it is called with ``resize_dims = input_size``; coordinates truncate toward zero, so
    a value in (-1, 0) lands on pixel 0; the last point written to a pixel wins in both maps; semantic is ``label >= 0``.

    CUDA points with ``fused=True`` take ``ocrf_point_labels``: two launches, an integer ``atomicMax`` over point indices
    and a resolving pass, deterministic, no host read.  Anything else takes ``point_label_maps_torch``.

    Precondition: every transformed coordinate lies inside (-32768, 32768), where numpy's ``astype(int16)`` is a plain
    truncation.  The numpy path refuses anything else; the kernel cannot tell the host and drops such a point."""
    if not (fused and points.is_cuda):
        return point_label_maps_torch(points, counts, augs, input_size)
    H, W = _check_points(points, counts, augs, input_size)
    if not counts.is_cuda:
        raise _lib.OcrfHipError('counts lives on the device of points')
    dev, cams = points.device, points.shape[0]
    if cams > 65535:
        raise ValueError(f'at most 65535 cameras per call, got {cams}')
    rows = torch.from_numpy(_point_rows(augs)).pin_memory().to(dev, non_blocking=True)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), cams, H, W)
    winner = _WINNERS.get(key)
    if winner is None:
        while len(_WINNERS) >= 4:
            _WINNERS.popitem(last=False)
        winner = _WINNERS[key] = torch.zeros(cams, H, W, dtype=torch.int32, device=dev)
    depth, semantic = torch.empty(2, cams, H, W, dtype=torch.float32, device=dev).unbind(0)
    _lib.launch('ocrf_point_labels', dev, cams, points.shape[1], H, W, points, counts, rows, winner, depth, semantic)
    return depth, semantic
