"""numpy oracles of the input stage (``ocrfdet_amd.inputs``), written from the libraries' own loops and sharing no code
with the package:

* Pillow's ``Image.resize`` (BICUBIC, 8 bits per channel: ``precompute_coeffs``, ``normalize_coeffs_8bpc``, the horizontal
  then the vertical pass with a uint8 intermediate), ``crop``, ``transpose(FLIP_LEFT_RIGHT)`` and ``rotate`` (NEAREST,
  ``affine_fixed``), output by output;
* mmcv's ``imnormalize(img, mean, std, to_rgb=True)`` as the float32 expression
  ``(float32(x) - float32(mean[c])) * float32(1 / float64(std[c]))`` on the channel-reversed array;
* ``point_label_transform`` point by point.

``tests/test_inputs_host.py`` holds the first against the installed Pillow bit for bit.
"""
import math

import numpy as np

MEAN = np.array([123.675, 116.28, 103.53], dtype=np.float32)
STD = np.array([58.395, 57.12, 57.375], dtype=np.float32)


def bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coefficients(in_size, out_size):
    """[(xmin, [k ...])] per output index, the coefficients as integers with 22 fractional bits."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((xmin, [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in w]))
    return out


def resample_axis(img, out_size, axis):
    """One pass over ``axis`` of a uint8 (H, W, 3) image; a pass that keeps the size is skipped."""
    if img.shape[axis] == out_size:
        return img
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for xx, (xmin, k) in enumerate(coefficients(img.shape[axis], out_size)):
        acc = np.full(src.shape[1:], 1 << 21, np.int64)
        for x, kx in enumerate(k):
            acc = acc + src[xmin + x] * kx
        out[xx] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, dims):
    newW, newH = dims
    return resample_axis(resample_axis(img, newW, 1), newH, 0)


def crop(img, box):
    x0, y0, x1, y1 = box
    out = np.zeros((y1 - y0, x1 - x0, 3), np.uint8)
    for y in range(max(y0, 0), min(y1, img.shape[0])):
        for x in range(max(x0, 0), min(x1, img.shape[1])):
            out[y - y0, x - x0] = img[y, x]
    return out


def flip_lr(img):
    return img[:, ::-1]


def rotate(img, angle):
    h, w = img.shape[:2]
    angle = angle % 360.0
    if angle == 0:
        return img.copy()
    an = -math.radians(angle)
    m = [round(math.cos(an), 15), round(math.sin(an), 15), 0.0, round(-math.sin(an), 15), round(math.cos(an), 15), 0.0]
    m[2] = m[0] * (-w / 2.0) + m[1] * (-h / 2.0) + m[2] + w / 2.0
    m[5] = m[3] * (-w / 2.0) + m[4] * (-h / 2.0) + m[5] + h / 2.0
    fix = lambda v: math.floor(v * 65536.0 + 0.5)      # noqa: E731
    a0, a1, a3, a4 = fix(m[0]), fix(m[1]), fix(m[3]), fix(m[4])
    a2, a5 = fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)
    out = np.zeros_like(img)
    for y in range(h):
        for x in range(w):
            xin, yin = (a2 + a1 * y + a0 * x) >> 16, (a5 + a4 * y + a3 * x) >> 16
            if 0 <= xin < w and 0 <= yin < h:
                out[y, x] = img[yin, xin]
    return out


def normalize(img, mean=MEAN, std=STD):
    """(H, W, 3) uint8 RGB -> (3, H, W) float32 as ``mmlabNormalize`` returns it."""
    mean = np.asarray(mean, np.float32)
    stdinv = (1 / np.float64(np.asarray(std, np.float32))).astype(np.float32)
    swapped = img[:, :, ::-1].astype(np.float32)
    return ((swapped - mean) * stdinv).astype(np.float32).transpose(2, 0, 1)


def prepare_image(src, dims, box, flip, angle, mean=MEAN, std=STD):
    """(imgs, imgs_wo_aug, imgs_wo_norm) of one frame, each (3, fH, fW) float32, and the uint8 stages."""
    plain = crop(resize(src, dims), box)
    flipped = flip_lr(plain) if flip else plain
    rotated = rotate(flipped, angle)
    return (normalize(rotated, mean, std), normalize(plain, mean, std),
            flipped.astype(np.float32).transpose(2, 0, 1)), dict(plain=plain, rotated=rotated)


def prepare_images(frames, augs, mean=MEAN, std=STD):
    """``frames`` (M, Hs, Ws, 3) uint8, ``augs``: (resize_dims, crop, flip, rotate) per camera, M / len(augs) frames each.
    Returns the three (M, 3, fH, fW) float32 arrays."""
    per = frames.shape[0] // len(augs)
    outs = [prepare_image(frames[m], *augs[m // per], mean=mean, std=std)[0] for m in range(frames.shape[0])]
    return tuple(np.stack([o[k] for o in outs]) for k in range(3))


def point_label_maps(points, resize, crop, flip, rotate, input_size):
    """One camera: ``points`` (P, 4) float64 -> (depth, semantic), (H, W) float32, written point by point in order."""
    H, W = input_size
    depth, semantic = np.zeros((H, W)), np.zeros((H, W))
    h = rotate / 180 * np.pi
    cos, sin = np.cos(h), np.sin(h)
    for u, v, d, label in points:
        x, y = np.float64(u) * resize, np.float64(v) * resize
        x, y = x - crop[0], y - crop[1]
        if flip:
            x = W - x
        x, y = x - W / 2.0, y - H / 2.0
        x, y = cos * x + sin * y, -sin * x + cos * y
        x, y = x + W / 2.0, y + H / 2.0
        assert abs(x) < 32768 and abs(y) < 32768
        cx, cy = int(x), int(y)                       # toward zero, as astype(int16) inside its range
        if 0 <= cx < W and 0 <= cy < H:
            depth[cy, cx] = d
            semantic[cy, cx] = float(label >= 0)
    return depth.astype(np.float32), semantic.astype(np.float32)


def point_label_maps_matmul(points, resize, crop, flip, rotate, input_size):
    """The same in the reference's array form: ``np.matmul`` with the 2 x 2 rotation, ``astype(np.int16)`` and indexed
    assignment (loading.py:858-891)."""
    p = np.array(points, np.float64)
    H, W = input_size
    p[:, :2] = p[:, :2] * resize
    p[:, 0] -= crop[0]
    p[:, 1] -= crop[1]
    if flip:
        p[:, 0] = input_size[1] - p[:, 0]
    p[:, 0] -= W / 2.0
    p[:, 1] -= H / 2.0
    h = rotate / 180 * np.pi
    p[:, :2] = np.matmul([[np.cos(h), np.sin(h)], [-np.sin(h), np.cos(h)]], p[:, :2].T).T
    p[:, 0] += W / 2.0
    p[:, 1] += H / 2.0
    coords = p[:, :2].astype(np.int16)
    depth, semantic = np.zeros(input_size), np.zeros(input_size)
    ok = (coords[:, 1] < H) & (coords[:, 0] < W) & (coords[:, 1] >= 0) & (coords[:, 0] >= 0)
    depth[coords[ok, 1], coords[ok, 0]] = p[ok, 2]
    semantic[coords[ok, 1], coords[ok, 0]] = p[ok, 3] >= 0
    return depth.astype(np.float32), semantic.astype(np.float32)
