"""Generates ``tests/golden/inputs.npz``: the reference's own ``PrepareImageInputs`` and ``LoadAnnotationsBEVDepth``
(mmdet3d/datasets/pipelines/loading.py:796-1258), run on the CPU with the installed Pillow.

    python tests/golden/make_golden_inputs.py

``loading.py`` is imported from where it lies (read-only tree, nothing copied) behind module shells: ``mmcv``,
``pyquaternion``, ``mmdet3d.core.points``, ``mmdet3d.core.bbox``, ``mmdet.datasets.pipelines`` and the ``PIPELINES``
registry as a no-op.  mmcv and cv2 are not dependencies of the tests, so ``mmcv.image.photometric.imnormalize`` is the
float32 expression mmcv hands to cv2: channels reversed, then ``(float32(x) - float32(mean[c])) * float32(1 / float64(std[c]))``.

What is written (``README_inputs.md`` lists the arrays): seeded ``sample_augmentation`` draws in training and test mode
at the reference's data config, ``img_transform``'s ``post_rot`` / ``post_tran`` for them, ``bev_transform`` on five
boxes under all four flip pairs, ``point_label_transform`` on a small point set, and the image stage (lines 1071-1104:
``img_transform_core`` through Pillow, ``mmlabNormalize``) on small seeded images.  The archive is written with fixed
timestamps: it regenerates byte for byte.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261019
# configs/ocrfdet/ocrfdet.py: data_config and bda_aug_conf
DATA_CONFIG = dict(Ncams=6, input_size=(256, 704), src_size=(900, 1600), resize=(-0.06, 0.11), rot=(-5.4, 5.4), flip=True,
                   crop_h=(0.0, 0.0), resize_test=0.00)
BDA_AUG_CONF = dict(rot_lim=(-22.5, 22.5), scale_lim=(0.95, 1.05), flip_dx_ratio=0.5, flip_dy_ratio=0.5)
N_DRAWS = 6
# (source H, W), resize_dims (newW, newH), crop, flip, rotate: an upscale by 1.3, a downscale by 0.5, a downscale whose
# crop runs off the right edge, an unchanged axis, a crop that starts left of and above the image
IMAGE_CASES = [((37, 53), (68, 48), (3, 2, 43, 26), True, 5.4),
               ((90, 160), (80, 45), (5, 10, 69, 42), False, -2.2),
               ((90, 160), (60, 34), (0, 2, 64, 34), True, 0),
               ((64, 64), (64, 80), (0, 10, 48, 50), False, 3.0),
               ((64, 64), (50, 64), (-3, -5, 45, 35), True, -5.4)]
POINT_INPUT_SIZE = (16, 44)


def imnormalize(img, mean, std, to_rgb=True):
    img = img.copy().astype(np.float32)
    mean = np.float64(mean.reshape(1, -1))
    stdinv = 1 / np.float64(std.reshape(1, -1))
    if to_rgb:
        img = img[..., ::-1]
    return (img - mean.astype(np.float32)) * stdinv.astype(np.float32)


def import_loading():
    import _ref_import
    REF = _ref_import.REF
    mod, pkg = _ref_import._mod, _ref_import._pkg
    mod('mmcv')
    mod('mmcv.image')
    mod('mmcv.image.photometric', imnormalize=imnormalize)
    mod('pyquaternion', Quaternion=object)
    mod('mmdet')
    mod('mmdet.datasets')
    mod('mmdet.datasets.pipelines', LoadAnnotations=object, LoadImageFromFile=object)
    pkg('mmdet3d', REF + '/mmdet3d')
    mod('mmdet3d.core')
    mod('mmdet3d.core.points', BasePoints=object, get_points_type=None)
    mod('mmdet3d.core.bbox', LiDARInstance3DBoxes=object)
    pkg('mmdet3d.datasets', REF + '/mmdet3d/datasets')
    mod('mmdet3d.datasets.builder', PIPELINES=_ref_import._Registry())
    pkg('mmdet3d.datasets.pipelines', REF + '/mmdet3d/datasets/pipelines')
    full = 'mmdet3d.datasets.pipelines.loading'
    spec = importlib.util.spec_from_file_location(full, f'{REF}/mmdet3d/datasets/pipelines/loading.py')
    loading = importlib.util.module_from_spec(spec)
    sys.modules[full] = loading
    spec.loader.exec_module(loading)
    return loading


def make_image(case, k):
    (Hs, Ws) = IMAGE_CASES[case][0]
    rng = np.random.RandomState(SEED + 100 * case + k)
    # smooth ramps plus noise: resampling sees gradients, edges and values at both ends of the range
    y, x = np.mgrid[0:Hs, 0:Ws]
    base = np.stack([(x * 255) // max(Ws - 1, 1), (y * 255) // max(Hs - 1, 1), ((x + y) * 7) % 256], -1)
    noise = rng.randint(-90, 91, (Hs, Ws, 3))
    img = np.clip(base + noise, 0, 255)
    img[rng.rand(Hs, Ws) < 0.05] = 255
    img[rng.rand(Hs, Ws) < 0.05] = 0
    return img.astype(np.uint8)


def make_points():
    """(P, 4) float64 source-pixel points for the test-mode augmentation of a 40 x 110 source into 16 x 44, chosen in
    the OUTPUT and mapped back: several on one pixel, coordinates in (-1, 0), exactly W, negative, labels -1, 0, 3."""
    rng = np.random.RandomState(SEED + 7)
    out = np.concatenate([rng.uniform(-3, 47, (40, 1)), rng.uniform(-3, 19, (40, 1))], 1)
    out = np.concatenate([out, [[5.2, 3.1], [5.7, 3.9], [5.4, 3.5], [-0.5, 2.0], [4.0, -0.25], [44.0, 5.0], [43.99, 15.99],
                                [-4.0, -2.0], [10.0, 16.0]]])
    depth = rng.uniform(1, 60, (out.shape[0], 1))
    label = rng.choice([-1.0, 0.0, 3.0], (out.shape[0], 1))
    return np.concatenate([out, depth, label], 1)


def main():
    from PIL import Image
    sys.path.insert(0, HERE)
    from make_golden_bev_encoder import save
    loading = import_loading()
    out = {}
    H, W = DATA_CONFIG['src_size']

    for mode, is_train in (('train', True), ('test', False)):
        prep = loading.PrepareImageInputs(DATA_CONFIG, is_train=is_train)
        np.random.seed(SEED)
        rows, rots, trans = [], [], []
        for _ in range(N_DRAWS if is_train else 1):
            resize, dims, crop, flip, rotate = prep.sample_augmentation(H=H, W=W)
            rows.append([resize, *dims, *crop, float(flip), rotate])
            _, rot, tran = prep.img_transform(Image.new('RGB', (8, 8)), torch.eye(2), torch.zeros(2), resize=resize,
                                              resize_dims=(8, 8), crop=crop, flip=flip, rotate=rotate)
            rots.append(rot.numpy())
            trans.append(tran.numpy())
        out[f'aug.{mode}'] = np.array(rows, np.float64)
        out[f'aug.{mode}.post_rot'], out[f'aug.{mode}.post_tran'] = np.stack(rots), np.stack(trans)
    prep = loading.PrepareImageInputs(DATA_CONFIG, is_train=False)
    resize, dims, crop, flip, rotate = prep.sample_augmentation(H=H, W=W, flip=True, scale=0.5)
    out['aug.test.flip_scale'] = np.array([resize, *dims, *crop, float(flip), rotate], np.float64)

    # bev_transform: five boxes, one drawn augmentation, all four flip pairs
    anno = loading.LoadAnnotationsBEVDepth(BDA_AUG_CONF, classes=None, is_train=True)
    np.random.seed(SEED + 1)
    rotate_bda, scale_bda, flip_dx, flip_dy = anno.sample_bda_augmentation()
    out['bda.draw'] = np.array([rotate_bda, scale_bda, float(flip_dx), float(flip_dy)], np.float64)
    gen = torch.Generator().manual_seed(SEED)
    boxes = torch.cat([40 * torch.rand(5, 3, generator=gen) - 20, 0.5 + 4 * torch.rand(5, 3, generator=gen),
                       6.28 * torch.rand(5, 1, generator=gen) - 3.14, 4 * torch.rand(5, 2, generator=gen) - 2], 1)
    out['bda.boxes'] = boxes.numpy().copy()
    for dx in (False, True):
        for dy in (False, True):
            got, mat = anno.bev_transform(boxes.clone(), rotate_bda, scale_bda, dx, dy)
            out[f'bda.boxes.{int(dx)}{int(dy)}'], out[f'bda.mat.{int(dx)}{int(dy)}'] = got.numpy(), mat.numpy()

    # point labels: output coordinates mapped back through a fixed augmentation of each kind
    prep = loading.PrepareImageInputs(DATA_CONFIG, is_train=True)
    pts_out = make_points()
    augs = [(0.4, (44, 16), (0, 0, 44, 16), False, 0.0), (0.43, (47, 17), (2, 1, 46, 17), True, 3.7),
            (0.37, (40, 14), (-3, -2, 41, 14), False, -5.1)]
    out['points.augs'] = np.array([[a[0], *a[1], *a[2], float(a[3]), a[4]] for a in augs], np.float64)
    for k, (resize, dims, crop, flip, rotate) in enumerate(augs):
        src = pts_out.copy()
        src[:, 0] = (src[:, 0] + crop[0]) / resize           # exact for the unrotated case up to rounding
        src[:, 1] = (src[:, 1] + crop[1]) / resize
        out[f'points.{k}.in'] = src
        depth, semantic = prep.point_label_transform(src.copy(), resize, POINT_INPUT_SIZE, crop, flip, rotate)
        out[f'points.{k}.depth'], out[f'points.{k}.semantic'] = depth.numpy(), semantic.numpy()

    # the image stage, lines 1071-1104 (key frame) for each case, two frames per case
    for case, (_, dims, crop, flip, rotate) in enumerate(IMAGE_CASES):
        for k in range(2):
            src = make_image(case, k)
            img = Image.fromarray(src)
            wo_aug = img.resize(dims).crop(crop)
            aug = prep.img_transform_core(img, dims, crop, flip, rotate)
            out[f'img.{case}.{k}.src'] = src
            out[f'img.{case}.{k}.core'] = np.array(aug)
            out[f'img.{case}.{k}.imgs'] = prep.normalize_img(aug).numpy()
            out[f'img.{case}.{k}.wo_aug'] = prep.normalize_img(np.array(wo_aug)).numpy()
            if flip:
                wo_aug = wo_aug.transpose(method=Image.FLIP_LEFT_RIGHT)
            out[f'img.{case}.{k}.wo_norm'] = torch.tensor(np.array(wo_aug)).float().permute(2, 0, 1).contiguous().numpy()
    import PIL
    out['pillow_version'] = np.array(PIL.__version__)
    path = os.path.join(HERE, 'inputs.npz')
    save(path, out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays, Pillow', PIL.__version__)


if __name__ == '__main__':
    main()
