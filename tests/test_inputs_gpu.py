"""GPU: ``ocrf_image_prep`` and ``ocrf_point_labels`` against the numpy oracles of ``tests/inputs_oracle.py``, bit for bit,
and their structure: three launches for the images and two for the labels whatever the batch, no host synchronisation."""
import numpy as np
import pytest
import torch

from ocrfdet_amd import inputs

from tests import inputs_oracle as oracle
from tests import test_inputs_host as host

pytestmark = pytest.mark.gpu
GI = host.GI
FH, FW = 24, 40
NAMES = ('imgs', 'imgs_wo_aug', 'imgs_wo_norm')


def device_kernels(fn):
    """(result, names of the kernels launched) of ``fn()`` under torch's sync debug mode 'error'."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'kernel' in e.name.lower()]


def check_images(cuda, frames, augs, size=(FH, FW)):
    want = oracle.prepare_images(frames, augs)
    got = inputs.prepare_images(torch.from_numpy(frames).to(cuda), augs, size)
    torch.cuda.synchronize()
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == w.shape, name
        g = g.cpu().numpy()
        assert np.array_equal(g, w), f'{name}: {(g != w).sum()} of {w.size} values differ, max {np.abs(g - w).max()}'
    return got


# The cases of tests/golden/make_golden_inputs.py: 37 x 53 upscaled x 1.3 (ksize 5) with flip and rotate +5.4; 90 x 160
# downscaled x 0.5 with rotate -2.2; a downscale to newW = 60 < fW = 64, where the crop runs off the right edge; 64 x 64
# with the horizontal size unchanged (that pass is skipped) and rotate 3; a crop that starts left of and above the image
@pytest.mark.parametrize('case', range(len(host.CASES)))
def test_images_equal_the_oracle_bit_for_bit(cuda, case):
    _, dims, crop, flip, rotate = host.CASES[case]
    frames = np.stack([GI.make_image(case, k) for k in range(2)])
    check_images(cuda, frames, [(dims, crop, flip, rotate)], (crop[3] - crop[1], crop[2] - crop[0]))


def two_camera_call(pair):
    """Two cameras x two frames of one source size with different augmentations, cropped to FH x FW."""
    augs = []
    for c in pair:
        _, dims, crop, flip, rotate = host.CASES[c]
        augs.append((dims, (crop[0], crop[1], crop[0] + FW, crop[1] + FH), flip, rotate))
    frames = np.stack([GI.make_image(c, k) for c in pair for k in range(2)])
    return frames, augs


@pytest.mark.parametrize('pair', [(1, 2), (3, 4)])
def test_cameras_with_different_augmentations_in_one_call(cuda, pair):
    """M = 2 cameras x 2 frames: (x 0.5, rotate -2.2, no flip) next to (x 0.375, rotate 0, flip); (unchanged axis, rotate
    3) next to (negative crop origin: zeros on the left and on top, flip, rotate -5.4).  The second call hits the table
    cache."""
    frames, augs = two_camera_call(pair)
    first = check_images(cuda, frames, augs)
    hits = inputs._pinned_image_table.cache_info().hits
    second = check_images(cuda, frames, augs)
    assert inputs._pinned_image_table.cache_info().hits == hits + 1
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    plain = inputs.prepare_images(torch.from_numpy(frames).to(cuda), augs, (FH, FW), fused=False)
    assert all(p.is_cuda and torch.equal(p, a) for p, a in zip(plain, first))


# fW = 301: a row of 903 bytes is no multiple of 4, so the vertical pass takes its byte-wide form, in four blocks of 256
# threads; fW = 344: 1032 bytes, the 4-byte form in two blocks (258 threads).  Both: two blocks per row in the other two
# passes, the second one partly idle.  An upscale by 7.2 (ksize 5), a crop that starts above the image.
@pytest.mark.parametrize('fW', [301, 344])
def test_wide_output_takes_more_than_one_block_per_row(cuda, fW):
    rng = np.random.RandomState(3)
    frames = rng.randint(0, 256, (1, 9, 50, 3)).astype(np.uint8)
    check_images(cuda, frames, [((360, 20), (11, -2, 11 + fW, 7), True, -3.3)], (9, fW))


def test_image_stage_is_three_launches_and_no_synchronisation(cuda):
    frames, augs = two_camera_call((1, 2))
    for reps in (1, 3):                                          # M = 4 and M = 12: the same three launches
        dev = torch.from_numpy(np.concatenate([frames] * reps)).to(cuda)
        call = lambda: inputs.prepare_images(dev, augs * reps, (FH, FW))      # noqa: E731
        call()                                                   # warm-up: the table, the scratch, the code object
        _, kernels = device_kernels(call)
        assert len(kernels) == 3, kernels
        for name, kernel in zip(('horizontal', 'vertical', 'epilogue'), kernels):
            assert f'image_prep_{name}_kernel' in kernel, kernels


# ------------------------------------------------------------------------------------------------ point labels
def label_case(gold):
    size = GI.POINT_INPUT_SIZE
    augs = [host.aug_of(r) for r in gold['points.augs']]
    rows = [gold[f'points.{k}.in'] for k in range(len(augs))]
    P = rows[0].shape[0] + 300                                   # two blocks of points per camera
    padded = np.full((len(augs), P, 4), 7.0)
    for k, pts in enumerate(rows):
        padded[k, :pts.shape[0]] = pts
    counts = np.array([r.shape[0] for r in rows], np.int32)
    return size, augs, rows, padded, counts


def test_point_labels_equal_the_oracle(cuda, golden):
    """The golden points: several on one pixel, coordinates in (-1, 0), exactly W, negative, labels -1, 0 and 3, three
    cameras (plain, flipped and rotated +3.7, a negative crop origin and rotated -5.1), rows padded beyond ``counts``."""
    size, augs, rows, padded, counts = label_case(golden('inputs.npz'))
    pts, cnt = torch.from_numpy(padded).to(cuda), torch.from_numpy(counts).to(cuda)
    call = lambda: inputs.point_label_maps(pts, cnt, augs, size)         # noqa: E731
    depth, semantic = call()
    (again_d, again_s), kernels = device_kernels(call)
    assert len(kernels) == 2 and 'point_labels_mark_kernel' in kernels[0] and 'point_labels_resolve_kernel' in kernels[1]
    assert torch.equal(depth, again_d) and torch.equal(semantic, again_s)        # two runs bit-identical
    for k, (aug, r) in enumerate(zip(augs, rows)):
        want_d, want_s = oracle.point_label_maps(r, aug[0], aug[2], aug[3], aug[4], size)
        assert np.array_equal(depth[k].cpu().numpy(), want_d), k
        assert np.array_equal(semantic[k].cpu().numpy(), want_s), k
    plain = inputs.point_label_maps(pts, cnt, augs, size, fused=False)
    assert torch.equal(plain[0], depth) and torch.equal(plain[1], semantic)
    # twice the cameras: the same two launches
    pts2, cnt2 = torch.cat([pts, pts]), torch.cat([cnt, cnt])
    inputs.point_label_maps(pts2, cnt2, augs * 2, size)
    (d2, _), kernels = device_kernels(lambda: inputs.point_label_maps(pts2, cnt2, augs * 2, size))
    assert len(kernels) == 2 and torch.equal(d2[:3], depth) and torch.equal(d2[3:], depth)


def test_point_label_quirks_on_the_device(cuda):
    """Many points on one pixel across blocks: the highest index wins in both maps; P = 0; counts shorter than the row."""
    size, aug = (4, 6), (1.0, (6, 4), (0, 0, 6, 4), False, 0.0)
    P = 700
    pts = np.zeros((1, P, 4))
    pts[0, :, 0], pts[0, :, 1] = 2.0 + 0.999 * np.arange(P) / P, 1.5
    pts[0, :, 2], pts[0, :, 3] = 1.0 + np.arange(P), np.where(np.arange(P) % 2, 3.0, -1.0)
    pts[0, 5, :2], pts[0, 6, :2], pts[0, 7, :2], pts[0, 8, :2] = (-0.5, -0.9), (6.0, 2.0), (-1.0, 2.0), (5.999, 3.999)
    dev = torch.from_numpy(pts).to(cuda)
    for count in (P, 601, 9, 0):
        cnt = torch.tensor([count], dtype=torch.int32, device=cuda)
        depth, semantic = inputs.point_label_maps(dev, cnt, [aug], size)
        want_d, want_s = oracle.point_label_maps(pts[0, :count], 1.0, aug[2], False, 0.0, size)
        assert np.array_equal(depth[0].cpu().numpy(), want_d) and np.array_equal(semantic[0].cpu().numpy(), want_s), count
    assert want_d.sum() == 0 and float(depth.sum()) == 0
    cnt = torch.tensor([P], dtype=torch.int32, device=cuda)
    depth, semantic = inputs.point_label_maps(dev, cnt, [aug], size)
    assert depth[0, 1, 2] == P and semantic[0, 1, 2] == 1 and depth[0, 0, 0] == 6 and depth[0, 3, 5] == 9
    empty = inputs.point_label_maps(torch.zeros(1, 0, 4, dtype=torch.float64, device=cuda), cnt, [aug], size)
    assert not empty[0].any() and not empty[1].any()
