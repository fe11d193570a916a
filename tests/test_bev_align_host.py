"""CPU: the temporal BEV alignment without a GPU (ocrfdet_amd/temporal.py, csrc/bev_align_index.h): the closed-form
transform and the torch formulation against the reference's own ``gen_grid`` / ``shift_feature``
(tests/golden/bev_align.npz, tests/golden/make_golden_bev_align.py), ``align_and_cat``'s torch path in both list orders,
the backward's box of candidates against a float64 brute force, and the C boundary's argument validation.

Bounds: tests/bev_align_oracle.py.  The fixture's ``tf`` / ``out`` are the float64 restatement of the reference's
formula (the truth); ``out_err`` is the reference's own float32 deviation from it.
"""
import ctypes

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib
from ocrfdet_amd import temporal
from tests import bev_align_oracle as bo

CASES = 'abcd'


def case(golden, tag):
    g = golden('bev_align.npz')
    t = {k[len(tag) + 1:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(tag + '.')}
    return t


def transform_of(t):
    return temporal.feature_transform([t['curr'], t['adj']], t['bda'], t['grid_interval'], t['grid_lower_bound'],
                                      bda_adj=t.get('bda_adj'))


@pytest.mark.parametrize('tag', CASES)
def test_feature_transform_against_the_float64_restatement(golden, tag):
    t = case(golden, tag)
    tf = transform_of(t)
    assert tf.dtype == torch.float64 and tf.shape == (3, 3, 3)
    err = float((tf - t['tf']).abs().max())
    print(f'{tag}: feature_transform - truth {err:.3e}')
    assert err <= 1e-9
    # grid_interval / grid_lower_bound as plain sequences give the same
    tf2 = temporal.feature_transform([t['curr'], t['adj']], t['bda'], t['grid_interval'].tolist(),
                                     t['grid_lower_bound'].tolist(), bda_adj=t.get('bda_adj'))
    assert torch.equal(tf, tf2)


def test_the_fixture_covers_what_it_says(golden):
    assert 'bda_adj' in case(golden, 'c') and 'bda_adj' not in case(golden, 'a')
    d = case(golden, 'd')['bda']
    assert float(torch.linalg.det(d[0].double())) < 0 and float(torch.linalg.det(d[1].double())) < 0     # flips
    assert {tuple(case(golden, k)['x'].shape) for k in CASES} == {(3, 2, 13, 10), (3, 2, 16, 24)}
    for k in CASES:
        assert float(case(golden, k)['grid_err_px']) < 1e-3


@pytest.mark.parametrize('tag', CASES)
def test_shift_feature_torch_against_truth_and_reference(golden, tag):
    t = case(golden, tag)
    n, c, h, w = t['x'].shape
    bound = bo.forward_bound(t['tf'].numpy(), h, w, float(t['x'].abs().max()))
    got = temporal.shift_feature_torch(t['x'], t['tf'])
    assert got.dtype == torch.float32
    e_truth = float((got.double() - t['out']).abs().max())
    e_ref = float((got - t['ref_out']).abs().max())
    print(f'{tag}: torch formulation - truth {e_truth:.3e} (bound {bound:.3e}), - reference {e_ref:.3e} '
          f'(bound {bound + float(t["out_err"]):.3e})')
    assert e_truth <= bound
    assert e_ref <= bound + float(t['out_err'])
    # from the poses, and in float64
    assert float((temporal.shift_feature_torch(t['x'], transform_of(t)).double() - t['out']).abs().max()) <= bound
    assert float((temporal.shift_feature_torch(t['x'].double(), t['tf']) - t['out']).abs().max()) <= 1e-12


@pytest.mark.parametrize('tag', CASES)
def test_gen_grid_and_the_method_form(golden, tag):
    """The drop-in methods on an object that has only ``img_view_transformer``: the reference's own grid within its
    measured float32 error, and ``shift_feature_method`` = the torch formulation on the CPU."""
    t = case(golden, tag)
    n, c, h, w = t['x'].shape
    det = type('Detector', (), {})()
    det.img_view_transformer = type('VT', (), dict(grid_interval=t['grid_interval'],
                                                   grid_lower_bound=t['grid_lower_bound']))()
    args = (t['x'], [t['curr'], t['adj']], t['bda'])
    grid = temporal.gen_grid(det, *args, bda_adj=t.get('bda_adj'))
    assert grid.shape == (n, h, w, 2) and grid.dtype == torch.float32
    scale = torch.tensor([(w - 1) / 2.0, (h - 1) / 2.0], dtype=torch.float64)
    assert float(((grid.double() - t['grid']).abs() * scale).max()) <= 2.0 ** -24 * max(h, w)
    assert float(((grid.double() - t['ref_grid'].double()).abs() * scale).max()) <= (float(t['grid_err_px'])
                                                                                     + 2.0 ** -24 * max(h, w))
    out = temporal.shift_feature_method(det, *args, bda_adj=t.get('bda_adj'))
    assert torch.equal(out, temporal.shift_feature_torch(t['x'], transform_of(t)))


@pytest.mark.parametrize('order', ['bevdet4d', 'ocrfdet4d'])
def test_align_and_cat_torch_path_in_both_list_orders(golden, order):
    """``BEVDet4D``: [key, adj1, adj2] warped with sensor2keyegos[adj_id] (bevdet.py:529-536); ``OcRFDet4D``: [oldest,
    ..., key] warped with sensor2keyegos[num_frame - 2 - adj_id] (ocrfdet.py:267-274).  Values and gradients against the
    plain loop."""
    a, b = case(golden, 'b'), case(golden, 'c')
    num_frame = 4 if order == 'ocrfdet4d' else 3         # OcRFDet4D's last frame is the extra stereo reference
    s2k = [a['curr'], a['adj'], b['adj']] + ([a['adj']] if order == 'ocrfdet4d' else [])
    gen = torch.Generator().manual_seed(3)
    feats = [torch.randn(3, 2, 16, 24, generator=gen, dtype=torch.float64).requires_grad_(True) for _ in range(3)]
    if order == 'bevdet4d':
        frame_ids = list(range(num_frame))
    else:
        frame_ids = [num_frame - 2 - k for k in range(num_frame - 2)] + [0]
    assert frame_ids == ([0, 1, 2] if order == 'bevdet4d' else [2, 1, 0])
    extra = (a['bda'], a['grid_interval'], a['grid_lower_bound'])
    got = temporal.align_and_cat(feats, frame_ids, s2k, *extra, fused=False)
    want = []
    for x, fid in zip(feats, frame_ids):
        if fid == 0:
            want.append(x)
        else:
            tf = temporal.feature_transform([s2k[0], s2k[fid]], *extra)
            want.append(temporal.shift_feature_torch(x, tf))
    want = torch.cat(want, 1)
    assert got.shape == (3, 6, 16, 24) and torch.equal(got, want)
    r = torch.randn(got.shape, generator=gen, dtype=torch.float64)
    g_got = torch.autograd.grad(got, feats, r)
    g_want = torch.autograd.grad(want, feats, r)
    for x, y in zip(g_got, g_want):
        assert torch.equal(x, y)
    key = frame_ids.index(0)
    assert torch.equal(g_got[key], r[:, 2 * key:2 * key + 2])
    # the default flag dispatches CPU maps to the same formulation
    assert torch.equal(temporal.align_and_cat(feats, frame_ids, s2k, *extra), want)
    with pytest.raises(ValueError):
        temporal.align_and_cat(feats, frame_ids[:2], s2k, *extra)


def test_the_ops_refuse_what_the_kernels_do_not_take(golden):
    t = case(golden, 'a')
    with pytest.raises(_lib.OcrfHipError):
        temporal.shift_feature(t['x'], t['tf'])                    # a CPU map: no fallback
    import ocrfdet_amd
    assert ocrfdet_amd.shift_feature is temporal.shift_feature and ocrfdet_amd.align_and_cat is temporal.align_and_cat
    assert ocrfdet_amd.feature_transform is temporal.feature_transform


# ------------------------------------------------------------------------------------------------ the box helper
def box_of(L, t, h, w, qx, qy):
    six = (ctypes.c_float * 6)(*[float(v) for v in np.asarray(t, np.float32).reshape(-1)[:6]])
    box = (ctypes.c_int * 4)(7, 7, 7, 7)
    assert L.ocrf_bev_align_source_box(six, h, w, qx, qy, box) == 0
    return tuple(box)


def boxes(L, t, h, w):
    """(4, h, w): first / last column, first / last row of every source pixel's box."""
    out = np.empty((4, h, w), np.int64)
    for qy in range(h):
        for qx in range(w):
            out[:, qy, qx] = box_of(L, t, h, w, qx, qy)
    return out


def inside_or_empty(box, h, w):
    x0, x1, y0, y1 = box
    return (x0, x1, y0, y1) == (0, -1, 0, -1) or (0 <= x0 <= x1 <= w - 1 and 0 <= y0 <= y1 <= h - 1)


@pytest.mark.parametrize('hw', [(13, 10), (9, 17)])
def test_source_box_holds_every_reader(hw):
    h, w = hw
    L = _lib.lib()
    transforms = bo.seeded_transforms(h, w, 200, seed=100 * h + w)
    transforms += [bo.IDENTITY, bo.integer_shift(3, -2), bo.rot90_flip(h, w), bo.affine(h, w, shift=(0.93 * w, 0))]
    largest = 0
    for t in transforms:
        b = boxes(L, t, h, w)
        assert all(inside_or_empty(b[:, qy, qx], h, w) for qy in range(h) for qx in range(w))
        i, j, qy, qx = bo.taps(t, h, w)
        x0, x1, y0, y1 = (b[k][qy, qx] for k in range(4))
        missed = ~((x0 <= j) & (j <= x1) & (y0 <= i) & (i <= y1))
        assert not missed.any(), (t, list(zip(i[missed], j[missed], qy[missed], qx[missed]))[:4])
        largest = max(largest, int(bo.readers(t, h, w).max()))
    assert largest >= 16                                  # the shrinking transforms are among them
    # and it is a box, not the plane: at most 5 x 5 candidates for the identity and for a realistic motion
    for t in (bo.IDENTITY, bo.affine(h, w, angle=0.1, scale=1.02, shift=(2.3, -1.7))):
        b = boxes(L, t, h, w)
        assert ((b[1] - b[0] + 1) * (b[3] - b[2] + 1)).max() <= 25


@pytest.mark.parametrize('hw', [(13, 10), (9, 17)])
def test_source_box_stays_inside_the_plane_for_any_float(hw):
    h, w = hw
    L = _lib.lib()
    base = bo.affine(h, w, angle=0.2, shift=(1.5, -0.5)).reshape(-1)
    specials = [float('nan'), float('inf'), float('-inf'), 1e30, -1e30, 0.0]
    for k in range(6):
        for v in specials:
            t = base.copy()
            t[k] = v
            for qx, qy in ((0, 0), (w - 1, h - 1), (w // 2, h // 2)):
                assert inside_or_empty(box_of(L, t, h, w, qx, qy), h, w), (t, qx, qy)
    for v in specials:
        t = np.full(6, v, np.float32)
        assert inside_or_empty(box_of(L, t, h, w, 1, 1), h, w), v
    # det = 0: an all-zero 2 x 2 block reads one place from everywhere, so the box is the whole plane
    assert box_of(L, np.array([0, 0, 2.5, 0, 0, 3.5], np.float32), h, w, 2, 3) == (0, w - 1, 0, h - 1)
    assert L.ocrf_bev_align_source_box(None, h, w, 0, 0, (ctypes.c_int * 4)()) == 1
    assert L.ocrf_bev_align_source_box((ctypes.c_float * 6)(), 0, w, 0, 0, (ctypes.c_int * 4)()) == 1


def test_c_boundary_refuses_two_gib_operands():
    """Argument validation alone (nothing is launched, no memory is touched): operands of 2 GiB or more, products that
    overflow, non-positive sizes and a batch stride smaller than a sample return hipErrorInvalidValue."""
    L = _lib.lib()
    p = ctypes.c_void_p(4096)
    invalid = 1
    S = ctypes.c_longlong

    def fwd(n, c, h, w, stride, x=p, tf=p, out=p):
        return L.ocrf_bev_align_forward(n, c, h, w, x, tf, out, S(stride), None)

    def bwd(n, c, h, w, stride, g=p, tf=p, gx=p):
        return L.ocrf_bev_align_backward(n, c, h, w, g, S(stride), tf, gx, None)
    for f in (fwd, bwd):
        assert f(8, 1 << 12, 128, 128, (1 << 12) * 128 * 128) == invalid          # exactly 2 GiB
        assert f(1 << 15, 1 << 15, 1 << 15, 1 << 15, 1 << 45) == invalid          # n c h w overflows 64 bits' worth of int
        assert f(1 << 20, 1 << 20, 1, 1, 1 << 20) == invalid
        assert f(2, 80, 128, 128, 1 << 29) == invalid                             # the strided operand reaches 2 GiB
        assert f(2, 80, 128, 128, 80 * 128 * 128 - 1) == invalid                  # samples would overlap
        for bad in ((0, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0), (-1, 1, 4, 4), (1, 1, 4, -4)):
            assert f(*bad, 16) == invalid
    assert fwd(1, 1, 4, 4, 16, x=None) == invalid and fwd(1, 1, 4, 4, 16, tf=None) == invalid
    assert fwd(1, 1, 4, 4, 16, out=None) == invalid
    assert bwd(1, 1, 4, 4, 16, g=None) == invalid and bwd(1, 1, 4, 4, 16, tf=None) == invalid
    assert bwd(1, 1, 4, 4, 16, gx=None) == invalid
