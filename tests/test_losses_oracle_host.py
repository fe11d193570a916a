"""CPU: the cases of tests/losses_oracle.py carry the edges they were built for, and its bar tells a right float32
formulation from a wrong one.  The fused kernels themselves run in test_losses_oracle_gpu.py, through the same cases and
the same checker."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ocrfdet_amd import losses
from tests import losses_oracle as lo

K = lo.K


def test_the_kernel_constants_the_shapes_rest_on():
    lo.assert_kernel_constants()
    assert [lo.tiles(H, W) for H, W in lo.SIZES] == [1, 1, 1, 4, 10, 261]
    assert lo.tiles(4161, 5) > K['kThreads'] and lo.tiles(16, 64) == 1
    assert [lo.l1_blocks(H, W) for H, W in lo.SIZES] == [1, 1, 1, 1, 2, 3]
    assert 65 * 127 == 8255 > K['kL1Pixels'] and min(5, 7) < 2 * K['kR'] + 1
    assert 17 % K['kTH'] and 65 % K['kTW'] and lo.MASK_SIZES == ((17, 65), (65, 127))


# ------------------------------------------------------------------------------------------------ depth labels
@pytest.mark.parametrize('D', lo.LABEL_D)
@pytest.mark.parametrize('ds', lo.LABEL_DS)
def test_label_cases_hold_every_edge_and_every_row_kind(ds, D):
    c = lo.label_case(ds, D)
    d0, d1, step = c.cfg
    labels, sem = c.want
    assert c.rows % 4 and c.rows == 15 * (c.gt_depth.shape[-2] // ds) and d1 == d0 + D * step
    assert torch.isfinite(c.gt_depth).all() and set(c.gt_semantic.unique().tolist()) <= {0.0, 1.0}
    have = set(c.gt_depth.unique().tolist())
    for k in range(D + 1):
        e = np.float32(d0 + k * step)
        for v in (np.nextafter(e, np.float32(-np.inf)), e, np.nextafter(e, np.float32(np.inf))):
            assert float(v) in have, (k, v)
    assert {0.0, -3.0, 1e5} <= have and float(np.float32(d1)) in have
    kinds = dict(zip(lo.LABEL_KINDS, range(5)))
    valid = lambda r: (c.patch(c.gt_depth, r) >= d0) & (c.patch(c.gt_depth, r) <= d1)      # noqa: E731
    r = kinds['none']
    assert not valid(r).any() and not labels[r].any() and sem[r].tolist() == [1.0, 0.0]
    r = kinds['all_valid']
    assert valid(r).all() and sem[r].tolist() == [0.0, 1.0] and float(labels[r].sum()) == pytest.approx(1.0, abs=1e-6)
    r = kinds['sem_outside']
    ps = c.patch(c.gt_semantic, r)
    assert ps.any() and not (ps.bool() & valid(r)).any() and sem[r].tolist() == [1.0, 0.0]
    r = kinds['nan']
    on = c.patch(c.gt_semantic, r).bool()
    assert on.sum() == 1 and float(c.patch(c.gt_depth, r)[on]) == d1 and torch.isnan(labels[r]).all()
    assert sem[r].tolist() == [0.0, 1.0]
    r = kinds['soft']
    assert sem[r].tolist() == [0.0, 1.0] and float(labels[r].sum()) == pytest.approx(1.0, abs=1e-6)
    if ds > 1 and D > 1:
        assert int((labels[r] > 0).sum()) >= 2 and float(labels[r].max()) < 1.0
    hard = (sem[:, 1] == 0) & (labels.max(1).values == 1.0)
    assert hard.any() and ((labels[hard] > 0).sum(1) == 1).all()


def test_a_bin_that_takes_its_upper_edge_breaks_bit_equality(monkeypatch):
    """Bins are [lower edge, upper edge): a depth on an edge belongs to the bin above it.  A formulation whose bins are
    (lower, upper] puts it one bin down; every case holds every edge, so it differs in bits from the oracle in every
    case, while on inputs moved off the edges it is the same function: the edges are what tells the two apart."""
    def upper_inclusive(v, d0, step, D):
        b = (v - (d0 - step)) / step
        return torch.where((b <= D + 1) & (b > 0.0), torch.ceil(b) - 1.0, torch.zeros_like(b))
    for ds in lo.LABEL_DS:
        for D in lo.LABEL_D:
            c = lo.label_case(ds, D)
            assert lo.same_labels(losses.depth_labels_torch(c.gt_depth, c.gt_semantic, c.cfg, D, ds), c.want)
            with monkeypatch.context() as m:
                m.setattr(losses, '_bins', upper_inclusive)
                wrong = losses.depth_labels_torch(c.gt_depth, c.gt_semantic, c.cfg, D, ds)
            assert not lo.same_labels(wrong, c.want), (ds, D)
            # off the edges the two agree: rows whose patch holds no edge value are the same
            gd = c.gt_depth.clone()
            edges = torch.tensor([d for d in c.special if (d - c.cfg[0]) / c.cfg[2] == int((d - c.cfg[0]) / c.cfg[2])])
            gd[torch.isin(gd, edges)] += 0.01
            with monkeypatch.context() as m:
                m.setattr(losses, '_bins', upper_inclusive)
                shifted = losses.depth_labels_torch(gd, c.gt_semantic, c.cfg, D, ds)
            assert lo.same_labels(shifted, losses.depth_labels_torch(gd, c.gt_semantic, c.cfg, D, ds)), (ds, D)


# ------------------------------------------------------------------------------------------------ depth / semantic BCE
def test_ds_cases_carry_their_rows():
    rows = {n: lo.ds_case(n).rows for n in lo.DS_SPECS}
    assert sorted(set(rows.values())) == [1, 8, 255, 256, 257, 513]
    assert any(c.BN > 1 and c.h * c.w > 1 for c in map(lo.ds_case, lo.DS_SPECS))
    assert sorted({lo.ds_case(n).D for n in lo.DS_SPECS}) == [5, 118]
    for n in ('ds_rows255', 'ds_rows256', 'ds_rows257_D118', 'ds_rows513'):
        c = lo.ds_case(n)
        nan = torch.isnan(c.labels).any(1)
        zero = ~nan & (c.labels.nan_to_num().max(1).values == 0)
        hard = c.in_mask() & (c.sem_labels[:, 1] == 0)
        soft = c.in_mask() & (c.sem_labels[:, 1] == 1)
        assert nan.any() and zero.any() and hard.any() and soft.any(), n
        assert ((c.labels[soft] > 0).sum(1) >= 2).any(), n
        assert not c.in_mask()[nan].any() and 0 < int(c.in_mask().sum()) < c.rows
    c = lo.ds_case('ds_rows1_single_hard_row')
    assert c.rows == 1 and bool(c.in_mask()[0]) and c.sem_labels[0].tolist() == [1.0, 0.0]
    wm = torch.where(c.sem_labels[:, 1] > 0, 0.9, 0.1)[c.in_mask()].sum()
    assert float(wm) == float(torch.tensor(0.1)), 'the weight sum sits on the 0.1 clamp'
    c = lo.ds_case('ds_rows257_no_row_in_mask')
    assert not c.in_mask().any() and torch.isnan(c.labels).any() and (c.labels.nan_to_num() == 0).all()
    assert all(not v.any() for v in c.want.values()), 'both losses and all gradients are exactly 0'
    c = lo.ds_case('ds_exact_0_and_1')
    assert c.per_element and c.in_mask().all()
    lab = c.labels.reshape(c.BN, c.h, c.w, c.D).permute(0, 3, 1, 2)
    for p in (0.0, 1.0):
        assert ((c.depth == p) & (lab > 0)).any() and ((c.depth == p) & (lab == 0)).any() and (c.sem == p).any()
    g = c.want['g_depth@0']
    assert float(g.abs().max()) > 1e10 and (g == 0).any() and float(g[g != 0].abs().min()) < 1e3
    assert ((c.depth > 0) & (c.depth < 1)).any()


@pytest.mark.parametrize('name', list(lo.DS_SPECS))
def test_ds_upstream_gradients_are_told_apart(name):
    """The float32 torch formulation passes its own bar; the two upstream gradients exchanged do not."""
    c = lo.ds_case(name)
    figs = lo.check(c, c.torch32)
    assert all(f.e_torch > 0 for f in figs if f.factor * f.e_torch > f.floor)
    if c.in_mask().any():
        swapped = lo.ds_run(losses.depth_semantic_loss_torch, c, upstream=[g[::-1] for g in lo.DS_UPSTREAM])
        assert any(not f.ok for f in lo.figures(c, swapped))


def test_ds_bar_rejects_exchanged_row_weights():
    """0.9 for the rows without a semantic pixel and 0.1 for those with one."""
    c = lo.ds_case('ds_rows255')
    flipped = lo.ds_run(losses.depth_semantic_loss_torch,
                        dataclasses.replace(c, sem_labels=c.sem_labels.flip(1).contiguous()))
    figs = {f.name: f for f in lo.figures(c, flipped)}
    assert not figs['loss_depth'].ok and not figs['g_depth@0'].ok


# ------------------------------------------------------------------------------------------------ masks
@pytest.mark.parametrize('size', lo.MASK_SIZES)
@pytest.mark.parametrize('variant', lo.MASK_VARIANTS)
def test_masks_have_the_extents_they_name(variant, size):
    H, W = size
    c = lo.render_case(f'mask_{variant}_{H}x{W}')
    assert c.use_mask and len(c.boxes) == 1
    m = c.masks()[0]
    assert torch.equal(m, lo.slice_mask(c.rects[0], H, W)), 'box_mask against Python slices on the wanted rectangles'
    rows = torch.nonzero(m.any(1))[:, 0].tolist()
    cols = torch.nonzero(m.any(0))[:, 0].tolist()
    if variant == 'zero':
        assert c.boxes[0].shape == (0, 4) and not m.any()
        for k in ('loss_color', 'loss_ssim', 'g_render0', 'g_render1', 'g_render2'):
            assert not c.want[k].any(), k
        assert c.want['loss_depth'] > 0
    elif variant == 'full':
        assert m.all()
    elif variant == 'tile_edges':
        assert m[15, 63] == 1 and m[16, 64] == 1 and m[15, 64] == 0 and m[16, 63] == 0 and m[7, 63] == 0
        assert m[2:6, 5:20].all() and m[1, 5] == 0 and m[6, 19] == 0 and m[2, 4] == 0 and m[2, 20] == 0
        assert int(m.sum()) == 8 * 32 + (H - 16) * (W - 64) + 4 * 15
    elif variant == 'wrap':
        assert float(c.boxes[0][0, 1]) * np.float32(W / 1600) < 158, 'the shifted bound is negative'
        assert rows == list(range(H - 3, H)) and cols == list(range(5, W - 5))
    elif variant == 'empty':
        assert c.rects[0][0][1] <= c.rects[0][0][0] and len(c.boxes[0]) == 2
        assert rows == list(range(5, 12)) and cols == list(range(10, 50)) and int(m.sum()) == 7 * 40
    elif variant == 'beyond':
        assert float(c.boxes[0][0, 2]) * np.float32(W / 1600) > W
        assert rows == list(range(2, H - 2)) and cols == list(range(W - 10, W))
    elif variant == 'nan':
        assert int(torch.isnan(c.boxes[0]).sum()) == 2 and torch.isnan(c.boxes[0][0, 0]) and torch.isnan(c.boxes[0][1, 3])
        assert rows == list(range(2, 10)) and cols == list(range(0, 30))
    elif variant == 'many':
        assert len(c.boxes[0]) == K['kMaxBoxes'] == losses._MAX_BOXES and 0 < int(m.sum()) < H * W
        assert len(rows) > K['kTH'] and len(cols) > K['kTW'] or (H, W) == (17, 65)


def test_a_nan_box_coordinate_is_a_very_negative_bound_on_both_axes():
    """``box_bounds`` used to hand NaN to the integer conversion: INT64_MIN on this CPU, and INT64_MIN - 158 wrapped
    to a bound of H for the y coordinates where the kernel's ``trunc_ll`` gives 0."""
    nan = float('nan')
    y0, y1, x0, x1 = losses.box_bounds(torch.tensor([[nan, nan, nan, nan], [-1e30, 1e30, 1e30, -1e30]]), 65, 17)
    assert y0.tolist() == [0, 17] and y1.tolist() == [0, 0] and x0.tolist() == [0, 0] and x1.tolist() == [0, 65]


# ------------------------------------------------------------------------------------------------ render cases
def test_render_cases_carry_their_properties():
    assert set(lo.SIZES) <= {(c.H, c.W) for c in lo.RENDER_SPECS.values()}
    for name, spec in lo.RENDER_SPECS.items():
        c = lo.render_case(name)
        B, H, W = spec.B, spec.H, spec.W
        assert c.gt_images.shape == (B + 1, 3, H, W) and c.gt_depth.shape == (B, lo.N_CAMS, H, W)
        assert len(set(c.cams)) == B and all(r.shape == (B, 3, H, W) for r in c.renders)
        assert lo.RENDER_UPSTREAM == (0.7, -1.3, 2.1)
        for rd in c.render_depths:
            d = (rd[:, 0].double() - c.targets).abs()
            assert ((d >= lo.TIE) | (d == 0)).all(), 'tie distance'
        for b in range(B):
            plane = c.gt_depth[b, c.cams[b]]
            kind = spec.depths[b]
            inside = (plane >= lo.D_MIN) & (plane <= lo.D_MAX)
            if kind == 'textured':
                assert inside.all() and float(plane.min()) > lo.D_MIN
            elif kind == 'edges':
                assert all((plane == e).any() for e in lo.EDGE_DEPTHS) and inside.any() and not inside.all()
                assert float(c.targets[b].max()) == pytest.approx(60.0 / 60.01, rel=1e-6)
            else:
                assert not inside.any() and not c.targets[b].any()
                ties = [(rd[b, 0] == 0) for rd in c.render_depths]
                assert all(t.any() and not t.all() for t in ties)
                for k, t in enumerate(ties):        # sign(0): the gradient of a tie is exactly 0, the others are not
                    g = c.want[f'g_depth{k}'][b, 0]
                    assert not g[t].any() and g[~t].all()
                # den = 0.01: a render depth of 0.5 is an error of 50
                assert float(lo.depth_target(plane + 0.0).max()) == 0.0
    c = lo.render_case('batch3_17x65')
    assert c.spec.B == 3 and c.cams == (2, 0, 1) and [len(b) for b in c.boxes] == [1, 1, 0]
    c = lo.render_case(lo.SMOOTH_CASE)
    assert float(c.gt_images.min()) >= 0.9 and float(c.gt_images.max()) <= 0.91
    s = lo.ssim_case()
    assert s.img1.shape == (2, 1, 17, 65)
    # the runs differentiate copies: the shared cases stay as they were built
    for c in list(map(lo.render_case, lo.RENDER_SPECS)) + [s]:
        assert not any(t.requires_grad for t in vars(c).values() if torch.is_tensor(t))
        assert not any(t.requires_grad for v in vars(c).values() if isinstance(v, tuple) for t in v if torch.is_tensor(t))


def test_torch_errors_are_positive_where_the_ratio_is_the_bar():
    """On textured images the float32 torch gradient is off by some 1e-6 of its largest entry, on the smooth pair by
    some 1e-4, and the loss by more than 1e-5: there the bar is the ratio to ``e_torch``, not the floor."""
    used = 0
    for name in lo.RENDER_SPECS:
        c = lo.render_case(name)
        for f in lo.check(c, c.torch32):
            if f.factor * f.e_torch > f.floor:
                assert f.e_torch > 0
                used += 1
    assert used > 50
    figs = {f.name: f for f in lo.figures(lo.render_case(lo.SMOOTH_CASE), lo.render_case(lo.SMOOTH_CASE).torch32)}
    for k in ('g_render0', 'g_render1', 'g_render2'):
        assert figs[k].e_torch > 100 * figs[k].floor, 'the smooth pair is where float32 loses the SSIM gradient'
    assert figs['loss_ssim'].e_torch > figs['loss_ssim'].floor
    lo.check(lo.ssim_case(), lo.ssim_case().torch32)


# ------------------------------------------------------------------------------------------------ wrong formulations
def _replicate_ssim(img1, img2, window_size=11, size_average=True, window=None):
    C = img1.shape[1]
    window = losses.gaussian_window(window_size, C, device=img1.device, dtype=img1.dtype)
    pad = window_size // 2

    def blur(x):
        if x.shape[-1] > pad and x.shape[-2] > pad:
            x = F.pad(x, (pad,) * 4, mode='replicate')
        else:                                       # replicate padding needs pad < size: pad in steps
            for _ in range(pad):
                x = F.pad(x, (1,) * 4, mode='replicate')
        return F.conv2d(x, window, groups=C)
    mu1, mu2 = blur(img1), blur(img2)
    s1, s2, s12 = blur(img1 * img1) - mu1 * mu1, blur(img2 * img2) - mu2 * mu2, blur(img1 * img2) - mu1 * mu2
    m = ((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return m.mean()


def _wrong(variant, c, monkeypatch):
    """A float32 torch evaluation of case ``c`` that is wrong in one named way."""
    if variant == 'replicate_padding':
        with monkeypatch.context() as m:
            m.setattr(losses, 'ssim_torch', _replicate_ssim)
            return lo.render_run_torch(c, torch.float32)
    if variant == 'mask_on_gt_only':
        gt = c.gt_images.clone()
        for b, m in enumerate(c.masks()):
            gt[b] *= m
        return lo.render_run_torch(c, torch.float32, masks=[None] * c.spec.B, gt_images=gt)
    if variant == 'upstream_exchanged':
        g = lo.RENDER_UPSTREAM
        return lo.render_run_torch(c, torch.float32, upstream=(g[1], g[0], g[2]))
    if variant == 'range_not_zeroed':
        return lo.render_run_torch(c, torch.float32, depth_range=(-float('inf'), float('inf')))
    if variant == 'wrong_camera':
        return lo.render_run_torch(dataclasses.replace(c, cams=tuple((k + 1) % lo.N_CAMS for k in c.cams)),
                                   torch.float32)
    if variant == 'sign_of_zero_is_one':
        out = dict(lo.render_run_torch(c, torch.float32))
        k = float(np.float32(lo.RENDER_UPSTREAM[2])) / (3 * c.spec.B * c.spec.H * c.spec.W)
        out['g_depth0'] = torch.where(c.render_depths[0] == 0, torch.full_like(out['g_depth0'], k), out['g_depth0'])
        return out
    raise KeyError(variant)


WRONG = {
    'replicate_padding': (['size_5x7', 'size_17x65', 'smooth_17x65', 'size_4161x5'], ('loss_ssim', 'g_render0')),
    'mask_on_gt_only': (['mask_tile_edges_17x65', 'mask_wrap_65x127', 'mask_many_17x65'], ('loss_color', 'g_render1')),
    'upstream_exchanged': (['size_1x1', 'size_16x64', 'mask_full_17x65', 'smooth_17x65'], ('g_render0', 'g_render2')),
    'range_not_zeroed': (['size_5x7', 'size_65x127', 'depth_outside_17x65', 'batch3_17x65'], ('loss_depth',)),
    'wrong_camera': (['size_17x65', 'depth_textured_17x65', 'batch3_17x65'], ('loss_depth',)),
    'sign_of_zero_is_one': (['depth_outside_17x65', 'batch3_17x65'], ('g_depth0',)),
}


@pytest.mark.parametrize('variant', list(WRONG))
def test_the_bar_rejects_a_wrong_formulation(variant, monkeypatch):
    cases, quantities = WRONG[variant]
    for name in cases:
        c = lo.render_case(name)
        figs = {f.name: f for f in lo.figures(c, _wrong(variant, c, monkeypatch))}
        for q in quantities:
            print(figs[q])
            assert not figs[q].ok, (variant, name, q)
        with pytest.raises(AssertionError):
            lo.check(c, _wrong(variant, c, monkeypatch))
    # and the right formulation passes where the wrong one was told apart
    assert all(f.ok for f in lo.figures(lo.render_case(cases[0]), lo.render_case(cases[0]).torch32))


def test_the_checker_refuses_a_missing_gradient_a_nan_and_a_non_zero_where_the_oracle_is_zero():
    c = lo.render_case('mask_wrap_17x65')
    got = dict(c.torch32)
    got['g_depth1'] = None
    with pytest.raises(AssertionError):
        lo.figures(c, got)
    got = dict(c.torch32)
    got['g_render0'] = got['g_render0'].clone()
    got['g_render0'][0, 0, 0, 0] = 1e-30                       # outside the mask: far below the floor, and still refused
    figs = {f.name: f for f in lo.figures(c, got)}
    assert c.want['g_render0'][0, 0, 0, 0] == 0 and not figs['g_render0'].zeros_kept and not figs['g_render0'].ok
    got['g_render0'] = torch.full_like(got['g_render0'], float('nan'))
    assert not {f.name: f for f in lo.figures(c, got)}['g_render0'].ok
