"""Host: the native CenterHead (ocrfdet_amd/center_head.py) against the reference's own head
(``tests/golden/center_head.npz``, tests/golden/make_golden_center_head.py): module surface, forward, and the torch
formulation of the targets and losses, one test per semantic of get_targets_single."""
import json

import numpy as np
import pytest
import torch

from ocrfdet_amd import center_head as ch

T = 6


@pytest.fixture(scope='module')
def g(golden):
    return golden('center_head.npz')


def _cfg(g):
    return json.loads(str(g['cfg']))


def make_head(g, task_specific=True):
    c = _cfg(g)
    common = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2))
    return ch.CenterHead(in_channels=c['in_ch'], tasks=c['tasks'], common_heads=common, share_conv_channel=c['share'],
                         separate_head=dict(type='SeparateHead', init_bias=-2.19, final_kernel=3,
                                            head_conv=c['head_conv']),
                         loss_bbox=dict(type='L1Loss', reduction='mean', loss_weight=0.25), norm_bbox=True,
                         train_cfg=c['train_cfg'], task_specific=task_specific)


def boxes(g, dev='cpu'):
    n = sum(1 for k in g.files if k.startswith('boxes'))
    return ([torch.from_numpy(g[f'boxes{b}']).to(dev) for b in range(n)],
            [torch.from_numpy(g[f'labels{b}']).to(dev) for b in range(n)])


def preds(g, dev='cpu', tag=None):
    out, leaves = [], []
    for t in range(T):
        d = {}
        for n in ('reg', 'height', 'dim', 'rot', 'vel', 'heatmap'):
            leaf = torch.from_numpy(g[f'fwd.t{t}.{n}'].copy()).to(dev).requires_grad_(True)
            leaves.append((t, n, leaf))
            d[n] = leaf
        out.append([d])
    return tuple(out), leaves


def close_ulp(a, b, ulps):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float32)
    return np.all(np.abs(a - b) <= ulps * sp)


def rel_close(got, want, rtol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(np.abs(want).max(), 1e-30)
    return np.abs(got - want).max() <= rtol * scale


@pytest.fixture(scope='module')
def targets(g):
    head = make_head(g)
    return head.get_targets(*boxes(g))


# --------------------------------------------------------------------------------------------- module surface
def test_reference_config_builds_and_keys_match(g):
    cfg = json.loads(str(g['ref_config']))
    cfg.pop('type')
    head = ch.CenterHead(**cfg)
    want = json.loads(str(g['ref_keys']))
    got = {k: list(v.shape) for k, v in head.state_dict().items()}
    assert got == want
    assert head.with_velocity and head.task_specific and head.num_classes == [1, 2, 2, 1, 2, 2]


def test_state_dict_loads_strict_and_forward_matches(g):
    head = make_head(g)
    state = {k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('state.')}
    assert {k: list(v.shape) for k, v in head.state_dict().items()} == json.loads(str(g['small_keys']))
    head.load_state_dict(state, strict=True)
    head.eval()
    with torch.no_grad():
        out = head([torch.from_numpy(g['x'])])
    assert isinstance(out, tuple) and len(out) == T and all(isinstance(o, list) and len(o) == 1 for o in out)
    for t in range(T):
        for n in ('reg', 'height', 'dim', 'rot', 'vel', 'heatmap'):
            np.testing.assert_allclose(out[t][0][n].numpy(), g[f'fwd.t{t}.{n}'], atol=1e-5, rtol=0)


def test_init_weights_fills_heatmap_bias(g):
    head = make_head(g)
    head.init_weights()
    for h in head.task_heads:
        assert torch.all(h.heatmap[-1].bias == torch.tensor(-2.19))
        assert h.reg[0].conv.bias is None


def test_get_bboxes_and_dcn_raise(g):
    head = make_head(g)
    with pytest.raises(NotImplementedError):
        head.get_bboxes(None, None)
    with pytest.raises(NotImplementedError):
        ch.DCNSeparateHead(16, 2, dict(), dict())


# --------------------------------------------------------------------------------------------- targets (torch)
def test_targets_shapes_and_dtypes(g, targets):
    hm, anno, ind, mask = targets
    for t in range(T):
        assert hm[t].shape == g[f'heatmap{t}'].shape and hm[t].dtype == torch.float32
        assert anno[t].shape == g[f'anno_box{t}'].shape and anno[t].dtype == torch.float32
        assert ind[t].dtype == torch.int64 and mask[t].dtype == torch.uint8


def test_heatmap_bit_exact(g, targets):
    for t in range(T):
        assert np.array_equal(targets[0][t].numpy(), g[f'heatmap{t}']), t


def test_ind_and_mask_bit_exact(g, targets):
    for t in range(T):
        assert np.array_equal(targets[2][t].numpy(), g[f'ind{t}']), t
        assert np.array_equal(targets[3][t].numpy(), g[f'mask{t}']), t


def test_anno_box_exact_and_transcendental_columns(g, targets):
    for t in range(T):
        a, w = targets[1][t].numpy(), g[f'anno_box{t}']
        assert np.array_equal(a[..., [0, 1, 2, 8, 9]], w[..., [0, 1, 2, 8, 9]]), t
        assert close_ulp(a[..., 3:8], w[..., 3:8], 2), t


def test_heatmap_ones_counts(g):
    head = make_head(g)
    *_, counts = head._targets(*boxes(g))
    assert np.array_equal(counts[:T].numpy(), np.array([g[f'num_pos{t}'] for t in range(T)], np.float32))
    assert np.array_equal(counts[T:].numpy(), np.array([g[f'mask{t}'].sum() for t in range(T)], np.float32))


def test_slot_order_is_class_by_class(g, targets):
    # task 1 of sample 0 has labels 2, 1, 2 in that order: slot 0 is the label-1 box (class 0 of the task)
    lab = g['labels0']
    first = int(np.nonzero(lab == 1)[0][0])
    bx = g['boxes0'][first]
    ix = int(np.float32(np.float32(bx[0] + 8.0) / np.float32(0.125)) / np.float32(4))
    assert int(targets[2][1][0, 0]) % 32 == ix
    assert np.array_equal(targets[2][1].numpy(), g['ind1'])


def test_truncation_at_max_objs(g, targets):
    # task 5 of sample 0 has 10 boxes for max_objs 8: every slot is used
    assert int(targets[3][5][0].sum()) == 8 and (g['labels0'] >= 8).sum() > 8


def test_skipped_objects_keep_their_slot(g, targets):
    # task 0 of sample 0: slots 3, 4 (out of range) and 5 (width 0) stay zero, the later corners are in slots 6, 7
    m, a, i = targets[3][0][0].numpy(), targets[1][0][0].numpy(), targets[2][0][0].numpy()
    assert list(m) == [1, 1, 1, 0, 0, 0, 1, 1]
    assert not a[3:6].any() and not i[3:6].any()


def test_centre_in_minus_one_cell_is_kept(g, targets):
    # the box at -0.5 cells in x truncates to cell 0
    assert int(targets[3][0][0, 2]) == 1 and int(targets[2][0][0, 2]) % 32 == 0
    assert targets[1][0][0, 2, 0].item() == pytest.approx(-0.5, abs=1e-5)


def test_gravity_centre_z(g, targets):
    bx = g['boxes0'][0]
    assert targets[1][0][0, 0, 2].item() == np.float32(bx[2] + np.float32(bx[5] * np.float32(0.5)))


def test_shared_cell_counts_once(g, targets):
    i = targets[2][0][0].numpy()
    assert i[0] == i[1]
    hm = targets[0][0][0, 0].numpy()
    assert hm.flat[i[0]] == 1.0


def test_radius_and_clipped_windows(g, targets):
    # the corner boxes draw clipped windows; the large truck draws a radius above min_radius
    hm = targets[0][0][0, 0].numpy()
    assert hm[0, 0] == 1.0 and hm[23, 31] == 1.0
    big = targets[0][1][0, 0].numpy()
    i = int(np.nonzero(g['ind1'][0] == np.argmax(big == 1.0))[0][0]) if (big == 1.0).any() else None
    assert i is not None
    # a radius of r puts non-zero values r cells away, and min_radius 2 at least 2
    nz = np.nonzero(big > 0)
    assert (nz[0].max() - nz[0].min()) > 5


def test_empty_sample_and_empty_task(g, targets):
    for t in range(T):
        assert not targets[0][t][1].any() and not targets[3][t][1].any()
    assert not targets[0][3].any() and not targets[3][3].any()


def test_box_objects_with_tensor_attribute(g):
    class Boxes:
        def __init__(self, t):
            self.tensor = t
    head = make_head(g)
    bx, lab = boxes(g)
    a = head.get_targets([Boxes(b) for b in bx], lab)
    b = head.get_targets(bx, lab)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert torch.equal(u, v)


def test_without_velocity_and_without_norm_bbox(g):
    head = make_head(g)
    head.with_velocity, head.norm_bbox = False, False
    _, anno, _, mask = head.get_targets(*boxes(g))
    assert anno[0].shape[-1] == 8
    w = g['anno_box0']
    m = g['mask0'].astype(bool)
    assert np.array_equal(anno[0].numpy()[..., [0, 1, 2, 6, 7]], w[..., [0, 1, 2, 6, 7]])
    assert close_ulp(np.log(anno[0].numpy()[m][:, 3:6]), w[m][:, 3:6], 2)


# --------------------------------------------------------------------------------------------- losses (torch)
def _losses(g, ts):
    head = make_head(g, task_specific=ts)
    head.fused_loss = False
    pd, leaves = preds(g)
    ld = head.loss(*boxes(g), pd)
    return head, pd, leaves, ld


@pytest.mark.parametrize('ts', [True, False])
def test_losses_and_gradients_torch(g, ts):
    tag = 'ts' if ts else 'all'
    _, pd, leaves, ld = _losses(g, ts)
    keys = json.loads(str(g[f'loss_keys.{tag}']))
    assert sorted(ld) == keys
    got = np.array([ld[k].item() for k in keys])
    want = g[f'losses32.{tag}'].astype(np.float64)
    assert np.all(np.abs(got - want) <= 1e-6 * np.maximum(np.abs(want), 1e-30)), (got, want)
    sum(ld.values()).backward()
    for t, n, leaf in leaves:
        assert rel_close(leaf.grad.numpy(), g[f'grad.{tag}.t{t}.{n}'], 1e-6), (t, n)


def test_loss_leaves_clipped_heatmap_and_anno_box(g):
    _, pd, leaves, _ = _losses(g, True)
    x = torch.from_numpy(g['fwd.t0.heatmap'])
    assert torch.equal(pd[0][0]['heatmap'].detach(), torch.clamp(x.sigmoid(), 1e-4, 1 - 1e-4))
    assert pd[0][0]['anno_box'].shape[1] == 10
    assert torch.equal(leaves[5][2].detach(), x)            # the logits are not overwritten


def test_all_empty_batch_torch(g):
    head = make_head(g)
    head.fused_loss = False
    pd, _ = preds(g)
    e = [torch.zeros(0, 9)] * 3
    ld = head.loss(e, [torch.zeros(0, dtype=torch.int64)] * 3, pd)
    for t in range(T):
        assert ld[f'task{t}.loss_xy'].item() == 0.0
        x = torch.from_numpy(g[f'fwd.t{t}.heatmap'])
        p = torch.clamp(x.sigmoid(), 1e-4, 1 - 1e-4)
        want = (-(1 - p + 1e-12).log() * p.pow(2)).sum() / np.float32(1 + ch.F32_EPS)
        assert torch.isfinite(ld[f'task{t}.loss_heatmap'])
        assert ld[f'task{t}.loss_heatmap'].item() == pytest.approx(want.item(), rel=1e-6)


def test_reduce_counts_single_process_group(tmp_path):
    import torch.distributed as dist
    dist.init_process_group('gloo', init_method=f'file://{tmp_path}/pg', rank=0, world_size=1)
    try:
        c = torch.tensor([3.0, 0.0, 5.0, 2.0])
        assert torch.equal(ch.reduce_counts(c), c)
    finally:
        dist.destroy_process_group()
