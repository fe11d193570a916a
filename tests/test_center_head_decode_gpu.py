"""GPU: the fused CenterHead decode and NMS (csrc/center_decode.hip) against the reference's values
(``tests/golden/center_head_decode.npz``) and against the torch formulation at full size (B = 8, 128 x 128, the
reference config's test_cfg and coder, K = 500) on a peaked and an at-initialisation heatmap; deterministic; no host
synchronisation; a fixed launch count; an all-empty batch; get_bboxes as the padded result sliced."""
import json

import numpy as np
import pytest
import torch

from ocrfdet_amd import center_head as ch
from ocrfdet_amd import synthetic

from .test_center_head_decode_host import check_padded, make_head, preds, ulp_close

pytestmark = pytest.mark.gpu

NUSC_TASKS = [dict(num_class=1, class_names=['car']), dict(num_class=2, class_names=['truck', 'construction_vehicle']),
              dict(num_class=2, class_names=['bus', 'trailer']), dict(num_class=1, class_names=['barrier']),
              dict(num_class=2, class_names=['motorcycle', 'bicycle']),
              dict(num_class=2, class_names=['pedestrian', 'traffic_cone'])]
NUSC_TRAIN = dict(point_cloud_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], grid_size=[1024, 1024, 40],
                  voxel_size=[0.1, 0.1, 0.2], out_size_factor=8, dense_reg=1, gaussian_overlap=0.1, max_objs=500,
                  min_radius=2, code_weights=[1.0] * 8 + [0.2, 0.2])
NUSC_CODER = dict(type='CenterPointBBoxCoder', pc_range=[-51.2, -51.2],
                  post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_num=500, score_threshold=0.1,
                  out_size_factor=8, voxel_size=[0.1, 0.1], code_size=9)
NUSC_TEST = dict(pc_range=[-51.2, -51.2], post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                 max_per_img=500, max_pool_nms=False, min_radius=[4, 12, 10, 1, 0.85, 0.175], score_threshold=0.1,
                 out_size_factor=8, voxel_size=[0.1, 0.1], pre_max_size=1000, post_max_size=83,
                 nms_type=['rotate', 'rotate', 'rotate', 'circle', 'rotate', 'rotate'],
                 nms_thr=[0.3, 0.1, 0.1, 0.1, 0.1, 0.5],
                 nms_rescale_factor=[1.0, [0.7, 0.7], [0.4, 0.55], 1.1, [1.0, 1.0], [4.5, 9.0]])


@pytest.fixture(scope='module')
def g(golden):
    return golden('center_head_decode.npz')


def full_head(dev):
    common = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2))
    return ch.CenterHead(in_channels=256, tasks=NUSC_TASKS, common_heads=common, share_conv_channel=64,
                         train_cfg=NUSC_TRAIN, test_cfg=NUSC_TEST, bbox_coder=NUSC_CODER).to(dev)


def full_preds(dev, kind, B=8, seed=0):
    """'peaked': logits of the targets of synthetic nuScenes boxes plus noise; 'init': the -2.19 bias plus small noise,
    so that every task carries 500 candidates into NMS; 'empty': nothing above the threshold."""
    gen = torch.Generator(device='cpu').manual_seed(seed)
    head = full_head(dev)
    if kind == 'peaked':
        bx, lab = synthetic.nuscenes_boxes(B, seed=seed, device=dev)
        heat = [h.clamp(1e-3, 1 - 1e-3).logit() for h in head.get_targets(bx, lab)[0]]
    out = []
    for t, task in enumerate(NUSC_TASKS):
        n = task['num_class']
        d = {k: (torch.randn(B, c, 128, 128, generator=gen) * s).to(dev)
             for k, c, s in (('reg', 2, 0.3), ('height', 1, 1.0), ('dim', 3, 0.4), ('rot', 2, 1.0), ('vel', 2, 1.0))}
        d['reg'] = d['reg'] + 0.5
        noise = torch.randn(B, n, 128, 128, generator=gen).to(dev)
        if kind == 'peaked':
            d['heatmap'] = heat[t] + 0.5 * noise
        elif kind == 'init':
            d['heatmap'] = -2.19 + 0.01 * noise
        else:
            d['heatmap'] = -10.0 + noise
        out.append([d])
    return head, tuple(out)


def test_fused_matches_reference(g, cuda):
    head = make_head(g).to(cuda)
    pd = preds(g, cuda)
    out = head.get_bboxes_padded(pd)
    assert out[0].is_cuda
    check_padded(g, *out)


@pytest.mark.parametrize('kind', ['peaked', 'init'])
def test_fused_matches_torch_full_size(cuda, kind):
    head, pd = full_preds(cuda, kind)
    head.fused_decode = True
    fb, fs, fl, fc = head.get_bboxes_padded(pd)
    head.fused_decode = False
    tb, ts, tl, tc = head.get_bboxes_padded(pd)
    fc, tc = fc.cpu(), tc.cpu()
    if kind == 'init':
        assert int(tc.min()) > 0
    for b in range(fc.shape[0]):
        n = int(tc[b])
        assert int(fc[b]) == n, f'sample {b}: count {int(fc[b])} fused, {n} torch'
        assert torch.equal(fl[b, :n].cpu(), tl[b, :n].cpu()), f'sample {b}: labels or order differ'
        ulp_close(fs[b, :n].cpu().numpy(), ts[b, :n].cpu().numpy(), 1)
        got, want = fb[b, :n].cpu().numpy(), tb[b, :n].cpu().numpy()
        ulp_close(got[:, [0, 1, 7, 8]], want[:, [0, 1, 7, 8]], 1)
        ulp_close(got[:, 3:7], want[:, 3:7], 2)
        tol = np.spacing(np.abs(want[:, 2])) + 2 * np.spacing(np.abs(want[:, 5] * np.float32(0.5))) + \
            np.spacing(np.abs(want[:, 2] + want[:, 5] * 0.5))
        assert (np.abs(got[:, 2].astype(np.float64) - want[:, 2]) <= tol).all()


def test_reruns_bit_identical(cuda):
    head, pd = full_preds(cuda, 'init', seed=1)
    a = head.get_bboxes_padded(pd)
    b = head.get_bboxes_padded(pd)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_padded_has_no_host_sync(cuda):
    head, pd = full_preds(cuda, 'peaked', seed=2)
    head.get_bboxes_padded(pd)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = head.get_bboxes_padded(pd)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert out[3].shape == (8,)


def kernel_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_launch_count_fixed(cuda):
    counts = []
    for B in (1, 8):
        head, pd = full_preds(cuda, 'init', B=B, seed=3)
        names = kernel_launches(lambda: head.get_bboxes_padded(pd))
        counts.append(len(names))
        assert len(names) <= 6, names
    assert counts[0] == counts[1]


def test_all_empty_batch(cuda):
    head, pd = full_preds(cuda, 'empty', B=2, seed=4)
    boxes, scores, labels, counts = head.get_bboxes_padded(pd)
    assert counts.tolist() == [0, 0] and not boxes.any() and not labels.any()
    res = head.get_bboxes(pd, None)
    assert [tuple(r[0].shape) for r in res] == [(0, 9), (0, 9)]
    assert res[0][2].dtype == torch.int32


def test_get_bboxes_is_padded_sliced(cuda):
    head, pd = full_preds(cuda, 'peaked', B=3, seed=5)
    boxes, scores, labels, counts = head.get_bboxes_padded(pd)
    res = head.get_bboxes(pd, [dict()] * 3)
    for i, (b, s, l) in enumerate(res):
        n = int(counts[i])
        assert torch.equal(b, boxes[i, :n]) and torch.equal(s, scores[i, :n]) and torch.equal(l, labels[i, :n])
    assert json.dumps([int(c) for c in counts.cpu()]) == json.dumps([r[0].shape[0] for r in res])
    np.testing.assert_array_equal(labels.cpu().numpy() >= 0, True)
