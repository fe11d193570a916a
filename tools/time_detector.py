"""Timing of the detector layer (``ocrfdet_amd.detector``).

Pose step, B = 8, N = 6 cameras, F = 3 frames (``temporal_frame`` 2): the frame poses plus the per-frame ``mlp_input``

* fused: ``frame_poses(..., fused=True)``, one launch of ``ocrf_frame_poses``;
* the reference's formulation, restated here in torch: ``torch.inverse`` on the float64 4 x 4 stacks
  (bevdet.py:435-456) and one ``get_mlp_input`` per frame (ocrfdet.py:229-231);
* ``frame_poses_torch``: float64 closed forms in torch, what the CPU and ``fused_poses = False`` take.

Per arm: device time and launch count from the torch profiler, wall time per call from a host clock around
synchronised blocks (the arms alternating), and the synchronising torch calls per call, counted with
``torch.cuda.set_sync_debug_mode('warn')``.  The acceptance condition is structural: one launch and no
synchronisation on the fused arm.

Whole detector: ``OcRFDet4D`` of the reference config (configs/ocrfdet/ocrfdet.py:44-154: ResNet-50, 6 cameras of
256 x 704, 3 frames, a 128 x 128 BEV), forward at B = 1 (``eval()``, ``forward_dummy`` under ``no_grad``) and forward +
backward at B = 2 (``train()``, the sum of the losses; the neck's MS_CAM has a batch norm behind a global average pool,
which cannot train on one sample), with ``fused_poses`` on and off.  Reported only; no threshold.

    python tools/time_detector.py [--iters N] [--out profiles/detector_time.txt]

Every case runs in a child process of its own under a time limit (``--limit`` seconds); the first case that fails or
runs out of time ends the run.
"""
import argparse
import math
import os
import subprocess
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = ['poses', 'detector forward', 'detector forward+backward']
POINT_CLOUD_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
INPUT_SIZE, N_CAMS, N_FRAMES = (256, 704), 6, 3


def reference_model():
    """The ``model`` dict of configs/ocrfdet/ocrfdet.py:44-154."""
    c = 80
    return dict(
        type='OcRFDet4D', align_after_view_transfromation=False, num_adj=1,
        img_backbone=dict(pretrained='torchvision://resnet50', type='ResNet', depth=50, num_stages=4,
                          out_indices=(0, 2, 3), frozen_stages=-1, norm_cfg=dict(type='BN', requires_grad=True),
                          norm_eval=False, with_cp=True, style='pytorch'),
        img_neck=dict(type='CustomFPN', in_channels=[1024, 2048], out_channels=256, num_outs=1, start_level=0,
                      out_ids=[0]),
        img_view_transformer=dict(
            type='OcRFViewTransformerFull',
            grid_config=dict(x=[-51.2, 51.2, 0.8], y=[-51.2, 51.2, 0.8], z=[-5, 3, 8], depth=[1.0, 60.0, 0.5]),
            input_size=INPUT_SIZE, in_channels=256, out_channels=c, pc_range=POINT_CLOUD_RANGE,
            depthnet_cfg=dict(use_dcn=False, aspp_mid_channels=96, stereo=True, bias=5.), downsample=16),
        img_bev_encoder_backbone=dict(type='CustomResNet', numC_input=c * 2, num_channels=[c * 2, c * 4, c * 8]),
        img_bev_encoder_neck=dict(type='FPN_LSS', in_channels=c * 8 + c * 2, out_channels=256),
        pre_process=dict(type='CustomResNet', numC_input=c, num_layer=[2, ], num_channels=[c, ], stride=[1, ],
                         backbone_output_ids=[0, ]),
        pts_bbox_head=dict(
            type='CenterHead', in_channels=256,
            tasks=[dict(num_class=1, class_names=['car']), dict(num_class=2, class_names=['truck', 'construction_vehicle']),
                   dict(num_class=2, class_names=['bus', 'trailer']), dict(num_class=1, class_names=['barrier']),
                   dict(num_class=2, class_names=['motorcycle', 'bicycle']),
                   dict(num_class=2, class_names=['pedestrian', 'traffic_cone'])],
            common_heads=dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2)), share_conv_channel=64,
            bbox_coder=dict(type='CenterPointBBoxCoder', pc_range=POINT_CLOUD_RANGE[:2],
                            post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_num=500, score_threshold=0.1,
                            out_size_factor=8, voxel_size=[0.1, 0.1], code_size=9),
            separate_head=dict(type='SeparateHead', init_bias=-2.19, final_kernel=3),
            loss_cls=dict(type='GaussianFocalLoss', reduction='mean'),
            loss_bbox=dict(type='L1Loss', reduction='mean', loss_weight=0.25), norm_bbox=True),
        train_cfg=dict(pts=dict(point_cloud_range=POINT_CLOUD_RANGE, grid_size=[1024, 1024, 40],
                                voxel_size=[0.1, 0.1, 0.2], out_size_factor=8, dense_reg=1, gaussian_overlap=0.1,
                                max_objs=500, min_radius=2, code_weights=[1.0] * 10)),
        test_cfg=dict(pts=dict(pc_range=POINT_CLOUD_RANGE[:2], post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                               max_per_img=500, max_pool_nms=False, min_radius=[4, 12, 10, 1, 0.85, 0.175],
                               score_threshold=0.1, out_size_factor=8, voxel_size=[0.1, 0.1], pre_max_size=1000,
                               post_max_size=83,
                               nms_type=['rotate', 'rotate', 'rotate', 'circle', 'rotate', 'rotate'],
                               nms_thr=[0.3, 0.1, 0.1, 0.1, 0.1, 0.5],
                               nms_rescale_factor=[1.0, [0.7, 0.7], [0.4, 0.55], 1.1, [1.0, 1.0], [4.5, 9.0]])))


def img_inputs(B, n_cams, n_frames, input_size, dev, seed=0):
    """A seeded 12-entry ``img_inputs``: the synthetic rig in every frame, the ego moving as ``synthetic.ego_motion``
    from a global pose about 1e3 m from the origin."""
    import numpy as np
    import torch
    from ocrfdet_amd import synthetic
    H, W = input_size
    gen = torch.Generator().manual_seed(seed)
    rig = synthetic.rig(n_cams, input_size, B)

    def per_frame(a):
        t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).unsqueeze(1)
        return t.expand(B, n_frames, *a.shape[1:]).reshape(B, n_frames * n_cams, *a.shape[2:]).contiguous()
    yaw = math.radians(35.0)
    G = np.eye(4)
    G[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]]
    G[:3, 3] = [612.5, -1104.25, 2.5]
    e2g = torch.from_numpy(np.stack([G @ synthetic.ego_motion(f) for f in range(n_frames)]).astype(np.float32))
    e2g = e2g.view(1, n_frames, 1, 4, 4).expand(B, n_frames, n_cams, 4, 4).reshape(B, n_frames * n_cams, 4, 4)
    raw = torch.rand(B, n_cams * n_frames, 3, H, W, generator=gen) * 255
    inputs = [(raw - 120.0) / 58.0] + [per_frame(rig[k]) for k in ('rots', 'trans', 'intrins', 'post_rots', 'post_trans')]
    inputs += [torch.from_numpy(rig['bda']), per_frame(rig['c2w']), e2g.contiguous(), raw, raw.clone(), per_frame(rig['c2w'])]
    return [t.to(dev) for t in inputs]


def _profile(fn, reps=5):
    """(launches per call, device ms per call, names of the kernels) from the torch profiler."""
    import collections

    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as p:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    names, dev_us = collections.Counter(), 0.0
    for e in p.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and e.name:
            names[e.name] += 1
            dev_us += e.device_time_total if hasattr(e, 'device_time_total') else e.cuda_time_total
    return sum(names.values()) / reps, dev_us / 1e3 / reps, names


def _syncs(fn):
    """Synchronising torch calls of one ``fn()``: the warnings of torch's sync debug mode."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    return sum('synchroniz' in str(w.message).lower() for w in caught)


def reference_poses(sensor2egos, ego2globals, rots, trans, intrins, post_rots, post_trans, bda, T):
    """The reference's formulation: bevdet.py:435-456 and one ``get_mlp_input`` per frame."""
    import torch
    from ocrfdet_amd.view_transformer_ocrf import OcRFViewTransformerFull
    keyego2global = ego2globals[:, 0, 0, ...].unsqueeze(1).unsqueeze(1)
    global2keyego = torch.inverse(keyego2global.double())
    sensor2keyegos = (global2keyego @ ego2globals.double() @ sensor2egos.double()).float()
    curr2adj = torch.inverse(ego2globals[:, 1:T + 1].double() @ sensor2egos[:, 1:T + 1].double()) \
        @ ego2globals[:, :T].double() @ sensor2egos[:, :T].double()
    mlp = [OcRFViewTransformerFull.get_mlp_input(None, rots[:, 0], trans[:, 0], intrins[:, f], post_rots[:, f],
                                                 post_trans[:, f], bda) for f in range(sensor2egos.shape[1])]
    return sensor2keyegos, curr2adj.float(), mlp


def run_poses(iters):
    import torch
    from time_bev_encoder import _wall
    from ocrfdet_amd import detector
    dev = torch.device('cuda:0')
    B, N, F, T = 8, N_CAMS, N_FRAMES, N_FRAMES - 1
    inp = img_inputs(B, N, F, (8, 8), dev)
    rots, trans, intrins, post_rots, post_trans, bda, s2e, e2g = inp[1:9]
    v = lambda t, *s: t.view(B, F, N, *s)         # noqa: E731
    args = (v(s2e, 4, 4), v(e2g, 4, 4), v(rots, 3, 3), v(trans, 3), v(intrins, 3, 3), v(post_rots, 3, 3),
            v(post_trans, 3), bda)
    arms = [('fused (ocrf_frame_poses)', lambda: detector.frame_poses(*args, T, fused=True)),
            ('reference formulation (torch.inverse, get_mlp_input per frame)', lambda: reference_poses(*args, T)),
            ('frame_poses_torch (float64 closed form)', lambda: detector.frame_poses_torch(*args, T))]
    for _, fn in arms:
        for _ in range(5):
            fn()
    a, b = arms[0][1](), arms[1][1]()
    torch.cuda.synchronize()
    err = max(float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max()))
    same = all(torch.equal(a[2][f], b[2][f]) for f in range(F))
    print(f'pose step, B = {B}, N = {N}, F = {F}, T = {T}: fused against the reference formulation: max |pose difference| '
          f'{err:.2e}, mlp_input bit-equal: {same}')
    walls = _wall([fn for _, fn in arms], iters)
    for (name, fn), (best, median) in zip(arms, walls):
        launches, dev_ms, names = _profile(fn)
        print(f'  {name}: {dev_ms * 1e3:.1f} us device, {launches:.0f} launches, wall best {best * 1e3:.1f} / median '
              f'{median * 1e3:.1f} us, {_syncs(fn)} synchronisations')
        if 'fused' in name:
            print(f'    kernels: {dict(names)}')


def run_detector(mode, iters):
    import random

    import torch
    from time_bev_encoder import _wall
    from ocrfdet_amd import detector
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    det = detector.OcRFDet4D(**reference_model()).to(dev)
    train = mode != 'forward'
    B = 2 if train else 1
    inp = img_inputs(B, N_CAMS, N_FRAMES, INPUT_SIZE, dev)
    H, W = INPUT_SIZE
    gen = torch.Generator().manual_seed(1)
    gt = dict(gt_depth=(torch.rand(B, N_CAMS, H, W, generator=gen) * 70 * (torch.rand(B, N_CAMS, H, W, generator=gen) < 0.05)),
              gt_semantic=(torch.rand(B, N_CAMS, H, W, generator=gen) < 0.05).float(),
              gt_bev_mask=(torch.rand(B, 128, 128, generator=gen) < 0.1).float())
    gt = {k: t.to(dev) for k, t in gt.items()}
    boxes = [torch.tensor([[4.0, -6.0, -1.0, 1.9, 4.5, 1.6, 0.3, 0.5, -0.2], [-18.0, 29.5, -1.2, 0.7, 0.7, 1.8, 1.0, 0.0, 0.0]],
                          device=dev)] * B
    labels = [torch.tensor([0, 8], device=dev)] * B
    boxes_2d = [[torch.tensor([[100.0, 80.0, 300.0, 200.0]], device=dev) for _ in range(N_CAMS)]] * B
    det.train(train)

    def arm(fused):
        def run():
            det.fused_poses = fused
            random.seed(0)
            if not train:
                with torch.no_grad():
                    return det.forward_dummy(img_inputs=inp)
            det.zero_grad(set_to_none=True)
            losses = det(return_loss=True, img_inputs=inp, gt_bboxes_3d=boxes, gt_labels_3d=labels, gt_bboxes=boxes_2d, **gt)
            sum(losses.values()).backward()
        return run
    fused, plain = arm(True), arm(False)
    for fn in (fused, plain):
        for _ in range(3):
            fn()
    (fb, fm), (pb, pm) = _wall([fused, plain], iters, blocks=3)
    fl, fd, _ = _profile(fused, reps=2)
    pl, pd, _ = _profile(plain, reps=2)
    print(f'OcRFDet4D, reference config, B = {B}, {mode}: fused_poses on {fd:.2f} ms device, {fl:.0f} launches, wall best '
          f'{fb:.2f} / median {fm:.2f} ms, {_syncs(fused)} synchronisations | off {pd:.2f} ms device, {pl:.0f} launches, '
          f'wall best {pb:.2f} / median {pm:.2f} ms, {_syncs(plain)} synchronisations')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--limit', type=int, default=300, help='seconds per case')
    ap.add_argument('--case', type=int, default=None, help='(internal) run this one case in this process')
    a = ap.parse_args()
    if a.case is not None:
        import torch
        assert torch.cuda.is_available(), 'timing needs the GPU: there is no CPU fallback for a measurement'
        if a.case == 0:
            run_poses(a.iters * 10)
        else:
            run_detector(CASES[a.case].split(' ', 1)[1], max(a.iters // 4, 2))
        return 0
    lines = []
    for k in range(len(CASES)):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', str(k), '--iters', str(a.iters)],
                               stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f'case {CASES[k]} ran out of its {a.limit} s: stopping', file=sys.stderr)
            return 124
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f'case {CASES[k]} ended with status {p.returncode}: stopping', file=sys.stderr)
            return p.returncode or 1
        lines.append(p.stdout)
    if a.out:
        import torch
        with open(a.out, 'w') as f:
            f.write(f'torch {torch.__version__}; the arms alternating block by block; device time and launches from the '
                    'torch profiler; synchronisations: warnings of torch.cuda.set_sync_debug_mode\n' + ''.join(lines))
    return 0


if __name__ == '__main__':
    sys.exit(main())
