"""GPU: ``ocrf_frame_poses`` against ``frame_poses_torch`` on the device, and the whole ``OcRFDet4D`` over the native
modules at the smallest shape the encoders and the neck accept."""
import copy
import json
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from ocrfdet_amd import detector as det_mod
from ocrfdet_amd import synthetic

from tests import test_detector_host as host      # the fixture loader, the oracle, the bound and the config dict

pytestmark = pytest.mark.gpu
GS = host.GS


def device_pose_args(cuda, b, f, n):
    inputs = GS.make_inputs(seed=GS.SEED + 7 * b + f, b=b, n=n, f=f)
    return [t.to(cuda) for t in host.pose_args(inputs, b, f, n)]


# (3, 9, 6): T = 8, the longest adjacency the alignment benchmarks use; B * F * N = 162 is no multiple of the 64 threads
# of a block and takes three blocks.  (1, 2, 1): two threads.  (2, 3, 2): the shape of the golden data.
@pytest.mark.parametrize('b, f, n', [(1, 2, 1), (2, 3, 2), (3, 9, 6)])
def test_kernel_matches_the_torch_formulation(cuda, b, f, n):
    from torch.profiler import ProfilerActivity, profile
    args, t = device_pose_args(cuda, b, f, n), f - 1
    want = det_mod.frame_poses_torch(*args, t)
    got = det_mod.frame_poses(*args, t, fused=True)              # warm-up: the library's first call
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            again = det_mod.frame_poses(*args, t, fused=True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert len(kernels) == 1 and 'frame_poses_kernel' in kernels[0], kernels
    for name, g, w, a in zip(('sensor2keyegos', 'curr2adjsensor', 'mlp_input'), got, want, again):
        assert g.shape == w.shape and g.dtype == torch.float32 and g.is_contiguous(), name
        assert torch.equal(g, a), f'{name}: a rerun differs'
    assert host.within_one_ulp(got[0].cpu().numpy(), want[0].cpu().numpy()).all()
    assert host.within_one_ulp(got[1].cpu().numpy(), want[1].cpu().numpy()).all()
    assert torch.equal(got[2], want[2])
    # and against the numpy float64 oracle, which shares no code with either
    s2k, c2a = host.oracle_poses(args[0].cpu(), args[1].cpu(), t)
    assert host.within_one_ulp(got[0].cpu().numpy(), s2k).all() and host.within_one_ulp(got[1].cpu().numpy(), c2a).all()


def test_kernel_dispatch_and_limits(cuda):
    from ocrfdet_amd import _lib
    args = device_pose_args(cuda, 2, 3, 2)
    s2k, c2a, mlp = det_mod.frame_poses(*args, 0)                # stereo=False: no adjacency
    assert c2a is None and s2k.shape == (2, 3, 2, 4, 4)
    views = [a.transpose(0, 1).contiguous().transpose(0, 1) for a in args[:7]] + [args[7]]   # not contiguous
    assert all(torch.equal(a, b) for a, b in zip(det_mod.frame_poses(*views, 2), det_mod.frame_poses(*args, 2)))
    grad = [a.clone().requires_grad_(True) for a in args]
    assert det_mod.frame_poses(*grad, 2)[0].requires_grad        # poses that record a gradient: the torch formulation
    with pytest.raises(_lib.OcrfHipError):                       # T >= F is refused by the entry point
        _lib.launch('ocrf_frame_poses', cuda, 2, 3, 2, 3, *args, s2k, s2k, mlp)


# ------------------------------------------------------------------------------------------------ the whole detector
# 64 x 176 (tests/helpers.py CORE_CFG): ResNet-18 gives 4 x 11 at stride 16 and 2 x 6 at stride 32, and CustomFPN's merge
# upsamples to the lateral's size, so odd sizes are fine and 64 x 192 is not needed.  Six cameras, not two: in training the
# neck draws the camera it renders from 0 ... 5, as the reference does (view_transformer_ocrf.py:1081), and picks that
# camera's row on the device; with fewer cameras the draw indexes past the rows.
H_IN, W_IN, N_CAMS = 64, 176, 6
LOSS_KEYS = host.REFERENCE_LOSS_KEYS + [f'task{t}.loss_{k}' for t in range(2)
                                        for k in ('xy', 'z', 'whl', 'yaw', 'vel', 'heatmap')]


def detector_inputs(dev, B):
    F = 3
    gen = torch.Generator().manual_seed(3)
    rig = synthetic.rig(N_CAMS, (H_IN, W_IN), B)
    per_frame = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).unsqueeze(1).expand(   # noqa: E731
        B, F, *a.shape[1:]).reshape(B, F * N_CAMS, *a.shape[2:]).contiguous()
    yaw = math.radians(35.0)
    G = np.eye(4)
    G[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]]
    G[:3, 3] = [612.5, -1104.25, 2.5]                            # a nuScenes-like global pose
    e2g = np.stack([G @ synthetic.ego_motion(f) for f in range(F)]).astype(np.float32)      # (F, 4, 4)
    e2g = torch.from_numpy(e2g).view(1, F, 1, 4, 4).expand(B, F, N_CAMS, 4, 4).reshape(B, F * N_CAMS, 4, 4).contiguous()
    raw = torch.rand(B, N_CAMS * F, 3, H_IN, W_IN, generator=gen) * 255
    inputs = [(raw - 120.0) / 58.0] + [per_frame(rig[k]) for k in ('rots', 'trans', 'intrins', 'post_rots', 'post_trans')]
    inputs += [torch.from_numpy(rig['bda']), per_frame(rig['c2w']), e2g, raw, raw.clone(), per_frame(rig['c2w'])]
    gt_depth = torch.rand(B, N_CAMS, H_IN, W_IN, generator=gen) * 70 * (torch.rand(B, N_CAMS, H_IN, W_IN, generator=gen) < 0.3)
    kw = dict(gt_depth=gt_depth, gt_semantic=(torch.rand(B, N_CAMS, H_IN, W_IN, generator=gen) < 0.3).float(),
              gt_bev_mask=(torch.rand(B, 48, 48, generator=gen) < 0.2).float())
    boxes = [torch.tensor([[4.0, -6.0, -1.0, 1.9, 4.5, 1.6, 0.3, 0.5, -0.2], [-8.0, 9.5, -1.2, 0.7, 0.7, 1.8, 1.0, 0.0, 0.0]])
             for _ in range(B)]
    labels = [torch.tensor([0, 1]) for _ in range(B)]
    boxes_2d = [[torch.tensor([[10.0, 8.0, 90.0, 50.0]]).to(dev) for _ in range(N_CAMS)] for _ in range(B)]
    return ([t.to(dev) for t in inputs], {k: v.to(dev) for k, v in kw.items()}, [b.to(dev) for b in boxes],
            [l.to(dev) for l in labels], boxes_2d)


def build_detector(dev, B):
    """The detector of ``host.MODEL`` with seeded weights, its inputs, and ``losses_of(fused_poses, images=None)``."""
    torch.manual_seed(0)
    det = det_mod.OcRFDet4D(**copy.deepcopy(host.MODEL)).to(dev)
    inputs, gt, boxes, labels, boxes_2d = detector_inputs(dev, B)

    def losses_of(fused_poses, images=None):
        det.fused_poses = fused_poses
        torch.manual_seed(1)                                     # the neck's dropout
        random.seed(1)                                           # and its random camera
        inp = inputs if images is None else [images] + inputs[1:]
        return det(return_loss=True, img_inputs=inp, gt_bboxes_3d=boxes, gt_labels_3d=labels, gt_bboxes=boxes_2d,
                   **gt)
    return det, inputs, losses_of


def print_losses_of_both_pose_paths():
    """The body of the child process of ``test_whole_detector_trains_and_tests``: the training-mode losses with the
    kernel's poses and with the torch formulation's, under deterministic convolutions, as one JSON line."""
    torch.backends.cudnn.deterministic = True
    det, _, losses_of = build_detector(torch.device('cuda:0'), 2)
    det.train()
    with torch.no_grad():
        fused, plain = losses_of(True), losses_of(False)
    print('LOSSES ' + json.dumps([{k: float(v) for k, v in d.items()} for d in (fused, plain)]))


def test_whole_detector_trains_and_tests(cuda):
    # Training runs at B = 2: the neck's MS_CAM puts a batch norm behind a global average pool (B, C, 1, 1), and torch
    # refuses a training-mode batch norm over one value per channel, in the reference's neck as in this one.  The test
    # step below runs at B = 1.
    B = 2
    det, inputs, losses_of = build_detector(cuda, B)
    det.train()
    seen = []
    hook = det.img_view_transformer.register_forward_hook(lambda m, a, out: seen.append(out[0].requires_grad))
    images = inputs[0].clone().requires_grad_(True)
    losses = losses_of(True, images)
    hook.remove()
    assert list(losses) == LOSS_KEYS
    assert all(torch.isfinite(v).all() for v in losses.values()), {k: float(v) for k, v in losses.items()}
    assert seen == [False, True]                                 # the adjacent frame under no_grad, then the key frame
    sum(losses.values()).backward()
    for name in ('img_backbone.conv1.weight', 'img_neck.lateral_convs.0.conv.weight',
                 'img_view_transformer.depth_net.reduce_conv.0.weight', 'pre_process_net.layers.0.0.conv1.weight',
                 'img_bev_encoder_neck.up2.4.bias', 'pts_bbox_head.shared_conv.conv.weight'):
        g = det.get_parameter(name).grad
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0, name
    # the images are (B, N, F, 3, H, W): a gradient reaches the key frame's and none the other frames'
    g = images.grad.view(B, N_CAMS, 3, 3, H_IN, W_IN)
    assert torch.isfinite(g).all() and g[:, :, 0].abs().max() > 0
    assert torch.equal(g[:, :, 1:], torch.zeros_like(g[:, :, 1:]))

    det.eval()
    det.fused_poses = True
    with torch.no_grad():
        results = det(return_loss=False, img_inputs=[t[:1] for t in inputs], img_metas=[dict()])
    assert len(results) == 1 and list(results[0]['pts_bbox']) == ['boxes_3d', 'scores_3d', 'labels_3d']
    bx, sc, lb = results[0]['pts_bbox'].values()
    assert bx.dim() == 2 and bx.shape[1] == 9 and sc.shape == lb.shape == (bx.shape[0],)


def test_fused_and_torch_poses_give_the_same_losses(cuda):
    """The kernel's poses and the torch formulation's may differ by one ulp: through the whole detector the losses agree
    within 1e-5 relative.  MIOpen's convolutions do not reproduce from run to run by themselves (the same forward twice
    differs by 2e-5 in a loss), so the two forwards run under ``torch.backends.cudnn.deterministic``; and they run in a
    process of their own, because that flag does not stay inside a test: the solvers MIOpen picks under it are kept for
    the process, some of them zero a workspace with a memset, and a later capture of the neck into a hipGraph
    (``GraphedNeck``, tests/test_neck_gpu.py) then refuses the graph for its memset node."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = subprocess.run([sys.executable, '-c', 'from tests import test_detector_gpu as t; '
                            't.print_losses_of_both_pose_paths()'], cwd=root, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-3000:]
    line = [ln for ln in child.stdout.splitlines() if ln.startswith('LOSSES ')][-1]
    fused, plain = json.loads(line[len('LOSSES '):])
    assert list(fused) == list(plain) == LOSS_KEYS
    for k in LOSS_KEYS:
        a, b = fused[k], plain[k]
        print(f'{k}: fused poses {a:.8g}  torch poses {b:.8g}')
        assert abs(a - b) <= 1e-5 * max(abs(a), abs(b)), (k, a, b)
