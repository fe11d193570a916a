"""GPU: ``OcRFDet4D.stream_step`` over the native modules against the batch forward, on ``tests/test_detector_host.MODEL``
at B = 1 with a sequence of 4 frames: the rig of ``tests/test_detector_gpu.detector_inputs`` in every frame (one
calibration, the streaming step's precondition), the ego moving as ``synthetic.ego_motion``, new images per frame."""
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

from tests import test_detector_gpu as whole      # the shapes and the rig
from tests import test_detector_host as host      # the config dict

pytestmark = pytest.mark.gpu
FRAMES = 4


def frames_of(dev, count=FRAMES):
    """``count`` single-frame 12-entry lists at B = 1, oldest first: frame t was taken ``count - 1 - t`` steps of
    ``synthetic.ego_motion`` behind the last one, from a nuScenes-like global pose."""
    N, H, W = whole.N_CAMS, whole.H_IN, whole.W_IN
    gen = torch.Generator().manual_seed(5)
    rig = synthetic.rig(N, (H, W), 1)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))      # noqa: E731
    yaw = math.radians(35.0)
    G = np.eye(4)
    G[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]]
    G[:3, 3] = [612.5, -1104.25, 2.5]
    frames = []
    for t in range(count):
        e2g = t32(G @ synthetic.ego_motion(count - 1 - t)).view(1, 1, 4, 4).expand(1, N, 4, 4).contiguous()
        raw = torch.rand(1, N, 3, H, W, generator=gen) * 255
        frame = [(raw - 120.0) / 58.0] + [t32(rig[k]) for k in ('rots', 'trans', 'intrins', 'post_rots', 'post_trans')]
        frame += [t32(rig['bda']), t32(rig['c2w']), e2g, raw, raw.clone(), t32(rig['c2w'])]
        frames.append([e.to(dev) for e in frame])
    return frames


def batch_inputs(frames, ids):
    """The multi-frame ``img_inputs`` of the frames ``ids`` (key frame first): images camera-major, poses frame-major."""
    out = []
    for k in range(12):
        if k == 6:
            out.append(frames[ids[0]][6])
        elif k in (0, 9, 10):
            e = torch.stack([frames[i][k] for i in ids], 2)
            out.append(e.reshape(1, -1, *e.shape[3:]))
        else:
            e = torch.stack([frames[i][k] for i in ids], 1)
            out.append(e.reshape(1, -1, *e.shape[3:]))
    return out


def print_stream_against_batch():
    """The body of the child process: every step of the stream and the batch forward on the same frames under
    deterministic convolutions, the neck's camera draw patched to a constant in both arms; one JSON line."""
    torch.backends.cudnn.deterministic = True
    random.randint = lambda a, b: 2
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    det = det_mod.OcRFDet4D(**copy.deepcopy(host.MODEL)).to(dev).eval()
    frames = frames_of(dev)
    backbone_batches = []
    hook = det.img_backbone.register_forward_hook(lambda m, args, out: backbone_batches.append(int(args[0].shape[0])))
    steps, state = [], None
    for t in range(FRAMES):
        del backbone_batches[:]
        if t > 0:                                     # the first step allocates the state and warms the library up
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode('error')
        try:
            (x, depth, _), state = det.stream_step(frames[t], state)
        finally:
            torch.cuda.set_sync_debug_mode('default')
        seen = list(backbone_batches)
        with torch.no_grad():
            want_x, want_depth, _ = det.extract_img_feat(batch_inputs(frames, [t, max(t - 1, 0), max(t - 2, 0)]), None)
        steps.append(dict(backbone=seen, valid=state.valid_host,
                          x=[float((x[0] - want_x[0]).abs().max()), float(want_x[0].abs().max())],
                          depth=[float((depth - want_depth).abs().max()), float(want_depth.abs().max())],
                          shape=list(x[0].shape)))
    hook.remove()
    results, _ = det.simple_test_stream(frames[0], img_metas=[dict()])
    keys = [[list(r), list(r['pts_bbox']), list(r['pts_bbox']['boxes_3d'].shape[1:]), r['pts_bbox']['boxes_3d'].device.type,
             list(r['pts_bbox']['scores_3d'].shape) == list(r['pts_bbox']['labels_3d'].shape)] for r in results]
    print('STREAM ' + json.dumps(dict(steps=steps, results=keys)))


def test_stream_steps_equal_the_batch_forward(cuda):
    """Deterministic convolutions, and therefore a process of its own: see
    ``test_detector_gpu.test_fused_and_torch_poses_give_the_same_losses``.  The steps after the first run under torch's
    sync debug mode set to 'error': a synchronising call ends the child."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = subprocess.run([sys.executable, '-c', 'from tests import test_stream_gpu as t; t.print_stream_against_batch()'],
                           cwd=root, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-3000:]
    line = [ln for ln in child.stdout.splitlines() if ln.startswith('STREAM ')][-1]
    got = json.loads(line[len('STREAM '):])
    assert len(got['steps']) == FRAMES
    for t, step in enumerate(got['steps']):
        print(f'step {t}: x {step["x"][0]:.3e} of {step["x"][1]:.3e}, depth {step["depth"][0]:.3e} of {step["depth"][1]:.3e}')
        assert step['backbone'] == [whole.N_CAMS], step        # one encoder pass, on B * N images
        assert step['valid'] == [1]                             # num_adj = 1
        assert step['shape'] == [1, 16, 48, 48]
        for name in ('x', 'depth'):
            err, largest = step[name]
            assert largest > 0 and err <= 1e-5 * largest, (t, name, err, largest)
    assert got['results'] == [[['pts_bbox'], ['boxes_3d', 'scores_3d', 'labels_3d'], [9], 'cpu', True]]


def test_new_sequence_flags_reach_the_device_without_a_synchronisation(cuda):
    """A step with mixed ``new_sequence`` flags uploads them from pinned memory, asynchronously, and selects the cached
    or the own stereo feature and poses per sample on the device: neither may synchronise."""
    from ocrfdet_amd import streaming
    B, N = 3, 2
    gen = torch.Generator().manual_seed(1)
    own, cached = (torch.randn(B * N, 4, 3, 5, generator=gen).to(cuda) for _ in range(2))
    own_pose, cached_pose = (torch.randn(B, N, 4, 4, generator=gen).to(cuda) for _ in range(2))
    valid = torch.tensor([2, 1, 2], dtype=torch.int32, device=cuda)
    flags = [False, True, False]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        mask = streaming._upload(flags, cuda)
        feat = streaming._select(mask, own, cached)
        pose = streaming._select(mask, own_pose, cached_pose)
        valid.masked_fill_(mask, 0)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert mask.tolist() == flags and valid.tolist() == [2, 0, 2]
    assert torch.equal(feat.view(B, N, 4, 3, 5)[1], own.view(B, N, 4, 3, 5)[1])
    assert torch.equal(feat.view(B, N, 4, 3, 5)[[0, 2]], cached.view(B, N, 4, 3, 5)[[0, 2]])
    assert torch.equal(pose[1], own_pose[1]) and torch.equal(pose[[0, 2]], cached_pose[[0, 2]])
