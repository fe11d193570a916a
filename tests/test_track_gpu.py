"""GPU: ``ocrf_track_step`` (csrc/track_assoc.hip) through ``tracking.track_step`` against the sequential float64 oracle
of ``tests/track_oracle.py``: ``ids``, ``hits``, ``count``, ``next_id`` and every state array bit-equal over sequences of
7 frames (both sides do IEEE float64 in the same order without contraction: equality is the condition).

The scenes (B = 3, 10 classes, M = 40, D = 9, max_age = 3; ``track_oracle.SCENES``, each with the property it is there
for asserted on the oracle's own results by ``check_scene``):
``crowd``: one class holds 30 of the 40 rows and its live tracks pass 64, so a lane walks more than one track;
``counts``: one sample with count 0 throughout, one with M, counts outside [0, M]; ``static``: objects that rest in the
global frame under an ego that yaws and translates around (2000, 1000) m, time lags that differ per sample; ``all_new``:
the state fills up to exactly max_age * M; ``missed``: a track found again after max_age - 1 misses, one lost after
max_age; ``untracked``: labels -1, 10 and beyond, radius-0 classes, NaN and inf centres and velocities, low scores;
``restart``: mixed ``new_sequence`` at frame 3; ``d7``: boxes without velocity.  The oracle of a scene is computed once
and shared with ``tests/test_track_host.py``.
"""
import copy
import math

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib, tracking
from tests import test_track_host as host
from tests import track_oracle as to

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(to.SCENES))
def test_kernel_equals_the_oracle(cuda, name):
    state = host.follow(name, tracking.track_step, cuda)
    assert state.pos.is_cuda and state.steps == to.FRAMES


@pytest.mark.parametrize('n_classes', [1, 16])
def test_the_smallest_and_the_largest_workgroup(cuda, n_classes):
    """One class runs on two wavefronts (the second ranks the old slots), 16 classes on 1 024 threads."""
    names = [f'class{c}' for c in range(n_classes)]
    radii = [2.0 + 0.5 * c for c in range(n_classes)]

    def world(b, rng, pool=120):
        w = dict(xy=rng.uniform(-40.0, 40.0, (pool, 2)), vxy=rng.normal(0.0, 2.0, (pool, 2)),
                 labels=rng.integers(0, n_classes, pool).astype(np.int32))
        w['seen'] = lambda t, rng: rng.permutation(pool)[:to.M - 3 * b]
        return w
    frames = to.sequence(20 + n_classes, world, frames=4)
    cfg = tracking.TrackConfig(names, max_dist=dict(zip(names, radii)))
    oracle = to.Oracle(to.B, to.M, max_dist=radii)
    state, matched = None, 0
    for t, f in enumerate(frames):
        ids, hits, state = tracking.track_step(*host.tensors(f, cuda), f['time_lag'].tolist(), state=state, cfg=cfg)
        want = oracle.step(f['boxes'], f['scores'], f['labels'], f['counts'], f['ego2global'], f['time_lag'])
        host.assert_step(ids, hits, state, (*want, oracle.arrays()), (n_classes, t))
        matched += int((want[1] > 1).sum())
    assert matched > 0


def test_one_launch_no_synchronisation_and_bit_identical_reruns(cuda, monkeypatch):
    """From frame 2 on a step is exactly one ``_lib.launch`` (``ocrf_track_step``) under torch's sync debug mode set to
    'error' (the mixed flags of frame 3 and the host time lags go up from pinned memory); a second run from a copy of the
    state before frame 2 gives the same bits, and both give the oracle's."""
    s = to.scene('restart')
    cfg = tracking.TrackConfig(**host.CFG)
    frames = [host.tensors(f, cuda) + [torch.from_numpy(f['time_lag']).to(cuda)] for f in s['frames']]
    calls = []
    real = _lib.launch
    monkeypatch.setattr(tracking._lib, 'launch', lambda name, *a, **k: calls.append(name) or real(name, *a, **k))

    def play(state, first, last):
        out = []
        for t in range(first, last):
            lag = s['frames'][t]['time_lag'].tolist() if t % 2 else frames[t][5]
            del calls[:]
            ids, hits, state = tracking.track_step(*frames[t][:5], lag, state=state, cfg=cfg,
                                                   new_sequence=s['frames'][t]['new_sequence'])
            assert calls == ['ocrf_track_step'], (t, calls)
            out.append((ids, hits, {k: v.clone() for k, v in state.current.items()}))
        return out, state
    _, state = play(None, 0, 2)
    start = state.clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        first, _ = play(state, 2, to.FRAMES)
        second, _ = play(start, 2, to.FRAMES)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    for t, ((ids, hits, arrays), (ids2, hits2, arrays2)) in enumerate(zip(first, second), start=2):
        want_ids, want_hits, want = s['want'][t]
        assert to.same_bits(ids.cpu().numpy(), want_ids) and to.same_bits(hits.cpu().numpy(), want_hits), t
        assert torch.equal(ids, ids2) and torch.equal(hits, hits2), t
        for name, array in want.items():
            assert to.same_bits(arrays[name].cpu().numpy(), array), (t, name)
            assert to.same_bits(arrays2[name].cpu().numpy(), array), (t, name)


def test_shapes_beyond_the_kernel_are_refused_before_a_launch(cuda, monkeypatch):
    monkeypatch.setattr(tracking._lib, 'launch', lambda *a, **k: pytest.fail('a launch beyond the LDS limit'))
    M = 628                                                       # 104 * M bytes of LDS at max_age 3: above 64 KiB
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=cuda)     # noqa: E731
    with pytest.raises(ValueError, match='LDS'):
        tracking.track_step(z(1, M, 9), z(1, M), z(1, M, dtype=torch.int32), z(1, dtype=torch.int32), z(1, 4, 4), 0.5,
                            cfg=tracking.TrackConfig(**host.CFG))
    with pytest.raises(ValueError, match='cuda'):                 # time lags on another device
        tracking.track_step(z(1, 8, 9), z(1, 8), z(1, 8, dtype=torch.int32), z(1, dtype=torch.int32), z(1, 4, 4),
                            torch.zeros(1), cfg=tracking.TrackConfig(**host.CFG))


def stream_frames(dev, B, count):
    """``count`` single-frame 12-entry lists at batch B, oldest first: one rig in every frame (the streaming step's
    precondition, ``bda`` the identity), new images per frame, the ego of sample b advancing by
    ``synthetic.ego_motion`` from a nuScenes-like global pose of its own."""
    from ocrfdet_amd import synthetic
    from tests import test_detector_gpu as whole
    N, H, W = whole.N_CAMS, whole.H_IN, whole.W_IN
    gen = torch.Generator().manual_seed(11)
    rig = synthetic.rig(N, (H, W), B)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))      # noqa: E731
    frames = []
    for t in range(count):
        poses = []
        for b in range(B):
            yaw = math.radians(35.0 + 50.0 * b)
            G = np.eye(4)
            G[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]]
            G[:3, 3] = [612.5 + 900.0 * b, -1104.25, 2.5]
            poses.append(G @ synthetic.ego_motion(count - 1 - t))
        e2g = t32(np.stack(poses)).view(B, 1, 4, 4).expand(B, N, 4, 4).contiguous()
        raw = torch.rand(B, N, 3, H, W, generator=gen) * 255
        frame = [(raw - 120.0) / 58.0] + [t32(rig[k]) for k in ('rots', 'trans', 'intrins', 'post_rots', 'post_trans')]
        frame += [t32(rig['bda']), t32(rig['c2w']), e2g, raw, raw.clone(), t32(rig['c2w'])]
        frames.append([e.to(dev) for e in frame])
    return frames


def test_track_stream_on_the_detector(cuda):
    """``OcRFDet4D.track_stream`` on ``tests.test_detector_host.MODEL``, B = 2, 4 frames: no synchronisation from frame 1
    on; the detections are bit-equal to ``get_bboxes_padded`` on the head outputs of the same step; the ids equal the
    oracle on those boxes; ``results_to_host`` trims to the counts."""
    from ocrfdet_amd import detector as det_mod
    from tests import test_detector_host as model
    B, FRAMES, lags = 2, 4, [0.5, 0.25]
    torch.manual_seed(0)
    det = det_mod.OcRFDet4D(**copy.deepcopy(model.MODEL)).to(cuda).eval()
    frames = stream_frames(cuda, B, FRAMES)
    head_outs = []
    hook = det.pts_bbox_head.register_forward_hook(lambda m, args, out: head_outs.append(out))
    results, state, tracks = [], None, None
    try:
        for t in range(FRAMES):
            if t > 0:                                 # the first step allocates both states and warms the library up
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode('error')
            try:
                result, state, tracks = det.track_stream(frames[t], state=state, tracks=tracks, time_lag=lags)
            finally:
                torch.cuda.set_sync_debug_mode('default')
            results.append(result)
    finally:
        hook.remove()
    torch.cuda.synchronize()
    assert len(head_outs) == FRAMES and tracks.steps == FRAMES and state.steps == FRAMES
    cfg = tracking.default_config(det)
    assert cfg.class_names == ('car', 'pedestrian', 'traffic_cone') and cfg.max_dist == (4.0, 1.0, 0.0)
    M = results[0]['boxes'].shape[1]
    oracle = to.Oracle(B, M, max_dist=cfg.max_dist, max_age=cfg.max_age)
    tracked = 0
    for t, (result, outs) in enumerate(zip(results, head_outs)):
        with torch.no_grad():
            want = det.pts_bbox_head.get_bboxes_padded(outs)
        for name, w in zip(('boxes', 'scores', 'labels', 'counts'), want):
            assert result[name].dtype == w.dtype and to.same_bits(result[name].cpu().numpy(), w.cpu().numpy()), (t, name)
        ids, hits = oracle.step(*(result[k].cpu().numpy() for k in ('boxes', 'scores', 'labels', 'counts')),
                                frames[t][8][:, 0].cpu().numpy(), lags)
        assert to.same_bits(result['ids'].cpu().numpy(), ids) and to.same_bits(result['hits'].cpu().numpy(), hits), t
        tracked += int((ids >= 0).sum())
        per_sample = tracking.results_to_host(result)
        counts = result['counts'].tolist()
        assert [len(r['track_ids']) for r in per_sample] == counts == [len(r['boxes_3d']) for r in per_sample]
        for b, r in enumerate(per_sample):
            assert r['boxes_3d'].device.type == 'cpu' and torch.equal(r['track_ids'], result['ids'][b, :counts[b]].cpu())
    assert tracked > 0
    for name, array in oracle.arrays().items():
        assert to.same_bits(getattr(tracks, name).cpu().numpy(), array), name
