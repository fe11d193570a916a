"""CPU: ``OcRFDet4D.stream_step`` against the batch forward, with the stand-in sub-modules of
``tests/golden/make_golden_detector.py`` (loaded as ``tests/test_detector_host.py`` loads them).

A sequence of K + 3 frames with one calibration for all frames (the streaming step's precondition) and a different ego
pose, different images per frame.  Step t must reproduce ``extract_img_feat`` (eval) on the frames
(t, max(t - 1, 0), ..., max(t - K - 1, 0)) within 1e-6, the stand-in tests' own tolerance."""
import numpy as np
import pytest
import torch

from ocrfdet_amd import detector as det_mod
from ocrfdet_amd import streaming
from tests import test_detector_host as host

GS = host.GS
B, N = GS.B, GS.N
IMAGE_ENTRIES = (0, 9, 10)                        # of the 12-entry list: (B, N * F, ...) camera-major; 6 is bda,
                                                  # every other entry (B, F * N, ...) frame-major


def sequence(length, seed=0):
    """``length`` single-frame 12-entry lists: the generator's inputs for that many frames, with frame 0's intrinsics and
    image augmentation in every frame (the mounts and ``bda`` are per sample already)."""
    inputs = GS.make_inputs(seed=GS.SEED + 100 + seed, f=length)
    frames = []
    for t in range(length):
        frame = []
        for k, e in enumerate(inputs):
            if k == 6:
                frame.append(e)
            elif k in IMAGE_ENTRIES:
                frame.append(e.view(B, N, length, *e.shape[2:])[:, :, t].contiguous())
            else:
                frame.append(e.view(B, length, N, *e.shape[2:])[:, t].contiguous())
        frames.append(frame)
    for frame in frames:
        for k in (3, 4, 5):
            frame[k] = frames[0][k]
    return frames


def batch_inputs(frames, ids):
    """The multi-frame ``img_inputs`` of the frames ``ids`` (key frame first)."""
    out = []
    for k in range(12):
        if k == 6:
            out.append(frames[ids[0]][6])
        elif k in IMAGE_ENTRIES:
            e = torch.stack([frames[i][k] for i in ids], 2)                    # (B, N, F, ...)
            out.append(e.reshape(B, N * len(ids), *e.shape[3:]))
        else:
            e = torch.stack([frames[i][k] for i in ids], 1)                    # (B, F, N, ...)
            out.append(e.reshape(B, len(ids) * N, *e.shape[3:]))
    return out


def stand_in_detector(num_adj=1, align=False, with_prev=True):
    det = det_mod.OcRFDet4D(img_backbone=GS.StandInBackbone(), img_neck=GS.StandInNeck(),
                            img_view_transformer=GS.StandInViewTransformer(), pre_process=GS.StandInPreProcess(),
                            img_bev_encoder_backbone=GS.StandInBEVBackbone(), img_bev_encoder_neck=GS.StandInBEVNeck(),
                            num_adj=num_adj, with_prev=with_prev, align_after_view_transfromation=align)
    return det.eval()


def history(t, K):
    return [max(t - a, 0) for a in range(K + 2)]


def assert_same(got, want, what):
    x, depth, bev_mask = got
    wx, wdepth, wmask = want
    for name, a, b in (('x', x[0], wx[0]), ('depth', depth, wdepth), ('bev_mask0', bev_mask[0], wmask[0]),
                       ('bev_mask1', bev_mask[1], wmask[1])):
        assert a.shape == b.shape, (what, name)
        err = float((a - b).abs().max())
        assert err <= 1e-6, (what, name, err)


def test_sequence_helper_gives_distinct_frames_with_one_calibration():
    frames = sequence(4)
    assert not torch.equal(frames[0][0], frames[1][0]) and not torch.equal(frames[0][8], frames[2][8])
    assert all(torch.equal(f[3], frames[0][3]) and torch.equal(f[1], frames[0][1]) for f in frames)
    back = streaming.key_frame_inputs(batch_inputs(frames, [2, 1, 0]), 3)
    assert all(torch.equal(a, b) for a, b in zip(back, frames[2]))


@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('K', [1, 2])
def test_every_step_reproduces_the_batch_forward(K, align):
    frames = sequence(K + 3, seed=K)
    stream, batch = stand_in_detector(K, align), stand_in_detector(K, align)
    assert stream.num_frame == K + 2
    state = None
    for t in range(K + 3):
        del stream.img_backbone.log[:], stream.img_view_transformer.log[:]
        got, state = stream.stream_step(frames[t], state)
        # one encoder pass (the backbone's forward evaluates layer1 itself) and one view transformer call per step
        assert stream.img_backbone.log == ['forward', 'layer1']
        assert [e['prev_is_none'] for e in stream.img_view_transformer.log] == [False]
        assert [e['grad'] for e in stream.img_view_transformer.log] == [False]
        want = batch.extract_img_feat(batch_inputs(frames, history(t, K)), None)
        assert len(batch.img_view_transformer.log) == (K + 1) * (t + 1)
        assert_same(got, want, f'K={K} align={align} step {t}')
        assert state.valid_host == [min(t + 1, K)] * B and state.valid.tolist() == state.valid_host
        assert state.head == (t + 1) % (K + 1) and state.steps == t + 1
    # the multi-frame list is accepted too: frame 0 of each entry is taken
    again, _ = stand_in_detector(K, align).stream_step(batch_inputs(frames, history(0, K)), None, multi_frame=True)
    first, _ = stand_in_detector(K, align).stream_step(frames[0], None)
    assert torch.equal(again[0][0], first[0][0])


@pytest.mark.parametrize('align', [False, True])
def test_a_new_sequence_restarts_one_sample_and_leaves_the_other(align):
    K = 2
    a, b = sequence(K + 3, seed=7), sequence(K + 3, seed=8)
    stream, alone, fresh = (stand_in_detector(K, align) for _ in range(3))
    state = ref_state = None
    for t in range(3):
        got, state = stream.stream_step(a[t], state)
        want, ref_state = alone.stream_step(a[t], ref_state)
    # step 3: sample 1 starts sequence b, sample 0 goes on with sequence a
    mixed = [torch.cat([a[3][k][:1], b[0][k][1:]]) for k in range(12)]
    got, state = stream.stream_step(mixed, state, new_sequence=[False, True])
    want, ref_state = alone.stream_step(a[3], ref_state)
    start, _ = fresh.stream_step(b[0], None)
    for g, w, s in ((got[0][0], want[0][0], start[0][0]), (got[1], want[1], start[1])):
        assert torch.equal(g[:1], w[:1])                          # untouched: bit for bit what it would have been
        assert float((g[1:] - s[1:]).abs().max()) <= 1e-6         # its t = 0 result
    assert state.valid_host == [K, 1] and state.valid.tolist() == [K, 1]
    # and the restarted sample goes on as a sequence of its own
    mixed = [torch.cat([a[4][k][:1], b[1][k][1:]]) for k in range(12)]
    got, state = stream.stream_step(mixed, state)
    batch = stand_in_detector(K, align)
    want_b = batch.extract_img_feat(batch_inputs(b, history(1, K)), None)
    want_a = batch.extract_img_feat(batch_inputs(a, history(4, K)), None)
    assert float((got[0][0][1:] - want_b[0][0][1:]).abs().max()) <= 1e-6
    assert float((got[0][0][:1] - want_a[0][0][:1]).abs().max()) <= 1e-6
    with pytest.raises(ValueError, match='new_sequence'):
        stream.stream_step(mixed, state, new_sequence=[True])


def test_training_mode_raises_and_the_old_names_stay_closed():
    frames = sequence(3)
    det = stand_in_detector().train()
    with pytest.raises(RuntimeError, match='eval'):
        det.stream_step(frames[0])
    with pytest.raises(RuntimeError):
        det.simple_test_stream(frames[0])
    det.eval()
    with pytest.raises(NotImplementedError):
        det.extract_img_feat(batch_inputs(frames, [0, 0, 0]), None, sequential=True, feat_prev=None)
    with pytest.raises(NotImplementedError):
        det.extract_img_feat(batch_inputs(frames, [0, 0, 0]), None, pred_prev=True)
    with pytest.raises(ValueError, match='ONE frame'):
        det.stream_step([t[None] for t in frames[0]])


@pytest.mark.parametrize('align', [False, True])
def test_without_previous_frames_the_step_is_the_batch_forward(align):
    """``with_prev=False``: zeros and the key frame, no state.  The batch forward hands the key frame ``k2s_sensor`` of
    its frame 1 all the same, so the frame is repeated there: the step knows no other."""
    frames = sequence(3, seed=3)
    stream, batch = stand_in_detector(1, align, with_prev=False), stand_in_detector(1, align, with_prev=False)
    for t in (0, 2):
        got, state = stream.stream_step(frames[t], None)
        assert state is None
        want = batch.extract_img_feat(batch_inputs(frames, [t, t, t]), None)
        assert_same(got, want, f'no history, frame {t}')
        assert torch.equal(got[0][0][:, :2], torch.zeros(B, 2, 4, 4))
    assert stream.img_backbone.log == ['forward', 'layer1'] * 2
    assert [e['prev_is_none'] for e in stream.img_view_transformer.log] == [True, True]


def test_simple_test_stream_returns_the_result_dicts():
    det = host.head_detector().eval()
    frames = sequence(3, seed=5)
    state = None
    for t in range(2):
        results, state = det.simple_test_stream(frames[t], state=state)
        assert len(results) == B and state.steps == t + 1
        for r in results:
            assert list(r) == ['pts_bbox'] and list(r['pts_bbox']) == ['boxes_3d', 'scores_3d', 'labels_3d']
            boxes, scores, labels = r['pts_bbox'].values()
            assert boxes.shape[1:] == (9,) and scores.shape == labels.shape == (boxes.shape[0],)
    with torch.no_grad():
        want = det(return_loss=False, img_inputs=batch_inputs(frames, [1, 0, 0]), img_metas=[dict() for _ in range(B)])
    for r, w in zip(results, want):
        assert r['pts_bbox']['boxes_3d'].shape == w['pts_bbox']['boxes_3d'].shape
        assert np.abs(r['pts_bbox']['scores_3d'].numpy() - w['pts_bbox']['scores_3d'].numpy()).max() <= 1e-5
