"""CPU: ``tracking.track_step_host`` (numpy float64, class by class) against the sequential float64 oracle of
``tests/track_oracle.py``, bit for bit, on the scenes the GPU test runs; three hand-computed cases as literals; refusals.

Both sides do IEEE float64 in the order include/ocrf_hip.h states, without contraction: equality is the condition."""
import numpy as np
import pytest
import torch

from ocrfdet_amd import tracking
from tests import track_oracle as to

CFG = dict(class_names=to.CLASSES, max_age=to.MAX_AGE)


def tensors(frame, device='cpu'):
    return [torch.from_numpy(frame[k]).to(device) for k in ('boxes', 'scores', 'labels', 'counts', 'ego2global')]


def assert_step(got_ids, got_hits, state, want, where):
    """One step's results and every state array against the oracle's, bit for bit."""
    ids, hits, arrays = want
    assert to.same_bits(got_ids.cpu().numpy(), ids), where
    assert to.same_bits(got_hits.cpu().numpy(), hits), where
    for name, array in arrays.items():
        assert to.same_bits(getattr(state, name).cpu().numpy(), array), (where, name)


def follow(name, step, device='cpu'):
    """The scene ``name`` through ``step`` (``track_step`` or ``track_step_host``), every frame against the oracle."""
    to.check_scene(name)
    s = to.scene(name)
    cfg = tracking.TrackConfig(min_score=s['min_score'], **CFG)
    assert cfg.max_dist == to.MAX_DIST
    state = None
    for t, (f, want) in enumerate(zip(s['frames'], s['want'])):
        lag = f['time_lag'].tolist() if t % 2 else torch.from_numpy(f['time_lag']).to(device)
        ids, hits, state = step(*tensors(f, device), lag, state=state, new_sequence=f['new_sequence'], cfg=cfg)
        assert ids.dtype == hits.dtype == torch.int32 and ids.device == hits.device == state.pos.device
        assert_step(ids, hits, state, want, (name, t))
    return state


@pytest.mark.parametrize('name', sorted(to.SCENES))
def test_host_step_equals_the_oracle(name):
    state = follow(name, tracking.track_step_host)
    assert state.steps == to.FRAMES and state.cap == to.MAX_AGE * to.M


def test_cpu_tensors_and_fused_false_take_the_host_step(monkeypatch):
    monkeypatch.setattr(tracking._lib, 'launch', lambda *a, **k: pytest.fail('a launch on CPU tensors'))
    follow('restart', tracking.track_step)
    follow('d7', lambda *a, **k: tracking.track_step(*a, fused=False, **k))


def hand(frames, max_dist=None):
    """``frames``: per frame a list of (x, y) car centres, identity ego, zero velocity; the ids and hits per frame."""
    cfg = tracking.TrackConfig(['car'], max_dist=max_dist)
    state, out = None, []
    for centres in frames:
        boxes = torch.zeros(1, 4, 9)
        boxes[0, :len(centres), :2] = torch.tensor(centres, dtype=torch.float32)
        ids, hits, state = tracking.track_step_host(
            boxes, torch.ones(1, 4), torch.zeros(1, 4, dtype=torch.int32), torch.tensor([len(centres)], dtype=torch.int32),
            torch.eye(4)[None], 0.5, state=state, cfg=cfg)
        out.append((ids[0].tolist(), hits[0].tolist()))
    return out, state


def test_two_detections_contend_for_one_track():
    # one track at (0, 0); row 0 at distance 1 comes first and wins, the nearer row 1 finds nothing else: a new id
    got, state = hand([[(0, 0)], [(1, 0), (0.5, 0)]])
    assert got == [([0, -1, -1, -1], [1, 0, 0, 0]), ([0, 1, -1, -1], [2, 1, 0, 0])]
    assert state.count.tolist() == [2] and state.next_id.tolist() == [2]
    assert state.pos[0, :2].tolist() == [[1.0, 0.0], [0.5, 0.0]] and state.id[0, :2].tolist() == [0, 1]
    # with a second track at (3, 0) the later row takes that one: d2 = 6.25 <= 16
    got, _ = hand([[(0, 0), (3, 0)], [(1, 0), (0.5, 0)]])
    assert got[1] == ([0, 1, -1, -1], [2, 2, 0, 0])


def test_an_exact_tie_goes_to_the_lowest_slot():
    # tracks at (-1, 0) in slot 0 and (1, 0) in slot 1, a detection at (0, 0): d2 = 1 to both
    got, _ = hand([[(-1, 0), (1, 0)], [(0, 0)]])
    assert got[1] == ([0, -1, -1, -1], [2, 0, 0, 0])
    got, state = hand([[(1, 0), (-1, 0)], [(0, 0)]])              # the slots follow the rows, not the coordinates
    assert got[1] == ([0, -1, -1, -1], [2, 0, 0, 0])
    assert state.id[0, :2].tolist() == [0, 1] and state.misses[0, :2].tolist() == [0, 1] and state.hits[0, 1] == 0


def test_a_distance_equal_to_the_radius_matches():
    got, _ = hand([[(0, 0)], [(4, 0)]], max_dist=dict(car=4.0))
    assert got[1] == ([0, -1, -1, -1], [2, 0, 0, 0])              # d2 == r2 == 16
    beyond = float(np.nextafter(np.float32(4), np.float32(5)))
    got, _ = hand([[(0, 0)], [(beyond, 0)]], max_dist=dict(car=4.0))
    assert got[1] == ([1, -1, -1, -1], [1, 0, 0, 0])              # one float32 step further: a new track


def test_a_missed_track_moves_on_with_its_velocity_and_ages_out():
    cfg = tracking.TrackConfig(['car'], max_age=2)
    boxes = torch.zeros(1, 2, 9)
    boxes[0, 0, 7:9] = torch.tensor([2.0, -4.0])
    args = (torch.ones(1, 2), torch.zeros(1, 2, dtype=torch.int32))
    one, none = torch.tensor([1], dtype=torch.int32), torch.tensor([0], dtype=torch.int32)
    _, _, state = tracking.track_step_host(boxes, *args, one, torch.eye(4)[None], 0.5, cfg=cfg)
    _, _, state = tracking.track_step_host(boxes, *args, none, torch.eye(4)[None], 0.25, state=state, cfg=cfg)
    assert state.count.tolist() == [1] and state.pos[0, 0].tolist() == [0.5, -1.0] and state.misses[0, 0] == 1
    _, _, state = tracking.track_step_host(boxes, *args, none, torch.eye(4)[None], 0.25, state=state, cfg=cfg)
    assert state.count.tolist() == [0] and state.next_id.tolist() == [1] and not state.pos.any()


def test_results_to_host_trims_to_the_counts():
    f = to.scene('counts')['frames'][1]                           # counts (-3, M, 17)
    boxes, scores, labels, counts, _ = tensors(f)
    ids = torch.arange(to.B * to.M, dtype=torch.int32).view(to.B, to.M)
    out = tracking.results_to_host(dict(boxes=boxes, scores=scores, labels=labels, counts=counts, ids=ids, hits=ids + 1))
    assert [len(o['track_ids']) for o in out] == [0, to.M, 17]
    assert sorted(out[2]) == ['boxes_3d', 'labels_3d', 'scores_3d', 'track_hits', 'track_ids']
    assert torch.equal(out[2]['boxes_3d'], boxes[2, :17]) and torch.equal(out[2]['track_hits'], ids[2, :17] + 1)


def test_bad_arguments_are_refused_before_any_launch(monkeypatch):
    monkeypatch.setattr(tracking._lib, 'launch', lambda *a, **k: pytest.fail('a launch with bad arguments'))
    f = to.scene('crowd')['frames'][0]
    cfg = tracking.TrackConfig(**CFG)
    good = tensors(f)
    for step in (tracking.track_step, tracking.track_step_host):
        def refused(error, index=None, value=None, **kwargs):
            args = list(good)
            if index is not None:
                args[index] = value
            kwargs.setdefault('cfg', cfg)
            with pytest.raises(error):
                step(*args, kwargs.pop('time_lag', 0.5), **kwargs)
        refused(TypeError, 2, good[2].long())                     # labels int64
        refused(TypeError, 0, good[0].double())
        refused(TypeError, 3, f['counts'])                        # not a tensor
        refused(ValueError, 0, good[0][:, :, :8])                 # D = 8
        refused(ValueError, 1, good[1][:, :-1])
        refused(ValueError, 3, good[3][:2])
        refused(ValueError, 4, good[4][:, :3])
        refused(ValueError, time_lag=[0.5, 0.5])
        refused(ValueError, time_lag=[0.5, float('nan'), 0.5])
        refused(ValueError, time_lag=torch.zeros(2))
        refused(TypeError, time_lag=torch.zeros(3, dtype=torch.float64))
        refused(TypeError, time_lag=None)
        refused(ValueError, new_sequence=[True])
        refused(TypeError, cfg=None)
        refused(TypeError, cfg=dict(CFG))
        refused(TypeError, state=object())
    for bad in (dict(class_names=[]), dict(class_names=['c'] * 17), dict(class_names=['car'], max_age=0),
                dict(class_names=['car'], max_age=1.5), dict(class_names=['car'], max_dist=dict(bus=1.0)),
                dict(class_names=['car'], max_dist=dict(car=-1.0)),
                dict(class_names=['car'], max_dist=dict(car=float('nan'))),
                dict(class_names=['car'], min_score=float('inf')), dict(class_names=[1, 2])):
        with pytest.raises(ValueError):
            tracking.TrackConfig(**bad)
    with pytest.raises(TypeError):
        tracking.TrackConfig(['car'], max_dist=[4.0])


def test_the_header_declares_the_entry_point_and_the_library_refuses_bad_sizes():
    """Argument validation alone: the calls return before anything is launched."""
    import ctypes
    from ocrfdet_amd import _lib
    protos = _lib.prototypes()
    assert 'ocrf_track_step' in _lib._ENQUEUEING and 'ocrf_track_step_lds_bytes' not in _lib._ENQUEUEING
    assert protos['ocrf_track_step'][1][5] is ctypes.c_float and len(protos['ocrf_track_step'][1]) == 34
    L = _lib.lib()
    assert L.ocrf_kernel_name(_lib.K_TRACK_STEP) == b'track_step_kernel'
    assert L.ocrf_track_step_lds_bytes(498, 3 * 498) == 32 * 498 + 24 * 3 * 498 <= _lib.OCRF_TRACK_MAX_LDS
    assert L.ocrf_track_step_lds_bytes(0, 3) == 0 and L.ocrf_track_step_lds_bytes(628, 3 * 628) > _lib.OCRF_TRACK_MAX_LDS
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)

    def call(B=3, M=40, D=9, n_classes=10, max_age=3, min_score=0.0, cap=120, boxes=p, new_sequence=None, pos_out=q):
        return L.ocrf_track_step(B, M, D, n_classes, max_age, min_score, cap, boxes, p, p, p, p, p, new_sequence, p,
                                 p, p, p, p, p, p, p, p, pos_out, q, q, q, q, q, q, q, p, p, None)
    invalid = 1
    for bad in (dict(B=0), dict(B=65536), dict(M=0), dict(D=8), dict(n_classes=0), dict(n_classes=17), dict(max_age=0),
                dict(cap=119), dict(M=628, cap=3 * 628), dict(boxes=None), dict(pos_out=p), dict(pos_out=None),
                dict(min_score=float('nan'))):
        assert call(**bad) == invalid, bad
