"""CPU: the lifecycle of ``_lib.StepCache`` — eager, recorded, replayed; a recording dropped when the scratch generation
moves; refusals — driven with stand-ins for the recorder, the memory pool and the scratch generation (no launch)."""
import contextlib
import types

import pytest
import torch

from ocrfdet_amd import _lib

STREAMS = [types.SimpleNamespace(cuda_stream=11), types.SimpleNamespace(cuda_stream=22)]


@pytest.fixture
def fake(monkeypatch):
    """``generation``: what ``workspace.generation`` reports; ``refuse``: why the next recordings fail (None: they do
    not); ``replay``: what a replay does to the outputs; ``replays``: the raw streams of every replay."""
    state = types.SimpleNamespace(generation=0, refuse=None, recordings=0, replay=lambda: None, replays=[])

    class Step:
        def run(self, *raw):
            state.replays.append(raw)
            state.replay()

    class Recorder:
        def __init__(self, streams):
            assert streams is STREAMS
            self.ok, self.why = state.refuse is None, state.refuse
            state.recordings += 1

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def build(self):
            assert self.ok
            return Step()
    monkeypatch.setattr(_lib, 'StepRecorder', Recorder)
    monkeypatch.setattr(torch.cuda, 'MemPool', object)
    monkeypatch.setattr(torch.cuda, 'use_mem_pool', lambda pool, device: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda device=None: None)
    monkeypatch.setattr(_lib.workspace, 'generation', lambda device: state.generation)
    return state


def _step(out, log, during_recording=lambda: None):
    def fn(rec):
        log.append('eager' if rec is None else 'recorded')
        if rec is not None:
            during_recording()
        return out
    return fn


def test_first_sighting_runs_eagerly_the_second_records_the_third_replays(fake):
    cache, out, log = _lib.StepCache('cuda:0', size=4, seen_size=16), (torch.ones(3),), []
    fn = _step(out, log)
    got = [cache('k', STREAMS, fn) for _ in range(4)]
    assert log == ['eager', 'recorded'] and fake.replays == [(11, 22), (11, 22)]
    assert all(g is out for g in got) and len(cache) == 1 and cache.refused is None
    assert next(iter(cache.values())).outputs is out
    cache('other', STREAMS, fn)                                  # another key starts over
    assert log == ['eager', 'recorded', 'eager'] and len(cache) == 1
    cache.clear()                                                # forgets the recordings and the first sightings
    cache('k', STREAMS, fn)
    assert not cache and log[-1] == 'eager'


def test_a_moved_generation_makes_a_new_recording(fake):
    cache, log = _lib.StepCache('cuda:0', size=4, seen_size=16), []
    fn = _step((torch.ones(3),), log)
    for _ in range(3):
        cache('k', STREAMS, fn)
    fake.generation += 1                                         # a scratch buffer the recording points into was replaced
    cache('k', STREAMS, fn)
    assert log == ['eager', 'recorded', 'recorded'] and fake.recordings == 2 and len(fake.replays) == 1
    cache('k', STREAMS, fn)
    assert len(fake.replays) == 2 and next(iter(cache.values())).generation == 1


def test_a_recording_during_which_the_generation_moved_is_not_stored(fake):
    cache, log = _lib.StepCache('cuda:0', size=4, seen_size=16), []
    moves = [1]

    def grow():                                                  # the first recording replaces a scratch buffer
        fake.generation += moves.pop() if moves else 0
    fn = _step((torch.ones(3),), log, grow)
    for _ in range(2):
        cache('k', STREAMS, fn)
    assert log == ['eager', 'recorded'] and not cache
    cache('k', STREAMS, fn)                                      # recorded again, this time with a steady generation
    assert log[-1] == 'recorded' and len(cache) == 1 and not fake.replays
    cache('k', STREAMS, fn)
    assert log[-1] == 'recorded' and len(fake.replays) == 1


def test_a_refused_recording_stays_eager_and_says_why(fake):
    cache, log = _lib.StepCache('cuda:0', size=4, seen_size=16), []
    fake.refuse = 'ocrf_x cannot be held by a step object'
    fn = _step((torch.ones(3),), log)
    for _ in range(4):
        cache('k', STREAMS, fn)
    assert log == ['eager', 'recorded', 'eager', 'eager'] and not cache and not fake.replays
    assert cache.refused == 'ocrf_x cannot be held by a step object'


def test_the_first_replay_is_held_to_the_eager_step_bit_for_bit(fake):
    nan = torch.tensor([1.0, float('nan'), -0.0])
    cache, log = _lib.StepCache('cuda:0', size=4, seen_size=16, check=lambda out: out), []
    fn = _step((nan,), log)
    for _ in range(3):
        cache('k', STREAMS, fn)
    assert len(cache) == 1 and cache.refused is None             # a NaN that reproduces itself is accepted
    assert log == ['eager', 'recorded'] and len(fake.replays) == 2

    for changed in (float('nan'), 0.0):
        out = (torch.tensor([1.0, 2.0, -0.0]),)
        cache, log = _lib.StepCache('cuda:0', size=4, seen_size=16, check=lambda out: out), []
        fake.replay = lambda: out[0].__setitem__(2, changed)     # a replay that misses a launch: another value
        fn = _step(out, log)
        for _ in range(3):
            cache('k', STREAMS, fn)
        assert not cache and 'did not reproduce' in cache.refused, changed
        assert log == ['eager', 'recorded', 'eager', 'eager']   # the step is issued again after the bad replay


def test_the_tables_stay_bounded(fake):
    cache, log = _lib.StepCache('cuda:0', size=2, seen_size=3, check=None), []
    fn = _step((torch.ones(1),), log)
    for key in 'abc':
        cache(key, STREAMS, fn)
        cache(key, STREAMS, fn)
    assert len(cache) == 2 and len(cache._seen) == 3              # 'a', the oldest recording, made room for 'c'
    cache('c', STREAMS, fn)
    assert len(fake.replays) == 1
    cache('d', STREAMS, fn)
    assert len(cache._seen) == 1                                  # the first sightings were forgotten to make room
