"""Host: the hot path's stream map (``_lib.StepStreams`` over every layout ``HotPath._step_streams`` produces), the
planned blend's automatic grid and the names ``hotpath`` re-exports.  No GPU: streams and events are stand-ins."""
import itertools
import types

import pytest

from ocrfdet_amd import _lib, hotpath, neck_path, sharded_hotpath


class _Stream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_event(self, ev):
        self.log.append(('wait_event', self.name, ev.recorded_on))

    def wait_stream(self, other):
        self.log.append(('wait_stream', self.name, other.name))


def _event_type(log):
    class _Event:
        recorded_on = None

        def record(self, stream):
            self.recorded_on = stream.name
            log.append(('record', stream.name))
    return _Event


class _Recorder:
    """``StepRecorder``'s marks, logged."""

    def __init__(self):
        self.items = []

    def fork(self, frm, to):
        self.items.append(('fork', frm, to))

    def join(self, frm, to):
        self.items.append(('join', frm, to))


def _layout(monkeypatch, log, render, render_streams, prep):
    """(streams, names) of the layout, from ``HotPath._step_streams`` itself on a path that has only what it reads."""
    monkeypatch.setattr(hotpath, 'shared_stream', lambda device, role: _Stream(role, log))
    hp = object.__new__(hotpath.HotPath)
    hp.cfg = types.SimpleNamespace(render=render, hoa=True)
    hp.device, hp.overlap, hp.render_streams = 'cpu', True, render_streams
    hp.index_prep_mode, hp.device_geometry, hp._calib_dev = ('per_step', True, []) if prep else ('cached', False, None)
    hp._side, hp._prep_stream, hp._prep_stream2, hp._streams = [], None, None, None
    cur = _Stream('caller', log)
    streams = hp._step_streams(cur)
    assert streams is hp._streams.streams and streams[0] is cur
    assert hp._step_streams(cur) is streams                    # the same object, step after step
    return streams, hp._streams.names


def _issue(ss, n_render, prep):
    """The hand-overs of a step in the order ``_step_eager`` / ``_main_chain`` issue them -> the edges as (kind, frm, to)."""
    edges = [('fork', 'main', f'render{k}') for k in range(n_render)]
    if prep:
        edges += [('fork', 'main', 'prep'), ('fork', 'main', 'prep2'), ('fork', 'prep', 'prep2'),
                  ('join', 'prep', 'main'), ('join', 'prep2', 'main')]
    edges += [('join', f'render{k}', 'main') for k in range(n_render)]
    for kind, frm, to in edges:
        getattr(ss, kind)(frm, to)
    return edges


@pytest.mark.parametrize('render,render_streams,prep', [(r, n, p) for r, n, p in itertools.product(
    (False, True), (1, 2), (False, True)) if r or n == 1])
def test_recorded_marks_are_the_issued_edges_in_every_layout(monkeypatch, render, render_streams, prep):
    log = []
    streams, names = _layout(monkeypatch, log, render, render_streams, prep)
    n_render = render_streams if render else 0
    assert names == ('main',) + tuple(f'render{k}' for k in range(n_render)) + (('prep', 'prep2') if prep else ())
    assert len(streams) == len(names) == 1 + n_render + 2 * prep
    assert [s.name for s in streams[1:]] == (['render', 'render1'][:n_render] + (['prep', 'prep2'] if prep else []))

    rec = _Recorder()
    ss = _lib.StepStreams(streams, names, rec, event=_event_type(log))
    for i, name in enumerate(names):
        assert ss.slot[name] == i and ss[name] is streams[i]                   # a stream's slot is its index in the list
    del log[:]
    edges = _issue(ss, n_render, prep)
    # every edge is one record on `frm` followed by one wait of `to` for THAT event, and nothing else is issued
    issued, slot_of = [], {s.name: i for i, s in enumerate(streams)}
    assert len(log) == 2 * len(edges) and not any(c[0] == 'wait_stream' for c in log)
    for (r_kind, r_on), (w_kind, w_by, w_for) in zip(log[0::2], log[1::2]):
        assert (r_kind, w_kind) == ('record', 'wait_event') and w_for == r_on
        issued.append((slot_of[r_on], slot_of[w_by]))
    assert [(frm, to) for _, frm, to in rec.items] == issued                   # the marks are the edges, in issue order
    assert rec.items == [(kind, ss.slot[frm], ss.slot[to]) for kind, frm, to in edges]

    # without a recorder: the same torch calls; a step later: the same events again (created once per edge)
    with_rec, events = list(log), dict(ss._events)
    del log[:]
    ss.bind(streams[0], None)
    _issue(ss, n_render, prep)
    assert log == with_rec and ss._events == events and len(rec.items) == len(edges)


def test_auto_blend_grid():
    f = hotpath.blend_workgroups_for
    assert f('auto', 0, 512 * 1024 - 1, 256, True) == 704 == 11 * 256 // 4
    assert f('auto', 0, 256 * 704, 256, True) == 704
    assert f('auto', 0, 512 * 1024, 256, True) == 832 == 13 * 256 // 4
    assert f('auto', 1, 512 * 1408, 256, True) == 832
    assert f('auto', 0, 512 * 1408, 256, False) == 0 == f('auto', 0, 256 * 704, 256, False)      # nothing beside the blend
    for beside in (False, True):                                    # an explicit grid passes through, beside or not
        assert f(640, 3, 512 * 1408, 256, beside) == 640 and f(0, 0, 1, 256, beside) == 0
        assert [f((512, 768), f0, 1, 256, beside) for f0 in (0, 1, 5)] == [512, 768, 768]


def test_hotpath_reexports_the_moved_classes():
    assert hotpath.ShardedHotPath is sharded_hotpath.ShardedHotPath
    assert hotpath.NeckPath is neck_path.NeckPath
    from ocrfdet_amd.hotpath import HotPath, NeckPath, PoolPlan, ShardedHotPath, shared_stream  # noqa: F401
    assert ShardedHotPath is sharded_hotpath.ShardedHotPath and NeckPath is neck_path.NeckPath
