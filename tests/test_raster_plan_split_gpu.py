"""GPU parity of SPLIT planned renders: ``RasterPlan.render(phase='update')`` followed by ``render(phase='blend', out=...)``
(``ocrf_rasterize_planned`` phase 1 / 2 — what ``HotPath._render_planned(entry, phase=...)`` and tools/timeline_hotpath.py
call), across the states a plan goes through: head only, second pass, deep views with this call's compaction, and back.

The oracle is the per-call pipeline (``rasterize_views``), bit for bit, as for the one-call form in
tests/test_raster_plan_gpu.py: no tolerances anywhere in this file.

What makes the split form different: each of the two host calls chooses by itself, from the pinned host word ``hint`` that the
device writes in a blend's close-out, whether the call compacts (update) and which build of the blend runs (blend).  The two
reads may disagree; the control words (``_ctl``: 19 any deep, 20 this call's compaction ran, 96 + v deep[v]) must make every
combination render this call's image."""
import types

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib
from ocrfdet_amd import diff_gaussian_rasterization as dgr
from ocrfdet_amd import raster_plan as rp
from tests.test_raster_plan_gpu import _cams, _head_mode, _heads, _same, _scene

pytestmark = pytest.mark.gpu

W, H = 176, 80                          # 11 x 5 tiles: the last tile pair has no lower tile
ALL = ('color', 'depth', 'final_T', 'radii')
# Gaussians of the deep scene — that of test_lists_that_never_saturate_are_prepared_once_and_whole, which draws 90 000.  A
# third of that still meets every precondition the tests below assert (hint and deep[v] up for both views after two renders
# of set A, word 20 up after the fourth, per-call images of A and B that differ): the views keep 29 260 and 27 585 records,
# well beyond kDeepReach (8 192) and the default head (4 096), and a bin holds ~ 16 segments of candidates to compact
# (200 383 candidates in 12 bins of (4, 2), kSegC = 1 024).  Measured with 20 000 .. 90 000: all meet them.
N_DEEP = 30000


def _ctl(plan):
    """The control words of the plan's per-call scratch (raster_plan.hip kCtl*): int32 view of its last 1024 bytes."""
    return plan._dyn[plan._dyn.numel() - 1024:].view(torch.int32).cpu().numpy()


def _per_call(xyz, rgb, opac, sc, rot, bg, cams, mode):
    return dgr.rasterize_views(xyz, rgb, opac, sc, rot, None, None, None, None, H, W, bg, depth_mode=mode,
                               packed_cameras=cams, want_n_contrib=False)


def _split(plan, args, **kw):
    o = plan.render(*args, phase='update', **kw)
    return plan.render(*args, phase='blend', out=o, **kw)


class _Scene(types.SimpleNamespace):
    """A scene, its named parameter sets ``sets[name] = (rgb, opac, sc, rot, bg)`` (the arguments of ``render``) and the
    per-call image of each, computed once per (set, depth mode) and never written to."""

    def want(self, name, mode='median'):
        key = (name, mode)
        if key not in self._wants:
            self._wants[key] = _per_call(self.xyz, *self.sets[name], self.cams, mode)
        return self._wants[key]

    def plan(self, bins=(4, 2)):
        return rp.RasterPlan(self.xyz, self.cams, H, W, scales=self.sc, rotations=self.rot, bins=bins)


def _deep_scene(cuda, n):
    """An object-centric opacity field (opacities x 0.01: no pixel saturates, every tile pair walks its whole candidate
    list).  Sets, all within the bound of a plan built with ``scales=sc`` (2 x the extent of ``sc``): A = half the scales,
    B = the scales with the faint opacities in reversed order, dense = the scales with the opacities as drawn."""
    rng = np.random.default_rng(37)
    xyz, rgb, opac, sc, rot = _scene(rng, n, cuda)
    cams = _cams(cuda, W, H, [(0, 0, 0), (1.5, -0.5, 2.0)])
    bg = torch.tensor([0.3, 0.2, 0.1], device=cuda)
    faint = opac * 0.01                                    # every alpha a few times 1/255 at most
    sets = dict(A=(rgb, faint, 0.5 * sc, rot, bg), B=(rgb, faint.flip(0).contiguous(), sc, rot, bg),
                dense=(rgb, opac, sc, rot, bg))
    return _Scene(xyz=xyz, sc=sc, rot=rot, cams=cams, sets=sets, _wants={})


@pytest.fixture(scope='module')
def deep(cuda):
    return _deep_scene(cuda, N_DEEP)


@pytest.fixture(scope='module')
def dense(cuda):
    rng = np.random.default_rng(2)
    xyz, rgb, opac, sc, rot = _scene(rng, 5000, cuda)
    cams = _cams(cuda, W, H, [(0, 0, 0), (1.5, -0.5, 2.0), (-3.0, 0.4, -1.0)])
    bg = torch.tensor([0.1, 0.2, 0.3], device=cuda)
    return _Scene(xyz=xyz, sc=sc, rot=rot, cams=cams, sets=dict(A=(rgb, opac, sc, rot, bg)), _wants={})


@pytest.fixture(autouse=True)
def _adaptive_heads(cuda):
    _head_mode(0)                        # the states asserted below are those of the product default (process-wide knob)


def _go_deep(plan, args):
    """One-call renders until the close-out has told the host that views are deep, then one more: that one compacts."""
    for _ in range(3):
        plan.render(*args)
        torch.cuda.synchronize()
        if int(plan._hint.item()) == 1:
            break
    assert int(plan._hint.item()) == 1
    out = plan.render(*args)
    torch.cuda.synchronize()
    ctl = _ctl(plan)
    assert ctl[20] == 1 and all(ctl[96 + v] == 1 for v in range(plan.V)), ctl[[19, 20, 96, 97]]
    return out


@pytest.mark.parametrize('which,bins', [('dense', None), ('dense', (4, 2)), ('deep', (4, 2)), ('deep', (8, 2)),
                                        ('deep', (6, 3))])
@pytest.mark.parametrize('mode', ['median', 'mean'])
def test_split_render_equals_one_call_equals_per_call(cuda, deep, dense, which, bins, mode):
    """Four split renders in a row, synchronised in between so that each call's host read of ``hint`` sees what the call
    before left.  On the deep scene that takes the plan through: the default head, whose tile pairs the second pass
    finishes and whose close-out marks the views deep; then whole lists prepared by the head kernel and a compaction that
    ran (bins of up to 32 tiles; (6, 3) = 36 tiles has no compaction path, raster_plan.hip "a bin of <= 32 tiles": word 20
    stays 0).  Then the one-call form, then split with the radii as an output (the full head kernel, one blend pass)."""
    scene = deep if which == 'deep' else dense
    args, want = scene.sets['A'], scene.want('A', mode)
    plan = scene.plan(bins)
    for k in range(4):
        got = _split(plan, args, depth_mode=mode)
        torch.cuda.synchronize()
        _same(want, got)
        if which == 'deep':
            ctl = _ctl(plan)
            print(f'render {k}: hint {int(plan._hint.item())} any-deep {ctl[19]} compacted {ctl[20]} '
                  f'deep {[int(x) for x in ctl[96:96 + plan.V]]} heads {_heads(plan)}')
            if k >= 1:
                assert int(plan._hint.item()) == 1 and all(ctl[96 + v] == 1 for v in range(plan.V))
            if k == 3:
                assert ctl[20] == (1 if bins[0] * 2 * bins[1] <= 32 else 0)
    _same(want, plan.render(*args, depth_mode=mode, phase='both'))
    _same(want, _split(plan, args, depth_mode=mode, want_radii=True), ALL)
    _same(want, _split(plan, args, depth_mode=mode))
    torch.cuda.synchronize()
    assert plan.check()


def test_split_render_of_items_and_sets(cuda, deep):
    """The form ``HotPath._render_planned`` uses: S = 2 Gaussian sets (here A and B of the deep scene), an ``item_view`` that
    gives each set a view of its own, ``views_disjoint=True`` (one copy of the per-call arrays, so deep views compact).
    Split equals one call equals the two per-call renders, while the plan goes deep."""
    a, b = deep.sets['A'], deep.sets['B']
    args = tuple(torch.stack((x, y)) for x, y in zip(a[:4], b[:4])) + (a[4],)
    choice = torch.tensor([1, 0], dtype=torch.int32, device=cuda)
    kw = dict(item_view=choice, views_disjoint=True)
    wants = [deep.want('A'), deep.want('B')]
    plan = deep.plan((4, 2))

    def same_items(got, keys=('color', 'depth', 'final_T')):
        for s in range(2):
            v = int(choice[s])
            for k in keys:
                assert torch.equal(wants[s][k][v], got[k][s]), (s, k)

    for _ in range(3):
        same_items(_split(plan, args, **kw))
        torch.cuda.synchronize()
        same_items(plan.render(*args, phase='both', **kw))
        torch.cuda.synchronize()
    ctl = _ctl(plan)
    assert ctl[20] == 1 and ctl[96] == 1 and ctl[97] == 1
    same_items(_split(plan, args, want_radii=True, **kw), ALL)
    torch.cuda.synchronize()
    assert plan.check()


def test_a_blend_after_an_update_ignores_an_earlier_calls_compaction(cuda, deep):
    """The two host calls of a split render read ``hint`` each on its own (raster_plan.hip, ``compact = ... *hint != 0`` in
    ``ocrf_rasterize_planned``), and the device writes the word asynchronously in a blend's close-out (``close_view``).
    The two host writes below stand for exactly that: ``_hint[0] = 0`` before the update is the host reading the word
    BEFORE the previous call's close-out wrote it (no compaction launched), ``_hint[0] = 1`` before the blend is the host
    reading it AFTER (the build with the deep-view code is selected).  The device is idle at both writes and nothing writes
    the word before the next blend's close-out.

    That blend takes a view for compacted when ``ctl[kCtlCompacted]`` (word 20) and ``ctl[kCtlDeep + v]`` are both up
    (``l_deep[v] = ... ctl[kCtlCompacted] != 0 ? ctl[kCtlDeep + v] : 0``).  Before the head kernel cleared word 20 in its
    bookkeeping thread (next to ``a.ctl[kCtlQueue] = 0``), ONLY ``raster_plan_compact_kernel`` wrote it
    (``a.ctl[kCtlCompacted] = on ? 1 : 0``, raster_plan.hip:708 then; the blend's read was line 950), and an update that
    launches no compaction left it at the 1 of the last call that did compact — here a call with set A's smaller rects,
    whose tables lack candidates B needs.  So on that code the ``ctl[20] == 0`` assertion below fails (the word reads 1),
    and the blend behind it would have rendered B from A's tables.

    The mirror case — compaction launched and fresh, plain blend — ends the test."""
    a, b = deep.sets['A'], deep.sets['B']
    want_a, want_b = deep.want('A'), deep.want('B')
    assert not torch.equal(want_a['color'], want_b['color']) and not torch.equal(want_a['final_T'], want_b['final_T'])
    plan = deep.plan((4, 2))
    _same(want_a, _go_deep(plan, a))                       # A's compaction is in the scratch now, word 20 is up
    plan._hint[0] = 0
    o = plan.render(*b, phase='update')
    torch.cuda.synchronize()
    ctl = _ctl(plan)
    assert ctl[20] == 0, 'an update that did not compact left an earlier call\'s "compaction ran" standing'
    assert ctl[96] == 1 and ctl[97] == 1                   # (the views ARE deep: whole lists prepared, plain candidates)
    plan._hint[0] = 1
    got = plan.render(*b, phase='blend', out=o)
    torch.cuda.synchronize()
    _same(want_b, got)
    # mirror: the update compacts (tables of THIS call), the blend-only call reads 0 and launches the plain build
    plan._hint[0] = 1
    o = plan.render(*b, phase='update')
    torch.cuda.synchronize()
    assert _ctl(plan)[20] == 1
    plan._hint[0] = 0
    got = plan.render(*b, phase='blend', out=o)
    torch.cuda.synchronize()
    _same(want_b, got)
    assert int(plan._hint.item()) == 1                     # (the close-out's own word again)
    _same(want_a, _split(plan, a))
    assert plan.check()


def test_alternating_sets_split_and_never_synchronised(cuda, deep):
    """Update + blend pairs on one stream with nothing read or waited for in between: which of the calls compact, and which
    build each blend is, depends on when the host happens to read ``hint`` — every timing must give the same bits."""
    plan = deep.plan((4, 2))
    order = ('A', 'A', 'B', 'dense', 'B', 'A', 'A', 'B', 'A')
    wants = {name: deep.want(name) for name in set(order)}
    torch.cuda.synchronize()
    kept = []
    for name in order:
        got = _split(plan, deep.sets[name])
        kept.append({k: got[k].clone() for k in ('color', 'depth', 'final_T')})
    torch.cuda.synchronize()
    for k, (name, got) in enumerate(zip(order, kept)):
        try:
            _same(wants[name], got)
        except AssertionError as e:
            raise AssertionError(f'call {k} (set {name}): {e}') from None
    assert plan.check()


def test_update_and_blend_on_two_streams(cuda, deep):
    """The usage the ``phase`` docstring names: the update on one stream, the blend on another that waits for the caller's
    event.  Deep scene, after the plan has gone deep (the update compacts, the blend reads its tables)."""
    args, want = deep.sets['A'], deep.want('A')
    plan = deep.plan((4, 2))
    one_call = {k: v.clone() for k, v in _go_deep(plan, args).items() if k != 'status'}
    _same(want, one_call)
    s1, s2 = torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)
    s1.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s1):
        o = plan.render(*args, phase='update')
        done = torch.cuda.Event()
        done.record(s1)
    with torch.cuda.stream(s2):
        s2.wait_event(done)
        got = plan.render(*args, phase='blend', out=o)
    s1.synchronize()
    s2.synchronize()
    assert got is o
    _same(one_call, got)
    assert _ctl(plan)[20] == 1
    assert plan.check()


def test_split_phases_refuse_the_device_guard_and_unknown_names(cuda, dense):
    """``guard='device'`` needs the whole call (the armed chain sits behind the blend): phase 1 / 2 with a guard is
    ``hipErrorInvalidValue`` from the entry point's argument check, in front of every launch.  A phase name the wrapper
    does not know is a ``KeyError``."""
    args = dense.sets['A']
    plan = dense.plan((4, 2))
    want = dense.want('A')
    got = {k: v.clone() for k, v in plan.render(*args).items() if k != 'status'}
    for phase in ('update', 'blend'):
        with pytest.raises(_lib.OcrfHipError, match='hipError_t 1\\b'):
            plan.render(*args, guard='device', phase=phase, out=dict(got))
    with pytest.raises(KeyError):
        plan.render(*args, phase='finish')
    torch.cuda.synchronize()
    _same(want, got)                                       # nothing was launched into the outputs
    _same(want, _split(plan, args))
    assert plan.check()
