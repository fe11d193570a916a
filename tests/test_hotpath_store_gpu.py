"""GPU: ``HotPath`` holds the Gaussian parameters once per phase (``hotpath_scene.GaussianStore``) — every consumer reads
a view of that stack, so an in-place edit of ``frame_gauss`` alone reaches the planned render, the per-call render and
HOA-1, recorded step or not — and the four-stream step replays as it was issued.  On configs[0] (1 camera, 128 x 352,
BEV 64 x 64 x 4) with two frames, the render and HOA switched on: the smallest configuration ``HotPath`` builds so."""
import pytest
import torch

from ocrfdet_amd import hotpath, synthetic
from ocrfdet_amd.hotpath_scene import GAUSS_KEYS

pytestmark = pytest.mark.gpu

CFG = synthetic.PathConfig(**{**synthetic.CONFIGS['cfg0_1cam_128x352_bev64x64x4'].__dict__, 'name': 'cfg0_2frame_render_hoa',
                              'n_frames': 2, 'render': True, 'hoa': True})


def _place(t):
    return t.untyped_storage().data_ptr(), t.storage_offset(), tuple(t.shape), tuple(t.stride())


def _flat(out):
    return list(hotpath.HotPath._flat_outputs(out))


def test_every_consumer_reads_a_view_of_the_phase_stack(cuda):
    hp = hotpath.HotPath(CFG, cuda, alternate=True)
    entries = hp._plans()
    assert sum(nf for _, _, nf, _ in entries) == hp.batch == 2
    places = {}
    for phase in (0, 1, 0):
        hp.set_phase(phase)
        stack = hp.store.stacks[phase]
        P = hp.voxel_xyz.shape[1] * hp.voxel_xyz.shape[2]
        seen = {}
        for k in GAUSS_KEYS:
            base, width = stack[k].untyped_storage().data_ptr(), stack[k].shape[-1]
            assert stack[k].is_contiguous() and stack[k].shape == (hp.batch, P, width) and stack[k].storage_offset() == 0
            for b in range(hp.batch):
                fg = hp.frame_gauss[b][k]
                assert _place(fg) == (base, b * P * width, (P, width), (width, 1)), (phase, k, b)
            assert hp.gauss[k] is hp.frame_gauss[0][k]
            for _, f0, nf, g in entries:
                alt = g['alt'][phase][k]
                assert _place(alt) == (base, f0 * P * width, (nf, P, width), (P * width, width, 1)), (phase, k, f0)
            assert _place(hp._per_call_sets()[k]) == _place(stack[k]) and hp._sets[k] is hp._per_call_sets()[k]
            seen[k] = [_place(hp.frame_gauss[b][k]) for b in range(hp.batch)] + [_place(hp._sets[k])]
        assert _place(hp._opac_flat) == (stack['opacity'].untyped_storage().data_ptr(), 0, (hp.batch * P, 1), (1, 1))
        seen['flat'] = _place(hp._opac_flat)
        assert places.setdefault(phase, seen) == seen             # set_phase moved no tensor: phase 0 again is where it was
    assert places[0]['flat'][0] != places[1]['flat'][0]           # ... and the two phases are two stacks


@pytest.mark.parametrize('render_mode', ['planned', 'per_call'])
def test_an_edit_of_frame_gauss_alone_reaches_every_consumer(cuda, render_mode):
    """Outputs of a step: LSS BEV, HT BEV, rendered frames, gated BEV, opacity BEV.  After the edit all five are bit-equal
    between the recorded step and the step issued call by call; the three that read the parameters (every frame's
    colour, the opacity BEV of HOA-1/2 and the BEV HOA-3 gates with it) differ from the step before it, the two
    poolings, which read none of them, do not."""
    one, ref = (hotpath.HotPath(CFG, cuda, render_mode=render_mode, one_call=oc) for oc in (True, False))
    depth, feat = ref.make_inputs(seed=4)
    for _ in range(3):                                             # call by call, recorded, replayed
        got, want = one.step(depth, feat), ref.step(depth, feat)
    torch.cuda.synchronize()
    assert one._compiled and one.one_call_refused is None and not ref._compiled
    assert all(torch.equal(a, b) for a, b in zip(_flat(got), _flat(want)))
    before, before_color = [t.clone() for t in _flat(got)], [fr['color'].clone() for fr in got[2]]
    for hp in (one, ref):
        g = torch.Generator(device='cpu').manual_seed(21)
        for b in range(hp.batch):
            fg = hp.frame_gauss[b]
            fg['opacity'].copy_((torch.rand(fg['opacity'].shape, generator=g) * 0.3 + 0.3).to(cuda))
            fg['rgb'].copy_(torch.rand(fg['rgb'].shape, generator=g).to(cuda))
    got, want = one.step(depth, feat), ref.step(depth, feat)
    torch.cuda.synchronize()
    assert len(got) == len(want) == 5 and len(got[2]) == one.batch
    flat_got, flat_want = _flat(got), _flat(want)
    assert len(flat_got) == len(flat_want) == len(before)
    for i, (a, b) in enumerate(zip(flat_got, flat_want)):
        assert torch.equal(a, b), i
    changed = [not torch.equal(a, b) for a, b in zip(flat_got, before)]
    assert changed[:2] == [False, False]                           # LSS, HT
    assert changed[-2:] == [True, True]                            # gated BEV, opacity BEV
    for fr_new, old in zip(got[2], before_color):
        assert not torch.equal(fr_new['color'], old)
    if render_mode == 'planned':
        one.check_render_plans(), ref.check_render_plans()


def test_four_stream_step_replays_as_it_was_issued(cuda):
    kw = dict(index_prep_mode='per_step', device_geometry=True)
    one, ref = hotpath.HotPath(CFG, cuda, **kw), hotpath.HotPath(CFG, cuda, one_call=False, **kw)
    depth, feat = ref.make_inputs(seed=5)
    for _ in range(4):
        got, want = one.step(depth, feat), ref.step(depth, feat)
        torch.cuda.synchronize()
        flat_got, flat_want = _flat(got), _flat(want)
        assert len(flat_got) == len(flat_want) >= 4 + 3 * one.batch
        assert all(torch.equal(a, b) for a, b in zip(flat_got, flat_want))
    streams = one._step_streams(torch.cuda.current_stream(cuda))
    assert len(streams) == 4 and one._streams.names == ('main', 'render0', 'prep', 'prep2')
    assert [one._streams.slot[n] for n in one._streams.names] == [0, 1, 2, 3]
    assert len(one._compiled) == 1 and one.one_call_refused is None
    items = next(iter(one._compiled.values())).step
    assert items.n_calls >= 7
    one.check_render_plans(), ref.check_render_plans()
