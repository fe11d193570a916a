"""GPU: bfloat16 streaming inference, ``OcRFDet4D.stream_step(bf16=True)`` / ``simple_test_stream(bf16=True)``, and the
packed stereo cache under it.

* The packed cache: ``stereo_cost_volume_hip_bf16`` with ``cv_feat_packed`` given for the previous feature, for both and
  for neither returns the same bits, by one, zero and two ``ocrf_stereo_pack_bf16`` launches.
* The whole detector (``tests/test_detector_host.MODEL``, B = 1, 4 frames, ``tests/test_stream_gpu``'s frames) in a child
  process with deterministic convolutions, as ``tests/test_stream_gpu.py`` arranges it.  Per step: the launches of the
  step, no synchronisation, one backbone pass, a bfloat16 ring; and closeness by three arms:

      A   the float32 ``stream_step`` (existing code),
      Bt  the batch ``extract_img_feat`` on the frames (t, max(t - 1, 0), max(t - 2, 0)) inside ``det.bf16_inference()``
          (the existing opt-in kernels only),
      S   the new step,

  with ``rms(S - A) <= 1.1 * rms(Bt - A)`` and ``rms(Bt - A) > 0`` for ``x[0]`` and ``depth``.  The yardstick is the
  existing batch arm, never the code under test.  The expected ratio is 1.000: both bfloat16 arms round at the same
  sites (the ring stores the bfloat16 map ``pre_process_net`` produced, and with ``align_after_view_transfromation``
  False every group is a bit copy).  The 10 % allow a convolution algorithm chosen differently for one arm; an RMS over
  16 x 48 x 48 values, not a maximum, so that one element cannot decide the test."""
import copy
import json
import os
import random
import subprocess
import sys

import pytest
import torch

from ocrfdet_amd import _lib, depthnet
from ocrfdet_amd import detector as det_mod

from tests import stereo_oracle as oracle
from tests import test_detector_gpu as whole
from tests import test_detector_host as host
from tests.test_stereo_bf16_gpu import bits, case
from tests.test_stream_gpu import FRAMES, batch_inputs, frames_of

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def recorded():
    """Every ``_lib.launch`` name from now on, in a list; the caller restores ``_lib.launch`` (``real``)."""
    names, real = [], _lib.launch
    _lib.launch = lambda name, *a, **k: names.append(name) or real(name, *a, **k)
    return names, real


def test_packed_entries_are_not_packed_again_and_give_the_same_volume(cuda, monkeypatch):
    c = case('extra_c12')                                              # three groups: a block and a half
    metas = oracle.to_device(c.metas, cuda)
    prev, curr = (f.reshape(-1, *f.shape[-3:]) for f in metas['cv_feat_list'])
    p, q = depthnet.stereo_pack_bf16(prev), depthnet.stereo_pack_bf16(curr)
    names = []
    real = _lib.launch
    monkeypatch.setattr(_lib, 'launch', lambda name, *a, **k: names.append(name) or real(name, *a, **k))
    packs = {}
    for raw in (True, False):
        outs = []
        for key, packed in (('none', None), ('prev', [p, None]), ('both', [p, q]), ('curr', [None, q])):
            del names[:]
            m = metas if packed is None else dict(metas, cv_feat_packed=packed)
            outs.append(depthnet.stereo_cost_volume_hip_bf16(m, c.bias, raw=raw))
            packs[key] = names.count('ocrf_stereo_pack_bf16')
            assert names.count('ocrf_stereo_cost_volume_bf16') == 1 and len(names) == packs[key] + 1
        assert packs == dict(none=2, prev=1, both=0, curr=1)
        for out in outs[1:]:
            assert torch.equal(bits(out), bits(outs[0]))
    # the public dispatch hands the metas through
    del names[:]
    got = depthnet.stereo_cost_volume(dict(metas, cv_feat_packed=[p, q]), c.bias, keep_bf16=True)
    assert names == ['ocrf_stereo_cost_volume_bf16'] and torch.equal(bits(got), bits(outs[0]))
    # a refused entry launches nothing
    del names[:]
    with pytest.raises(ValueError, match='cv_feat_packed'):
        depthnet.stereo_cost_volume_hip_bf16(dict(metas, cv_feat_packed=[p.cpu(), None]), c.bias)
    assert names == []


def rms(a, b):
    return float((a.float() - b.float()).double().pow(2).mean().sqrt())


def print_bf16_stream_against_the_arms():
    """The body of the child process; one JSON line."""
    torch.backends.cudnn.deterministic = True
    random.randint = lambda a, b: 2
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    det = det_mod.OcRFDet4D(**copy.deepcopy(host.MODEL)).to(dev).eval()
    frames = frames_of(dev)
    backbone_batches = []
    hook = det.img_backbone.register_forward_hook(lambda m, args, out: backbone_batches.append(int(args[0].shape[0])))
    names, real = recorded()
    steps, state, state32 = [], None, None
    try:
        for t in range(FRAMES):
            del backbone_batches[:], names[:]
            if t > 0:                                 # the first step allocates the state and warms the library up
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode('error')
            try:
                (x, depth, _), state = det.stream_step(frames[t], state, bf16=True)
            finally:
                torch.cuda.set_sync_debug_mode('default')
            seen, launched = list(backbone_batches), list(names)
            switches = [det.autocast_bf16, det.img_view_transformer.depth_net.fused_cost_volume_bf16,
                        det.pts_bbox_head.fused_decode_bf16, torch.is_autocast_enabled('cuda')]
            (ax, adepth, _), state32 = det.stream_step(frames[t], state32)                  # arm A
            with torch.no_grad(), det.bf16_inference():                                     # arm Bt
                bx, bdepth, _ = det.extract_img_feat(batch_inputs(frames, [t, max(t - 1, 0), max(t - 2, 0)]), None)
            steps.append(dict(
                backbone=seen, launches=launched, valid=state.valid_host, switches_after=switches,
                ring=str(state.ring.dtype), packed=list(state.stereo_packed.shape), x_dtype=str(x[0].dtype),
                shape=list(x[0].shape), depth_dtype=[str(depth.dtype), str(bdepth.dtype)],
                x=[rms(x[0], ax[0]), rms(bx[0], ax[0]), float((x[0].float() - bx[0].float()).abs().max())],
                depth=[rms(depth, adepth), rms(bdepth, adepth), float((depth.float() - bdepth.float()).abs().max())]))
        hook.remove()
        # a float32 step on the bfloat16 state starts a new sequence (and the other way round)
        _, mixed = det.stream_step(frames[1], state)
        _, back = det.stream_step(frames[2], state32, bf16=True)
        modes = dict(mixed=[mixed is not state, mixed.bf16, str(mixed.ring.dtype), mixed.valid_host, mixed.steps],
                     back=[back is not state32, back.bf16, str(back.ring.dtype), back.valid_host, back.steps])
        del names[:]
        results, _ = det.simple_test_stream(frames[0], img_metas=[dict()], bf16=True)
        decode = [n for n in names if 'center_decode' in n]
        want, _ = det.simple_test_stream(frames[0], img_metas=[dict()])
    finally:
        _lib.launch = real
    keys = [[list(r), list(r['pts_bbox']), list(r['pts_bbox']['boxes_3d'].shape[1:]), r['pts_bbox']['boxes_3d'].device.type,
             str(r['pts_bbox']['boxes_3d'].dtype), str(r['pts_bbox']['scores_3d'].dtype),
             list(r['pts_bbox']['scores_3d'].shape) == list(r['pts_bbox']['labels_3d'].shape)] for r in results]
    same_keys = [list(r['pts_bbox']) for r in results] == [list(r['pts_bbox']) for r in want]
    print('STREAMBF16 ' + json.dumps(dict(steps=steps, modes=modes, results=keys, decode=decode, same_keys=same_keys)))


def test_bf16_stream_steps_stay_on_the_kernels_and_close_to_the_batch_arm(cuda):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = subprocess.run([sys.executable, '-c',
                            'from tests import test_stream_bf16_gpu as t; t.print_bf16_stream_against_the_arms()'],
                           cwd=root, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-3000:]
    line = [ln for ln in child.stdout.splitlines() if ln.startswith('STREAMBF16 ')][-1]
    got = json.loads(line[len('STREAMBF16 '):])
    assert len(got['steps']) == FRAMES
    for t, step in enumerate(got['steps']):
        for name in ('x', 'depth'):
            s_a, bt_a, s_bt = step[name]
            print(f'step {t} {name}: rms(S - A) {s_a:.4e}, rms(Bt - A) {bt_a:.4e}, ratio '
                  f'{s_a / bt_a if bt_a else float("nan"):.4f}, max|S - Bt| {s_bt:.3e}')
    for t, step in enumerate(got['steps']):
        assert step['backbone'] == [whole.N_CAMS], step                # one encoder pass, on B * N images
        assert step['valid'] == [1] and step['ring'] == 'torch.bfloat16'
        assert step['x_dtype'] == 'torch.bfloat16' and step['shape'] == [1, 16, 48, 48]
        assert step['depth_dtype'][0] == step['depth_dtype'][1]        # as the neck returns it, in either arm
        assert len(step['packed']) == 5 and step['packed'][0] == whole.N_CAMS and step['packed'][-1] == 8
        assert step['switches_after'] == [False, False, False, False]  # the step put everything back
        if t > 0:
            launched = step['launches']
            for name in ('ocrf_stereo_pack_bf16', 'ocrf_stereo_cost_volume_bf16', 'ocrf_bev_stream_align_bf16'):
                assert launched.count(name) == 1, (t, name, launched)
            assert 'ocrf_stereo_cost_volume' not in launched and 'ocrf_bev_stream_align' not in launched
        for name in ('x', 'depth'):
            s_a, bt_a, _ = step[name]
            assert bt_a > 0 and s_a <= 1.1 * bt_a, (t, name, s_a, bt_a)
    assert got['modes']['mixed'] == [True, False, 'torch.float32', [1], 1]
    assert got['modes']['back'] == [True, True, 'torch.bfloat16', [1], 1]
    assert got['results'] == [[['pts_bbox'], ['boxes_3d', 'scores_3d', 'labels_3d'], [9], 'cpu', 'torch.float32',
                               'torch.float32', True]]
    assert got['decode'] == ['ocrf_center_decode_bf16'] and got['same_keys']
