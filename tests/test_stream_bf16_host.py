"""CPU: the bfloat16 switch of the streaming detector, as far as it goes without a GPU: ``OcRFDet4D.bf16_inference()`` sets
and restores its three opt-ins, ``stream_step(bf16=True)`` refuses CPU inputs before any module runs, and
``stereo_cost_volume_hip_bf16`` refuses a ``cv_feat_packed`` entry that ``stereo_pack_bf16`` cannot have written."""
import pytest
import torch

from ocrfdet_amd import depthnet, streaming
from ocrfdet_amd import detector as det_mod
from tests import test_detector_host as host
from tests import test_stream_host as sh
from tests.test_center_head_decode_host import make_head

GS = host.GS
BF16 = torch.bfloat16


def switches(det):
    return (det.autocast_bf16, det.img_view_transformer.depth_net.fused_cost_volume_bf16,
            det.pts_bbox_head.fused_decode_bf16)


@pytest.fixture()
def det(golden):
    """The stand-in detector with a real ``DepthNet`` and a real ``CenterHead`` hung on it: the context manager only
    touches attributes."""
    d = sh.stand_in_detector()
    d.img_view_transformer.depth_net = depthnet.DepthNet(8, 8, 4, 6, use_dcn=False, use_aspp=False, stereo=True)
    d.pts_bbox_head = make_head(golden('center_head_decode.npz'))
    return d


def test_bf16_inference_sets_and_restores_the_three_switches(det):
    depth_net, head = det.img_view_transformer.depth_net, det.pts_bbox_head
    assert switches(det) == (False, False, False)
    assert not torch.is_autocast_enabled('cuda')
    with det.bf16_inference() as inside:
        assert inside is det and switches(det) == (True, True, True)
        # (that autocast is on inside is checked where there is a GPU: without one torch switches it off)
        # on the instances: the classes keep their defaults
        assert depthnet.DepthNet.fused_cost_volume_bf16 is False and type(head).fused_decode_bf16 is False
        assert det_mod.OcRFDet4D.autocast_bf16 is False
    assert switches(det) == (False, False, False) and not torch.is_autocast_enabled('cuda')
    for obj, name in ((det, 'autocast_bf16'), (depth_net, 'fused_cost_volume_bf16'), (head, 'fused_decode_bf16')):
        assert name not in vars(obj)                                   # what was a class default is one again
    # previous instance values come back, after an exception too
    det.autocast_bf16, depth_net.fused_cost_volume_bf16 = True, False
    with pytest.raises(RuntimeError, match='inside'):
        with det.bf16_inference():
            assert switches(det) == (True, True, True)
            raise RuntimeError('inside')
    assert switches(det) == (True, False, False) and not torch.is_autocast_enabled('cuda')
    assert vars(det)['autocast_bf16'] is True and vars(depth_net)['fused_cost_volume_bf16'] is False
    assert depthnet.DepthNet.fused_cost_volume_bf16 is False


def test_bf16_inference_skips_sub_modules_that_are_not_there():
    d = sh.stand_in_detector()                                         # a stand-in neck without depth_net, no head
    assert not d.with_pts_bbox and getattr(d.img_view_transformer, 'depth_net', None) is None
    with d.bf16_inference():
        assert d.autocast_bf16 is True
    assert d.autocast_bf16 is False and 'autocast_bf16' not in vars(d)


def test_a_bf16_step_refuses_cpu_inputs_before_any_module_runs():
    d = sh.stand_in_detector()
    frame = sh.sequence(1)[0]
    del d.img_backbone.log[:], d.img_view_transformer.log[:]
    with pytest.raises(ValueError, match='GPU'):
        d.stream_step(frame, bf16=True)
    with pytest.raises(ValueError, match='GPU'):
        d.simple_test_stream(frame, bf16=True)
    assert d.img_backbone.log == [] and d.img_view_transformer.log == []
    assert d.autocast_bf16 is False and not torch.is_autocast_enabled('cuda')
    with pytest.raises(RuntimeError, match='eval'):                    # training mode raises as it does without bf16
        d.train().stream_step(frame, bf16=True)
    # the float32 step is untouched by the keyword, and its state knows its mode
    _, state = d.eval().stream_step(frame, bf16=False)
    assert state.bf16 is False and state.stereo_packed is None and state.ring.dtype == torch.float32
    assert streaming.StreamState(1, bf16=True).ring_dtype(torch.zeros(1)) == BF16


def test_cost_volume_refuses_a_packed_entry_of_the_wrong_shape_or_dtype():
    """The check precedes ``require_cuda``, so it runs on CPU tensors: nothing is launched."""
    BN, C, H, W, D = 2, 12, 3, 5, 4
    feats = [torch.zeros(1, BN, C, H, W, dtype=BF16) for _ in range(2)]
    metas = dict(cv_feat_list=feats, frustum=torch.zeros(D, H, W, 3), post_trans=torch.zeros(1, BN, 3))
    good = torch.zeros(BN, depthnet.packed_blocks(C), H, W, 8, dtype=BF16)
    assert good.shape[1] == 2
    bad = dict(blocks=good[:, :1], pack=torch.zeros(BN, 2, H, W, 4, dtype=BF16), dtype=good.float(),
               strided=good.transpose(2, 3).contiguous().transpose(2, 3), unpacked=feats[0][0], other='packed')
    for name, entry in bad.items():
        for packed in ([entry, None], [None, entry], [good, entry]):
            with pytest.raises(ValueError, match='cv_feat_packed'):
                depthnet.stereo_cost_volume_hip_bf16(dict(metas, cv_feat_packed=packed), 0.0)
    with pytest.raises(ValueError, match='cv_feat_packed'):
        depthnet.stereo_cost_volume_hip_bf16(dict(metas, cv_feat_packed=[good]), 0.0)
    # good entries pass the check: what stops the call on the CPU is the GPU-only refusal behind it
    from ocrfdet_amd import _lib
    for packed in ([good, good], [good, None], None):
        with pytest.raises(_lib.OcrfHipError, match='GPU'):
            depthnet.stereo_cost_volume_hip_bf16(dict(metas, cv_feat_packed=packed), 0.0)
