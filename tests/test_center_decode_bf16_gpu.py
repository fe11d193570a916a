"""GPU: ``ocrf_center_decode_bf16`` (csrc/center_decode.hip) through ``CenterHead.get_bboxes_padded`` with
``fused_decode_bf16`` on: the head tensors read as bfloat16 in place.

The heads are those of ``tests/golden/center_head_decode.npz`` (B = 3, 24 x 32, six tasks, ``max_num`` 16) rounded to
bfloat16.  The contract is bit equality with ``ocrf_center_decode`` on ``.float()`` of the same heads (the float32 arm,
which the existing decode tests hold to the reference and to the float64 oracle), so there is no tolerance.  The
precondition makes the comparison mean something: the rounded heads still detect (counts 21, 0, 25 over all ten labels),
and bfloat16 scores tie at the selection boundary (the 16th and 17th largest of a (task, sample) pair are equal), where
only the (class, cell) index order decides which cell is decoded."""
import pytest
import torch

from ocrfdet_amd import _lib
from ocrfdet_amd import center_decode as cd
from tests.test_center_head_decode_host import make_head, preds

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def rounded(g, dev, with_velocity=True):
    return tuple([{k: v.to(BF16) for k, v in p[0].items()}] for p in preds(g, dev, with_velocity))


def widened(preds_dicts):
    return tuple([{k: v.float() for k, v in p[0].items()}] for p in preds_dicts)


@pytest.fixture(scope='module')
def g(golden):
    return golden('center_head_decode.npz')


_ARMS = {}


def float32_arm(g, with_velocity=True):
    """The four outputs of ``ocrf_center_decode`` on the widened rounded heads, computed once per variant and shared."""
    if with_velocity not in _ARMS:
        head = make_head(g, with_velocity)
        _ARMS[with_velocity] = head.get_bboxes_padded(widened(rounded(g, 'cuda:0', with_velocity)))
    return _ARMS[with_velocity]


def launches_of(monkeypatch):
    names = []
    real = _lib.launch
    monkeypatch.setattr(_lib, 'launch', lambda name, *a, **k: names.append(name) or real(name, *a, **k))
    return names


def test_precondition_the_rounded_heads_detect_and_tie_at_the_boundary(cuda, g):
    want = float32_arm(g)
    head = make_head(g)
    wide = widened(rounded(g, 'cpu'))
    boxes, scores, labels, counts = cd.decode_torch(wide, head._decode_cfg(), head.norm_bbox)
    assert counts.tolist() == [21, 0, 25]
    assert sorted({int(x) for i, n in enumerate(counts.tolist()) for x in labels[i, :n]}) == list(range(10))
    K = int(head.bbox_coder.max_num)
    assert K == 16
    ties = 0
    for p in wide:
        s = p[0]['heatmap'].sigmoid().flatten(1).sort(dim=1, descending=True)[0]
        ties += int((s[:, K - 1] == s[:, K]).sum())
    print(f'{ties} of {len(wide) * 3} (task, sample) pairs tie at the selection boundary')
    assert ties >= 3
    # and the float32 kernel agrees with the torch formulation on what is kept
    assert want[3].tolist() == [21, 0, 25]
    for i, n in enumerate(counts.tolist()):
        assert torch.equal(want[2][i, :n].cpu(), labels[i, :n])


@pytest.mark.parametrize('with_velocity', [True, False])
def test_bit_equal_to_the_float32_decode_by_one_launch_of_the_new_entry(cuda, g, monkeypatch, with_velocity):
    want = float32_arm(g, with_velocity)
    head = make_head(g, with_velocity)
    p = rounded(g, cuda, with_velocity)
    names = launches_of(monkeypatch)
    head.fused_decode_bf16 = True
    got = head.get_bboxes_padded(p)
    assert names == ['ocrf_center_decode_bf16']
    again = head.get_bboxes_padded(p)
    head.fused_decode_bf16 = False
    del names[:]
    off = head.get_bboxes_padded(p)
    assert names == ['ocrf_center_decode']
    assert got[0].shape[-1] == (9 if with_velocity else 7)
    assert int(got[3].sum()) > 0
    for a, b, c, d in zip(got, want, again, off):
        assert a.dtype == b.dtype and torch.equal(a, b)                 # the float32 arm, bit for bit
        assert torch.equal(a, c) and torch.equal(a, d)                  # a rerun; the cast path
    assert got[0].dtype == got[1].dtype == torch.float32 and got[2].dtype == got[3].dtype == torch.int32


def test_a_mixed_list_goes_the_existing_way(cuda, g, monkeypatch):
    want = float32_arm(g)
    head = make_head(g)
    head.fused_decode_bf16 = True
    p = rounded(g, cuda)
    p[2][0]['dim'] = p[2][0]['dim'].float()
    names = launches_of(monkeypatch)
    got = head.get_bboxes_padded(p)
    assert names == ['ocrf_center_decode']
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    with pytest.raises(_lib.OcrfHipError, match='all float32 or all bfloat16'):
        cd.decode_fused(p, head._decode_cfg(), head.norm_bbox)


def test_no_host_synchronisation(cuda, g):
    want = float32_arm(g)
    head = make_head(g)
    head.fused_decode_bf16 = True
    p = rounded(g, cuda)
    head.get_bboxes_padded(p)                                           # warm-up: the workspace
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = head.get_bboxes_padded(p)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[3], want[3])
