"""CPU: ``ocrfdet_amd.distill`` and ``OcRFDet4DVGGT``: the torch formulations of the correlation volume and the two
losses against the float64 oracle (``tests/distill_oracle.py``) and the reference's own results
(``tests/golden/distill.npz``, ``README_distill.md``), the aligner's parity, the pair draw, and the detector's branch on
stand-in sub-modules."""
import os
import random

import numpy as np
import pytest
import torch
from torch import nn

from ocrfdet_amd import detector as det_mod
from ocrfdet_amd import distill

from tests import distill_oracle as oracle
from tests import test_detector_host as host      # the stand-in sub-modules, the inputs and the head's config

HERE = os.path.dirname(os.path.abspath(__file__))
GS = host.GS
B, N = 2, 6                                       # the pair draw names cameras 0 .. 5


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(HERE, 'golden', 'distill.npz')))


def randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ the volume
# (B, C, H, W, G, D): W = 1, W < D, Cg = 1 with D = 1, Cg = 3 over a wide row, the largest D
SHAPES = [(1, 4, 1, 1, 1, 5), (2, 6, 2, 3, 3, 5), (1, 7, 3, 5, 7, 1), (2, 12, 3, 9, 4, 5), (1, 8, 2, 20, 2, 16)]


@pytest.mark.parametrize('shape', SHAPES)
def test_torch_volume_and_its_gradients_match_the_oracle(shape):
    b, c, h, w, g, d = shape
    feats = randn(b, 2, c, h, w, seed=sum(shape)).requires_grad_(True)
    grad_out = randn(b, g, d, h, w, seed=1 + sum(shape))
    got = distill.build_cost_volume(feats, max_disp=d - 1, method='group_corr', groups=g)
    assert got.shape == (b, g, d, h, w) and got.dtype == torch.float32
    assert torch.equal(got, distill.group_corr_volume_torch(feats, d - 1, g))        # the CPU dispatch
    left, right = feats.detach()[:, 0].numpy(), feats.detach()[:, 1].numpy()
    want, n, mag = oracle.volume(left, right, g, d)
    assert (np.abs(got.detach().numpy() - want) <= oracle.sum_bound(n, mag)).all()
    got.backward(grad_out)
    gL, nL, magL, gR, nR, magR = oracle.volume_grads(left, right, grad_out.numpy(), g, d)
    grad = feats.grad.numpy()
    assert (np.abs(grad[:, 0] - gL) <= oracle.sum_bound(nL, magL)).all()
    assert (np.abs(grad[:, 1] - gR) <= oracle.sum_bound(nR, magR)).all()
    # column 0 of the right view collects every clamped read: up to D (D + 1) / 2 addends
    assert nR[0] == sum(min(k, w - 1) + 1 for k in range(d)) and (w == 1 or nR[1] == min(d, w - 1))


def test_oracle_is_the_written_sum():
    """The oracle itself, element by element, on a shape small enough for loops."""
    b, c, h, w, g, d = 1, 4, 2, 3, 2, 4
    L, R = randn(b, c, h, w, seed=3).double().numpy(), randn(b, c, h, w, seed=4).double().numpy()
    want = np.zeros((b, g, d, h, w))
    for gi in range(g):
        for di in range(d):
            for y in range(h):
                for x in range(w):
                    want[0, gi, di, y, x] = sum(L[0, gi * 2 + k, y, x] * R[0, gi * 2 + k, y, max(x - di, 0)]
                                                for k in range(2))
    assert np.allclose(oracle.volume(L, R, g, d)[0], want, rtol=0, atol=1e-14)


def test_the_volume_reproduces_the_reference(golden):
    for tag, cfg in (('a', dict(max_disp=4, groups=4)), ('b', dict(max_disp=4, groups=3))):
        feats = torch.from_numpy(golden[f'vol.{tag}.feats'])
        got = distill.build_cost_volume(feats, method='group_corr', **cfg).numpy()
        ref = golden[f'vol.{tag}.out']
        assert got.shape == ref.shape
        want, n, mag = oracle.volume(feats[:, 0].numpy(), feats[:, 1].numpy(), cfg['groups'], cfg['max_disp'] + 1)
        bound = oracle.sum_bound(n, mag)
        assert (np.abs(got - ref) <= bound).all() and (np.abs(ref - want) <= bound).all()


def test_methods_the_reference_cannot_run_raise():
    feats = randn(1, 2, 4, 2, 3)
    for method in ('concat', 'variance'):
        with pytest.raises(NotImplementedError, match="reference's own code"):
            distill.build_cost_volume(feats, method=method)
    with pytest.raises(NotImplementedError):
        distill.build_cost_volume(feats)                        # the signature's default is 'concat'
    with pytest.raises(ValueError):
        distill.build_cost_volume(feats, method='other')
    with pytest.raises(ValueError, match='groups'):
        distill.build_cost_volume(feats, method='group_corr', groups=3)
    with pytest.raises(ValueError, match='B, 2, C, H, W'):
        distill.build_cost_volume(feats[:, :1], method='group_corr', groups=2)
    from ocrfdet_amd import _lib
    with pytest.raises(_lib.OcrfHipError):                       # the kernels on request: no CPU tensors
        distill.build_cost_volume(feats, method='group_corr', groups=2, fused=True)
    with pytest.raises(_lib.OcrfHipError):
        distill.kd_losses(feats, feats, fused=True)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Argument validation alone: every call returns hipErrorInvalidValue before anything is enqueued, so it runs
    without a device.  Pointers are small integers that a refused call never dereferences."""
    import ctypes
    from ocrfdet_amd import _lib
    L = _lib.lib()
    invalid, p = 1, ctypes.c_void_p(4096)

    def forward(B=2, C=12, H=3, W=7, G=4, D=5, left=p, out=p, stride=2 * 12 * 21):
        return L.ocrf_group_corr_forward(B, C, H, W, G, D, left, p, stride, out, None)

    def backward(B=2, C=12, H=3, W=7, G=4, D=5, left=p, out=p, stride=2 * 12 * 21):
        return L.ocrf_group_corr_backward(B, C, H, W, G, D, p, left, p, stride, out, p, stride, None)
    for fn in (forward, backward):
        assert fn(G=5) == invalid and fn(D=0) == invalid and fn(D=17) == invalid                   # C % G, D
        assert fn(left=None) == invalid and fn(out=None) == invalid and fn(B=0) == invalid
        assert fn(stride=12 * 21 - 1) == invalid                                                   # overlapping samples
        assert fn(B=2, C=2048, H=512, W=512, stride=2 * 2048 * 512 * 512) == invalid               # 2^31 elements
        assert fn(B=64, C=64, H=512, W=1024, G=64, D=16, stride=2 * 64 * 512 * 1024) == invalid    # the volume alone
    assert L.ocrf_kd_losses_workspace_bytes(4, 248640) >= 4 * 4 * 8
    assert L.ocrf_kd_losses_workspace_bytes(0, 5) == 0 and L.ocrf_kd_losses_workspace_bytes(2, 1 << 30) == 0
    size = ctypes.c_size_t(L.ocrf_kd_losses_workspace_bytes(2, 40))
    assert L.ocrf_kd_losses_forward(2, 40, None, p, p, p, p, p, size, None) == invalid
    assert L.ocrf_kd_losses_forward(2, 40, p, p, p, p, p, p, ctypes.c_size_t(size.value - 1), None) == invalid
    assert L.ocrf_kd_losses_forward(2, 1 << 30, p, p, p, p, p, p, size, None) == invalid
    assert L.ocrf_kd_losses_backward(2, 40, p, p, None, p, p, p, None) == invalid
    assert L.ocrf_kd_losses_backward(2, 1 << 30, p, p, p, p, p, p, None) == invalid


# ------------------------------------------------------------------------------------------------ the two losses
def kd_operands(b, n, seed):
    """s, t with differences exactly at the smooth-L1 kink, just inside and just outside it."""
    s, t = randn(b, n, seed=seed), randn(b, n, seed=seed + 1)
    for k, delta in enumerate((1.0, -1.0, 1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20, -1.0 + 2.0 ** -20, 0.0)):
        if k < n:
            t[0, k] = 0.25 * (k + 1)
            s[0, k] = t[0, k] + delta
    return s, t


@pytest.mark.parametrize('b, n', [(1, 1), (3, 40), (2, 255), (2, 840)])
def test_torch_losses_and_their_gradient_match_the_oracle(b, n):
    s, t = kd_operands(b, n, seed=10 * b + n)
    if b == 3:
        s[1] = 0.0                                               # the clamp of the norm: a finite gradient
    s.requires_grad_(True)
    smooth, cos = distill.kd_losses(s, t)
    want = oracle.kd_losses(s.detach().numpy(), t.numpy())
    assert abs(smooth.item() - want[0]) <= oracle.loss_bound(want[0])
    assert abs(cos.item() - want[1]) <= oracle.loss_bound(want[1])
    g_smooth, g_cos = 0.75, -1.5
    (g_smooth * smooth + g_cos * cos).backward()
    grad, mag = oracle.kd_grad(s.detach().numpy(), t.numpy(), g_smooth, g_cos)
    assert np.isfinite(grad).all() and torch.isfinite(s.grad).all()
    assert (np.abs(s.grad.numpy() - grad) <= oracle.grad_bound(mag) + 1e-30).all()
    if b == 3:                                                   # -t / (eps |t|) / B, as torch gives it
        assert np.allclose(grad[1] - 0.1 * np.clip(-t[1].numpy(), -1, 1) / (b * n) * g_smooth,
                           -g_cos / b * t[1].numpy() / (1e-8 * np.linalg.norm(t[1].double().numpy())), rtol=1e-12)


def test_losses_of_equal_volumes_and_of_the_golden_pair(golden):
    v = randn(2, 4, 5, 3, 7, seed=5)
    smooth, cos = distill.kd_losses(v, v.clone())
    assert smooth.item() == 0.0 and abs(cos.item()) <= oracle.loss_bound(0.0)
    vs, vt = torch.from_numpy(golden['kd.volume_s']), torch.from_numpy(golden['kd.volume_t'])
    got = distill.kd_losses(vs, vt)
    want = oracle.kd_losses(vs.flatten(1).numpy(), vt.flatten(1).numpy())
    for g, ref, w in zip(got, golden['kd.losses'], want):
        assert g.dim() == 0 and abs(g.item() - float(ref)) <= oracle.loss_bound(ref)
        assert abs(g.item() - w) <= oracle.loss_bound(w)


# ------------------------------------------------------------------------------------------------ modules
def test_aligner_loads_the_reference_state_and_reproduces_its_output(golden):
    cfg = dict(res_dim=6, vit_dim=16, num_heads=2)               # make_golden_distill.ALIGN
    aligner = distill.CrossAttentionAlign(**cfg).eval()
    state = {k[len('align.state.'):]: torch.from_numpy(v) for k, v in golden.items() if k.startswith('align.state.')}
    assert {k.split('.')[0] for k in state} == {'query_proj', 'key_proj', 'value_proj', 'attn', 'output_proj'}
    aligner.load_state_dict(state, strict=True)
    with torch.no_grad():
        got = aligner(torch.from_numpy(golden['align.res_feat']), torch.from_numpy(golden['align.vit_feat']))
    want = golden['align.out']
    assert got.shape == want.shape == (1, 2, 16, 3, 5) and got.is_contiguous()
    assert np.abs(got.numpy() - want).max() <= 1e-5 * np.abs(want).max()
    assert list(distill.CrossAttentionAlign().state_dict())[:2] == ['query_proj.weight', 'query_proj.bias']


def test_resize_img_is_bilinear_without_aligned_corners():
    img = randn(2, 3, 3, 5, 7)
    out = distill.resize_img(img, 8, 9)
    want = torch.nn.functional.interpolate(img.view(6, 3, 5, 7), size=(8, 9), mode='bilinear', align_corners=False)
    assert out.shape == (2, 3, 3, 8, 9) and torch.equal(out.view(6, 3, 8, 9), want)
    assert distill.resize_img(img[:1, :1]).shape == (1, 1, 3, 294, 518)


def test_pair_indices(golden):
    class Draw:
        def __init__(self, value):
            self.value = value

        def randint(self, lo, hi):
            assert (lo, hi) == (0, 5)
            return self.value
    assert [distill.get_pair_indices(Draw(i)) for i in range(6)] == [(0, 1), (1, 2), (2, 5), (3, 4), (4, 3), (5, 0)]
    random.seed(GS_DISTILL_SEED)
    assert [distill.get_pair_indices() for _ in range(len(golden['pairs']))] == [tuple(p) for p in golden['pairs'].tolist()]
    rng = random.Random(GS_DISTILL_SEED)                         # an own generator draws the same sequence
    assert distill.get_pair_indices(rng) == tuple(golden['pairs'][0].tolist())


GS_DISTILL_SEED = 20261020                                       # make_golden_distill.SEED


# ------------------------------------------------------------------------------------------------ the detector
class ScaledBackbone(GS.StandInBackbone):
    """The stand-in with one parameter, so that 'no gradient reaches the image encoder' says something."""

    def __init__(self):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor(1.25))

    def forward(self, x):
        stereo, feat = super().forward(x)
        return [stereo * self.scale, feat * self.scale]


class ScaledNeck(GS.StandInNeck):
    def __init__(self):
        super().__init__()
        self.shift = nn.Parameter(torch.tensor(0.5))

    def forward(self, feats):
        return [super().forward(feats)[0] + self.shift]


class StandInAggregator(nn.Module):
    """VGGT's ``Aggregator`` call on a small scale: a 14 x 14 patch projection to ``vit_dim`` behind ``lead`` leading
    tokens; two list entries, the last one the tokens the detector reads.  The dropout makes a teacher left in
    training mode visible."""

    def __init__(self, vit_dim=8, lead=3):
        super().__init__()
        gen = torch.Generator().manual_seed(7)
        self.proj = nn.Conv2d(3, vit_dim, 14, stride=14)
        with torch.no_grad():
            self.proj.weight.copy_(torch.randn(vit_dim, 3, 14, 14, generator=gen) * 0.05)
            self.proj.bias.copy_(torch.randn(vit_dim, generator=gen) * 0.1)
        self.lead = nn.Parameter(torch.randn(lead, vit_dim, generator=gen))
        self.drop = nn.Dropout(0.5)
        self.calls = 0

    def forward(self, images):
        self.calls += 1
        b, v = images.shape[:2]
        assert images.shape[2] == 3 and not torch.is_grad_enabled()
        patches = self.proj(images.flatten(0, 1)).flatten(2).transpose(1, 2)          # (b v, h w, vit)
        tokens = torch.cat([self.lead.expand(b * v, -1, -1), patches], dim=1)
        tokens = self.drop(tokens).view(b, v, tokens.shape[1], tokens.shape[2])
        return [0.5 * tokens, tokens], self.lead.shape[0]


class RaisingAggregator(nn.Module):
    def forward(self, images):
        raise AssertionError('the teacher must not run outside training')


ALIGNER = dict(res_dim=3, vit_dim=8, num_heads=2)                 # the stand-in encoder's feature is 3 channels wide
DISTILL = dict(max_disp=4, groups=4, resize=(28, 42), patch_size=14)          # 2 x 3 patches: W < D


def stand_ins(head=None, vt=None):
    return dict(img_backbone=ScaledBackbone(), img_neck=ScaledNeck(),
                img_view_transformer=vt or GS.StandInViewTransformer(), pre_process=GS.StandInPreProcess(),
                img_bev_encoder_backbone=GS.StandInBEVBackbone(), img_bev_encoder_neck=GS.StandInBEVNeck(),
                pts_bbox_head=head, num_adj=1)


def vggt_detector(aggregator, head=None, vt=None, **kw):
    torch.manual_seed(11)
    return det_mod.OcRFDet4DVGGT(**stand_ins(head, vt), aggregator=aggregator, aligner=dict(ALIGNER),
                                 distill=dict(DISTILL), type='OcRFDet4DVGGT', **kw)


@pytest.fixture(scope='module')
def inputs():
    return GS.make_inputs(n=N)


def test_constructor_and_types():
    from ocrfdet_amd import OcRFDet4DVGGT                        # exported from the package
    det = vggt_detector(StandInAggregator())
    assert isinstance(det, OcRFDet4DVGGT) and isinstance(det, det_mod.OcRFDet4D)
    assert det.distill == DISTILL and isinstance(det.aligner, distill.CrossAttentionAlign)
    keys = {k.split('.')[0] for k in det.state_dict()}
    assert {'aggregator', 'aligner', 'img_backbone', 'img_neck'} <= keys
    assert 'aggregator.proj.weight' in det.state_dict() and 'aligner.attn.in_proj_weight' in det.state_dict()
    assert not any(p.requires_grad for p in det.aggregator.parameters())
    assert all(p.requires_grad for p in det.aligner.parameters())
    # the defaults are the reference config's
    plain = det_mod.OcRFDet4DVGGT(**stand_ins(), aligner=dict(res_dim=4, vit_dim=16, num_heads=2))
    assert plain.distill == dict(max_disp=4, groups=64, resize=(294, 518), patch_size=14) and plain.aggregator is None
    # the parent still refuses every type but its own, and the child every type but its own
    with pytest.raises(NotImplementedError, match='only OcRFDet4D'):
        det_mod.OcRFDet4D(**stand_ins(), type='OcRFDet4DVGGT')
    with pytest.raises(NotImplementedError):
        det_mod.OcRFDet4DVGGT(**stand_ins(), type='OcRFDet4D')


def test_the_teacher_stays_frozen_and_in_eval_mode():
    det = vggt_detector(StandInAggregator())
    assert det.train() is det and det.training and det.aligner.training
    assert not det.aggregator.training and not det.aggregator.drop.training
    det.eval().train(True)
    assert not det.aggregator.training


def test_training_without_a_teacher_raises(inputs):
    det = vggt_detector(None).train()
    with pytest.raises(RuntimeError, match='aggregator=None'):
        det.extract_img_feat(inputs, None)
    det.eval()
    assert len(det.extract_img_feat(inputs, None)) == 3           # testing needs no teacher


def test_extract_img_feat_carries_the_two_volumes_in_training(inputs):
    det = vggt_detector(StandInAggregator()).train()
    random.seed(3)
    out = det.extract_img_feat(inputs, None)
    assert len(out) == 5 and det.aggregator.calls == 1            # the key frame only
    volume_t, volume_s = out[4]
    assert volume_t.shape == volume_s.shape == (B, DISTILL['groups'], DISTILL['max_disp'] + 1, 2, 3)
    assert volume_s.requires_grad and not volume_t.requires_grad
    feat = det.extract_feat(None, inputs)
    assert len(feat) == 6 and feat[1] is None and len(feat[5]) == 2
    # the same draw gives the same volumes, another pair other ones
    random.seed(3)
    again = det.extract_img_feat(inputs, None)[4]
    assert torch.equal(again[0], volume_t) and torch.equal(again[1], volume_s)
    # what the branch computes, rebuilt from its parts for the pair the seed draws
    random.seed(3)
    i1, i2 = distill.get_pair_indices()
    imgs = inputs[0].view(B, N, 3, 3, 8, 8)[:, :, 0]              # the key frame's cameras
    x_t = distill.resize_img(torch.stack([imgs[:, i1], imgs[:, i2]], 1), 28, 42)
    with torch.no_grad():
        tokens = det.aggregator(x_t)[0][-1][:, :, 3:]
    token_img = tokens.reshape(B * 2, 6, 8).permute(0, 2, 1).reshape(B, 2, 8, 2, 3)
    assert torch.equal(distill.group_corr_volume_torch(token_img, 4, 4), volume_t)


def head_and_transformer():
    return host.head_detector().pts_bbox_head, host.LossViewTransformer()


def train_kwargs(inputs):
    boxes = [torch.tensor([[0.3, -0.4, -1.0, 0.4, 0.5, 1.6, 0.3, 0.5, -0.2]]), torch.zeros(0, 9)]
    labels = [torch.tensor([0]), torch.zeros(0, dtype=torch.long)]
    gen = torch.Generator().manual_seed(2)
    return dict(img_inputs=inputs, gt_bboxes_3d=boxes, gt_labels_3d=labels, gt_bboxes=[[torch.zeros(0, 4)] * N] * B,
                gt_depth=torch.rand(B, N, 8, 8, generator=gen), gt_semantic=torch.rand(B, N, 8, 8, generator=gen),
                gt_bev_mask=torch.rand(B, 4, 4, generator=gen))


def test_forward_train_adds_the_two_losses_and_they_train_the_aligner_only(inputs):
    head, vt = head_and_transformer()
    det = vggt_detector(StandInAggregator(), head, vt).train()
    random.seed(5)
    losses = det(return_loss=True, **train_kwargs(inputs))
    keys = list(losses)
    assert keys[:7] == host.REFERENCE_LOSS_KEYS[:5] + ['loss_Smoothl1_KD', 'loss_cos_KD']
    assert keys[7:11] == host.REFERENCE_LOSS_KEYS[5:]
    head_keys = [f'task{t}.loss_{k}' for t in range(2) for k in ('xy', 'z', 'whl', 'yaw', 'vel', 'heatmap')]
    assert sorted(keys[11:]) == sorted(head_keys)
    assert all(torch.isfinite(v).all() for v in losses.values())
    assert losses['loss_Smoothl1_KD'].dim() == 0 and losses['loss_cos_KD'].dim() == 0
    (losses['loss_Smoothl1_KD'] + losses['loss_cos_KD']).backward()
    for name, p in det.aligner.named_parameters():
        assert p.grad is not None and p.grad.abs().max() > 0, name
    frozen = [det.img_backbone, det.img_neck, det.aggregator, det.pts_bbox_head]
    for module in frozen:
        params = list(module.parameters())
        assert params and all(p.grad is None or p.grad.abs().max() == 0 for p in params)
    assert not det.aggregator.training


def test_eval_never_touches_the_teacher_and_equals_the_parent(inputs):
    head, vt = head_and_transformer()
    det = vggt_detector(RaisingAggregator(), head, vt).eval()
    parent = det_mod.OcRFDet4D(**stand_ins(host.head_detector().pts_bbox_head, host.LossViewTransformer())).eval()
    own = det.state_dict()
    parent.load_state_dict({k: own[k] for k in parent.state_dict()}, strict=True)
    with torch.no_grad():
        got, want = det.extract_img_feat(inputs, None), parent.extract_img_feat(inputs, None)
        outs, outs_parent = det.forward_dummy(img_inputs=inputs), parent.forward_dummy(img_inputs=inputs)
        results = det(return_loss=False, img_inputs=inputs)
    assert len(got) == len(want) == 3
    assert torch.equal(got[0][0], want[0][0]) and torch.equal(got[1], want[1])
    assert all(torch.equal(a, b) for a, b in zip(got[2], want[2]))
    for task, task_parent in zip(outs, outs_parent):
        assert all(torch.equal(task[0][k], task_parent[0][k]) for k in task[0])
    assert len(results) == B and list(results[0]) == ['pts_bbox']
