"""GPU: the package under ``torch.autocast('cuda', dtype=torch.bfloat16)``.

* The image encoder (``ResNet`` + ``CustomFPN``) and ``CustomResNet`` keep their fused passes: every residual tail and
  the top-down merge reach ``add_relu`` / ``upsample_add`` with bfloat16 operands, and what the ops return is, call by
  call, bit-equal to the torch formulation of the same operands.  (Whole-network outputs are not compared between the
  fused and the torch arm: the convolution library may choose its algorithm per call.)
* What is float32 by rule stays float32 and on its kernels: ``align_and_cat``, ``CenterHead.loss`` / ``get_bboxes``, the
  stereo cost volume and the neck's ``view_transform`` give, for bfloat16 inputs under autocast, bit for bit what they
  give outside autocast for the same inputs cast to float32 by hand.
"""
import copy
import json
import random

import numpy as np
import pytest
import torch
from torch.utils import checkpoint

from ocrfdet_amd import _lib, bev_encoder, blocks, depthnet, temporal
from ocrfdet_amd import image_encoder as ie
from tests import helpers
from tests import stereo_fixture as sf

from .test_bev_align_gpu import frames, poses
from .test_center_head_decode_host import make_head as make_decode_head
from .test_center_head_host import boxes, make_head

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def autocast():
    return torch.autocast('cuda', dtype=BF16)


def same_bits(a, b):
    as_int = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(as_int),
                                                                     b.contiguous().view(as_int))


@pytest.fixture
def ops(monkeypatch):
    """Every call of the two ops through the modules: (name, operands, result)."""
    calls = []
    real_tail, real_merge = ie.add_relu, ie.upsample_add

    def tail(a, b):
        out = real_tail(a, b)
        calls.append(('tail', (a.detach(), b.detach()), {}, out.detach()))
        return out

    def merge(dst, src, **kw):
        out = real_merge(dst, src, **kw)
        calls.append(('merge', (dst.detach(), src.detach()), kw, out.detach()))
        return out
    monkeypatch.setattr(blocks, 'add_relu', tail)
    monkeypatch.setattr(ie, 'upsample_add', merge)
    return calls


@pytest.fixture
def launches(monkeypatch):
    """The names of the library's entry points as they are launched."""
    names = []
    real = _lib.launch
    monkeypatch.setattr(_lib, 'launch', lambda name, *a, **k: names.append(name) or real(name, *a, **k))
    return names


def check_calls(calls):
    for name, operands, kw, out in calls:
        assert all(t.dtype == BF16 and t.is_cuda for t in operands) and out.dtype == BF16, name
        want = ie.add_relu_torch(*operands) if name == 'tail' else ie.upsample_add_torch(*operands, **kw)
        assert same_bits(out, want), name


@pytest.mark.parametrize('with_cp', [False, True])
def test_resnet_and_fpn_keep_their_fused_passes(cuda, ops, with_cp):
    torch.manual_seed(0)
    net = ie.ResNet(depth=18, out_indices=(2, 3), with_cp=with_cp).to(cuda).train()
    fpn = ie.CustomFPN([256, 512], 32, num_outs=1, start_level=0, out_ids=[0]).to(cuda).train()
    net.fused_tail = net.fused_tail_bf16 = True
    fpn.fused_merge = fpn.fused_merge_bf16 = True
    img = torch.randn(2, 3, 32, 64, device=cuda)
    # without the early stop a checkpointed block's recomputation runs to its end, so that its tail returns and is seen
    with autocast(), checkpoint.set_checkpoint_early_stop(False):
        feats = net(img)
        out = fpn(feats)
    assert [c[0] for c in ops] == ['tail'] * 8 + ['merge']             # 8 blocks, one top-down step
    check_calls(ops)
    assert out.dtype == BF16 and out.shape == (2, 32, 2, 4) and torch.isfinite(out).all()
    assert all(f.dtype == BF16 and torch.isfinite(f).all() for f in feats)
    out.float().square().mean().backward()
    # a checkpointed block runs again in the backward, under the autocast state of its forward: the op again
    assert [c[0] for c in ops].count('tail') == (16 if with_cp else 8)
    check_calls(ops)
    params = [p for m in (net, fpn) for p in m.parameters() if p.requires_grad]
    assert params and all(p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all()
                          for p in params)
    assert any(float(p.grad.abs().max()) > 0 for p in params)

    del ops[:]
    with torch.no_grad(), autocast():
        net.fused_tail_bf16 = fpn.fused_merge_bf16 = False            # the bf16 switches alone
        assert fpn(net(img)).dtype == BF16 and not ops
        net.fused_tail_bf16 = fpn.fused_merge_bf16 = True
        net.fused_tail = fpn.fused_merge = False                      # the module flags switch everything off
        assert fpn(net(img)).dtype == BF16 and not ops
        net.fused_tail = fpn.fused_merge = True
        assert fpn(net(img)).dtype == BF16 and len(ops) == 9
    del ops[:]
    with torch.no_grad():                          # float16 keeps the torch formulation; float32 its own kernels
        half_net, half_fpn = copy.deepcopy(net).half(), copy.deepcopy(fpn).half()
        assert half_fpn(half_net(img.half())).dtype == torch.float16 and not ops
        assert fpn(net(img)).dtype == torch.float32 and len(ops) == 9
        assert all(t.dtype == torch.float32 for c in ops for t in c[1])


def test_a_mixed_pair_stays_on_torch(cuda, ops):
    block = ie.BasicBlock(4, 4).to(cuda).eval()
    block.fused_tail = block.fused_tail_bf16 = True
    out32, id16 = torch.randn(2, 4, 6, 8, device=cuda), torch.randn(2, 4, 6, 8, device=cuda).bfloat16()
    assert block._tail(out32, id16).dtype == torch.float32 and block._tail(id16, out32).dtype == torch.float32
    assert not ops
    assert block._tail(id16, id16).dtype == BF16 and len(ops) == 1


def test_custom_resnet_tails_take_the_op(cuda, ops):
    torch.manual_seed(1)
    net = bev_encoder.build_pre_process(dict(type='CustomResNet', numC_input=8, num_layer=[2], num_channels=[8],
                                             stride=[1], backbone_output_ids=[0])).to(cuda).train()
    for m in net.modules():
        if isinstance(m, blocks._Block):           # CustomResNet leaves its tails off by default
            m.fused_tail = m.fused_tail_bf16 = True
    x = torch.randn(2, 8, 12, 20, device=cuda, requires_grad=True)
    with autocast():
        y = net(x)[0]
    assert [c[0] for c in ops] == ['tail'] * 2 and y.dtype == BF16
    check_calls(ops)
    y.float().sum().backward()
    assert x.grad.dtype == torch.float32 and torch.isfinite(x.grad).all()


def test_align_and_cat_takes_bf16_maps_on_the_kernels(cuda, launches):
    s2k, extra = poses(cuda)
    maps = [f.detach().bfloat16().requires_grad_(True) for f in frames(cuda)]
    with autocast():
        got = temporal.align_and_cat(maps, [0, 1, 2], s2k, *extra, fused=True)
    assert launches == ['ocrf_bev_align_forward'] * 2 and got.dtype == torch.float32
    want = temporal.align_and_cat([m.detach().float() for m in maps], [0, 1, 2], s2k, *extra, fused=True)
    assert same_bits(got.detach(), want)
    got.sum().backward()
    assert launches.count('ocrf_bev_align_backward') == 2
    assert all(m.grad.dtype == BF16 and torch.isfinite(m.grad).all() for m in maps)
    # shift_feature and the detector method: the same cast
    tf = temporal.feature_transform([s2k[0], s2k[1]], *extra)
    with autocast():
        one = temporal.shift_feature(maps[1].detach(), tf)
    assert one.dtype == torch.float32 and same_bits(one, temporal.shift_feature(maps[1].detach().float(), tf))
    # float16 maps keep their path: the same cast as before
    del launches[:]
    halves = temporal.align_and_cat([m.detach().half() for m in maps], [0, 1, 2], s2k, *extra, fused=True)
    assert launches == ['ocrf_bev_align_forward'] * 2 and halves.dtype == torch.float32


def by_hand(preds):
    return tuple([{k: v.detach().float() for k, v in p[0].items()}] for p in preds)


def test_center_head_loss_takes_bf16_predictions_on_the_kernels(cuda, golden, launches):
    g = golden('center_head.npz')
    torch.manual_seed(2)
    head = make_head(g).to(cuda).train()
    bx, lab = boxes(g, cuda)
    cfg = head.train_cfg
    W, H = (int(s) // int(cfg['out_size_factor']) for s in cfg['grid_size'][:2])
    x = torch.randn(len(lab), json.loads(str(g['cfg']))['in_ch'], H, W, device=cuda)
    with autocast():
        preds = head([x])
        leaves = [v for p in preds for v in p[0].values()]
        assert all(v.dtype == BF16 for v in leaves)
        losses = head.loss(bx, lab, tuple([dict(p[0])] for p in preds))
    assert 'ocrf_center_head_heatmap_loss' in launches and 'ocrf_center_head_reg_loss' in launches
    want = head.loss(bx, lab, by_hand(preds))
    assert sorted(losses) == sorted(want) and len(losses) > 1
    for k, v in losses.items():
        assert v.dtype == torch.float32 and same_bits(v.detach(), want[k].detach()), k
    grads = torch.autograd.grad(sum(losses.values()), leaves)
    assert all(gr.dtype == BF16 and torch.isfinite(gr).all() for gr in grads)
    assert any(float(gr.float().abs().max()) > 0 for gr in grads)
    assert 'ocrf_center_head_heatmap_loss_backward' in launches and 'ocrf_center_head_reg_loss_backward' in launches


def test_center_head_get_bboxes_takes_bf16_predictions_on_the_kernels(cuda, golden, launches):
    g = golden('center_head_decode.npz')
    torch.manual_seed(3)
    head = make_decode_head(g).to(cuda).eval()
    B, _, H, W = g['t0.heatmap'].shape
    x = torch.randn(B, 8, H, W, device=cuda)
    with torch.no_grad(), autocast():
        preds = head([x])
        assert all(v.dtype == BF16 for p in preds for v in p[0].values())
        got = head.get_bboxes_padded(preds)
        lists = head.get_bboxes(preds, None)
    assert launches.count('ocrf_center_decode') == 2
    want = head.get_bboxes_padded(by_hand(preds))
    assert int(got[3].sum()) > 0
    for a, b in zip(got, want):
        assert same_bits(a, b)
    assert got[0].dtype == got[1].dtype == torch.float32
    for i, (b, s, lab) in enumerate(lists):
        n = int(got[3][i])
        assert b.dtype == s.dtype == torch.float32 and same_bits(b, want[0][i, :n]) and same_bits(s, want[1][i, :n])


def test_stereo_cost_volume_takes_bf16_features_on_the_kernel(cuda, launches):
    metas = sf.metas(sf.load(), cuda)
    prev, curr = metas['cv_feat_list']
    with autocast():
        same = depthnet.stereo_cost_volume(metas, 5.0)                 # float32 features under autocast
        got = depthnet.stereo_cost_volume(dict(metas, cv_feat_list=[prev.bfloat16(), curr.bfloat16()]), 5.0)
    assert launches == ['ocrf_stereo_cost_volume'] * 2
    assert same_bits(same, depthnet.stereo_cost_volume(metas, 5.0))
    want = depthnet.stereo_cost_volume(dict(metas, cv_feat_list=[prev.bfloat16().float(), curr.bfloat16().float()]), 5.0)
    assert got.dtype == torch.float32 and same_bits(got, want)


@pytest.fixture(scope='module')
def neck():
    """The neck of tests/test_neck_gpu.py: the golden core_small configuration."""
    from ocrfdet_amd import view_transformer_ocrf as vto
    cfg, g, state = helpers.core_fixture()
    m = vto.OcRFViewTransformerFull(
        pc_range=list(cfg.pc_range), bev_h=48, bev_w=48, num_height=13, grid_config=cfg.grid,
        input_size=cfg.input_size, downsample=16, in_channels=256, out_channels=80)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    m.cuda().eval()
    B = int(g['batch'])
    voxel, pix, mask, rig = helpers.core_geometry(cfg, B)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    raw = t(g['raw'].astype(np.float32))
    inp = [t(g['x'].astype(np.float32))] + [t(rig[k]) for k in ('rots', 'trans', 'intrins', 'post_rots', 'post_trans', 'bda')]
    inp += [torch.zeros(B, 6, 27).cuda(), raw.clone(), raw, raw.clone(), t(rig['c2w'])]
    return m, cfg, inp, t(g['pre'])


def test_view_transform_is_float32_under_autocast(cuda, neck):
    """The convolutions of the step run without the convolution library here: it may choose another algorithm from one
    call to the next, and bits are compared.  (``cudnn.deterministic`` would pin it too, but the algorithm it makes the
    library prepare stays selected in the process, and that one puts a memset node into a later graph capture.)"""
    from ocrfdet_amd import neck_ops
    m, cfg, inp, pre = neck
    inp16 = [inp[0].bfloat16()] + inp[1:]
    by_hand_inp = [inp16[0].float()] + inp[1:]

    def run(inputs, depthnet_out):
        random.seed(0)                             # the camera choice of view_transform
        depth, fdepth, sem, feat_cl = neck_ops.prefilter(depthnet_out.float(), cfg.D, cfg.channels, m.depth_threshold,
                                                         m.semantic_threshold)
        return m.view_transform(inputs, fdepth, None, feat_cl)
    picked = ((0,), (2,), (3, 0), (3, 4), (3, 6))  # BEV feature, mask logits, rendered image, opacity view, depth

    def pick(out, path):
        for i in path:
            out = out[i]
        return out
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
        run(by_hand_inp, pre)                      # warm-up: plans, scratch
        want = run(by_hand_inp, pre)
        again = run(by_hand_inp, pre)
        with autocast():
            got = run(inp16, pre)
    for path in picked:
        assert same_bits(pick(again, path), pick(want, path)), f'output {path} differs from run to run'
        a = pick(got, path)
        assert a.dtype == torch.float32 and same_bits(a, pick(want, path)), f'output {path}'
    assert got[3][5] == want[3][5]
