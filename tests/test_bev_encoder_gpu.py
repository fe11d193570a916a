"""GPU: ``ocrfdet_amd.bev_encoder`` against ``tests/golden/bev_encoder.npz`` with the fused upsample-concat and without
it, fused against unfused gradients, and the chain neck output -> pre_process -> cat -> BEVEncoder -> CenterHead ->
loss / get_bboxes at toy size."""
import pytest
import torch

from ocrfdet_amd import bev_encoder as be
from ocrfdet_amd import center_head as ch
from tests import bev_encoder_fixture as fx

pytestmark = pytest.mark.gpu

RESNETS, FPNS, _ = fx.cases()


@pytest.mark.parametrize('mode', ['eval', 'train'])
@pytest.mark.parametrize('tag', list(RESNETS))
def test_custom_resnet_matches_the_reference(cuda, tag, mode):
    fx.check_case(tag, mode, cuda)


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('mode', ['eval', 'train'])
@pytest.mark.parametrize('tag', list(FPNS))
def test_fpn_lss_matches_the_reference(cuda, monkeypatch, tag, mode, fused):
    real, calls = be.upsample_cat, []
    monkeypatch.setattr(be, 'upsample_cat', lambda *a: calls.append(1) or real(*a))
    fx.check_case(tag, mode, cuda, fused=fused)
    want = (2 if FPNS[tag].get('extra_upsample', 2) is not None else 1) if fused else 0
    assert len(calls) == want                       # up + cat, and up2[0]


@pytest.mark.parametrize('tag', list(FPNS))
def test_fused_against_unfused_gradients(cuda, tag):
    """The two paths differ by the last bits of lambda: per upsampling at most (in * 2^-22 + 2^-20) of the upsampled
    map's largest magnitude (tests/test_upsample_cat_gpu.py).  Here ``up`` reads a 2 x 3 map (in = 3: 1.75 * 2^-20) and
    ``up2[0]`` an 8 x 12 map (in = 12: 2^-18): 1.44 * 2^-18 = 5.5e-6 in all.  Everything else is the same convolutions
    and batch norms on the same shapes in both runs.  The perturbation passes through at most four conv + norm + ReLU
    layers forward and back; the fixture's weights are scaled by fan_in^-1/2 and the norms divide by a standard deviation
    of order 1, so a layer passes a relative perturbation on at about its size; an allowance of 11 for all of them gives
    the bound used: 2^-14 = 6.1e-5 of each tensor's largest magnitude, outputs and gradients alike.  That is below the
    1e-4 at which either path is held to the reference."""
    bound = 2.0 ** -14
    res = {}
    for fused in (True, False):
        m = fx.build(tag)
        m.load_state_dict(fx.state_dict(tag))
        m = m.to(cuda).train()
        m.fused_upsample = fused
        leaves = [x.to(cuda).requires_grad_(True) for x in fx.inputs(tag)]
        out = m(leaves)
        (out * torch.from_numpy(fx.golden()[f'{tag}.R0']).to(cuda)).sum().backward()
        res[fused] = [out.detach()] + [x.grad for x in leaves if x.grad is not None] + \
                     [p.grad for p in m.parameters()]
    for a, b in zip(res[True], res[False]):
        err, ref = float((a - b).abs().max()), float(b.abs().max())
        assert err <= bound * ref, (tuple(a.shape), err, bound * ref)


def test_chain_from_neck_output_to_losses_and_boxes(cuda):
    torch.manual_seed(0)
    C = 8
    pre = be.build_pre_process(dict(type='CustomResNet', numC_input=C, num_layer=[2], num_channels=[C], stride=[1],
                                    backbone_output_ids=[0])).to(cuda)
    enc = be.BEVEncoder(dict(type='CustomResNet', numC_input=2 * C, num_channels=[2 * C, 4 * C, 8 * C]),
                        dict(type='FPN_LSS', in_channels=8 * C + 2 * C, out_channels=16)).to(cuda)
    tasks = [dict(num_class=1, class_names=['car']), dict(num_class=2, class_names=['pedestrian', 'traffic_cone'])]
    common = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2))
    train_cfg = dict(point_cloud_range=[-6.4, -6.4, -5.0, 6.4, 6.4, 3.0], grid_size=[128, 128, 40],
                     voxel_size=[0.1, 0.1, 0.2], out_size_factor=8, dense_reg=1, gaussian_overlap=0.1, max_objs=20,
                     min_radius=2, code_weights=[1.0] * 8 + [0.2, 0.2])
    coder = dict(type='CenterPointBBoxCoder', pc_range=[-6.4, -6.4], post_center_range=[-8.0, -8.0, -10.0, 8.0, 8.0, 10.0],
                 max_num=50, score_threshold=0.05, out_size_factor=8, voxel_size=[0.1, 0.1], code_size=9)
    test_cfg = dict(pc_range=[-6.4, -6.4], post_center_limit_range=[-8.0, -8.0, -10.0, 8.0, 8.0, 10.0], max_per_img=50,
                    max_pool_nms=False, min_radius=[4, 0.175], score_threshold=0.05, out_size_factor=8,
                    voxel_size=[0.1, 0.1], pre_max_size=100, post_max_size=20, nms_type=['circle', 'rotate'],
                    nms_thr=[0.2, 0.2], nms_rescale_factor=[1.0, [1.0, 1.0]])
    head = ch.CenterHead(in_channels=16, tasks=tasks, common_heads=common, share_conv_channel=16, train_cfg=train_cfg,
                         test_cfg=test_cfg, bbox_coder=coder,
                         loss_bbox=dict(type='L1Loss', reduction='mean', loss_weight=0.25)).to(cuda)
    frames = [torch.randn(2, C, 16, 16, device=cuda) for _ in range(2)]      # the neck's output, per frame
    boxes = [torch.tensor([[1.0, -2.0, -1.0, 1.9, 4.5, 1.6, 0.3, 0.5, -0.2],
                           [-3.0, 3.5, -1.2, 0.7, 0.7, 1.8, 1.0, 0.0, 0.0]], device=cuda),
             torch.tensor([[4.0, 4.0, -0.8, 0.4, 0.4, 1.0, -2.0, 0.0, 0.0]], device=cuda)]
    labels = [torch.tensor([0, 1], device=cuda), torch.tensor([2], device=cuda)]

    def forward():
        bev = torch.cat([pre(f)[0] for f in frames], dim=1)
        assert bev.shape == (2, 2 * C, 16, 16)
        feat = enc(bev)
        assert feat.shape == (2, 16, 16, 16) and feat.dtype == torch.float32
        return head([feat])

    for m in (pre, enc, head):
        m.train()
    preds = forward()
    assert len(preds) == 2 and preds[0][0]['heatmap'].shape == (2, 1, 16, 16)
    assert preds[1][0]['heatmap'].shape == (2, 2, 16, 16)
    losses = head.loss(boxes, labels, preds)
    assert len(losses) == 12 and all(torch.isfinite(v) for v in losses.values())
    sum(losses.values()).backward()
    grad = pre.layers[0][0].conv1.weight.grad
    assert grad is not None and torch.isfinite(grad).all() and grad.abs().max() > 0
    assert enc.img_bev_encoder_neck.up2[4].bias.grad is not None

    for m in (pre, enc, head):
        m.eval()
    with torch.no_grad():
        dets = head.get_bboxes(forward(), [dict(), dict()])
    assert isinstance(dets, list) and len(dets) == 2
    for det in dets:
        assert isinstance(det, (list, tuple)) and len(det) == 3
        bx, sc, lb = det
        assert bx.shape[1:] == (9,) and sc.shape == lb.shape == (bx.shape[0],)
