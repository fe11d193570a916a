"""CPU: ``ocrfdet_amd.bev_encoder`` against ``tests/golden/bev_encoder.npz`` — the reference's own ``FPN_LSS`` and
``CustomResNet`` over the generator's restatement of the two mmdet 2.x blocks — forward and gradients in ``eval()`` and
``train()`` at 1e-4 of each tensor's largest magnitude; ``strict=True`` loads; the exact ``state_dict`` keys and shapes
of the reference config's three dicts; ``upsample_cat_torch`` against the float64 oracle of the kernel's sampling rule;
the refusals."""
import json

import numpy as np
import pytest
import torch

from ocrfdet_amd import bev_encoder as be
from tests import bev_encoder_fixture as fx
from tests import upsample_oracle as uo

RESNETS, FPNS, _ = fx.cases()
ALL = list(RESNETS) + list(FPNS)


def test_fixture_holds_the_cases_of_the_issue():
    assert RESNETS['resnet'] == dict(numC_input=8, num_channels=[16, 32, 64])
    assert fx.golden()['x'].shape == (2, 8, 16, 24)
    assert RESNETS['pre'] == dict(numC_input=8, num_layer=[2], num_channels=[8], stride=[1], backbone_output_ids=[0])
    assert RESNETS['bottle']['block_type'] == 'BottleNeck'
    assert FPNS['fpn'] == dict(in_channels=80, out_channels=12)
    assert FPNS['fpn_noextra']['extra_upsample'] is None and FPNS['fpn_lateral']['lateral'] == 16
    assert FPNS['fpn_inconv']['use_input_conv'] is True
    for tag in ALL:                                # non-trivial BatchNorm running statistics
        st = fx.state_dict(tag)
        var = torch.cat([v.reshape(-1) for k, v in st.items() if k.endswith('running_var')])
        mean = torch.cat([v.reshape(-1) for k, v in st.items() if k.endswith('running_mean')])
        assert var.min() >= 0.5 and var.std() > 0.1 and mean.abs().max() > 0.25


@pytest.mark.parametrize('tag', ALL)
def test_state_dict_loads_strictly_with_the_reference_key_order(tag):
    m = fx.build(tag)
    want = json.loads(str(fx.golden()[f'{tag}.keys']))
    assert [[k, list(v.shape), bool(v.dtype.is_floating_point)] for k, v in m.state_dict().items()] == want
    res = m.load_state_dict(fx.state_dict(tag), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


@pytest.mark.parametrize('mode', ['eval', 'train'])
@pytest.mark.parametrize('tag', ALL)
def test_modules_match_the_reference_forward_and_gradients(tag, mode):
    fx.check_case(tag, mode, torch.device('cpu'))


def test_reference_config_key_lists():
    """The three dicts of configs/ocrfdet/ocrfdet.py:79-93 at full channel counts: built, never run."""
    g = fx.golden()
    cfg, keys = json.loads(str(g['ref_config'])), json.loads(str(g['ref_keys']))
    assert cfg['img_bev_encoder_backbone'] == dict(type='CustomResNet', numC_input=160, num_channels=[160, 320, 640])
    assert cfg['img_bev_encoder_neck'] == dict(type='FPN_LSS', in_channels=800, out_channels=256)
    enc = be.BEVEncoder(cfg['img_bev_encoder_backbone'], cfg['img_bev_encoder_neck'])
    pre = be.build_pre_process(cfg['pre_process'])
    assert isinstance(pre, be.CustomResNet) and list(pre.backbone_output_ids) == [0]
    want = {f'img_bev_encoder_backbone.{k}': v for k, v in keys['img_bev_encoder_backbone'].items()}
    want.update({f'img_bev_encoder_neck.{k}': v for k, v in keys['img_bev_encoder_neck'].items()})
    got = {k: list(v.shape) for k, v in enc.state_dict().items()}
    assert list(got.items()) == list(want.items())
    assert list({k: list(v.shape) for k, v in pre.state_dict().items()}.items()) == list(keys['pre_process'].items())
    assert got['img_bev_encoder_neck.up2.4.bias'] == [256] and got['img_bev_encoder_neck.conv.0.weight'] == [512, 800, 3, 3]
    assert 'img_bev_encoder_backbone.layers.2.0.downsample.bias' in got


def test_bev_encoder_is_backbone_then_neck_in_float32():
    resnets, fpns, _ = fx.cases()
    enc = be.BEVEncoder(dict(type='CustomResNet', **resnets['resnet']), dict(type='FPN_LSS', **fpns['fpn'])).eval()
    enc.img_bev_encoder_backbone.load_state_dict(fx.state_dict('resnet'))
    enc.img_bev_encoder_neck.load_state_dict(fx.state_dict('fpn'))
    x = torch.from_numpy(fx.golden()['x'])
    with torch.no_grad():
        y = enc(x)
        fx.close(y.numpy(), fx.golden()['fpn.eval.out0'], 'encoder')
        with torch.autocast('cpu', dtype=torch.bfloat16):
            y16 = enc(x.bfloat16())
    assert y16.dtype == torch.float32
    fx.close(y16.numpy(), enc(x.bfloat16().float()).detach().numpy(), 'encoder under autocast')


def test_with_cp_gives_the_same_gradients():
    cfg = fx.cases()[0]['resnet']
    a, b = be.CustomResNet(**cfg), be.CustomResNet(with_cp=True, **cfg)
    a.load_state_dict(fx.state_dict('resnet'))
    b.load_state_dict(fx.state_dict('resnet'))
    x = torch.from_numpy(fx.golden()['x'])
    grads = []
    for m in (a, b):
        xi = x.clone().requires_grad_(True)
        sum(f.square().sum() for f in m(xi)).backward()
        grads.append(xi.grad)
    assert torch.allclose(grads[0], grads[1], rtol=1e-5, atol=1e-6)


def test_refusals():
    with pytest.raises(NotImplementedError):
        be.FPN_LSS(80, 12, norm_cfg=dict(type='GN', num_groups=4))
    with pytest.raises(NotImplementedError):
        be.CustomResNet(8, norm_cfg=dict(type='LN'))
    with pytest.raises(NotImplementedError):
        be.CustomResNet(8, block_type='Wide')
    for kind in ('BN', 'BN2d', 'SyncBN'):
        m = be.FPN_LSS(80, 12, norm_cfg=dict(type=kind))
        assert isinstance(m.conv[1], torch.nn.SyncBatchNorm if kind == 'SyncBN' else torch.nn.BatchNorm2d)
    with pytest.raises(NotImplementedError):
        be.BEVEncoder(dict(type='ResNet', numC_input=8), dict(type='FPN_LSS', in_channels=80, out_channels=12))
    with pytest.raises(NotImplementedError):
        be.BEVEncoder(dict(type='CustomResNet', numC_input=8), dict(type='CustomFPN', in_channels=80, out_channels=12))
    with pytest.raises(NotImplementedError):
        be.build_pre_process(dict(type='ResNet', numC_input=8))
    assert isinstance(be.build_pre_process(dict(numC_input=8, num_layer=[2], stride=[1])), be.CustomResNet)


def test_fpn_lss_dispatch_on_the_cpu_is_the_torch_formulation():
    m = be.FPN_LSS(80, 12)
    assert m.fused_upsample is True
    m.load_state_dict(fx.state_dict('fpn'))
    m.eval()
    with torch.no_grad():
        a = m(fx.inputs('fpn'))
        m.fused_upsample = False
        b = m(fx.inputs('fpn'))
    assert torch.equal(a, b)
    from ocrfdet_amd import _lib
    with pytest.raises(_lib.OcrfHipError):
        be.upsample_cat(None, torch.zeros(1, 1, 2, 2), 2)


@pytest.mark.parametrize('scale', [2, 4])
@pytest.mark.parametrize('hw', [(1, 1), (1, 5), (2, 3), (5, 7), (16, 12)])
def test_upsample_cat_torch_against_the_float64_oracle(hw, scale):
    """torch's lambda comes from the float product d * ((in - 1) / (out - 1)): off by up to in * 2^-23 from the rule's,
    which moves the value by at most 2 max|x1| * that per axis; 2^-20 covers the float32 arithmetic of the blend."""
    rng = np.random.default_rng(3)
    x1 = rng.standard_normal((2, 3, *hw)).astype(np.float32)
    x2 = rng.standard_normal((2, 2, hw[0] * scale, hw[1] * scale)).astype(np.float32)
    got = be.upsample_cat_torch(torch.from_numpy(x2), torch.from_numpy(x1), scale).numpy()
    want = uo.upsample_cat(x2, x1, scale)
    assert np.array_equal(got[:, :2], x2)
    bound = (max(hw) * 2.0 ** -22 + 2.0 ** -20) * np.abs(x1).max()
    assert np.abs(got[:, 2:] - want[:, 2:]).max() <= bound
    assert np.array_equal(be.upsample_cat_torch(None, torch.from_numpy(x1), scale).numpy(), got[:, 2:])


def test_oracle_transpose_is_the_adjoint_of_the_oracle():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((1, 2, 3, 5))
    g = rng.standard_normal((1, 2, 12, 20))
    assert abs((uo.upsample(x, 4) * g).sum() - (x * uo.upsample_transpose(g, 4)).sum()) <= 1e-12 * np.abs(g).sum()
    # a constant stays a constant: the weights of an output pixel sum to 1
    assert np.abs(uo.upsample(np.ones((1, 1, 3, 2)), 2) - 1.0).max() <= 1e-15
