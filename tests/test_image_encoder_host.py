"""CPU: ``ocrfdet_amd.image_encoder`` — ``ResNet``'s torchvision ``state_dict`` layout, shapes, freezing and
checkpointing, and its agreement with the float64 oracle of ``tests/resnet_oracle.py``; ``CustomFPN`` against the
reference's own class through ``tests/golden/image_encoder.npz``; ``ImageEncoder`` against the reference's own
``BEVDet.image_encoder`` / ``extract_stereo_ref_feat`` (bevdet.py:44-64, :600-614) through the same file and against a
restatement of their reshapes and slices; the dispatch on the CPU and the refusals of the four entry points of
``csrc/resnet_fuse.hip`` at the C boundary."""
import ctypes
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ocrfdet_amd import _lib
from ocrfdet_amd import image_encoder as ie
from tests import image_encoder_fixture as fx
from tests import resnet_oracle

BN = ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')


def torchvision_layout(blocks, bottleneck, base=64, in_channels=3):
    """{key: shape} of torchvision's resnet without ``fc``, by formula."""
    want = {'conv1.weight': (base, in_channels, 7, 7)}

    def bn(name, c):
        for leaf in BN:
            want[f'{name}.{leaf}'] = () if leaf == 'num_batches_tracked' else (c,)
    bn('bn1', base)
    inplanes, expansion = base, 4 if bottleneck else 1
    for i, n in enumerate(blocks):
        planes, stride = base * 2 ** i, 1 if i == 0 else 2
        for j in range(n):
            p = f'layer{i + 1}.{j}'
            if bottleneck:
                convs = [(planes, inplanes, 1, 1), (planes, planes, 3, 3), (planes * 4, planes, 1, 1)]
            else:
                convs = [(planes, inplanes, 3, 3), (planes, planes, 3, 3)]
            for k, shape in enumerate(convs, 1):
                want[f'{p}.conv{k}.weight'] = shape
                bn(f'{p}.bn{k}', shape[0])
            if j == 0 and (stride != 1 or inplanes != planes * expansion):
                want[f'{p}.downsample.0.weight'] = (planes * expansion, inplanes, 1, 1)
                bn(f'{p}.downsample.1', planes * expansion)
            inplanes = planes * expansion
    return want


def shapes(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def randomise_stats(module, seed=0):
    """Running statistics and affine parameters that make no norm an identity."""
    gen = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.rand(m.num_features, generator=gen) - 0.5)
            m.running_var.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.bias.copy_(torch.rand(m.num_features, generator=gen) - 0.5)


# ------------------------------------------------------------------------------------------------ ResNet
def test_resnet50_state_dict_is_the_torchvision_layout():
    m = ie.ResNet(depth=50)
    want = torchvision_layout((3, 4, 6, 3), True)
    assert shapes(m) == want and set(m.state_dict()) == set(want)
    convs = [k for k, s in want.items() if len(s) == 4]
    assert len(convs) == 53
    for k in convs:                                # each convolution has a norm behind it
        norm = k.replace('conv', 'bn').replace('downsample.0', 'downsample.1').rsplit('.', 1)[0]
        assert f'{norm}.running_var' in want, k
    assert not any(k.startswith('fc') or k.endswith('.bias') and 'bn' not in k and 'downsample.1' not in k
                   for k in want)
    other = ie.ResNet(depth=50)
    randomise_stats(other)
    res = m.load_state_dict(other.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), other.state_dict().values()))


@pytest.mark.parametrize('depth,blocks,bottleneck', [(18, (2, 2, 2, 2), False), (34, (3, 4, 6, 3), False),
                                                     (101, (3, 4, 23, 3), True), (152, (3, 8, 36, 3), True)])
def test_other_depths_have_the_right_block_counts_and_widths(depth, blocks, bottleneck):
    m = ie.ResNet(depth=depth)
    assert shapes(m) == torchvision_layout(blocks, bottleneck)
    assert m.feat_dim == (2048 if bottleneck else 512)
    assert [len(getattr(m, name)) for name in m.res_layers] == list(blocks)


def test_attributes_the_detector_reads():
    m = ie.ResNet(depth=50, pretrained='torchvision://resnet50', init_cfg=dict(type='Pretrained', checkpoint='x'))
    assert m.pretrained == 'torchvision://resnet50' and m.init_cfg['checkpoint'] == 'x'      # stored, never fetched
    c = m.conv1
    assert (c.kernel_size, c.stride, c.padding, c.bias) == ((7, 7), (2, 2), (3, 3), None)
    assert m.norm1 is m.bn1 and m.norm1_name == 'bn1' and isinstance(m.relu, torch.nn.ReLU)
    p = m.maxpool
    assert (p.kernel_size, p.stride, p.padding) == (3, 2, 1)
    assert m.deep_stem is False and m.res_layers == ['layer1', 'layer2', 'layer3', 'layer4'] and m.feat_dim == 2048
    assert all(hasattr(m, name) for name in m.res_layers)
    d = m.layer2[0].downsample
    assert (d[0].kernel_size, d[0].stride, d[0].bias) == ((1, 1), (2, 2), None) and m.layer1[0].downsample is not None
    assert m.layer1[1].downsample is None and ie.ResNet(depth=18).layer1[0].downsample is None
    assert m.layer2[0].norm3 is m.layer2[0].bn3
    small = ie.ResNet(depth=18, num_stages=2, strides=(1, 2), dilations=(1, 1), out_indices=(1,), stem_channels=8,
                      base_channels=16, in_channels=5)
    assert small.res_layers == ['layer1', 'layer2'] and small.feat_dim == 32
    assert small.conv1.weight.shape == (8, 5, 7, 7) and small.layer1[0].downsample is not None


def test_output_shapes_and_strides():
    m = ie.ResNet(depth=50, out_indices=(0, 2, 3)).eval()
    with torch.no_grad():
        outs = m(torch.zeros(2, 3, 64, 96))
    assert isinstance(outs, tuple)
    assert [tuple(o.shape) for o in outs] == [(2, 256, 16, 24), (2, 1024, 4, 6), (2, 2048, 2, 3)]      # strides 4, 16, 32
    with torch.no_grad():
        odd = ie.ResNet(depth=18, out_indices=(0, 1, 2, 3)).eval()(torch.zeros(1, 3, 50, 70))
    assert [tuple(o.shape) for o in odd] == [(1, 64, 13, 18), (1, 128, 7, 9), (1, 256, 4, 5), (1, 512, 2, 3)]


def test_caffe_style_moves_the_stride():
    a, b = ie.ResNet(depth=50), ie.ResNet(depth=50, style='caffe')
    assert (a.layer2[0].conv1.stride, a.layer2[0].conv2.stride) == ((1, 1), (2, 2))
    assert (b.layer2[0].conv1.stride, b.layer2[0].conv2.stride) == ((2, 2), (1, 1))
    assert b.layer2[1].conv1.stride == (1, 1) and shapes(a) == shapes(b)
    dil = ie.ResNet(depth=50, strides=(1, 2, 1, 1), dilations=(1, 1, 2, 4))
    assert dil.layer4[0].conv2.dilation == (4, 4) and dil.layer4[0].conv2.padding == (4, 4)


@pytest.mark.parametrize('kwargs,word', [
    (dict(deep_stem=True), 'deep_stem'), (dict(avg_down=True), 'avg_down'),
    (dict(dcn=dict(type='DCNv2', deform_groups=1)), 'dcn'), (dict(plugins=[dict(cfg=dict(type='ContextBlock'))]), 'plugins'),
    (dict(conv_cfg=dict(type='ConvWS')), 'conv_cfg'), (dict(norm_cfg=dict(type='GN', num_groups=32)), 'norm_cfg')])
def test_unsupported_arguments_raise_and_name_the_argument(kwargs, word):
    with pytest.raises(NotImplementedError, match=word):
        ie.ResNet(depth=50, **kwargs)


def test_supported_neighbours_build():
    assert isinstance(ie.ResNet(depth=18, conv_cfg=dict(type='Conv2d'), norm_cfg=dict(type='BN2d')).bn1,
                      torch.nn.BatchNorm2d)
    assert isinstance(ie.ResNet(depth=18, norm_cfg=dict(type='SyncBN')).bn1, torch.nn.SyncBatchNorm)
    with pytest.raises(KeyError):
        ie.ResNet(depth=20)
    frozen = ie.ResNet(depth=18, norm_cfg=dict(type='BN', requires_grad=False))
    assert not frozen.bn1.weight.requires_grad and frozen.conv1.weight.requires_grad


def _stats(m):
    return {k: v.clone() for k, v in m.state_dict().items() if 'running_' in k}


def _changed(m, before):
    return {k.split('.')[0] for k, v in _stats(m).items() if not torch.equal(v, before[k])}


def test_frozen_stages_and_norm_eval():
    x = torch.randn(2, 3, 32, 48)
    m = ie.ResNet(depth=18, frozen_stages=1, norm_eval=True)
    for _ in range(2):                             # train() / eval() re-apply the freeze
        m.eval()
        m.train()
        assert m.training and not m.bn1.training and not m.layer1.training
        assert not any(mod.training for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d))
        assert m.layer2.training and m.layer2[0].conv1.training
        frozen = [p for mod in (m.conv1, m.bn1, m.layer1) for p in mod.parameters()]
        assert frozen and not any(p.requires_grad for p in frozen)
        assert all(p.requires_grad for p in m.layer2.parameters())
    before = _stats(m)
    sum(o.sum() for o in m(x)).backward()
    assert _changed(m, before) == set()            # norm_eval: no running statistic moves anywhere
    assert all(p.grad is None for p in frozen) and m.layer2[0].conv1.weight.grad is not None

    m = ie.ResNet(depth=18, frozen_stages=1, norm_eval=False).train()
    before = _stats(m)
    sum(o.sum() for o in m(x)).backward()
    assert _changed(m, before) == {'layer2', 'layer3', 'layer4'}      # exactly the stages that are not frozen
    assert m.conv1.weight.grad is None and m.layer1[0].conv1.weight.grad is None

    m = ie.ResNet(depth=18, frozen_stages=-1, norm_eval=False).train()
    before = _stats(m)
    m(x)
    assert _changed(m, before) == {'bn1', 'layer1', 'layer2', 'layer3', 'layer4'}
    m.eval()
    before = _stats(m)
    m(x)
    assert _changed(m, before) == set()


def test_init_weights():
    m = ie.ResNet(depth=50)
    m.init_weights()
    assert all(float(b.bn3.weight.detach().abs().max()) == 0.0 for layer in (m.layer1, m.layer4) for b in layer)
    assert torch.equal(m.bn1.weight, torch.ones(64)) and torch.equal(m.layer1[0].bn1.bias, torch.zeros(64))
    w = m.layer3[0].conv2.weight                   # fan_out = 256 * 9: std = sqrt(2 / fan_out)
    assert abs(float(w.detach().std()) / (2.0 / (256 * 9)) ** 0.5 - 1.0) < 0.02
    m = ie.ResNet(depth=18, zero_init_residual=False)
    m.init_weights()
    assert torch.equal(m.layer1[0].bn2.weight, torch.ones(64))
    m = ie.ResNet(depth=18)
    m.init_weights()
    assert float(m.layer1[0].bn2.weight.detach().abs().max()) == 0.0 and torch.equal(m.layer1[0].bn1.weight, torch.ones(64))


def test_with_cp_gives_the_same_outputs_and_parameter_gradients():
    torch.manual_seed(0)
    a = ie.ResNet(depth=18, norm_eval=False, with_cp=False)
    b = ie.ResNet(depth=18, norm_eval=False, with_cp=True)
    randomise_stats(a)
    b.load_state_dict(a.state_dict())
    x = torch.randn(2, 3, 32, 48)
    res = []
    for m in (a, b):
        m.train()
        outs = m(x)
        sum(o.square().sum() for o in outs).backward()
        res.append(([o.detach() for o in outs], [p.grad for p in m.parameters()]))
    assert all(torch.equal(p, q) for p, q in zip(res[0][0], res[1][0]))
    assert all(torch.allclose(p, q, rtol=1e-5, atol=1e-6 * float(p.abs().max())) for p, q in zip(res[0][1], res[1][1]))
    # the recomputation runs the norms' training-mode forward a second time, as mmdet's checkpointing does: the running
    # statistics take two momentum steps per iteration
    assert int(a.bn1.num_batches_tracked) == 1 and int(a.layer1[0].bn1.num_batches_tracked) == 1
    assert int(b.bn1.num_batches_tracked) == 1 and int(b.layer1[0].bn1.num_batches_tracked) == 2


@pytest.mark.parametrize('depth', [18, 50])
def test_resnet_agrees_with_the_float64_oracle(depth):
    torch.manual_seed(depth)
    m = ie.ResNet(depth=depth).eval()
    randomise_stats(m, seed=depth)
    x = torch.randn(2, 3, 64, 96)
    with torch.no_grad():
        got = m(x)
    want = resnet_oracle.resnet_eval(m.state_dict(), x)
    assert len(got) == len(want) == 4
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == torch.float32 and w.dtype == torch.float64
        err, ref = float((g.double() - w).abs().max()), float(w.abs().max())
        print(f'depth {depth} out{i}: max|err| {err:.3e}, max|ref| {ref:.3e}, ratio {err / ref:.2e}')
        assert ref > 0 and err <= 1e-5 * ref


def test_oracle_follows_the_style_and_is_not_the_module():
    m = ie.ResNet(depth=50, style='caffe', num_stages=2, strides=(1, 2), dilations=(1, 1), out_indices=(0, 1)).eval()
    randomise_stats(m, seed=3)
    x = torch.randn(1, 3, 33, 47)
    with torch.no_grad():
        got = m(x)
    want = resnet_oracle.resnet_eval(m.state_dict(), x, strides=(1, 2), style='caffe')
    other = resnet_oracle.resnet_eval(m.state_dict(), x, strides=(1, 2), style='pytorch')
    assert len(want) == 2
    for g, w in zip(got, want):
        assert float((g.double() - w).abs().max()) <= 1e-5 * float(w.abs().max())
    assert float((other[1] - want[1]).abs().max()) > 1e-3 * float(want[1].abs().max())


# ------------------------------------------------------------------------------------------------ CustomFPN
def test_fixture_holds_the_cases_of_the_issue():
    g = fx.golden()
    assert list(fx.CASES) == ['odd', 'start1', 'scale2', 'bn', 'ref']
    assert fx.CASES['odd'][1] == [(2, 8, 15, 21), (2, 16, 8, 11)] and fx.CASES['odd'][0]['in_channels'] == [8, 16]
    assert fx.CASES['start1'][0]['start_level'] == 1 and len(fx.CASES['start1'][1]) == 3
    assert fx.CASES['scale2'][0]['upsample_cfg'] == dict(mode='nearest', scale_factor=2)
    assert fx.CASES['bn'][0]['norm_cfg'] == dict(type='BN')
    backbone, neck = fx.reference_dicts()
    assert {k: v for k, v in neck.items() if k != 'type'} == fx.CASES['ref'][0] and neck['type'] == 'CustomFPN'
    assert backbone == dict(pretrained='torchvision://resnet50', type='ResNet', depth=50, num_stages=4,
                            out_indices=(0, 2, 3), frozen_stages=-1, norm_cfg=dict(type='BN', requires_grad=True),
                            norm_eval=False, with_cp=True, style='pytorch')
    for tag in fx.CASES:                           # the seeded stream is the one the generator saw
        for i, x in enumerate(fx.seeded_inputs(tag)):
            assert np.array_equal(x.numpy(), g[f'{tag}.x{i}'])
        flat = torch.cat([v.double().reshape(-1) for v in fx.seeded_state(fx.build(tag), tag).values()])
        assert np.array_equal(np.array([flat.sum().item(), flat.abs().sum().item()]), g[f'{tag}.check'])


@pytest.mark.parametrize('tag', list(fx.CASES))
def test_custom_fpn_has_the_reference_keys(tag):
    m = fx.build(tag)
    want = json.loads(str(fx.golden()[f'{tag}.keys']))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want
    assert isinstance(m.lateral_convs, torch.nn.ModuleList) and isinstance(m.fpn_convs, torch.nn.ModuleList)
    with_norm = 'norm_cfg' in fx.CASES[tag][0]
    for conv in list(m.lateral_convs) + list(m.fpn_convs):
        assert hasattr(conv, 'bn') == with_norm and (conv.conv.bias is None) == with_norm
        assert not hasattr(conv, 'activate')


@pytest.mark.parametrize('tag,mode', [(t, mode) for t, c in fx.CASES.items() for mode in c[2]])
def test_custom_fpn_matches_the_reference(tag, mode):
    fx.check_case(tag, mode, torch.device('cpu'))


def test_custom_fpn_options():
    x = [torch.randn(1, 4, 16, 16), torch.randn(1, 8, 8, 8), torch.randn(1, 16, 4, 4)]
    m = ie.CustomFPN([4, 8, 16], 6, num_outs=5, out_ids=[0, 1, 2], add_extra_convs=True, act_cfg=dict(type='ReLU'),
                     relu_before_extra_convs=True)
    assert m.add_extra_convs == 'on_input' and len(m.fpn_convs) == 5 and m.fpn_convs[3].conv.in_channels == 16
    assert m.fpn_convs[3].conv.stride == (2, 2) and isinstance(m.fpn_convs[0].activate, torch.nn.ReLU)
    assert m(x).shape == (1, 6, 16, 16)
    for where in ('on_lateral', 'on_output'):
        m = ie.CustomFPN([4, 8, 16], 6, num_outs=4, out_ids=[0, 1, 2], add_extra_convs=where)
        assert m.fpn_convs[3].conv.in_channels == 6 and m(x).shape == (1, 6, 16, 16)
    m = ie.CustomFPN([4, 8, 16], 6, num_outs=5, out_ids=[0, 1, 2])                  # max_pool2d extra levels
    assert len(m.fpn_convs) == 3 and m(x).shape == (1, 6, 16, 16)
    m = ie.CustomFPN([4, 8, 16], 6, num_outs=2, end_level=2, out_ids=[0, 1])
    assert len(m.lateral_convs) == 2 and m(x).shape == (1, 6, 16, 16)
    m = ie.CustomFPN([4, 8, 16], 6, num_outs=3, out_ids=[0], norm_cfg=dict(type='BN'), no_norm_on_lateral=True)
    assert not hasattr(m.lateral_convs[0], 'bn') and m.lateral_convs[0].conv.bias is not None
    assert hasattr(m.fpn_convs[0], 'bn') and m.fpn_convs[0].conv.bias is None
    m = ie.CustomFPN([4, 8, 16], 6, num_outs=1, out_ids=[0], upsample_cfg=dict(mode='bilinear', align_corners=False))
    lat = [c(t) for c, t in zip(m.lateral_convs, x)]
    lat[1] = lat[1] + F.interpolate(lat[2], size=(8, 8), mode='bilinear', align_corners=False)
    lat[0] = lat[0] + F.interpolate(lat[1], size=(16, 16), mode='bilinear', align_corners=False)
    assert torch.allclose(m(x), m.fpn_convs[0](lat[0]), rtol=1e-5, atol=1e-6)
    m.init_weights()
    w = m.fpn_convs[0].conv.weight                 # Xavier uniform: |w| <= sqrt(6 / (fan_in + fan_out))
    assert float(w.detach().abs().max()) <= (6.0 / (6 * 9 + 6 * 9)) ** 0.5
    assert float(m.fpn_convs[0].conv.bias.detach().abs().max()) == 0
    with pytest.raises(NotImplementedError):
        ie.CustomFPN([4, 8], 6, num_outs=1, out_ids=[0], norm_cfg=dict(type='GN', num_groups=2))
    with pytest.raises(NotImplementedError):
        ie.CustomFPN([4, 8], 6, num_outs=1, out_ids=[0], conv_cfg=dict(type='ConvWS'))
    with pytest.raises(NotImplementedError):
        ie.CustomFPN([4, 8], 6, num_outs=1, out_ids=[0], act_cfg=dict(type='Mish'))


# ------------------------------------------------------------------------------------------------ ImageEncoder
def small_encoder():
    torch.manual_seed(1)
    enc = ie.ImageEncoder(dict(type='ResNet', depth=18, out_indices=(0, 2, 3), norm_eval=False, base_channels=8),
                          dict(type='CustomFPN', in_channels=[32, 64], out_channels=6, num_outs=1, start_level=0,
                               out_ids=[0]))
    randomise_stats(enc)
    return enc


def test_image_encoder_wiring():
    enc = small_encoder().eval()
    assert enc.with_img_neck and isinstance(enc.img_backbone, ie.ResNet) and isinstance(enc.img_neck, ie.CustomFPN)
    keys = list(enc.state_dict())
    assert 'img_backbone.conv1.weight' in keys and 'img_backbone.layer4.1.bn2.running_var' in keys
    assert 'img_neck.lateral_convs.1.conv.bias' in keys and 'img_neck.fpn_convs.0.conv.weight' in keys
    assert all(k.startswith(('img_backbone.', 'img_neck.')) for k in keys)
    img = torch.randn(2, 3, 3, 64, 96)
    with torch.no_grad():
        x, stereo = enc.image_encoder(img, stereo=True)
        feats = enc.img_backbone(img.view(6, 3, 64, 96))
        assert torch.equal(stereo, feats[0]) and stereo.shape == (6, 8, 16, 24)      # layer1's map
        want = enc.img_neck(feats[1:])                                            # the neck sees x[1:]
        assert x.shape == (2, 3, 6, 4, 6) and torch.equal(x, want.view(2, 3, 6, 4, 6))
        assert torch.equal(enc.extract_stereo_ref_feat(img), stereo)              # bit for bit in eval mode
        enc.img_backbone.out_indices = (2, 3)                                     # stereo=False: every level to the neck
        y, none = enc(img)                                                        # forward = image_encoder
        assert none is None and torch.equal(y, x)
    bare = ie.ImageEncoder(dict(depth=18, out_indices=(3,), base_channels=8)).eval()
    assert not bare.with_img_neck and not any(k.startswith('img_neck') for k in bare.state_dict())
    with pytest.raises(AttributeError):            # the reference, too, needs a neck to turn the tuple into a map
        bare(img)


def test_image_encoder_matches_the_reference_wiring():
    """``wiring.*`` of the fixture: the reference's own ``BEVDet.image_encoder`` and ``extract_stereo_ref_feat`` over
    this package's ``ResNet`` and the reference's ``CustomFPN``."""
    g = fx.golden()
    enc = ie.ImageEncoder(fx.WIRING['img_backbone'], fx.WIRING['img_neck']).eval()
    enc.img_backbone.load_state_dict(fx.seeded_state(enc.img_backbone, 'wiring.backbone'), strict=True)
    enc.img_neck.load_state_dict(fx.seeded_state(enc.img_neck, 'wiring.neck'), strict=True)
    img, = fx.seeded_inputs('wiring')
    with torch.no_grad():
        x, stereo_feat = enc(img, stereo=True)
        ref_feat = enc.extract_stereo_ref_feat(img)
        enc.img_backbone.out_indices = (2, 3)
        x_mono, none = enc(img, stereo=False)
    assert none is None and x.shape == (1, 2, 6, 4, 6) and stereo_feat.shape == (2, 8, 16, 24)
    fx.close(x.numpy(), g['wiring.x'], 'x')
    fx.close(stereo_feat.numpy(), g['wiring.stereo_feat'], 'stereo_feat')
    fx.close(ref_feat.numpy(), g['wiring.ref_feat'], 'extract_stereo_ref_feat')
    fx.close(x_mono.numpy(), g['wiring.x_mono'], 'x without stereo')
    assert float(np.abs(g['wiring.x']).max()) > 0.1 and float(np.abs(g['wiring.stereo_feat']).max()) > 0.1


def test_image_encoder_of_the_reference_config_builds_with_the_detector_keys():
    backbone, neck = fx.reference_dicts()
    enc = ie.ImageEncoder(backbone, neck)
    net = enc.img_backbone
    assert net.with_cp and not net.norm_eval and net.out_indices == (0, 2, 3) and net.frozen_stages == -1
    assert net.pretrained == 'torchvision://resnet50'
    got = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    want = {f'img_backbone.{k}': s for k, s in torchvision_layout((3, 4, 6, 3), True).items()}
    want.update({f'img_neck.{k}': tuple(s) for k, s in json.loads(str(fx.golden()['ref.keys']))})
    assert got == want
    assert got['img_neck.lateral_convs.0.conv.weight'] == (256, 1024, 1, 1)
    assert got['img_neck.lateral_convs.1.conv.bias'] == (256,) and got['img_neck.fpn_convs.0.conv.weight'][2:] == (3, 3)


def test_other_types_are_refused():
    with pytest.raises(NotImplementedError):
        ie.ImageEncoder(dict(type='SwinTransformer', depth=50))
    with pytest.raises(NotImplementedError):
        ie.ImageEncoder(dict(type='ResNet', depth=18), dict(type='FPN_LSS', in_channels=[8], out_channels=4, num_outs=1))


def test_exports():
    import ocrfdet_amd
    assert ocrfdet_amd.ResNet is ie.ResNet and ocrfdet_amd.CustomFPN is ie.CustomFPN
    assert ocrfdet_amd.ImageEncoder is ie.ImageEncoder


# ------------------------------------------------------------------------------------------------ dispatch and the C ABI
def test_fused_ops_raise_on_the_cpu_and_the_modules_take_the_torch_path():
    a, b = torch.randn(2, 3, 4, 5), torch.randn(2, 3, 4, 5)
    with pytest.raises(_lib.OcrfHipError):
        ie.add_relu(a, b)
    with pytest.raises(_lib.OcrfHipError):
        ie.upsample_add(torch.randn(1, 2, 4, 6), torch.randn(1, 2, 2, 3), size=(4, 6))
    assert torch.equal(ie.add_relu_torch(a, b), torch.relu(a + b))
    assert torch.equal(ie.upsample_add_torch(torch.ones(1, 1, 2, 2), torch.tensor([[[[3.0]]]]), scale_factor=2),
                       torch.full((1, 1, 2, 2), 4.0))
    net = ie.ResNet(depth=18, base_channels=8).eval()
    fpn = ie.CustomFPN([8, 16], 4, num_outs=1, out_ids=[0])
    x, maps = torch.randn(1, 3, 32, 32), [torch.randn(1, 8, 8, 8), torch.randn(1, 16, 4, 4)]
    res = []
    for flag in (True, False):
        net.fused_tail = flag
        fpn.fused_merge = flag
        assert net.fused_tail is flag and all(b.fused_tail is flag for b in net.layer3)
        with torch.no_grad():
            res.append((net(x), fpn(maps)))
    assert all(torch.equal(p, q) for p, q in zip(res[0][0], res[1][0])) and torch.equal(res[0][1], res[1][1])


def test_nearest_rule_is_torchs():
    """The kernel's index rule, stated in numpy float32, against ``F.interpolate(size=...)`` on the CPU for every
    in <= 96 and out < 200, and against integer ``scale_factor`` 2, 3 and 4 (where torch scales by 1 / factor)."""
    pairs = 0
    for n_in in range(1, 97):
        src = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
        for n_out in range(1, 200):
            want = F.interpolate(src, size=(1, n_out)).view(-1).long().numpy()
            d = np.arange(n_out, dtype=np.float32)
            got = np.minimum(np.floor(d * (np.float32(n_in) / np.float32(n_out))).astype(np.int64), n_in - 1)
            assert np.array_equal(got, want), (n_in, n_out)
            pairs += 1
        for s in (2, 3, 4):
            want = F.interpolate(src.expand(1, 1, 2, n_in), scale_factor=s).long()[0, 0, 0].numpy()
            d = np.arange(n_in * s, dtype=np.float32)
            got = np.minimum(np.floor(d * (np.float32(n_in) / np.float32(n_in * s))).astype(np.int64), n_in - 1)
            assert np.array_equal(got, want) and np.array_equal(got, np.arange(n_in * s) // s), (n_in, s)
    assert pairs == 19104


def test_c_boundary_refuses_two_gib_operands():
    """Argument validation alone: the calls return before anything is launched, the pointers are never dereferenced."""
    L = _lib.lib()
    p = ctypes.c_void_p(4096)
    invalid = 1                                    # hipErrorInvalidValue
    for fn in (L.ocrf_add_relu_forward, L.ocrf_add_relu_backward):
        assert fn(1 << 29, p, p, p, None) == invalid                      # exactly 2 GiB
        assert fn((1 << 29) + 1, p, p, p, None) == invalid
        assert fn(1 << 40, p, p, p, None) == invalid
        assert fn(0, p, p, p, None) == invalid and fn(-4, p, p, p, None) == invalid
        assert fn(16, None, p, p, None) == invalid and fn(16, p, p, None, None) == invalid
    fwd, bwd = L.ocrf_upsample_add_forward, L.ocrf_upsample_add_backward
    # 48 x 256 x 256 x 704 floats = 8.25 GiB of destination; 1 x 2048 x 512 x 512 = exactly 2 GiB
    for shape in [(48, 256, 128, 352, 256, 704), (1, 2048, 256, 256, 512, 512), (1 << 16, 1 << 16, 1, 1, 1, 1),
                  (1 << 20, 1 << 20, 1, 1, 2, 2)]:
        assert fwd(*shape, p, p, p, None) == invalid
        assert bwd(*shape, p, p, None) == invalid
    assert fwd(1, 1, 8, 8, 4, 16, p, p, p, None) == invalid               # a smaller target
    assert bwd(1, 1, 8, 8, 16, 4, p, p, None) == invalid
    assert fwd(1, 1, 8, 8, 4096, 4097, p, p, p, None) == invalid          # Hout + Wout > 8192
    assert fwd(1, 1, 0, 8, 16, 16, p, p, p, None) == invalid
    assert fwd(1, 1, 8, 8, 16, 16, p, None, p, None) == invalid and bwd(1, 1, 8, 8, 16, 16, None, p, None) == invalid
