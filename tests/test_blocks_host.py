"""CPU: ``ocrfdet_amd.blocks`` is the one definition of the residual blocks and of ``ConvModule`` that the encoders,
``DepthNet`` and ``CenterHead`` build from; the blocks keep their ``state_dict`` layout; only ``ResNet``'s blocks take the
fused residual tail."""
import ast
import inspect

from torch import nn

from ocrfdet_amd import bev_encoder as be
from ocrfdet_amd import blocks, depthnet
from ocrfdet_amd import center_head as ch
from ocrfdet_amd import image_encoder as ie

BN = ['weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked']


def _blocks(module):
    found = [m for m in module.modules() if isinstance(m, blocks._Block)]
    assert found
    return found


def test_every_module_builds_the_same_classes():
    assert depthnet.BasicBlock is blocks.BasicBlock and 'BasicBlock' in depthnet.__all__
    assert be.BasicBlock is blocks.BasicBlock and be.Bottleneck is blocks.Bottleneck
    assert ie.BasicBlock is blocks.BasicBlock and ie.Bottleneck is blocks.Bottleneck
    assert ie.ConvModule is blocks.ConvModule and issubclass(ch.ConvBNReLU, blocks.ConvModule)
    assert 'ConvBNReLU' in ch.__all__


def test_image_encoder_imports_nothing_from_bev_encoder():
    for node in ast.walk(ast.parse(inspect.getsource(ie))):
        if isinstance(node, ast.ImportFrom):
            assert 'bev_encoder' not in (node.module or '') and all(a.name != 'bev_encoder' for a in node.names)
        elif isinstance(node, ast.Import):
            assert all('bev_encoder' not in a.name for a in node.names)


def test_only_resnets_blocks_take_the_fused_tail():
    assert blocks.FUSED_TAIL_DEFAULT is True and ie.FUSED_TAIL_DEFAULT is True
    for block_type, kind in (('Basic', blocks.BasicBlock), ('BottleNeck', blocks.Bottleneck)):
        found = _blocks(be.CustomResNet(8, block_type=block_type))
        assert len(found) == 6 and all(type(m) is kind and m.fused_tail is False for m in found)
    found = _blocks(depthnet.DepthNet(8, 8, 4, 6, use_dcn=False, stereo=True))
    assert len(found) == 3 and all(type(m) is blocks.BasicBlock and m.fused_tail is False for m in found)
    for depth, kind, n in ((18, blocks.BasicBlock, 8), (50, blocks.Bottleneck, 16)):
        net = ie.ResNet(depth)
        found = _blocks(net)
        assert len(found) == n and all(type(m) is kind and m.fused_tail is True for m in found) and net.fused_tail


def test_state_dict_keys_of_the_blocks():
    assert list(blocks.BasicBlock(4, 4).state_dict()) == \
        ['conv1.weight'] + [f'bn1.{k}' for k in BN] + ['conv2.weight'] + [f'bn2.{k}' for k in BN]
    downsample = nn.Sequential(nn.Conv2d(8, 8, 1, stride=2, bias=False), nn.BatchNorm2d(8))
    assert list(blocks.Bottleneck(8, 2, stride=2, downsample=downsample).state_dict()) == \
        ['conv1.weight'] + [f'bn1.{k}' for k in BN] + ['conv2.weight'] + [f'bn2.{k}' for k in BN] + \
        ['conv3.weight'] + [f'bn3.{k}' for k in BN] + ['downsample.0.weight'] + [f'downsample.1.{k}' for k in BN]
    assert list(ch.ConvBNReLU(3, 4, 3, padding=1).state_dict()) == ['conv.weight'] + [f'bn.{k}' for k in BN]
