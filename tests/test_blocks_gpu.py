"""GPU: the blocks that ``CustomResNet`` and ``DepthNet`` build run the torch residual tail (no ``add_relu`` launch),
forward and backward: the dispatch that keeps their speed where it was measured."""
import pytest
import torch

from ocrfdet_amd import bev_encoder as be
from ocrfdet_amd import blocks, depthnet

pytestmark = pytest.mark.gpu


def test_bev_encoder_and_depthnet_make_no_add_relu_launch(cuda, monkeypatch):
    real, calls = blocks.add_relu, []
    monkeypatch.setattr(blocks, 'add_relu', lambda *a: calls.append(1) or real(*a))
    torch.manual_seed(0)
    enc = be.BEVEncoder(dict(type='CustomResNet', numC_input=8),
                        dict(type='FPN_LSS', in_channels=8 * 8 + 8 * 2, out_channels=8)).to(cuda)
    x = torch.randn(1, 8, 16, 16, device=cuda, requires_grad=True)
    out = enc(x)
    out.square().mean().backward()
    assert out.shape == (1, 8, 16, 16) and torch.isfinite(x.grad).all()
    net = depthnet.DepthNet(8, 8, 4, 6, use_dcn=False).to(cuda)
    y = net(torch.randn(2, 8, 4, 6, device=cuda), torch.randn(2, 27, device=cuda))
    assert y.shape == (2, 6 + 4, 4, 6) and torch.isfinite(y).all()
    assert calls == []
    block = blocks.BasicBlock(8, 8).to(cuda)       # the patch does count: a block with the flag on launches
    block(torch.randn(1, 8, 4, 4, device=cuda))
    assert calls == [1]
