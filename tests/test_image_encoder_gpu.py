"""GPU: ``ocrfdet_amd.image_encoder``'s modules with the fused tail / merge on and off, ``CustomFPN`` against
``tests/golden/image_encoder.npz``, and the reference config's ``ImageEncoder`` at toy size.

The fused ops are exact (tests/test_resnet_fuse_gpu.py), so both settings compute the same values, and they are held to
1e-5 of each tensor's largest magnitude.  The convolution library's own choice of algorithm is not this package's to
pin, but a test has to keep it out of the comparison: measured on one MI355X, the UNFUSED ResNet-50 in training mode on
(2, 3, 64, 96) differs from its own second run by up to 2.7e-5 of the largest magnitude in ``layer4``'s output, 6.5e-4 in
the input gradient and 7.3e-3 in a parameter gradient (``layer4``'s batch norms see 12 values per channel and amplify
the last bits of a non-deterministic convolution); fused against unfused differs by no more (2.5e-5, 3.2e-5, 5.2e-5).
With ``torch.backends.cudnn.deterministic = True`` the unfused model reproduces itself bit for bit, and fused against
unfused is bit-equal in every output and gradient, in ``eval()`` and in ``train()``.  So every test of this file runs
with that flag set; the bound stays where the issue put it."""
import copy

import pytest
import torch

from ocrfdet_amd import blocks
from ocrfdet_amd import image_encoder as ie
from tests import image_encoder_fixture as fx

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(autouse=True)
def deterministic_convolutions():
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


def assert_close(got, want, what):
    assert got.shape == want.shape, what
    err, ref = float((got - want).abs().max()), float(want.abs().max())
    print(f'{what}: max|diff| {err:.3e}, max|ref| {ref:.3e}')
    assert err <= TOL * ref, f'{what}: {err:.3e} > {TOL * ref:.3e}'


def count_calls(monkeypatch):
    calls = []
    tail, merge = ie.add_relu, ie.upsample_add
    monkeypatch.setattr(blocks, 'add_relu', lambda *a: calls.append('tail') or tail(*a))
    monkeypatch.setattr(ie, 'upsample_add', lambda *a, **k: calls.append('merge') or merge(*a, **k))
    return calls


def test_resnet50_fused_tail_on_and_off(cuda, monkeypatch):
    calls = count_calls(monkeypatch)
    torch.manual_seed(0)
    on = ie.ResNet(depth=50, out_indices=(0, 2, 3), norm_eval=False, with_cp=True)
    gen = torch.Generator().manual_seed(1)
    for m in on.modules():                         # norms that are no identities
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.rand(m.num_features, generator=gen) - 0.5)
            m.running_var.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
    on = on.to(cuda)
    off = copy.deepcopy(on)                        # shared weights
    on.fused_tail, off.fused_tail = True, False
    x = torch.randn(2, 3, 64, 96, device=cuda)
    for m in (on, off):
        m.eval()
    with torch.no_grad():
        a, b = on(x), off(x)
    assert calls == ['tail'] * 16 and [tuple(o.shape) for o in a] == [(2, 256, 16, 24), (2, 1024, 4, 6), (2, 2048, 2, 3)]
    for i, (p, q) in enumerate(zip(a, b)):
        assert_close(p, q, f'eval out{i}')
    res = []
    for m in (on, off):
        m.train()
        xi = x.clone().requires_grad_(True)
        outs = m(xi)
        sum((o * o).mean() for o in outs).backward()
        res.append(([o.detach() for o in outs], xi.grad, {k: p.grad for k, p in m.named_parameters()}))
    assert len(calls) == 16 + 2 * 16               # every block once forward and once in the checkpoint's recomputation
    for i, (p, q) in enumerate(zip(res[0][0], res[1][0])):
        assert_close(p, q, f'train out{i}')
    assert_close(res[0][1], res[1][1], 'input gradient')
    assert set(res[0][2]) == set(res[1][2]) and all(g is not None for g in res[0][2].values())
    for k in res[0][2]:
        assert_close(res[0][2][k], res[1][2][k], f'gradient of {k}')


def test_custom_fpn_fused_merge_on_and_off(cuda, monkeypatch):
    calls = count_calls(monkeypatch)
    _, neck = fx.reference_dicts()
    torch.manual_seed(0)
    on = ie.CustomFPN(**{k: v for k, v in neck.items() if k != 'type'}).to(cuda)
    off = copy.deepcopy(on)
    on.fused_merge, off.fused_merge = True, False
    maps = [torch.randn(2, 1024, 4, 6, device=cuda), torch.randn(2, 2048, 2, 3, device=cuda)]
    res = []
    for m in (on, off):
        leaves = [t.clone().requires_grad_(True) for t in maps]
        out = m(leaves)
        (out * out).mean().backward()
        res.append([out.detach()] + [t.grad for t in leaves] + [p.grad for p in m.parameters()])
    assert calls == ['merge'] and res[0][0].shape == (2, 256, 4, 6)
    names = ['out', 'gx0', 'gx1'] + [k for k, _ in on.named_parameters()]
    for name, p, q in zip(names, res[0], res[1]):
        assert_close(p, q, name)


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('tag,mode', [(t, mode) for t, c in fx.CASES.items() for mode in c[2]])
def test_custom_fpn_matches_the_reference(cuda, monkeypatch, tag, mode, fused):
    calls = count_calls(monkeypatch)
    fx.check_case(tag, mode, cuda, fused=fused)
    assert calls == (['merge'] if fused else [])   # every case has two laterals: one top-down step


def test_image_encoder_of_the_reference_config(cuda):
    backbone, neck = fx.reference_dicts()
    torch.manual_seed(0)
    enc = ie.ImageEncoder(backbone, neck).to(cuda).train()
    enc.img_backbone.fused_tail = True
    enc.img_neck.fused_merge = True
    img = torch.randn(1, 2, 3, 64, 96, device=cuda)

    def step():
        enc.zero_grad(set_to_none=True)
        x, stereo_feat = enc(img, stereo=True)
        (x.sum() + stereo_feat.sum()).backward()
        return x, stereo_feat
    x, stereo_feat = step()                        # warm-up: library, code objects, the convolutions' algorithm search
    assert x.shape == (1, 2, 256, 4, 6) and stereo_feat.shape == (2, 256, 16, 24)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    grad = enc.img_backbone.conv1.weight.grad
    assert grad is not None and torch.isfinite(grad).all() and float(grad.abs().max()) > 0
    assert enc.img_neck.lateral_convs[1].conv.weight.grad is not None
    enc.eval()
    with torch.no_grad():
        assert_close(enc.extract_stereo_ref_feat(img), enc(img, stereo=True)[1], 'extract_stereo_ref_feat')
