"""GPU: the opt-in bfloat16 stereo cost volume, ``ocrf_stereo_pack_bf16`` + ``ocrf_stereo_cost_volume_bf16``
(csrc/stereo_bf16.hip).

* The pack kernel against ``stereo_pack_bf16_torch``, bit for bit, into a destination pre-filled with NaN bits.
* On every case of ``tests/stereo_oracle.CASES`` and on C = 4 ... 36 at W = 65 (blocks of 8 channels whole, half and
  with a partial group behind them), the features rounded to bfloat16: raw and softmax equal, as int32 bits,
  ``stereo_cost_volume_hip`` on the same features widened with ``.float()`` (that kernel is held to the float64 oracle by
  tests/test_stereo_oracle_gpu.py), and, independently, lie within ``stereo_oracle.check``'s bounds of the float64 oracle
  evaluated on the rounded features.  Rounding the features moves no sample position, so each case's ambiguous cells are
  the ones the existing test accepts.
* The upper half of the last block of an odd group count is never read into the result; reruns are bit-identical; a
  refused call writes nothing; a ``DepthNet`` with the switch on gives the bits of the same net with it off, by the new
  launches and without host synchronisation.

Refusals whose guard, if broken, would let a kernel read through a null pointer are checked at the C boundary on the
host only (tests/test_stereo_bf16_host.py)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib, depthnet

from . import stereo_fixture as sf
from . import stereo_oracle as oracle
from .test_stereo_oracle_gpu import RERUN

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
EXTRA_C = [4, 7, 8, 12, 16, 20, 36]
EXTRA = {f'extra_c{C}': C for C in EXTRA_C}
NAMES = list(oracle.CASES) + list(EXTRA)
ODD_G = ['w2_h2_c4_d7_behind', 'w65_c4_d1', 'w128_h3_c5_d32', 'bias_channel_zero', 'extra_c4', 'extra_c7', 'extra_c12',
         'extra_c20', 'extra_c36']


def bits(t):
    return t.contiguous().view(torch.int32)


def _round(t):
    return t.to(BF16)


@functools.lru_cache(maxsize=None)
def case(name):
    """namespace(metas: CPU metas with bfloat16 features, bias, res: the float64 oracle on those features)."""
    if name in EXTRA:
        BN, C, H, W, D, bias = 2, EXTRA[name], 3, 65, 9, 5.0
        rng = np.random.default_rng(100 + C)
        prev, curr = oracle.relu_features(rng, BN, C, H, W), oracle.relu_features(rng, BN, C, H, W)
        metas = oracle.make_metas(oracle.default_cameras(BN, H, W), prev, curr, np.geomspace(1.0, 40.0, D), H, W)
        base, cols = None, None
    else:
        base = oracle.build(name)
        metas, bias, cols = base.metas, base.bias, base.cols
    feats = [_round(f) for f in metas['cv_feat_list']]
    wide = [f.float() for f in feats]
    if base is not None and all(torch.equal(w, f) for w, f in zip(wide, metas['cv_feat_list'])):
        res = base.res                                 # the features are bfloat16 values already: the oracle's case as is
    else:
        res = oracle.evaluate(dict(metas, cv_feat_list=wide), bias, cols)
    assert not res.amb_z_in_map.any()
    if base is not None:                               # no sample position moved
        assert np.array_equal(res.amb, base.res.amb) and np.array_equal(res.ix, base.res.ix, equal_nan=True)
    else:
        assert res.amb.mean() <= 0.02
    return SimpleNamespace(metas=dict(metas, cv_feat_list=feats), bias=bias, res=res)


def _widened(metas):
    return dict(metas, cv_feat_list=[f.float() for f in metas['cv_feat_list']])


# --------------------------------------------------------------------------------------------- the pack kernel
@pytest.mark.parametrize('W', [2, 65, 129])
@pytest.mark.parametrize('C', [4, 7, 8, 12, 16, 20])
def test_pack_kernel_matches_torch(cuda, C, W):
    BN, H = 2, 3
    gen = torch.Generator(device='cpu').manual_seed(C * 1000 + W)
    x = torch.randn(BN, C, H, W, generator=gen).to(BF16).to(cuda)
    x[0, 0, 0, 0], x[1, C - 1, H - 1, W - 1] = -0.0, float('inf')
    want = depthnet.stereo_pack_bf16_torch(x)
    NB = depthnet.packed_blocks(C)
    dst = torch.full((BN, NB, H, W, 8), 0x7FC0, dtype=torch.int16, device=cuda)          # NaN bits everywhere
    _lib.launch('ocrf_stereo_pack_bf16', cuda, BN, C, H, W, x, dst)
    assert torch.equal(dst, want.view(torch.int16))
    got = depthnet.stereo_pack_bf16(x)
    assert got.dtype == BF16 and got.shape == want.shape and torch.equal(got.view(torch.int16), want.view(torch.int16))
    # the CPU formulation gives the same layout
    assert torch.equal(depthnet.stereo_pack_bf16_torch(x.cpu()).view(torch.int16), want.cpu().view(torch.int16))


# --------------------------------------------------------------------------------------------- the cost volume
@pytest.mark.parametrize('name', NAMES)
def test_matches_the_float32_kernel_and_the_oracle(cuda, name):
    c = case(name)
    metas = oracle.to_device(c.metas, cuda)
    wide = _widened(metas)
    out = {}
    for raw in (True, False):
        got = depthnet.stereo_cost_volume_hip_bf16(metas, c.bias, raw=raw)
        want = depthnet.stereo_cost_volume_hip(wide, c.bias, raw=raw)
        assert got.dtype == torch.float32 and got.shape == want.shape
        differ = int((bits(got) != bits(want)).sum())
        print(f'{name} {"raw" if raw else "softmax"}: {differ} of {got.numel()} cells differ in bits; '
              f'max |diff| {(got - want).abs().max().item():.3e}')
        assert differ == 0
        # the public dispatch takes the same path
        assert torch.equal(bits(depthnet.stereo_cost_volume(metas, c.bias, raw=raw, keep_bf16=True)), bits(got))
        out[raw] = got
    got = oracle.check(oracle.take(out[True], c.res), oracle.take(out[False], c.res), c.res)
    print(f'{name}: raw err / bound {got["raw"]:.2e} (ambiguous cells {got["raw_amb"]:.2e}, {got["flips"]} bias flips), '
          f'softmax {got["soft"]:.2e}')


def _launch_packed(metas, prev, curr, C, bias, raw, out=None, over=()):
    """``ocrf_stereo_cost_volume_bf16`` on packed features, as ``stereo_cost_volume_hip_bf16`` calls it; ``over``
    replaces arguments of the C entry by name."""
    dev = prev.device
    D, H, W, _ = metas['frustum'].shape
    BN = metas['post_trans'].shape[0] * metas['post_trans'].shape[1]
    cal = [metas[k].to(dev, torch.float32).reshape(BN, -1).contiguous()
           for k in ('k2s_sensor', 'intrins', 'post_rots', 'post_trans')]
    fr = metas['frustum'].to(dev, torch.float32)
    u, v, d = fr[0, 0, :, 0], fr[0, :, 0, 1], fr[:, 0, 0, 2]
    if out is None:
        out = torch.empty(BN, D, H, W, device=dev)
    a = dict(BN=BN, C=C, H=H, W=W, D=D, prev=prev, curr=curr, mode=1 if raw else 0)
    assert set(over) <= set(a)
    a.update(over)
    _lib.launch('ocrf_stereo_cost_volume_bf16', dev, a['BN'], a['C'], a['H'], a['W'], a['D'], a['prev'], a['curr'],
                u, u.stride(0), v, v.stride(0), d, d.stride(0), *cal, float(bias), a['mode'], out)
    return out


@pytest.mark.parametrize('name', ODD_G)
def test_padding_half_is_never_added(cuda, name):
    c = case(name)
    metas = oracle.to_device(c.metas, cuda)
    prev, curr = (f.reshape(-1, *f.shape[-3:]) for f in metas['cv_feat_list'])
    C = curr.shape[1]
    assert (C // 4) % 2 == 1
    p, q = depthnet.stereo_pack_bf16(prev), depthnet.stereo_pack_bf16(curr)
    assert not p[:, -1, :, :, 4:].view(torch.int16).any() and not q[:, -1, :, :, 4:].view(torch.int16).any()
    pn, qn = p.clone(), q.clone()
    pn[:, -1, :, :, 4:] = float('nan')
    qn[:, -1, :, :, 4:] = float('nan')
    for raw in (True, False):
        want = _launch_packed(metas, p, q, C, c.bias, raw)
        assert torch.equal(bits(want), bits(depthnet.stereo_cost_volume_hip_bf16(metas, c.bias, raw=raw)))
        assert torch.equal(bits(_launch_packed(metas, pn, qn, C, c.bias, raw)), bits(want))


@pytest.mark.parametrize('name', RERUN)
def test_reruns_bit_identical(cuda, name):
    c = case(name)
    metas = oracle.to_device(c.metas, cuda)
    for raw in (True, False):
        a = depthnet.stereo_cost_volume_hip_bf16(metas, c.bias, raw=raw)
        b = depthnet.stereo_cost_volume_hip_bf16(metas, c.bias, raw=raw)
        assert torch.equal(bits(a), bits(b))


# --------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(cuda):
    c = case('extra_c8')
    metas = oracle.to_device(c.metas, cuda)
    prev, curr = (f.reshape(-1, *f.shape[-3:]) for f in metas['cv_feat_list'])
    BN, C, H, W = curr.shape
    D = metas['frustum'].shape[0]
    # packed features with 16 bytes of slack behind them, so that a view 8 bytes in is still inside the allocation
    n = BN * H * W * 8
    store = [torch.zeros(n + 8, dtype=BF16, device=cuda) for _ in range(2)]
    for s, f in zip(store, (prev, curr)):
        s[:n] = depthnet.stereo_pack_bf16(f).flatten()
    p, q = store[0][:n], store[1][:n]
    out = torch.full((BN, D, H, W), 7.0, device=cuda)
    _launch_packed(metas, p, q, C, 5.0, True, out=out)                     # the arguments are good ones
    assert torch.equal(bits(out), bits(depthnet.stereo_cost_volume_hip_bf16(metas, 5.0, raw=True)))
    out.fill_(7.0)
    refused = [dict(C=3), dict(H=1), dict(W=1), dict(D=0), dict(BN=0), dict(mode=2), dict(mode=-1),
               dict(prev=store[0][4:n + 4]), dict(curr=store[1][4:n + 4]),   # 8 bytes off a 16-byte boundary
               # 2^31 workgroups (2^20 cameras x 2048 rows x one block of 64 w): a launch of that many is impossible
               dict(BN=1 << 20, H=2048, W=2, D=1)]
    for over in refused:
        with pytest.raises(_lib.OcrfHipError, match='hipError_t 1$'):
            _launch_packed(metas, p, q, C, 5.0, True, out=out, over=over)
    dst = torch.full((n,), 0x7FC0, dtype=torch.int16, device=cuda)
    for over in (dict(C=3), dict(H=1), dict(W=1), dict(BN=0), dict(dst=dst[4:]), dict(BN=1 << 20, H=1024, W=512)):
        a = dict(BN=BN, C=C, H=H, W=W, dst=dst)
        a.update(over)
        with pytest.raises(_lib.OcrfHipError, match='hipError_t 1$'):
            _lib.launch('ocrf_stereo_pack_bf16', cuda, a['BN'], a['C'], a['H'], a['W'], prev, a['dst'])
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (dst == 0x7FC0).all()
    # the Python entries refuse before they allocate
    with pytest.raises(ValueError, match='channel count'):
        depthnet.stereo_cost_volume_hip_bf16(dict(metas, cv_feat_list=[prev[:, :3], curr[:, :3]]), 5.0)
    with pytest.raises(ValueError, match='bfloat16'):
        depthnet.stereo_cost_volume_hip_bf16(_widened(metas), 5.0)


def test_sizes_past_the_limits_are_refused(cuda):
    """One camera's packed tensor of 2^32 bytes (C = 256: 32 blocks of 2048 x 4096 pixels), and D H W = 2^31, by the
    Python entry and by the C entry itself.  The buffers cover the whole extents, so a broken guard would show as a wrong
    return value, not as an access out of bounds."""
    feat = torch.empty(1 << 31, dtype=BF16, device=cuda)                   # 2^32 bytes; read-only: both features
    try:
        cam = oracle.camera(2048, 4096)
        t = lambda i: torch.from_numpy(np.ascontiguousarray(cam[i][None, None])).to(cuda)     # noqa: E731
        cal = dict(k2s_sensor=t(0), intrins=t(1), post_rots=t(2), post_trans=t(3))
        for C, H, W, D in ((256, 2048, 4096, 1), (8, 2048, 2048, 512)):
            assert depthnet.packed_blocks(C) * H * W * 16 > depthnet.PACKED_BYTES_MAX or D * H * W >= 2 ** 31
            fr = torch.zeros(D, 1, 1, 3, device=cuda).expand(D, H, W, 3)
            f = feat[:C * H * W].view(1, 1, C, H, W)
            metas = dict(cal, frustum=fr, cv_feat_list=[f[0], f[0]])
            with pytest.raises(ValueError, match='2\\^32' if D == 1 else '2\\^31'):
                depthnet.stereo_cost_volume_hip_bf16(metas, 5.0, raw=True)
            out = torch.full((1, D, H, W), 7.0, device=cuda)
            with pytest.raises(_lib.OcrfHipError, match='hipError_t 1$'):
                _launch_packed(metas, feat, feat, C, 5.0, True, out=out)
            if D == 1:
                with pytest.raises(ValueError, match='2\\^32'):
                    depthnet.stereo_pack_bf16(f[0])
                with pytest.raises(_lib.OcrfHipError, match='hipError_t 1$'):
                    _lib.launch('ocrf_stereo_pack_bf16', cuda, 1, C, H, W, feat, feat)
            torch.cuda.synchronize()
            assert (out == 7.0).all()
            del out
    finally:
        del feat
        torch.cuda.empty_cache()


# --------------------------------------------------------------------------------------------- DepthNet
def test_depthnet_switch_gives_the_same_bits_by_the_new_launches(cuda, monkeypatch):
    """The convolutions run without the convolution library: it may choose another algorithm from one call to the next,
    and bits are compared."""
    g = sf.load()
    net = sf.build(g, cuda).eval()
    metas = sf.metas(g, cuda)
    metas = dict(metas, cv_feat_list=[f.to(BF16) for f in metas['cv_feat_list']])
    x, mlp = torch.from_numpy(g['x']).to(cuda), torch.from_numpy(g['mlp_input']).to(cuda)
    names = []
    real = _lib.launch
    monkeypatch.setattr(_lib, 'launch', lambda name, *a, **k: names.append(name) or real(name, *a, **k))

    def run(flag):
        net.fused_cost_volume_bf16 = flag
        del names[:]
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            out = net(x, mlp, metas)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        return out, [n for n in names if 'stereo' in n]
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False), torch.autocast('cuda', dtype=BF16):
        for flag in (False, True):                     # warm-up outside the synchronisation check
            net.fused_cost_volume_bf16 = flag
            net(x, mlp, metas)
        want, default = run(False)
        got, opted = run(True)
        again, _ = run(False)
    assert default == ['ocrf_stereo_cost_volume']
    assert opted == ['ocrf_stereo_pack_bf16', 'ocrf_stereo_pack_bf16', 'ocrf_stereo_cost_volume_bf16']
    assert want.dtype == got.dtype and torch.isfinite(got.float()).all()
    as_int = {2: torch.int16, 4: torch.int32}[want.element_size()]
    assert torch.equal(again.view(as_int), want.view(as_int)), 'the default path differs from run to run'
    assert torch.equal(got.view(as_int), want.view(as_int))
