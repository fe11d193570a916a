"""CPU: the host side of the opt-in bfloat16 stereo cost volume (csrc/stereo_bf16.hip, ``ocrfdet_amd/depthnet.py``): the
packed layout by torch ops against a plain loop, the two entry points in the header and the library, their refusals at
the C boundary (argument validation alone: the calls return before anything is launched), and the switches' defaults."""
import ctypes

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib, depthnet

from . import stereo_oracle as oracle

INVALID = 1                                       # hipErrorInvalidValue
P = ctypes.c_void_p(4096)                         # any non-null, 16-byte aligned value: never dereferenced
ODD = ctypes.c_void_p(4096 + 8)                   # 8-byte aligned only


@pytest.mark.parametrize('C', [4, 7, 8, 12, 20])
def test_pack_torch_matches_a_plain_loop(C):
    BN, H, W = 2, 3, 5
    x = (torch.arange(BN * C * H * W, dtype=torch.float32).view(BN, C, H, W) % 251 + 1).bfloat16()    # no zero inside
    got = depthnet.stereo_pack_bf16_torch(x)
    G = C // 4
    NB = (G + 1) // 2
    assert got.shape == (BN, NB, H, W, 8) and got.dtype == torch.bfloat16 and got.is_contiguous()
    assert NB == depthnet.packed_blocks(C)
    want = np.zeros((BN, NB, H, W, 8), np.int16)
    src = x.view(torch.int16).numpy()
    for n in range(BN):
        for b in range(NB):
            for k in range(8):
                if 8 * b + k < 4 * G:
                    want[n, b, :, :, k] = src[n, 8 * b + k]
    assert np.array_equal(got.view(torch.int16).numpy(), want)         # values, and +0 (all bits clear) in the padding
    assert (want != 0).sum() == BN * 4 * G * H * W


def test_header_declares_and_library_exports_the_entries():
    protos = _lib.prototypes()
    L = _lib.lib()
    pack, cv = protos['ocrf_stereo_pack_bf16'], protos['ocrf_stereo_cost_volume_bf16']
    c = ctypes
    assert pack == (c.c_int, [c.c_int] * 4 + [c.c_void_p] * 3)
    assert cv == protos['ocrf_stereo_cost_volume']                    # the float32 entry's arguments
    assert hasattr(L, 'ocrf_stereo_pack_bf16') and hasattr(L, 'ocrf_stereo_cost_volume_bf16')
    assert {'ocrf_stereo_pack_bf16', 'ocrf_stereo_cost_volume_bf16'} <= _lib._ENQUEUEING
    # appended at the end of the enum: the ids in front of them keep their values
    assert (_lib.K_STEREO_COST_VOLUME, _lib.K_BEV_ALIGN_BWD_BF16) == (90, 120)
    assert (_lib.K_STEREO_PACK_BF16, _lib.K_STEREO_COST_VOLUME_BF16) == (121, 122)
    assert L.ocrf_kernel_name(_lib.K_STEREO_PACK_BF16) == b'stereo_pack_bf16_kernel'
    assert L.ocrf_kernel_name(_lib.K_STEREO_COST_VOLUME_BF16) == b'stereo_cost_volume_bf16_kernel'


def _cv(BN, C, H, W, D, prev=P, curr=P, out=P, mode=0, fu=P):
    return _lib.lib().ocrf_stereo_cost_volume_bf16(BN, C, H, W, D, prev, curr, fu, 1, P, 1, P, 1, P, P, P, P, 5.0, mode,
                                                   out, None)


def _pack(BN, C, H, W, src=P, dst=P):
    return _lib.lib().ocrf_stereo_pack_bf16(BN, C, H, W, src, dst, None)


def test_entries_refuse_at_the_c_boundary():
    # dimensions
    assert _cv(1, 3, 4, 4, 2) == INVALID and _pack(1, 3, 4, 4) == INVALID                    # C = 3: no whole group
    assert _cv(1, 8, 1, 4, 2) == INVALID and _pack(1, 8, 1, 4) == INVALID
    assert _cv(1, 8, 4, 1, 2) == INVALID and _pack(1, 8, 4, 1) == INVALID
    assert _cv(0, 8, 4, 4, 2) == INVALID and _pack(0, 8, 4, 4) == INVALID
    assert _cv(1, 8, 4, 4, 0) == INVALID
    assert _cv(1, 8, 4, 4, 2, mode=2) == INVALID and _cv(1, 8, 4, 4, 2, mode=-1) == INVALID
    # pointers: null, and a packed pointer that is not 16-byte aligned
    assert _cv(1, 8, 4, 4, 2, prev=None) == INVALID and _cv(1, 8, 4, 4, 2, curr=None) == INVALID
    assert _cv(1, 8, 4, 4, 2, out=None) == INVALID and _cv(1, 8, 4, 4, 2, fu=None) == INVALID
    assert _pack(1, 8, 4, 4, src=None) == INVALID and _pack(1, 8, 4, 4, dst=None) == INVALID
    assert _cv(1, 8, 4, 4, 2, prev=ODD) == INVALID and _cv(1, 8, 4, 4, 2, curr=ODD) == INVALID
    assert _pack(1, 8, 4, 4, dst=ODD) == INVALID
    # NB H W 16 = 2^32 exactly: C = 256 is 32 blocks, 2048 x 4096 pixels of 16 bytes each
    assert 32 * 2048 * 4096 * 16 == 2 ** 32 == depthnet.PACKED_BYTES_MAX + 1
    assert _cv(1, 256, 2048, 4096, 1) == INVALID and _pack(1, 256, 2048, 4096) == INVALID
    assert _cv(1, 252, 2048, 4096, 1) == INVALID                                             # G = 63: still 32 blocks
    # D H W = 2^31 (the packed tensor is small: one block)
    assert _cv(1, 8, 2048, 2048, 512) == INVALID
    # 2^31 workgroups: 2^20 cameras x 2048 rows x one block of 64 w; 2^20 x 2^11 chunks of 256 pixels
    assert _cv(1 << 20, 8, 2048, 2, 1) == INVALID
    assert _pack(1 << 20, 8, 1024, 512) == INVALID


def test_python_limits_are_named():
    assert depthnet.PACKED_BYTES_MAX == 2 ** 32 - 1 and depthnet.PACK == 8
    assert [depthnet.packed_blocks(C) for C in (4, 7, 8, 12, 16, 20, 256)] == [1, 1, 1, 2, 2, 3, 32]


def test_keep_bf16_on_cpu_tensors_takes_the_torch_formulation(monkeypatch):
    rng = np.random.default_rng(0)
    BN, C, H, W, D = 2, 8, 3, 9, 5
    prev, curr = oracle.relu_features(rng, BN, C, H, W), oracle.relu_features(rng, BN, C, H, W)
    metas = oracle.make_metas(oracle.default_cameras(BN, H, W), prev, curr, np.geomspace(1.0, 40.0, D), H, W)
    calls = []
    real = depthnet.stereo_cost_volume_torch
    monkeypatch.setattr(depthnet, 'stereo_cost_volume_torch', lambda *a: calls.append(1) or real(*a))
    monkeypatch.setattr(depthnet, 'stereo_cost_volume_hip_bf16', lambda *a: pytest.fail('the bf16 kernel path was taken'))
    for feats in ([torch.from_numpy(prev), torch.from_numpy(curr)],
                  [torch.from_numpy(prev).bfloat16(), torch.from_numpy(curr).bfloat16()]):
        m = dict(metas, cv_feat_list=feats)
        for raw in (False, True):
            assert torch.equal(depthnet.stereo_cost_volume(m, 5.0, raw=raw, keep_bf16=True), real(m, 5.0, raw))
    assert len(calls) == 4


def test_the_switch_is_off_by_default():
    assert depthnet.DepthNet.fused_cost_volume_bf16 is False
    net = depthnet.DepthNet(16, 16, 8, 7, use_dcn=False, stereo=True, bias=5.0, aspp_mid_channels=8)
    assert net.fused_cost_volume_bf16 is False and net.fused_cost_volume is True
    assert 'fused_cost_volume_bf16' not in net.__dict__
