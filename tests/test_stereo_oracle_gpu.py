"""GPU: ``ocrf_stereo_cost_volume`` (csrc/stereo.hip) against the float64 oracle of tests/stereo_oracle.py on its sweep
of cases (row blocks of 64 lanes full and partial, W = 2; depth counts around the 8-bin chunks and the 4 waves, D = 1;
channel counts 4 to 256 with partial groups; bias 0, 5, -3 and the channel the bias test reads; cells behind the
camera and near its z threshold; samples on lattice lines, across every border, under image augmentation; costs that
underflow the softmax; the detector's full size on sampled columns), in raw and softmax mode, with the bounds of
``stereo_oracle.check``; bit-identical reruns; and one camera's prev past 2^31 bytes, accepted up to 2^32 - 1 bytes and
refused beyond."""
import functools

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib, depthnet

from . import stereo_oracle as oracle

pytestmark = pytest.mark.gpu

RERUN = ['bn12_c64_w129_d33', 'w129_h3_c7_d33', 'full_size']


@functools.lru_cache(maxsize=None)
def case(name):
    return oracle.build(name)


@pytest.mark.parametrize('name', list(oracle.CASES))
def test_kernel_matches_oracle(cuda, name):
    c = case(name)
    metas = oracle.to_device(c.metas, cuda)
    raw = depthnet.stereo_cost_volume_hip(metas, c.bias, raw=True)
    soft = depthnet.stereo_cost_volume_hip(metas, c.bias)
    got = oracle.check(oracle.take(raw, c.res), oracle.take(soft, c.res), c.res)
    D = soft.shape[1]
    if D == 1:
        assert torch.equal(soft, torch.ones_like(soft))
    if name == 'all_off_map':                          # raw constant over D: exp(0) / D, exactly
        assert torch.equal(soft, torch.full_like(soft, float(np.float32(1.0) / np.float32(D))))
    print(f'{name}: ambiguous {c.amb_frac:.2e}, raw err / bound {got["raw"]:.2e} '
          f'(ambiguous cells {got["raw_amb"]:.2e}, {got["flips"]} bias flips), softmax {got["soft"]:.2e}')


@pytest.mark.parametrize('name', RERUN)
def test_kernel_reruns_bit_identical(cuda, name):
    metas = oracle.to_device(case(name).metas, cuda)
    for raw in (True, False):
        a = depthnet.stereo_cost_volume_hip(metas, case(name).bias, raw=raw)
        b = depthnet.stereo_cost_volume_hip(metas, case(name).bias, raw=raw)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# --------------------------------------------------------------------------------------------- 32-bit planes
def _prev_value(cam, c, y, x):
    r = (3 * y + 5 * x + 7 * c) % 17 - 10              # 0 at 11 of 17 points: the bias test fires inside the map
    return r * (r > 0)


def _curr_value(cam, c, y, x):
    return (2 * y + 3 * x + 11 * c) % 13


def test_planes_past_2_31_bytes(cuda):
    """prev and curr of 2^30 floats each.  Accepted: C = 256, 2047 x 2048 (C H W 4 = 2^32 - 2^21 bytes), channels from
    128 on at plane offsets past 2^31 bytes, checked on sampled columns against the oracle reading the same integer
    formula.  Refused: C = 256, 2048 x 2048 (2^32 bytes) on the same buffers, by the Python entry and by the C entry
    itself; both pointers cover the whole extent, so a broken guard shows as a wrong return value, not as a read out of
    bounds."""
    n = 1 << 30
    prev = torch.empty(n, device=cuda)
    curr = torch.empty(n, device=cuda)
    try:
        C, H, W, D = 256, 2047, 2048, 2
        assert C * H * W * 4 <= depthnet.PLANE_BYTES_MAX < C * 2048 * 2048 * 4
        P, Q = prev[:C * H * W].view(1, C, H, W), curr[:C * H * W].view(1, C, H, W)
        yy = torch.arange(H, device=cuda, dtype=torch.int32).view(H, 1)
        xx = torch.arange(W, device=cuda, dtype=torch.int32).view(1, W)
        for c in range(C):
            P[0, c] = _prev_value(0, c, yy, xx).float()
            Q[0, c] = _curr_value(0, c, yy, xx).float()
        cam = oracle.camera(H, W, rot=(0.3, 0.2, 0.0), t=(0.4, 0.05, 0.1))
        d = np.array([6.0, 11.0])
        u = np.linspace(0, 4 * W - 1, W).astype(np.float32)
        v = np.linspace(0, 4 * H - 1, H).astype(np.float32)
        fr = torch.stack(torch.broadcast_tensors(torch.from_numpy(u)[None, None, :], torch.from_numpy(v)[None, :, None],
                                                 torch.tensor(d, dtype=torch.float32)[:, None, None]), -1)
        t = lambda i: torch.from_numpy(np.ascontiguousarray(cam[i][None, None]))     # noqa: E731
        metas = dict(k2s_sensor=t(0), intrins=t(1), post_rots=t(2), post_trans=t(3), frustum=fr, cv_downsample=4,
                     downsample=16, grid_config=None, cv_feat_list=[P, Q])
        rng = np.random.default_rng(0)
        cols = (np.zeros(256, np.int64), rng.integers(100, H - 100, 256), rng.integers(200, W - 200, 256))
        feats = (oracle.FormulaFeatures(_prev_value, C, np.full(C, 6.0)),
                 oracle.FormulaFeatures(_curr_value, C, np.full(C, 12.0)))
        res = oracle.evaluate(metas, 5.0, cols, feats)
        assert (res.corners == 4).all() and res.amb.mean() < 0.1      # delta ~ 0.02 px at |ix| ~ 2000
        assert res.bias_zero.any() and not res.bias_zero.all()      # channel 252: plane offset 4.2e9 bytes
        dev_metas = dict(metas, frustum=fr.to(cuda), cv_feat_list=[P, Q],
                         **{k: metas[k].to(cuda) for k in ('k2s_sensor', 'intrins', 'post_rots', 'post_trans')})
        raw = depthnet.stereo_cost_volume_hip(dev_metas, 5.0, raw=True)
        soft = depthnet.stereo_cost_volume_hip(dev_metas, 5.0)
        got = oracle.check(oracle.take(raw, res), oracle.take(soft, res), res)
        print(f'2^32 - 2^21 bytes per camera: raw err / bound {got["raw"]:.2e} '
          f'(ambiguous cells {got["raw_amb"]:.2e}, {got["flips"]} bias flips), softmax {got["soft"]:.2e}')
        del raw, soft

        # refused: 2^32 bytes
        H = 2048
        P, Q = prev.view(1, C, H, W), curr.view(1, C, H, W)
        fr = fr[:, :1].expand(D, H, W, 3).to(cuda)
        big = dict(dev_metas, frustum=fr, cv_feat_list=[P, Q])
        with pytest.raises(ValueError, match='2\\^32'):
            depthnet.stereo_cost_volume_hip(big, 5.0, raw=True)
        out = torch.full((1, D, H, W), 7.0, device=cuda)
        cal = [dev_metas[k].reshape(1, -1).contiguous() for k in ('k2s_sensor', 'intrins', 'post_rots', 'post_trans')]
        fu, fv, fd = fr[0, 0, :, 0], fr[0, :, 0, 1], fr[:, 0, 0, 2]
        with pytest.raises(_lib.OcrfHipError, match='hipError_t 1$'):
            _lib.launch('ocrf_stereo_cost_volume', cuda, 1, C, H, W, D, P, Q, fu, fu.stride(0), fv, fv.stride(0),
                        fd, fd.stride(0), *cal, 5.0, 1, out)
        torch.cuda.synchronize()
        assert (out == 7.0).all()                          # nothing was launched
    finally:
        del prev, curr
        torch.cuda.empty_cache()
