"""Generates ``tests/golden/stereo.npz``: the reference's own stereo ``DepthNet`` (view_transformer.py:464-626), run on
the CPU.

    python tests/golden/make_golden_stereo.py

Imports the reference's ``view_transformer`` behind the stubs of ``_ref_import.py`` (read-only tree, nothing copied).
``_ref_import.py`` stubs mmdet's ``BasicBlock`` as ``nn.Identity``; here ``vt.BasicBlock`` is patched with a
restatement of mmdet 2.x's ``BasicBlock`` (mmdet is not part of the reference tree), the same kind of restatement
``_ref_import.py`` makes for ``LearnedPositionalEncoding``.

Small case: ``DepthNet(32, 32, 16, D + 2, use_dcn=False, stereo=True, bias=5, aspp_mid_channels=8)``, input 64 x 176
(x at downsample 16: 4 x 11, stereo features at 4: 16 x 44), depth bins [1, 13, 1] (D = 12), B = 2, N = 3, the
synthetic rig with each camera's adjacent frame from ``synthetic.stereo_k2s``.  Stored:

* the seeded ``state_dict`` (floats rounded to float16 first, so float16 stores them exactly), x, mlp_input, the
  calibration and the stereo features (C = 18: the last two channels are ignored by the cost volume; ReLU of a k / 16
  grid, about half exact zeros, stored as int8 k);
* camera (1, 2) gets a k2s_sensor rotated 100 degrees about the camera's y axis, so that part of its cells fall behind
  the camera (the z < 1e-3 branch); camera (0, 1) a 6 m sideways translation, so samples leave the feature map;
* the cost volume (softmax) and its raw -(cost + bias [warp == 0]) (the reference's own call with softmax patched to
  the identity), and the reference's sample grid (for the ambiguity map of the tests);
* the eval forward with stereo metas, with ``cv_feat_list[0] = None`` (the zeros branch), and one train-mode forward
  (seed 7 before the call: ASPP's dropout draws from the global generator);
* the key names and shapes of the DepthNet at the reference config's sizes (256 / 256 / 80 / 120, aspp_mid 96).
"""
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from ocrfdet_amd import index_prep, synthetic  # noqa: E402

B, N, IN, MID, CTX, C_ST = 2, 3, 32, 32, 16, 18
INPUT = (64, 176)
DEPTH = [1.0, 13.0, 1.0]
BIAS, ASPP_MID = 5.0, 8


class BasicBlock(nn.Module):
    """mmdet 2.x BasicBlock (expansion 1, style pytorch, BN, no plugins)."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style='pytorch', with_cp=False,
                 conv_cfg=None, norm_cfg=None, dcn=None, plugins=None, init_cfg=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.add_module('bn1', nn.BatchNorm2d(planes))
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.add_module('bn2', nn.BatchNorm2d(planes))
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


def calibration():
    r = synthetic.rig(N, INPUT, batch=B)
    k2s = synthetic.stereo_k2s(N, batch=B).astype(np.float64)
    a = math.radians(100.0)
    Ry = np.array([[math.cos(a), 0, math.sin(a), 0], [0, 1, 0, 0], [-math.sin(a), 0, math.cos(a), 0], [0, 0, 0, 1]])
    k2s[1, 2] = Ry @ k2s[1, 2]
    k2s[0, 1, 0, 3] += 6.0
    # augmentation on one camera: a small in-plane rotation and shift of the image
    pr = r['post_rots'].astype(np.float64).copy()
    pt = r['post_trans'].astype(np.float64).copy()
    c, s = math.cos(0.05), math.sin(0.05)
    pr[0, 0, :2, :2] = pr[0, 0, :2, :2] @ np.array([[c, -s], [s, c]])
    pt[0, 0, :2] += [3.0, -2.0]
    f = lambda v: torch.from_numpy(np.asarray(v, np.float32))        # noqa: E731
    return dict(k2s_sensor=f(k2s), intrins=f(r['intrins']), post_rots=f(pr), post_trans=f(pt))


def quantise_state(model):
    sd = model.state_dict()
    for k, v in sd.items():
        if v.is_floating_point():
            v.copy_(v.half().float())
    return {k: v.clone() for k, v in sd.items()}          # a snapshot: the train-mode forward moves the BN statistics


def main(path=os.path.join(HERE, 'stereo.npz')):
    from _ref_import import install
    vt = install()[0]
    vt.BasicBlock = BasicBlock
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    D = torch.arange(*DEPTH).shape[0]
    net = vt.DepthNet(IN, MID, CTX, D + 2, use_dcn=False, stereo=True, bias=BIAS, aspp_mid_channels=ASPP_MID)
    # non-trivial BN statistics
    for m in net.modules():
        if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.uniform_(-0.2, 0.2)
    sd = quantise_state(net)

    h, w = INPUT[0] // 16, INPUT[1] // 16
    hs, ws = INPUT[0] // 4, INPUT[1] // 4
    x = torch.from_numpy((np.round(rng.standard_normal((B * N, IN, h, w)) * 16) / 16).astype(np.float32))
    mlp = torch.from_numpy((np.round(rng.standard_normal((B, N, 27)) * 16) / 16).astype(np.float32))
    q = lambda: np.clip(np.round(rng.standard_normal((B * N, C_ST, hs, ws)) * 24), 0, 127).astype(np.int8)  # noqa
    prev_q, curr_q = q(), q()
    prev, curr = (torch.from_numpy(v.astype(np.float32) / 16) for v in (prev_q, curr_q))
    cal = calibration()
    frustum = index_prep.create_frustum(DEPTH, INPUT, 4)
    metas = dict(cal, frustum=frustum, cv_downsample=4, downsample=16, grid_config=None, cv_feat_list=[prev, curr])

    net.eval()
    with torch.no_grad():
        cost = net.calculate_cost_volumn(metas)
        grid = net.gen_grid(metas, B, N, D, hs, ws, hs * 4, ws * 4)
        soft = torch.Tensor.softmax
        torch.Tensor.softmax = lambda self, dim=None: self
        try:
            raw = net.calculate_cost_volumn(metas)
        finally:
            torch.Tensor.softmax = soft
        out_eval = net(x, mlp, metas)
        out_none = net(x, mlp, dict(metas, cv_feat_list=[None, curr]))
    net.train()
    torch.manual_seed(7)
    with torch.no_grad():
        out_train = net(x, mlp, metas)

    full = vt.DepthNet(256, 256, 80, 120, use_dcn=False, stereo=True, bias=BIAS, aspp_mid_channels=96)
    full_keys = {k: list(v.shape) for k, v in full.state_dict().items()}

    out = {'meta': np.array(json.dumps(dict(B=B, N=N, IN=IN, MID=MID, CTX=CTX, D=D, INPUT=INPUT, DEPTH=DEPTH, BIAS=BIAS,
                                            ASPP_MID=ASPP_MID, full_keys=full_keys,
                                            small_keys={k: list(v.shape) for k, v in sd.items()})))}
    for k, v in sd.items():
        out['sd.' + k] = v.numpy().astype(np.float16) if v.is_floating_point() else v.numpy()
    out.update(x=x.numpy(), mlp_input=mlp.numpy(), prev_q=prev_q, curr_q=curr_q,
               **{k: v.numpy() for k, v in cal.items()}, cost_volume=cost.numpy(), cost_raw=raw.numpy(),
               grid=grid.numpy(), out_eval=out_eval.numpy(), out_none=out_none.numpy(), out_train=out_train.numpy())
    np.savez_compressed(path, **out)
    neg = (grid[..., 0] == -2).float().mean().item()
    outside = ((grid.abs() > 1).any(-1)).float().mean().item()
    print(f'wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB): behind {neg:.3f}, outside {outside:.3f}, '
          f'zero-prev fraction {(prev == 0).float().mean().item():.2f}')


if __name__ == '__main__':
    main()
