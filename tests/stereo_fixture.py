"""Loading ``tests/golden/stereo.npz`` (see ``tests/golden/make_golden_stereo.py``) for the host and GPU tests of the
stereo DepthNet: the seeded state_dict, the inputs as stereo metas, and the ambiguity map of the reference's grid."""
import json
import os

import numpy as np
import torch

from ocrfdet_amd import depthnet, index_prep

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stereo.npz')
# a sample coordinate within this many feature pixels of a corner line may keep or drop that corner depending on the
# last bits of the 3x3 inverses (closed-form here, LAPACK in the reference): the == 0 bias test can flip there
AMBIGUOUS_PX = 1e-3


def load():
    z = np.load(PATH)
    meta = json.loads(str(z['meta']))
    g = {k: z[k] for k in z.files}
    g['meta'] = meta
    return g


def state_dict(g):
    return {k[3:]: torch.from_numpy(v.astype(np.float32) if v.dtype == np.float16 else v)
            for k, v in g.items() if k.startswith('sd.')}


def build(g, device='cpu'):
    m = g['meta']
    net = depthnet.DepthNet(m['IN'], m['MID'], m['CTX'], m['D'] + 2, use_dcn=False, stereo=True, bias=m['BIAS'],
                            aspp_mid_channels=m['ASPP_MID'])
    net.load_state_dict(state_dict(g), strict=True)
    return net.to(device)


def metas(g, device='cpu'):
    m = g['meta']
    t = lambda k: torch.from_numpy(g[k]).to(device)                 # noqa: E731
    prev, curr = (torch.from_numpy(g[k].astype(np.float32) / 16).to(device) for k in ('prev_q', 'curr_q'))
    return dict(k2s_sensor=t('k2s_sensor'), intrins=t('intrins'), post_rots=t('post_rots'), post_trans=t('post_trans'),
                frustum=index_prep.create_frustum(m['DEPTH'], tuple(m['INPUT']), 4).to(device), cv_downsample=4,
                downsample=16, grid_config=None, cv_feat_list=[prev, curr])


def near_lines(ix, iy, H, W, tol=AMBIGUOUS_PX):
    """Bool, the shape of ``ix``: sample positions in feature pixels (any shape, float64) that reach the map and lie
    within ``tol`` (a scalar or one value per sample) of a corner line, the map's border included."""
    ix, iy = torch.as_tensor(ix, dtype=torch.float64), torch.as_tensor(iy, dtype=torch.float64)
    tol = torch.as_tensor(tol, dtype=torch.float64)
    near = lambda a: (a - a.round()).abs() < tol                   # noqa: E731
    inside = (ix > -1 - tol) & (ix < W + tol) & (iy > -1 - tol) & (iy < H + tol)
    return (near(ix) | near(iy)) & inside


def ambiguity(grid, H, W, other=None, tol=AMBIGUOUS_PX):
    """(BN, D, H, W) bool: cells whose sample reaches the map and lies within ``tol`` feature pixels of a corner line
    (the map's border included), or whose behind-camera status differs between ``grid`` and ``other`` (same
    shape), if given."""
    grid = torch.as_tensor(grid, dtype=torch.float64)
    BN = grid.shape[0]
    ix = (grid[..., 0] + 1) / 2 * (W - 1)
    iy = (grid[..., 1] + 1) / 2 * (H - 1)
    amb = near_lines(ix, iy, H, W, tol) & (grid[..., 0] != -2)
    if other is not None:
        other = torch.as_tensor(other, dtype=torch.float64).reshape(grid.shape)
        amb |= (grid[..., 0] == -2) != (other[..., 0] == -2)
    return amb.reshape(BN, -1, H, W)
