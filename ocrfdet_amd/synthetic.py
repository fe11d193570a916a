"""Synthetic nuScenes-like workload for tests, ``smoke()`` and ``bench.py``.

Everything is closed-form or drawn from a seeded ``numpy`` generator, so the same inputs can be
rebuilt bit-for-bit anywhere (the GPU box has no dataset and no reference tree).

Rig: 6 cameras at yaw [55, 0, -55, 110, 180, -110] deg, ``R_cam->ego = Rz(yaw) @ [[0,0,1],[-1,0,0],
[0,-1,0]]``, ``t = Rz @ (1.5,0,0) + (0,0,1.5)``; ``K = [[1266,0,816],[0,1266,491],[0,0,1]]`` for a
1600x900 sensor; image augmentation ``post_rot = diag(s,s,1)``, ``post_tran = (0,-crop_h,0)`` with
``s = W_in/1600`` and ``crop_h = int(900*s) - H_in``; ``bda = I``.  These are the 7 geometry tensors
of the reference's ``img_inputs`` tuple (mmdet3d/models/detectors/bevdet.py:412-476).
"""
import math
from dataclasses import dataclass, field

import numpy as np
import torch

YAWS_DEG = (55.0, 0.0, -55.0, 110.0, 180.0, -110.0)


@dataclass
class PathConfig:
    """Shapes of one configuration of the hot path (BASELINE.json ``configs``)."""
    name: str
    n_cams: int = 6
    n_frames: int = 1
    batch: int = 1
    input_size: tuple = (256, 704)          # (H_in, W_in)
    downsample: int = 16
    channels: int = 80
    grid: dict = field(default_factory=lambda: dict(
        x=[-51.2, 51.2, 0.8], y=[-51.2, 51.2, 0.8], z=[-5.0, 3.0, 8.0], depth=[1.0, 60.0, 0.5]))
    pc_range: tuple = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)
    num_height: int = 13
    render: bool = False
    hoa: bool = False

    @property
    def feat_hw(self):
        return self.input_size[0] // self.downsample, self.input_size[1] // self.downsample

    @property
    def D(self):
        d = self.grid['depth']
        return len(np.arange(d[0], d[1], d[2]))

    @property
    def bev_xyz(self):
        return tuple(int(round((self.grid[a][1] - self.grid[a][0]) / self.grid[a][2])) for a in 'xyz')


def _grid(lim, step, z):
    return dict(x=[-lim, lim, step], y=[-lim, lim, step], z=list(z), depth=[1.0, 60.0, 0.5])


CONFIGS = {
    # BASELINE.json configs[0]: plumbing case, CPU-runnable
    'cfg0_1cam_128x352_bev64x64x4': PathConfig(
        'cfg0_1cam_128x352_bev64x64x4', n_cams=1, input_size=(128, 352),
        grid=_grid(25.6, 0.8, (-5.0, 3.0, 2.0)), pc_range=(-25.6, -25.6, -5.0, 25.6, 25.6, 3.0)),
    # configs[1]
    'cfg1_6cam_256x704_bev128x128x8': PathConfig(
        'cfg1_6cam_256x704_bev128x128x8', grid=_grid(51.2, 0.8, (-5.0, 3.0, 1.0))),
    # the reference's own shape (configs/ocrfdet/ocrfdet.py:19-40): 128x128x1
    'ref_6cam_256x704_bev128x128x1': PathConfig('ref_6cam_256x704_bev128x128x1'),
    # configs[2]: the headline — 6 cams x 2 frames, 200x200 BEV (+-40 m @ 0.4 m), render + HOA
    'cfg2_6cam_2frame_bev200x200_render_hoa': PathConfig(
        'cfg2_6cam_2frame_bev200x200_render_hoa', n_frames=2,
        grid=_grid(40.0, 0.4, (-5.0, 3.0, 8.0)), pc_range=(-40.0, -40.0, -5.0, 40.0, 40.0, 3.0),
        render=True, hoa=True),
    # configs[4]: test-set shape
    'cfg4_6cam_8frame_512x1408_bev200x200': PathConfig(
        'cfg4_6cam_8frame_512x1408_bev200x200', n_frames=8, input_size=(512, 1408),
        grid=_grid(40.0, 0.4, (-5.0, 3.0, 8.0)), pc_range=(-40.0, -40.0, -5.0, 40.0, 40.0, 3.0),
        render=True, hoa=True),
}


def ego_motion(k):
    """4x4 transform of frame k's ego into the key frame's (k = 0: identity): an adjacent frame of a
    multi-frame sample was taken 4 m further back along the lane, 0.25 m to the side, yawed 1.5 degrees
    (mmdet3d/models/detectors/bevdet.py:437-455 composes sensor2keyego the same way)."""
    a = math.radians(1.5 * k)
    T = np.eye(4)
    T[:3, :3] = [[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = [-4.0 * k, 0.25 * k, 0.0]
    return T


def rig(n_cams=6, input_size=(256, 704), batch=1, dtype=np.float32, frame_motion=False, frame_offset=0):
    """-> dict of numpy arrays: rots (B,N,3,3), trans (B,N,3), intrins (B,N,3,3), post_rots
    (B,N,3,3), post_trans (B,N,3), bda (B,3,3), c2w (B,N,4,4).  ``frame_motion``: batch entry b is frame
    ``frame_offset + b`` of a multi-frame sample, its cameras expressed in the key frame's ego
    (``ego_motion``); default: every entry is the key frame's rig."""
    H_in, W_in = input_size
    base = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], dtype=np.float64)
    rots, trans, c2w = [], [], []
    for yaw in YAWS_DEG[:n_cams]:
        a = math.radians(yaw)
        Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
        R = Rz @ base
        t = Rz @ np.array([1.5, 0.0, 0.0]) + np.array([0.0, 0.0, 1.5])
        M = np.eye(4)
        M[:3, :3] = R
        M[:3, 3] = t
        rots.append(R), trans.append(t), c2w.append(M)
    K = np.array([[1266.0, 0, 816.0], [0, 1266.0, 491.0], [0, 0, 1.0]])
    s = W_in / 1600.0
    crop_h = int(900 * s) - H_in
    post_rot = np.diag([s, s, 1.0])
    post_tran = np.array([0.0, -float(crop_h), 0.0])
    rep = lambda a: np.broadcast_to(np.asarray(a, dtype=dtype), (batch,) + np.shape(a)).copy()  # noqa: E731
    N = n_cams
    out = dict(
        rots=rep(np.stack(rots)), trans=rep(np.stack(trans)), intrins=rep(np.stack([K] * N)),
        post_rots=rep(np.stack([post_rot] * N)), post_trans=rep(np.stack([post_tran] * N)),
        bda=rep(np.eye(3)), c2w=rep(np.stack(c2w)), resize=s, crop_h=crop_h)
    if frame_motion:
        for b in range(batch):
            T = ego_motion(frame_offset + b)
            for n in range(N):
                M = T @ c2w[n]
                out['rots'][b, n] = M[:3, :3].astype(dtype)
                out['trans'][b, n] = M[:3, 3].astype(dtype)
                out['c2w'][b, n] = M.astype(dtype)
    return out


def stereo_k2s(n_cams=6, batch=1, k=1, dtype=np.float32):
    """(batch, n_cams, 4, 4) ``k2s_sensor`` of the stereo cost volume: each key-frame camera's sensor frame into the
    same camera of adjacent frame k, whose ego pose is ``ego_motion(k)`` (bevdet.py:437-455 builds curr2adjsensor the
    same way: inv(adjacent sensor -> key ego) . key sensor -> key ego)."""
    r = rig(n_cams, batch=1, dtype=np.float64)
    T = ego_motion(k)
    out = [np.linalg.inv(T @ M) @ M for M in r['c2w'][0]]
    return np.broadcast_to(np.stack(out).astype(dtype), (batch, n_cams, 4, 4)).copy()


def rig_tensors(cfg, device='cpu'):
    r = rig(cfg.n_cams, cfg.input_size, cfg.batch)
    return {k: (torch.from_numpy(v).to(device) if isinstance(v, np.ndarray) else v) for k, v in r.items()}


def depth_and_feat(cfg, seed=0, device='cpu'):
    """Softmax depth over D bins with sub-threshold bins zeroed and masked image features, as
    ``OcRFViewTransformerFull.forward`` hands them to the pooling (view_transformer_ocrf.py:1327-1331).
    -> depth (B*N, D, H, W), feat (B*N, C, H, W) float32."""
    rng = np.random.default_rng(seed)
    H, W = cfg.feat_hw
    BN = cfg.batch * cfg.n_cams
    logits = rng.standard_normal((BN, cfg.D, H, W)).astype(np.float32)
    logits -= logits.max(1, keepdims=True)
    p = np.exp(logits)
    p /= p.sum(1, keepdims=True)
    p[p < np.float32(1.0 / cfg.D)] = 0
    feat = rng.standard_normal((BN, cfg.channels, H, W)).astype(np.float32)
    feat *= (rng.random((BN, 1, H, W)) < 0.5).astype(np.float32)
    return torch.from_numpy(p).to(device), torch.from_numpy(feat).to(device)


GAUSSIAN_SETS = ('init', 'stress', 'objects')


def grid_gaussians(kind, xyz, seed=0):
    """Parameters for Gaussians whose means are the fixed voxel grid ``xyz`` (P,3) numpy (the OcRF render's means,
    view_transformer_ocrf.py:651-673,690-692) -> dict of numpy float32 arrays ``scales`` (P,3), ``rotations`` (P,4),
    ``opacity`` (P,1), ``rgb`` (P,3).

    ``init``    what the reference's S/R/A/C heads give at seeded init (SURVEY §8d probe): scales U(0.69,0.84) m, opacity
                U(0.35,0.45) on EVERY voxel — each pixel saturates after ~80 records: the rasteriser's best case.
    ``stress``  SURVEY §8d's second set on the same means: scales U(0.2,1.0), opacity U(0.05,0.95), random unit quaternions.
    ``objects`` object-centric, what a trained ``A_MLP`` (sigmoid under a foreground-mask loss, :177-201,1130) gives:
                ~30 boxes of 4 x 2 x 1.5 m (random place / yaw, standing on the ground) whose voxels carry opacity
                U(0.6,0.95); every other voxel sigmoid(U(-7,-4)) — half of them under 1/255 (never blended), half faint
                above it.  Most pixels never saturate, so nothing ends a tile's list early."""
    assert kind in GAUSSIAN_SETS
    rng = np.random.default_rng(seed)
    P = int(xyz.shape[0])
    q = rng.standard_normal((P, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    if kind == 'init':
        # (draw order kept from rounds 1-5: the committed figures and tests were made with these values)
        scales = rng.uniform(0.69, 0.84, (P, 3)).astype(np.float32)
        opacity = rng.uniform(0.35, 0.45, (P, 1)).astype(np.float32)
        rgb = rng.uniform(0.0, 1.0, (P, 3)).astype(np.float32)
    elif kind == 'stress':
        scales = rng.uniform(0.2, 1.0, (P, 3)).astype(np.float32)
        opacity = rng.uniform(0.05, 0.95, (P, 1)).astype(np.float32)
        rgb = rng.uniform(0.0, 1.0, (P, 3)).astype(np.float32)
    else:
        scales = rng.uniform(0.69, 0.84, (P, 3)).astype(np.float32)
        rgb = rng.uniform(0.0, 1.0, (P, 3)).astype(np.float32)
        logit = rng.uniform(-7.0, -4.0, (P, 1))
        opacity = (1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
        lim = float(np.abs(xyz[:, :2]).max()) - 5.0
        inside = np.zeros(P, dtype=bool)
        for _ in range(30):
            c = np.array([rng.uniform(-lim, lim), rng.uniform(-lim, lim), rng.uniform(-1.6, -0.8)])
            yaw = rng.uniform(0.0, math.pi)
            d = xyz.astype(np.float64) - c
            u = d[:, 0] * math.cos(yaw) + d[:, 1] * math.sin(yaw)
            w = -d[:, 0] * math.sin(yaw) + d[:, 1] * math.cos(yaw)
            inside |= (np.abs(u) <= 2.0) & (np.abs(w) <= 1.0) & (np.abs(d[:, 2]) <= 0.75)
        n_in = int(inside.sum())
        opacity[inside] = rng.uniform(0.6, 0.95, (n_in, 1)).astype(np.float32)
    return dict(scales=scales, rotations=q, opacity=opacity, rgb=rgb)


def stress_gaussians(n, seed=0, extent=40.0, device='cpu'):
    """The 'stress' Gaussian set of SURVEY §8d: scales U(0.2,1.0), opacity U(0.05,0.95), random unit
    quaternions, RGB U(0,1), centres uniform in a +-extent box (z in [-4.5, 2.5])."""
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-extent, extent, n), rng.uniform(-extent, extent, n),
                    rng.uniform(-4.5, 2.5, n)], 1).astype(np.float32)
    scales = rng.uniform(0.2, 1.0, (n, 3)).astype(np.float32)
    q = rng.standard_normal((n, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    opacity = rng.uniform(0.05, 0.95, (n, 1)).astype(np.float32)
    rgb = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    return dict(xyz=t(xyz), scales=t(scales), rotations=t(q), opacity=t(opacity), rgb=t(rgb))


def nuscenes_boxes(batch=8, seed=0, n_range=(30, 40), n_out=4, pc_range=(-51.2, -51.2, -5.0, 51.2, 51.2, 3.0),
                   device='cpu'):
    """nuScenes-like gt for the detection head: per sample (boxes (n, 9) float32 as LiDARInstance3DBoxes.tensor --
    x, y, bottom z, dx, dy, dz, yaw, vx, vy -- and labels (n,) int64 over the ten classes), 30-40 boxes inside the
    range and ``n_out`` outside it.  Sizes follow the classes' typical dimensions."""
    # car, truck, construction_vehicle, bus, trailer, barrier, motorcycle, bicycle, pedestrian, traffic_cone
    dims = np.array([[1.9, 4.6, 1.7], [2.5, 6.9, 2.8], [2.8, 6.4, 3.2], [2.9, 11.0, 3.5], [2.9, 12.3, 3.9],
                     [2.5, 0.5, 1.0], [0.8, 2.1, 1.5], [0.6, 1.7, 1.3], [0.7, 0.7, 1.8], [0.4, 0.4, 1.1]], np.float32)
    freq = np.array([0.40, 0.07, 0.02, 0.02, 0.03, 0.13, 0.02, 0.02, 0.19, 0.10])
    rng = np.random.default_rng(seed)
    boxes, labels = [], []
    for _ in range(batch):
        n = int(rng.integers(n_range[0], n_range[1] + 1))
        lab = rng.choice(10, size=n + n_out, p=freq / freq.sum())
        xy = rng.uniform(pc_range[0] + 1, pc_range[3] - 1, (n + n_out, 2))
        xy[n:] = np.sign(rng.uniform(-1, 1, (n_out, 2))) * rng.uniform(pc_range[3] + 1, pc_range[3] + 10, (n_out, 2))
        d = dims[lab] * rng.uniform(0.85, 1.15, (n + n_out, 3))
        z = rng.uniform(-2.5, 0.5, (n + n_out, 1))
        yaw = rng.uniform(-np.pi, np.pi, (n + n_out, 1))
        vel = rng.normal(0, 2, (n + n_out, 2)) * (lab[:, None] < 8)
        b = np.concatenate([xy, z, d, yaw, vel], 1).astype(np.float32)
        boxes.append(torch.from_numpy(b).to(device))
        labels.append(torch.from_numpy(lab.astype(np.int64)).to(device))
    return boxes, labels
