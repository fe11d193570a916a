"""The synthetic scene ``HotPath`` runs on: render cameras in both conventions, Gaussian store, HOA modules + inputs."""
import math

import numpy as np
import torch

from . import gaussian_renderer, hoa, synthetic
from .diff_gaussian_rasterization import pack_cameras

GAUSS_KEYS = ('rgb', 'opacity', 'scales', 'rotations')


def synthetic_inputs(cfg, n_frames, seed=0):
    """Host tensors depth (F, N, D, Hf, Wf) and feat (F, N, Hf, Wf, C) (channels-last view) of ``n_frames`` frames."""
    depth, feat = synthetic.depth_and_feat(synthetic.PathConfig(**{**cfg.__dict__, 'batch': n_frames}), seed)
    Hf, Wf = cfg.feat_hw
    return (depth.view(n_frames, cfg.n_cams, cfg.D, Hf, Wf),
            feat.view(n_frames, cfg.n_cams, cfg.channels, Hf, Wf).permute(0, 1, 3, 4, 2))


def bev_voxels(cfg, n_frames):
    X, Y, Z = cfg.bev_xyz
    return n_frames * Z * Y * X


def frames_of(out, n_cams, n_frames):
    """A batch render's output dict cut into one dict per frame (``n_cams`` views each; ``status`` is shared)."""
    return [{k: (v[i * n_cams:(i + 1) * n_cams] if k != 'status' else v) for k, v in out.items()} for i in range(n_frames)]


def consumed_on(frames, stream):
    """Rendered frames, allocated while a render stream was current, are read on ``stream``: the caching allocator
    must not hand their blocks to the next render-stream call meanwhile."""
    for frame in frames:
        for v in frame.values():
            if torch.is_tensor(v):
                v.record_stream(stream)


def render_cameras(r, cams, batch, input_size, device, convention='corrected'):
    """Per frame the cameras ``cams`` of rig ``r`` for the OcRF render: dict of ``vm``, ``pm`` (V, 4, 4),
    ``tfx``, ``tfy`` and ``packed``, the C ABI's camera block (the rig is fixed: packed once, not on every render call).

    convention 'reference': the reference's own set-up, quirks included (view_transformer_ocrf.py:1135-1152: unscaled
    1600x900 intrinsics with the network-input viewport, c2w fed as world->view); 'corrected': intrinsics scaled/cropped
    to the network input and a proper world->view transform (the headline of SURVEY.md 8d)."""
    H, W = input_size
    frames = []
    for b in range(batch):
        vms, pms, tfx, tfy = [], [], [], []
        for n in cams:
            K = r['intrins'][b, n].astype(np.float64)
            c2w = r['c2w'][b, n].astype(np.float64)
            if convention == 'corrected':
                s, crop = r['resize'], r['crop_h']
                K = np.array([[K[0, 0] * s, 0, K[0, 2] * s], [0, K[1, 1] * s, K[1, 2] * s - crop], [0, 0, 1.0]])
                w2c = np.linalg.inv(c2w)
                c2w_arg = np.eye(4)
                c2w_arg[:3, :3] = c2w[:3, :3]          # getWorld2View2 transposes R itself
                c2w_arg[:3, 3] = w2c[:3, 3]
            else:
                c2w_arg = c2w
            cam = gaussian_renderer.camera_from_calibration(K.astype(np.float32), c2w_arg.astype(np.float32), H, W)
            vms.append(cam['world_view_transform']), pms.append(cam['full_proj_transform'])
            tfx.append(math.tan(float(cam['FovX']) * 0.5)), tfy.append(math.tan(float(cam['FovY']) * 0.5))
        rc = dict(vm=torch.stack(vms).to(device), pm=torch.stack(pms).to(device), tfx=tfx, tfy=tfy)
        rc['packed'] = pack_cameras(rc['vm'], rc['pm'], tfx, tfy, H, W, device)
        frames.append(rc)
    return frames


class GaussianStore:
    """The Gaussian parameters of every frame, once: per phase ``stacks[phase][k]`` is ``(batch, P, width of k)``,
    contiguous, for k in ``GAUSS_KEYS``; everything else is a view of it, so an in-place edit through any of them reaches
    every consumer.  ``frames[phase][b][k]`` is ``stacks[phase][k][b]``, a plan's parameters are a slice of frames, the
    per-call set is the stack itself and ``opac_flat[phase]`` is the opacity as the ``(batch * P, 1)`` column HOA-1 reads
    (P = Zh*Y*X: the memory order A_MLP hands over, view_transformer_ocrf.py:1130).

    The kernels read all four arrays with scalar loads (``rasterize.hip``, ``raster_plan.hip``: ``scales[3 * gi]``,
    ``rotations[4 * gi]``, ``opacities[gi]``; ``hoa.hip`` reads the opacity column element-wise), so a frame's view needs
    the 4-byte alignment every float32 view has; at cfg2 (P = 520 000) its offset is a multiple of 16 bytes besides."""

    def __init__(self, kind, voxel_xyz, n_sets, seeds, device):
        """``voxel_xyz``: (batch, Zh, Y*X, 3), the means; ``seeds[b]``: the seed of frame b's draw
        (``synthetic.grid_gaussians``: ranges of the reference's heads at seeded init, SURVEY.md 8d probe)."""
        means = [xyz.reshape(-1, 3).cpu().numpy() for xyz in voxel_xyz]
        self.stacks = []
        for ph in range(n_sets):
            drawn = [synthetic.grid_gaussians(kind, xyz, seed + 1000 * ph) for xyz, seed in zip(means, seeds)]
            self.stacks.append({k: torch.from_numpy(np.stack([d[k] for d in drawn])).to(device) for k in GAUSS_KEYS})
        self.frames = [[{k: st[k][b] for k in GAUSS_KEYS} for b in range(len(means))] for st in self.stacks]
        self.opac_flat = [st['opacity'].reshape(-1, 1) for st in self.stacks]

    def frames_slice(self, f0, nf):
        """[phase] -> the stacked parameters of frames ``f0 .. f0 + nf`` (views)."""
        return [{k: st[k][f0:f0 + nf] for k in GAUSS_KEYS} for st in self.stacks]


def hoa_scene(cfg, batch, device, seed=0):
    """HOA blocks with seeded random-init weights of the reference architecture (view_transformer_ocrf.py:590-648) and
    the synthetic NeRF-branch inputs they consume -> (modules, alpha volume (B, Zh, Y, X), positional BEV (B, 4, Y, X))."""
    X, Y, _ = cfg.bev_xyz
    torch.manual_seed(seed)
    mods = dict(
        dca=hoa.DeformableAttention2D(dim=cfg.num_height, dim_head=8, heads=1, dropout=0.1, downsample_factor=4,
                                      offset_scale=4, offset_groups=None, offset_kernel_size=6),
        v2b=hoa.OpacityVoxelToBEVConverter(input_channel=cfg.num_height), mask=hoa.ObatinOpacityMask())
    for m in mods.values():
        m.to(device).eval()
    g = torch.Generator(device='cpu').manual_seed(seed)
    alpha_lidar = torch.rand(batch, cfg.num_height, Y, X, generator=g).to(device)
    return mods, alpha_lidar, (torch.randn(batch, 4, Y, X, generator=g) * 0.1).to(device)
