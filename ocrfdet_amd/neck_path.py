"""The whole neck as one step on the synthetic rig (``bench.py --scope neck``)."""
import torch

from . import synthetic
from .hotpath_scene import bev_voxels


class NeckPath:
    """The whole neck as one step: pre-filter + ``OcRFViewTransformerFull.view_transform`` (both
    poolings, colour / alpha sampling, Gaussian heads, NeRF branch, one rendered view per sample, HOA,
    BEV fusion) with random-init weights of the reference architecture on the synthetic rig — what
    ``bench.py --scope neck`` and ``tools/time_neck.py`` drive.  Frames ride along as batch entries."""

    def __init__(self, cfg, device, accelerate=True, seed=0, parallel_branches=True, host_calibration=False):
        from . import neck_ops
        from . import view_transformer_ocrf as vto
        self.cfg, self.device, self._ops = cfg, torch.device(device), neck_ops
        self.batch = cfg.batch * cfg.n_frames
        X, Y, _ = cfg.bev_xyz
        torch.manual_seed(seed)
        self.module = vto.OcRFViewTransformerFull(
            pc_range=list(cfg.pc_range), bev_h=Y, bev_w=X, num_height=cfg.num_height, grid_config=cfg.grid,
            input_size=cfg.input_size, downsample=cfg.downsample, in_channels=256, out_channels=cfg.channels,
            accelerate=accelerate).to(self.device).eval()
        # strands on side streams pay off inside a captured graph (parallel branches, no host cost); issued
        # eagerly the extra stream / event calls cost more than the overlap returns (1.58 -> 1.81 ms)
        self._graph_parallel = parallel_branches
        self._capture_stream = None                              # the stream ``capture`` captures on (None: its own)
        self._graphed = None
        r = synthetic.rig(cfg.n_cams, cfg.input_size, self.batch)
        Hf, Wf = cfg.feat_hw
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(self.batch, cfg.n_cams, 256, Hf, Wf, generator=g)
        raw = torch.randint(0, 256, (self.batch, cfg.n_cams, 3, *cfg.input_size), generator=g).float()
        inp = [x] + [torch.from_numpy(r[k]) for k in ('rots', 'trans', 'intrins', 'post_rots', 'post_trans', 'bda')]
        inp += [torch.zeros(self.batch, cfg.n_cams, 27), raw, raw, raw, torch.from_numpy(r['c2w'])]
        # host_calibration: the six calibration tensors and c2w stay host tensors (what the dataloader produced);
        # the module then needs no device -> host read-back per forward (OcRFViewTransformerFull._to_host)
        keep = {1, 2, 3, 4, 5, 6, 11} if host_calibration else set()
        self.inputs = [t if i in keep else t.to(self.device) for i, t in enumerate(inp)]
        pre = torch.randn(self.batch * cfg.n_cams, cfg.D + 2 + cfg.channels, Hf, Wf, generator=g)
        pre[:, :cfg.D] *= 3                                       # stand-in for the DepthNet output
        self.depthnet_out = pre.to(self.device)

    @torch.no_grad()
    def step(self):
        m = self.module
        depth, fdepth, sem, feat_cl = self._ops.prefilter(self.depthnet_out, m.D, m.out_channels, m.depth_threshold,
                                                          m.semantic_threshold)
        return m.view_transform(self.inputs, fdepth, None, feat_cl)

    # ---- the same step as ONE hipGraph launch (cached geometry only) -------------------------------
    def capture(self, warmup=3):
        """Capture ``step`` into a hipGraph (view_transformer_ocrf.GraphedNeck).  The only per-step host
        decision — the random camera of each sample (view_transformer_ocrf.py:1081) — lives in two small
        static device tensors that ``step_graphed`` refreshes before every replay."""
        from .view_transformer_ocrf import GraphedNeck
        self._graphed = GraphedNeck(self.module, self.inputs, self.depthnet_out, warmup=warmup,
                                    parallel_branches=self._graph_parallel,
                                    capture_stream=self._capture_stream)
        return self

    def step_graphed(self, cam_idx_list=None):
        """-> (bev_feat, depth, bev_mask_logit, extras) like ``step`` (static tensors, overwritten by the next
        replay)."""
        bev, depth, (bev_mask, _sem), extras = self._graphed.replay(cam_idx_list)
        return bev, depth, bev_mask, extras

    @property
    def bev_voxels_per_step(self):
        return bev_voxels(self.cfg, self.batch)

    @property
    def views_per_step(self):
        return self.batch                                         # one random camera per sample (:1081)
