"""The hot path as one object: cached index preparation + LSS pool + HT pool (+ render + HOA).

This is the build's analogue of ``OcRFViewTransformerFull.view_transform_core``
(mmdet3d/models/necks/view_transformer_ocrf.py:1040-1201) restricted to the custom-kernel stages,
with the rank vectors pre-computed once per calibration as the reference's ``accelerate=True``
path intends (``pre_compute``, view_transformer_ocrf.py:854-866).  ``bench.py``,
``__graft_entry__.smoke()`` and the sharded runner drive it; frames are treated as extra batch
entries because they are independent until the channel concat (detectors/ocrfdet.py:274).  Its synthetic scene is
``hotpath_scene``; ``sharded_hotpath.ShardedHotPath`` and ``neck_path.NeckPath`` are still handed out from here.
"""
import contextlib

import torch

from . import _lib, bevpool, hoa, hotpath_scene, index_prep, raster_plan, synthetic
from .diff_gaussian_rasterization import rasterize_sets, rasterize_views
from .hotpath_scene import bev_voxels, consumed_on, frames_of


PoolPlan = bevpool.PoolPlan


_STREAMS = {}


def shared_stream(device, role):
    """One side HIP stream per (device, role) for the whole process: every HotPath reuses the same streams ('render',
    'render1', ..., 'prep', 'prep2') instead of creating its own — the streams of a process share a few hardware queues
    in creation order, and which queue a stream lands on decides whether it really runs beside the main stream."""
    key = (torch.device(device).index or 0, role)
    if key not in _STREAMS:
        _STREAMS[key] = torch.cuda.Stream(device)
    return _STREAMS[key]


def blend_workgroups_for(setting, f0, pixels_per_view, n_cu, beside):
    """Size of the planned blend's persistent grid for the plan whose first frame is ``f0`` (0 = what the device holds).
    ``setting``: an int, a sequence with one entry per frame, or 'auto': while another chain runs ``beside`` the blend it
    keeps to 11/4 workgroups per CU, 13/4 from 512 x 1024 pixels per view on, and takes the whole chip when nothing does
    (the sweeps behind both figures: DESIGN 4.6b)."""
    if setting == 'auto':
        return (13 if pixels_per_view >= 512 * 1024 else 11) * n_cu // 4 if beside else 0
    return setting if isinstance(setting, int) else int(setting[min(f0, len(setting) - 1)])


def _on(streams, i):
    return torch.cuda.stream(streams[i]) if streams is not None else contextlib.nullcontext()


class HotPath:
    def __init__(self, cfg, device, cams=None, index_prep_mode='cached', overlap=True, device_geometry=False,
                 render_mode='planned', render_guard='host', frame_motion=True, frame_offset=0, plan_margin=1.25,
                 ht_pool_backend=None, fuse_frames='auto', render_streams=1, blend_workgroups='auto',
                 lss_pool_backend=None, lss_mfma_group=2, plan_rebuild='never', hoa_first=None, one_call=True,
                 gaussians='init', alternate=None, fuse_hoa_stats=True, yield_word=None):
        """``cams``: optional list of camera indices this instance owns (camera sharding).
        ``index_prep_mode``: 'cached' — rank vectors computed once per calibration, the reference's
        ``accelerate=True`` intent; 'per_step' — recomputed inside every ``step()`` by the HIP index
        preparation (csrc/index_prep.hip), what the reference does with ``accelerate=False``.
        ``overlap``: the renders run on side HIP streams (``render_streams`` of them, the frames dealt over them) beside
        the poolings + HOA of the caller's stream: the blend is VALU-bound with a ragged tail, the poolings and the small
        HOA kernels are latency / L2-bound, they interleave.  One stream is the default: two blends at once slow each
        other more than the overlap returns (0.66 vs 0.60 ms).
        ``device_geometry``: per-step mode only: the per-camera calibration algebra on the GPU too
        (ocrf_geometry_blocks; ~1 ulp from the host formulation, so a 1e-5 fraction of border points may change cell).
        ``render_mode``: 'planned' — the render's calibration-only front end (cull, depth order, projected centres)
        is cached per frame like the rank vectors (``raster_plan.RasterPlan``; the Gaussian means are the fixed voxel
        grid, view_transformer_ocrf.py:651-673); 'per_call' — recomputed by every render (``rasterize_views``).
        ``render_guard``: 'host' (the plan's extent bound is checked by ``check_render_plans()``) or 'device'.
        ``plan_rebuild``: 'never' — a render plan lives as long as its calibration; 'per_step' — every step rebuilds it
        on the device from the sample's camera block before rendering (``RasterPlan.rebuild``: no host read), what a
        per-SAMPLE pose costs: the reference builds the render cameras from the dataloader's c2w for every sample
        (view_transformer_ocrf.py:1140-1152, detectors/ocrfdet.py:215-223).
        ``frame_motion``: batch entry b is frame ``frame_offset + b`` of a multi-frame sample with its own ego pose
        (``synthetic.ego_motion``) and its own Gaussian parameters, instead of every frame repeating frame 0.
        ``plan_margin``: ``RasterPlan``'s margin on the extent bound.
        ``lss_pool_backend`` / ``ht_pool_backend``: 'tile' | 'mfma' | 'panel'; None = 'panel' for both, the latency
        kernel of csrc/bev_pool_panel.hip ('mfma': per-tile MFMA panels, csrc/bev_pool_mfma.hip; 'tile': the VALU tile
        kernel; ``lss_mfma_group``: the MFMA form's group size for the LSS ranks; measurements: DESIGN 4.1, 4.6b).
        ``fuse_frames``: planned renders put consecutive frames into one plan / one launch pair.  'auto' and True: as
        many as fit 32 views; False: a launch pair per frame.
        ``blend_workgroups``: size of the planned blend's persistent grid (``blend_workgroups_for``).
        ``hoa_first``: HOA-1/2 before the poolings (None: with the per-call render or the per-step index preparation).
        ``gaussians``: the synthetic Gaussian parameter set (``synthetic.grid_gaussians``): 'init' | 'stress' | 'objects'.
        ``alternate``: draw TWO parameter sets per frame and let the caller switch between them from step to step
        (``set_phase``; default: only for 'objects') — new parameters every step, as a network's heads produce them: the
        planned render's adaptive head then always works from the OTHER set's reach.
        ``one_call``: after its first, recorded, issue a step is ONE host call (``ocrf_hotpath_step``: the library calls
        of the step replayed from C, ``_lib.StepCache``) instead of ~14 ctypes calls + torch stream / event calls
        (225 -> ~60 us of host work at cfg2).  The step's outputs are then the SAME tensors every step (overwritten by
        the next one, like a replayed graph's), and ``depth`` / ``feat`` have to be the tensors of the recorded call
        (another pair is recorded anew).
        ``fuse_hoa_stats``: HOA-3's channel statistics of the HT BEV leave the HT pooling with its tiles
        (``bevpool.bev_pool_v2_panel(..., stats=...)``) instead of being read back from the BEV by a launch of their own
        (``_fused_stats``: cached rank vectors and the panel backend; False: always that launch).
        ``yield_word``: the "another chain is still running" word of an owner that renders this path on ITS side stream
        (``ShardedHotPath``); this path's planned blends then yield to it as they do to their own (``_use_busy``)."""
        self.cfg, self.device = cfg, torch.device(device)
        on_gpu = self.device.type == 'cuda'
        assert render_mode in ('planned', 'per_call') and render_guard in ('host', 'device')
        assert plan_rebuild in ('never', 'per_step') and index_prep_mode in ('cached', 'per_step')
        assert gaussians in synthetic.GAUSSIAN_SETS
        self.fuse_hoa_stats, self.plan_rebuild, self.gaussians = bool(fuse_hoa_stats), plan_rebuild, gaussians
        self.plan_bins = (4, 2)                # candidate lists of the render plans: bins of 4 x 2 tile pairs (64 x 64 px)
        self.alternate = (gaussians == 'objects') if alternate is None else bool(alternate)
        self.phase = 0
        self.render_mode, self.render_guard, self.plan_margin = render_mode, render_guard, float(plan_margin)
        self.frame_motion, self.frame_offset = bool(frame_motion), int(frame_offset)
        self.overlap = bool(overlap) and on_gpu
        lss_pool_backend, ht_pool_backend = lss_pool_backend or 'panel', ht_pool_backend or 'panel'
        assert ht_pool_backend in ('mfma', 'tile', 'panel') and lss_pool_backend in ('mfma', 'tile', 'panel')
        self.ht_pool_backend, self.lss_pool_backend, self.lss_mfma_group = ht_pool_backend, lss_pool_backend, int(lss_mfma_group)
        self.hoa_first, self.one_call = hoa_first, bool(one_call) and on_gpu
        # the recorded steps: (two phases x two input pairs, with room)
        self._compiled = _lib.StepCache(self.device, size=4, seen_size=16, check=self._flat_outputs)
        self.fuse_frames, self.render_streams, self.blend_workgroups = fuse_frames, max(1, int(render_streams)), blend_workgroups
        self._n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count if on_gpu else 0
        self._busy = torch.zeros(1, dtype=torch.int32, device=self.device) if on_gpu else None
        self._yield_word = yield_word
        self.cams = list(range(cfg.n_cams)) if cams is None else list(cams)
        self.batch = cfg.batch * cfg.n_frames                  # frames ride along as batch entries
        self.index_prep_mode, self.device_geometry = index_prep_mode, bool(device_geometry)
        self._side = []                                         # the render streams (a tool may put its own here)
        self._prep_stream = self._prep_stream2 = None
        self._streams = None                                    # _lib.StepStreams of the last step's layout
        # what _prepare fills where the configuration has it
        self._calib_dev = None
        self.frame_cams, self.store, self.render_plans, self._call_sets = [], None, None, None
        self.bg = self.render_convention = None
        self.hoa_mods = self.alpha_lidar = self.bev_pos1 = self._hoa_stats = None
        self._prepare()

    def _prepare(self):
        cfg, dev = self.cfg, self.device
        r = synthetic.rig(cfg.n_cams, cfg.input_size, self.batch, frame_motion=self.frame_motion,
                          frame_offset=self.frame_offset)
        sel = self.cams
        X, Y, _ = cfg.bev_xyz
        # Rank vectors of both branches from the HIP index preparation (csrc/index_prep.hip), which is pinned
        # bit-exactly to the reference's vectors at every configuration (tests/test_index_prep_gpu.py).  The same
        # formulas as torch ops ON THE GPU are not: torch's elementwise GPU kernels contract multiply-adds, and at
        # 512x1408 three pillar samples land on the other side of a .round() (view_transformer_ocrf.py:810).
        # The tiny per-camera 3x3 algebra runs on the host, as the same torch calls the reference makes.
        self._calib_host = [torch.from_numpy(r[k][:, sel] if k != 'bda' else r[k]) for k in
                            ('rots', 'trans', 'intrins', 'post_rots', 'post_trans', 'bda')]
        frustum = index_prep.create_frustum(cfg.grid['depth'], cfg.input_size, cfg.downsample)
        self._frustum_dev = frustum.to(dev).contiguous()
        self._ref_template = index_prep.get_reference_points_3d(Y, X, bs=1, num_points_in_pillar=cfg.num_height,
                                                                device='cpu')[0].to(dev).contiguous()
        self._grid = index_prep.grid_infos(cfg.grid)
        self._lss_bufs, self._ht_bufs = index_prep._RankBuffers(), index_prep._RankBuffers()
        # the cached ranks are the reference's bit for bit: host algebra, whatever ``device_geometry`` says
        self.lss, self.ht = self.prepare_indices_hip(sync=True, host_algebra=True)
        # contiguous fp32 on the device: ocrf_geometry_blocks then reads THESE tensors (a conversion inside the per-step
        # path would be a torch kernel per step — one that a recorded step would not replay)
        self._calib_dev = [t.to(dev).float().contiguous() for t in self._calib_host]
        # cached plans must not alias the grow-only buffers the per-step preparation writes into
        for plan in (self.lss, self.ht):
            for name in ('ranks_bev', 'ranks_depth', 'ranks_feat', 'starts', 'lengths'):
                setattr(plan, name, getattr(plan, name).clone())
        # metric voxel centres (B, Zh, Y*X, 3): the Gaussian means of the render (ocrf_ht_project, bit-exact vs the
        # oracle of get_sampling_point's in-place scaling, view_transformer_ocrf.py:690-692)
        lidar2img, img_aug, _, _ = index_prep.get_projection(*self._calib_host)
        ht_block = index_prep.ht_camera_block(lidar2img, img_aug).to(dev)
        _, _, voxel = index_prep.ht_project_hip(self._ref_template, ht_block, self.batch, len(sel), list(cfg.pc_range),
                                                cfg.input_size, cfg.grid['depth'])
        self.voxel_xyz = voxel

        if cfg.render or cfg.hoa:      # (HOA-1 reads the Gaussian opacities: the parameter sets exist without the render too)
            self._prepare_render(r)
        if cfg.hoa:
            self.hoa_mods, self.alpha_lidar, self.bev_pos1 = hotpath_scene.hoa_scene(cfg, self.batch, dev)
            # channel mean / max of the HT BEV, written by the HT pooling and read by HOA-3's gate (``fuse_hoa_stats``): one
            # buffer for every step, like the step's other persistent scratch (a recorded step replays its address)
            if dev.type == 'cuda':
                self._hoa_stats = torch.empty(self.batch, 2, Y, X, dtype=torch.float32, device=dev)

    def _prepare_render(self, r, convention='corrected', seed=0):
        """The render scene of rig ``r`` (``hotpath_scene``): per frame the owned cameras in ``convention`` and, per
        phase, the Gaussian parameters of frame (frame_offset + b) — with frame_motion every frame draws its own."""
        self.frame_cams = hotpath_scene.render_cameras(r, self.cams, self.batch, self.cfg.input_size, self.device, convention)
        seeds = [seed + (self.frame_offset + b if self.frame_motion else 0) for b in range(self.batch)]
        self.store = hotpath_scene.GaussianStore(self.gaussians, self.voxel_xyz, 2 if self.alternate else 1, seeds, self.device)
        self.bg, self.render_convention = torch.zeros(3, device=self.device), convention
        self.render_plans = self._call_sets = None               # built on first use

    # ---- the Gaussian parameters of the current phase: views of the store ---------------------------------------------
    @property
    def frame_gauss(self):
        return self.store.frames[self.phase]                     # [frame] -> parameter dict of the current phase

    @property
    def gauss(self):
        return self.frame_gauss[0]                               # frame 0 (tests, tools)

    @property
    def render_cams(self):
        return self.frame_cams[0]

    @property
    def _opac_flat(self):
        return self.store.opac_flat[self.phase]                  # HOA-1's input column: never laid out per step

    @property
    def _sets(self):
        return self._per_call_sets()

    def set_phase(self, phase):
        """Switch to parameter set ``phase`` of every frame (``alternate``): the next step renders (and HOA reads) the
        other tensors — new parameters, as a network's heads hand them over every step.  A recorded step is per phase."""
        self.phase = int(phase) % (2 if self.alternate else 1)

    @torch.no_grad()
    def hoa_opacity_bev(self):
        """HOA-1/2 (view_transformer_ocrf.py:1159-1161, 1196): opacity BEV (B,1,Y,X).  Independent of the pooled
        BEV (it reads the Gaussian opacities and the NeRF-branch alpha volume).  Every frame has its own opacity
        volume; the reference loops samples (:1090)."""
        X, Y, _ = self.cfg.bev_xyz
        oa = hoa.hoa1(self.hoa_mods['dca'], self._opac_flat, self.alpha_lidar, self.cfg.num_height, Y, X)
        return self.hoa_mods['v2b'](oa, self.bev_pos1)

    @torch.no_grad()
    def hoa_step(self, geom_feat, opacity_bev=None, stats=None):
        """HOA-1/2/3 (view_transformer_ocrf.py:1159-1161, 1196-1199): -> (gated BEV, opacity BEV).  ``stats``:
        ``hoa.channel_stats(geom_feat)`` if the caller has it already (``_fused_stats``)."""
        if opacity_bev is None:
            opacity_bev = self.hoa_opacity_bev()
        _, gated = self.hoa_mods['mask'].gate(geom_feat, opacity_bev, stats=stats)
        return gated, opacity_bev

    def _fused_stats(self):
        """The buffer the HT pooling fills with HOA-3's channel statistics, or None where they are a launch of their own:
        without HOA, with the per-step index preparation (``bev_pool_v2_nchw_dyn``) and with the tile / MFMA backends."""
        if (self.fuse_hoa_stats and self.cfg.hoa and self.index_prep_mode == 'cached' and self._hoa_stats is not None
                and self.ht.writes_stats(self.ht_pool_backend)):
            return self._hoa_stats
        return None

    def _plans(self):
        """Render plans: every frame sees the SAME Gaussian means (the voxel grid) through its own cameras with its own
        parameter set, so consecutive frames share one plan of up to 32 views (``raster_plan.RasterPlan`` with one
        Gaussian set per frame): one update launch and one persistent blend launch for all of them instead of a pair
        per frame, also when the batch needs several plans.  -> list of (plan, first frame, n frames,
        parameters), the parameters views of the store."""
        if self.render_plans is None:
            H, W = self.cfg.input_size
            n_cam = len(self.cams)
            same = all(torch.equal(self.voxel_xyz[b], self.voxel_xyz[0]) for b in range(1, self.batch))
            fuse = True if self.fuse_frames == 'auto' else bool(self.fuse_frames)
            per = max(1, 32 // n_cam) if (same and fuse) else 1
            self.render_plans = []
            for f0 in range(0, self.batch, per):
                nf = min(per, self.batch - f0)
                cams = torch.cat([self.frame_cams[b]['packed'] for b in range(f0, f0 + nf)])
                alts = self.store.frames_slice(f0, nf)
                g = alts[0]
                # (the extent bound has to hold for every parameter set the plan will render)
                ext_sc = torch.cat([a['scales'].reshape(-1, 3) for a in alts])
                ext_rot = torch.cat([a['rotations'].reshape(-1, 4) for a in alts])
                # record capacity: what these cameras keep + 10 % — + 25 % when the plan is rebuilt per step for poses that
                # may keep more (a plan beyond its capacity is refused on the device: status bit 8, zero images; read
                # check_render_plans() before the images are consumed, or render with render_guard='device')
                plan = raster_plan.RasterPlan(self.voxel_xyz[f0].reshape(-1, 3), cams, H, W, scales=ext_sc,
                                              rotations=ext_rot, margin=self.plan_margin,
                                              headroom=1.25 if self.plan_rebuild == 'per_step' else 1.1,
                                              # a plan rebuilt per SAMPLE does not build candidate lists every step
                                              bins=None if self.plan_rebuild == 'per_step' else self.plan_bins)
                # item z = view z of the plan (frame-major), rendered with the parameter set of its frame
                item_view = torch.arange(nf * n_cam, dtype=torch.int32, device=self.device)
                for a in alts:
                    a['item_view'] = item_view
                    a['cams'] = plan.cameras             # the sample's camera block: a per-step rebuild reads it in place
                g['alt'] = alts                          # [phase] -> parameter dict (alts[0] is g)
                self.render_plans.append((plan, f0, nf, g))
        return self.render_plans

    def check_render_plans(self):
        """Synchronising check of the render plans' extent bound (``render_guard='host'``): raises if a planned
        render since the last check was not valid."""
        for p in self.render_plans or []:
            p[0].check()

    def _render_per_call(self, b, want_n_contrib, tag):
        cfg, rc, g = self.cfg, self.frame_cams[b], self.frame_gauss[b]
        H, W = cfg.input_size
        xyz = self.voxel_xyz[b].reshape(-1, 3)
        return rasterize_views(xyz, g['rgb'], g['opacity'], g['scales'], g['rotations'], rc['vm'], rc['pm'], rc['tfx'],
                               rc['tfy'], H, W, self.bg, packed_cameras=rc['packed'], want_n_contrib=want_n_contrib,
                               workspace_tag=tag)

    def _use_busy(self):
        # the hint pays when a step has several blend launches; with ONE launch per step every extra workgroup would
        # leave at once anyway, and the two stream writes are not free
        return bool(self.overlap and self._busy is not None and self.render_plans is not None and len(self.render_plans) > 1)

    def _set_busy(self, value):
        if self._use_busy():
            _lib.launch('ocrf_stream_write_value32', self.device, self._busy, int(value))

    def _render_planned(self, entry, phase='both', out=None):
        plan, f0, nf, g = entry
        g = g['alt'][self.phase]
        # the "other chain still running" word: the owner's (``yield_word``), or this path's own (several blends per step)
        word = self._yield_word if self._yield_word is not None else (self._busy if self._use_busy() else None)
        H, W = self.cfg.input_size
        bw = blend_workgroups_for(self.blend_workgroups, f0, H * W, self._n_cu, self.overlap or self._yield_word is not None)
        call_cams = None
        if self.plan_rebuild == 'per_step':
            if phase != 'blend':
                plan.rebuild(g['cams'])
            call_cams = g['cams']                       # ... and the call is checked against the plan's cameras on the device
        out = plan.render(g['rgb'], g['opacity'], g['scales'], g['rotations'], self.bg, guard=self.render_guard,
                          item_view=g['item_view'] if nf > 1 else None, blend_workgroups=bw, phase=phase, out=out,
                          yield_if=word if bw else None, cameras=call_cams, views_disjoint=True, want_radii=False)
        return out if phase == 'update' else frames_of(out, len(self.cams), nf)

    def render(self, streams=None, want_n_contrib=False):
        """All owned cameras of every frame: list (one per frame) of dicts (``color``, ``depth``, ``final_T``, ...).
        ``streams``: a HIP stream per frame (frames on different streams get their own scratch buffer); the caller
        joins them.  The step is inference: the per-pixel contributor index (read only by the backward) is not
        tracked unless ``want_n_contrib`` (which renders per call, one call per frame)."""
        planned = self.render_mode == 'planned' and not want_n_contrib
        outs = []
        if planned:
            for entry in self._plans():       # built (one synchronisation each) before anything is enqueued
                with _on(streams, entry[1]):
                    outs.extend(self._render_planned(entry))
            return outs
        one_stream = streams is None or all(st is streams[0] for st in streams)
        if self.batch > 1 and one_stream and not want_n_contrib and self._per_call_sets() is not None:
            # every frame its own Gaussian set and cameras, all on one stream: ONE set of launches for the batch
            # (ocrf_rasterize_forward_sets: one preprocess / scan / scatter / blend over all frames' views — cfg2's two
            # frames 2 x 5 launches -> 5, and one blend of twelve views fills the chip better than two of six)
            g = self._per_call_sets()
            H, W = self.cfg.input_size
            with _on(streams, 0):
                o = rasterize_sets(g['xyz'], g['rgb'], g['opacity'], g['scales'], g['rotations'], g['cams'], H, W, self.bg,
                                   workspace_tag='raster_sets')
            return frames_of(o, len(self.cams), self.batch)
        for b in range(self.batch):
            with _on(streams, b):      # (frames on different streams: a scratch buffer each)
                tag = 'raster' if streams is None else f'raster{streams.index(streams[b])}'
                outs.append(self._render_per_call(b, want_n_contrib, tag))
        return outs

    def _per_call_sets(self):
        """The current phase's parameters for one per-call render of the whole batch (up to 64 views; else None): the
        store's stacks themselves, beside the frames' means and cameras stacked once."""
        if self._call_sets is None:
            self._call_sets = False
            if self.batch * len(self.cams) <= 64:
                shared = dict(xyz=self.voxel_xyz.reshape(self.batch, -1, 3).contiguous(),
                              cams=torch.cat([rc['packed'] for rc in self.frame_cams]).contiguous())
                self._call_sets = [{**st, **shared} for st in self.store.stacks]
        return self._call_sets[self.phase] if self._call_sets else None

    @property
    def views_per_step(self):
        return self.batch * len(self.cams) if self.cfg.render else 0

    def _or_empty(self, five):
        if five[0] is None:
            e = torch.zeros(0, dtype=torch.int32, device=self.device)
            return e, e, e, e, e
        return five

    def make_inputs(self, seed=0):
        """depth (B, N, D, H, W), feat (B, N, H, W, C) channels-last, on the device."""
        depth, feat = hotpath_scene.synthetic_inputs(self.cfg, self.batch, seed)
        return depth[:, self.cams].contiguous().to(self.device), feat[:, self.cams].contiguous().to(self.device)

    def _branch(self, plan):
        """(backend, branch) of ``plan``, read at call time; a plan object that is neither ``self.lss`` nor ``self.ht``
        pools with the tile kernel."""
        if plan is self.ht:
            return self.ht_pool_backend, 'ht'
        return (self.lss_pool_backend, 'lss') if plan is self.lss else ('tile', None)

    def pool(self, plan, depth, feat, out=None, weights_ready=False, stats=None):
        """``bevpool.PoolPlan.pool`` with this path's backend for ``plan`` -> (B, Z*C, Y, X)."""
        return plan.pool(depth, feat, *self._branch(plan), self.lss_mfma_group, out, weights_ready, stats)

    def _device_algebra(self):
        """The calibration algebra runs on the device (``device_geometry``, once the device copy of the calibration exists)."""
        return self.device_geometry and self._calib_dev is not None

    def _camera_blocks(self, host_algebra=False):
        cfg, dev, args = self.cfg, self.device, self._calib_host
        if self._device_algebra() and not host_algebra:
            lss_block, ht_block, _ = index_prep.geometry_blocks_hip(*self._calib_dev, None, cfg.input_size)
        else:
            lss_block = index_prep.lss_camera_block(*args).to(dev, non_blocking=True)
            lidar2img, img_aug, _, _ = index_prep.get_projection(*args)
            ht_block = index_prep.ht_camera_block(lidar2img, img_aug).to(dev, non_blocking=True)
        return lss_block, ht_block

    def _prepare_lss(self, lss_block):
        B, N = self._calib_host[1].shape[:2]
        return index_prep.voxel_pooling_prepare_v2_hip(self._frustum_dev, lss_block, B, N, *self._grid,
                                                       buffers=self._lss_bufs, sync=False)

    def _prepare_ht(self, ht_block):
        cfg = self.cfg
        B, N = self._calib_host[1].shape[:2]
        Hf, Wf = cfg.feat_hw
        return index_prep.fast_sample_prepare_hip(self._ref_template, ht_block, B, N, list(cfg.pc_range), cfg.input_size,
                                                  cfg.grid['depth'], Wf, Hf, cfg.D, buffers=self._ht_bufs, sync=False)

    def prepare_indices_hip(self, sync=True, host_algebra=False):
        """Rank vectors of both poolings from the calibration, on the device (view_transformer.py:108-147,
        197-255; view_transformer_ocrf.py:675-740,785-852): tiny per-camera algebra (on the host, or with
        ``device_geometry`` and not ``host_algebra`` on the device), then csrc/index_prep.hip.
        -> (lss PoolPlan, ht PoolPlan)."""
        cfg = self.cfg
        X, Y, Z = cfg.bev_xyz
        lss_block, ht_block = self._camera_blocks(host_algebra)
        lss = self._prepare_lss(lss_block)
        ht = self._prepare_ht(ht_block)
        if not sync:
            return lss, ht                                      # ((five capacity vectors), counts) each
        counts = torch.stack((lss[1], ht[1])).cpu()           # ONE device->host read for both (4 ints)
        return (PoolPlan(*self._or_empty(index_prep._trim(lss[0], counts[0])), (self.batch, Z, Y, X, cfg.channels)),
                PoolPlan(*self._or_empty(index_prep._trim(ht[0], counts[1])), (self.batch, 1, Y, X, cfg.channels)))

    def _pool_prepared(self, plan, depth, feat, prepared, **kw):
        """``plan``'s pooling from ``prepared`` = (five capacity vectors, device-side counts): no host read."""
        v, counts = prepared
        return bevpool.bev_pool_v2_device_counts(depth, feat, v[1], v[2], v[0], plan.bev_shape, v[3], v[4], counts, **kw)

    def pool_step(self, depth, feat, prepared=None, ht_stats=None):
        """Both poolings (index preparation first in 'per_step' mode): LSS BEV (B, Z*C, Y, X) and
        HT BEV (B, C, Y, X) (view_transformer.py:194, view_transformer_ocrf.py:781).  ``prepared``: what
        ``prepare_indices_hip(sync=False)`` returned, if the caller already issued it.  ``ht_stats``: ``_fused_stats()``."""
        if self.index_prep_mode == 'per_step':
            # ranks stay on the device, their lengths too: no host read anywhere in the step
            lss, ht = prepared if prepared is not None else self.prepare_indices_hip(sync=False)
            return self._pool_prepared(self.lss, depth, feat, lss), self._pool_prepared(self.ht, depth, feat, ht)
        if self.lss.route(self.lss_pool_backend) == 'panel' == self.ht.route(self.ht_pool_backend):
            # both poolings read the same depth tensor: ONE launch sums the cell weights of both plans
            bevpool.bev_pool_cell_weights(depth, self.lss.panel_plan('lss', 'panel'), self.ht.panel_plan('ht', 'panel'))
            return (self.pool(self.lss, depth, feat, weights_ready=True),
                    self.pool(self.ht, depth, feat, weights_ready=True, stats=ht_stats))
        return self.pool(self.lss, depth, feat), self.pool(self.ht, depth, feat, stats=ht_stats)

    def step(self, depth, feat):
        """One pass of the hot path: pools (+ render + HOA where the configuration has them).
        -> (lss, ht[, rendered][, gated, opacity_bev]), everything ordered on the caller's stream.  With ``one_call``
        the returned tensors are the same objects every step (see ``__init__``)."""
        if self.cfg.render and self.render_mode == 'planned':
            self._plans()             # first step: built on the caller's stream BEFORE the side streams branch off it
        if not self.one_call:
            return self._step_eager(depth, feat)
        if self._compiled.refused is None and self.index_prep_mode == 'per_step' and not self._device_algebra():
            # the per-step index preparation with the calibration algebra on the HOST (torch CPU ops + uploads per step,
            # which a replay would not repeat): issued call by call
            self._compiled.refused = 'per-step calibration algebra on the host is issued call by call'
        out = self._compiled(self._step_key(depth, feat), self._step_streams(torch.cuda.current_stream(self.device)),
                             lambda rec: self._step_eager(depth, feat, rec))
        # a replay does not go through RasterPlan.render, which marks a host-guarded render for check_render_plans()
        for entry in (self.render_plans or []) if self.cfg.render and self.render_mode == 'planned' else []:
            entry[0]._host_guarded = entry[0]._host_guarded or self.render_guard == 'host'
        return out

    @property
    def one_call_refused(self):
        """Why steps are issued call by call although ``one_call`` asked for one host call (None: they are not)."""
        return self._compiled.refused

    def _step_key(self, depth, feat):
        """Everything ``_step_eager`` reads that decides WHICH launches a step is (a recorded step must not outlive a
        changed mode attribute): the input tensors (address, shape, dtype), the parameter phase and the modes."""
        bw = self.blend_workgroups
        return (depth.data_ptr(), feat.data_ptr(), tuple(depth.shape), tuple(feat.shape), depth.dtype, feat.dtype, self.phase,
                self.index_prep_mode, self.plan_rebuild, self.overlap, bw if isinstance(bw, (int, str)) else tuple(bw),
                self.render_mode, self.render_guard, self.hoa_first, self.lss_pool_backend, self.ht_pool_backend,
                self.render_streams, self.fuse_frames, self.device_geometry, self.fuse_hoa_stats)

    def _forks(self):
        return self.overlap and self.cfg.render

    def _prep_forks(self):
        """The per-step index preparation on two streams of its own (``_main_chain``)."""
        return self.index_prep_mode == 'per_step' and self.cfg.hoa and self.overlap and self._device_algebra()

    def _step_streams(self, cur, rec=None):
        """The step's streams in slot order: the caller's ('main'), the render streams ('render0'..), the two
        index-preparation streams ('prep', 'prep2').  The one place that decides them; ``self._streams`` is the same
        list as a ``_lib.StepStreams``, bound to ``cur`` and to the recorder ``rec`` of the step about to be issued."""
        forks, prep = bool(self._forks()), bool(self._prep_forks())
        st = [cur]
        if forks:
            if not self._side:
                self._side = [shared_stream(self.device, 'render' if k == 0 else f'render{k}')
                              for k in range(self.render_streams)]
            st += self._side
        if prep:
            if self._prep_stream is None:
                self._prep_stream = shared_stream(self.device, 'prep')
                self._prep_stream2 = shared_stream(self.device, 'prep2')
            st += [self._prep_stream, self._prep_stream2]
        ss = self._streams
        if ss is None or ss.streams[1:] != st[1:]:                # (another layout, or a tool put its own streams in)
            names = ['main'] + [f'render{k}' for k in range(len(self._side) if forks else 0)] + ['prep', 'prep2'][:2 * prep]
            ss = self._streams = _lib.StepStreams(st, names)
        return ss.bind(cur, rec).streams

    @staticmethod
    def _flat_outputs(out):
        for o in out:
            if torch.is_tensor(o):
                yield o
            elif isinstance(o, dict):
                yield from (v for k, v in o.items() if torch.is_tensor(v) and k != 'status')
            elif isinstance(o, (list, tuple)):
                yield from HotPath._flat_outputs(o)

    def _step_eager(self, depth, feat, rec=None):
        cur = torch.cuda.current_stream(self.device) if self.device.type == 'cuda' else None
        self._step_streams(cur, rec)
        ss = self._streams
        if not self._forks():
            main = self._main_chain(depth, feat, ss)
            rendered = [self.render()] if self.cfg.render else []
            return tuple(main[:2]) + tuple(rendered) + tuple(main[2:])
        # "the main chain is running": the persistent blends of the render streams keep to a part of the chip while it is
        # up and take the whole chip once it is down (cfg4: the renders outlast the poolings + HOA)
        self._set_busy(1)
        for name in ss.names[1:1 + len(self._side)]:
            ss.fork('main', name)                 # inputs (and last step's consumers) are ordered before
        # host issue order: the render call first (measured against the LSS pooling / both poolings first: within 1 %)
        rendered = self.render([self._side[b % len(self._side)] for b in range(self.batch)])
        main = self._main_chain(depth, feat, ss)
        self._set_busy(0)
        for name in ss.names[1:1 + len(self._side)]:
            ss.join(name, 'main')                 # everything the step returns is ordered on `cur`
        consumed_on(rendered, cur)
        return tuple(main[:2]) + (rendered,) + tuple(main[2:])

    def _main_chain(self, depth, feat, ss=None):
        """Pools + HOA on the current stream -> (lss, ht[, gated, opacity_bev]).  ``ss``: the step's ``_lib.StepStreams``
        (None: this chain is the whole step, on the current stream, and nothing records it)."""
        # HOA-1/2 do not read the pooled BEV and are latency chains of small kernels
        prep_forks, stats = self._prep_forks(), None
        if prep_forks:
            if ss is None:
                self._step_streams(torch.cuda.current_stream(self.device))
                ss = self._streams
            # the index preparation needs nothing HOA-1/2 produce: its two independent chains on a stream each beside
            # them (their look-back scratch is per stream, index_prep._prep_tag), the calibration blocks computed once on
            # the first and handed over; each pooling is issued behind its own ranks, the critical LSS chain first, then
            # the HT pair, then HOA-1/2 on the caller's stream (why, and what else was measured: DESIGN 4.6b)
            ss.fork('main', 'prep')
            ss.fork('main', 'prep2')
            with torch.cuda.stream(ss['prep']):
                lss_block, ht_block = self._camera_blocks()
                ht_block.record_stream(ss['prep2'])
                ss.fork('prep', 'prep2')                             # the blocks are ready: taken before the LSS chain
                lss = self._pool_prepared(self.lss, depth, feat, self._prepare_lss(lss_block))
            with torch.cuda.stream(ss['prep2']):
                ht = self._pool_prepared(self.ht, depth, feat, self._prepare_ht(ht_block), scratch_tag='bev_pool_nchw_b')
        # HOA-1/2 need nothing of the poolings and the poolings nothing of them: with the planned render the poolings go
        # FIRST — they meet the start of the side stream's blend instead of its middle; with the per-call render, whose
        # chip-filling preprocess opens the side stream, and with the per-step index preparation (which the poolings have
        # to wait for anyway) HOA-1/2 first.
        hoa_first = self.hoa_first
        if hoa_first is None:
            hoa_first = self.render_mode != 'planned' or self.index_prep_mode == 'per_step'
        ob = self.hoa_opacity_bev() if (self.cfg.hoa and hoa_first) else None
        if prep_forks:
            ss.join('prep', 'main')
            ss.join('prep2', 'main')
            lss.record_stream(ss['main'])
            ht.record_stream(ss['main'])
        else:
            # the HT BEV is what HOA-3 gates below: its channel statistics leave the pooling with its tiles
            stats = self._fused_stats()
            lss, ht = self.pool_step(depth, feat, ht_stats=stats)
        if self.cfg.hoa and not hoa_first:
            ob = self.hoa_opacity_bev()
        out = [lss, ht]
        if self.cfg.hoa:
            # stand-in for geom_feat: the HT BEV has its shape (B,C,Y,X); the fusion convs between
            # the pools and HOA-3 are MIOpen territory, not part of this path
            out.extend(self.hoa_step(ht, ob, stats=stats))
        return out

    @property
    def bev_voxels_per_step(self):
        return bev_voxels(self.cfg, self.batch)


def __getattr__(name):      # the two classes that lived here, resolved on first use (the sharded path imports this module)
    if name in ('ShardedHotPath', 'NeckPath'):
        from . import neck_path, sharded_hotpath
        return getattr(sharded_hotpath if name == 'ShardedHotPath' else neck_path, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
