"""The hot path of one sample sharded over the ranks of a ``torch.distributed`` job."""
import torch

from . import _lib, hoa, hotpath_scene, synthetic
from .hotpath import HotPath, shared_stream
from .hotpath_scene import bev_voxels, consumed_on


class ShardedHotPath:
    """The hot path of ONE sample with its camera-frames sharded over the ranks of a ``torch.distributed`` job
    (``sharding.CameraFramePlan``; BASELINE.json north_star, configs[3] / [4]): this rank pools and renders only
    the camera-frames it owns and runs HOA only for the frames it has a part in.  Per step:
      renders (side HIP stream) | pools of the owned cameras into the fused grid's plane blocks
      step 1 of the exchange: the partial grids are summed inside each frame's group (reduce_scatter over plane blocks)
      HOA-1/2 of the OWN frames (they read nothing of the pooled BEV: issued beside step 1)
      HOA-3 on the rank's finished plane blocks, in place (``sharding.gate_blocks``: per-block channel statistics, one
        small all_gather inside the group, the gate of the own channels) — the opacity BEV goes into an extra plane
      step 2: ONE world all_gather — it carries the LSS planes, the GATED height-sampling planes and the opacity BEVs:
        the complete fused grid ``(n_frames, Z*C + C + 1, Y, X)`` on every rank.
    HOA is a per-sample loop in the reference (view_transformer_ocrf.py:1090-1161,1196-1199) and frames are independent
    until the concat (detectors/ocrfdet.py:274): at configs[4] on 8 ranks (whole frames per rank, no reduce) a rank runs the
    ten HOA launches of ONE frame, not of eight; with groups, HOA-1/2 are replicated inside a frame's group only and
    HOA-3 is split over it.  The collectives are asynchronous: the renders and HOA-1/2 run beside them.  With
    ``world == 1`` it is ``HotPath`` with the same fused output buffer, bit for bit."""

    def __init__(self, cfg, device, rank, world, index_prep_mode='cached', render_mode='planned', render_guard='host',
                 sparse_exchange=True, collectives=None, one_call=True):
        from . import sharding
        self.cfg, self.device, self.rank, self.world = cfg, torch.device(device), rank, world
        # one_call: the rank's COMPUTE between the collectives — (poolings + renders) and (HOA-1/2) — is recorded once and
        # replayed by one host call each (``_lib.StepCache``, as ``HotPath.step``): a rank of eight has ~ 0.1 ms of
        # device work per step and would otherwise spend ~ 0.2 ms issuing its ~ 16 library calls through ctypes
        self._one_call = bool(one_call) and self.device.type == 'cuda' and index_prep_mode == 'cached'
        self._segments = _lib.StepCache(self.device, size=16, seen_size=32)     # (four segments x two buffer sets, with room)
        X, Y, Z = cfg.bev_xyz
        C = cfg.channels
        self.n_frames = cfg.batch * cfg.n_frames
        self.planes_lss = Z * C
        self.planes_pool = (Z + 1) * C                          # LSS planes, then HT planes: what the poolings write
        # the frame's opacity BEV rides along as one more plane of the fused grid (written by the rank whose block holds it)
        self.opacity_plane = self.planes_pool if cfg.hoa else None
        self.plan = sharding.CameraFramePlan(cfg.n_cams, self.n_frames, world, self.planes_pool + (1 if cfg.hoa else 0))
        self.exchange = sharding.BevExchange(self.plan, rank, self.device, (Y, X), collectives=collectives)
        self._side = shared_stream(self.device, 'render') if self.device.type == 'cuda' and cfg.render else None
        self._streams = _lib.StepStreams([None, self._side], ['main', 'render0']) if self._side is not None else None
        # the renders run on the side stream beside this rank's poolings, the exchange and HOA: their persistent blends
        # keep to a part of the chip while that chain is running and take the whole chip once it is done (the same
        # occupancy split as HotPath.step; a hint, the images do not depend on it)
        self._busy = None
        if self._side is not None and render_mode == 'planned':
            self._busy = torch.zeros(1, dtype=torch.int32, device=self.device)
        one = synthetic.PathConfig(**{**cfg.__dict__, 'batch': 1, 'n_frames': 1, 'hoa': False})
        self.subs = {f: HotPath(one, self.device, cams=self.plan.cams_of(rank, f), index_prep_mode=index_prep_mode,
                                overlap=False, frame_offset=f, render_mode=render_mode, render_guard=render_guard,
                                one_call=False, yield_word=self._busy)
                     for f in self.plan.frames_of(rank)}
        # HOA weights and inputs: drawn for ALL frames exactly as the unsharded HotPath draws them (one generator), then
        # only the own frames' slices are kept on the device for the steps
        self.my_frames = self.plan.frames_of(rank)
        self.base = self._hoa_in = None
        if cfg.hoa:
            self.base = HotPath(synthetic.PathConfig(**{**cfg.__dict__, 'render': cfg.render or cfg.hoa}), self.device,
                                cams=[0], index_prep_mode='cached', overlap=False, one_call=False)
            fr = self.my_frames
            if fr:
                opac = self.base.store.stacks[0]['opacity'][fr].reshape(-1, 1)      # (a copy: the own frames' columns)
                self._hoa_in = (opac, self.base.alpha_lidar[fr].contiguous(), self.base.bev_pos1[fr].contiguous())
        self.hoa_launch_frames = 0                              # frames whose HOA-1/2 this rank issued in its last step
        # the pipelined step's exchange (``step_pipelined``), the renders it holds back one step, its step count
        self.pipe, self._held, self._pipe_k = None, None, 0
        # ONE rank of a sharded job run without its peers may gate on its own channels' statistics (else refused)
        self.partial_statistics_ok = False
        # wedge-sparse step 1: a member's partial grid is zero outside the strips its cameras' rank vectors touch
        # (static per calibration) — only those strips of the other members' plane blocks cross xGMI
        # The decision is a function of the PLAN (the same on every rank), never of this rank's own buffers: set_touched
        # is a world collective, so idle ranks and owners of whole frames take part with an empty dict.  Only with cached
        # rank vectors: with per-step index preparation (the reference's accelerate=False, calibration per sample) a new
        # calibration may touch tiles outside a stale list and its contributions would be dropped from the sum.
        self.sparse_exchange = bool(sparse_exchange) and self.plan.any_shared and index_prep_mode == 'cached'
        if self.sparse_exchange:
            ex, touched = self.exchange, {}
            for f, sub in self.subs.items():
                if f in ex.partial:
                    yx = torch.cat((sub.lss.ranks_bev.long() % (Y * X), sub.ht.ranks_bev.long() % (Y * X)))
                    touched[f] = torch.unique(ex.tile_of_voxel(yx))
            ex.set_touched(touched)

    def make_inputs(self, seed=0):
        """Per owned frame: depth (1, n_owned_cams, D, H, W), feat (1, n_owned_cams, H, W, C) — the same values
        the unsharded ``HotPath.make_inputs(seed)`` holds for those camera-frames."""
        depth, feat = hotpath_scene.synthetic_inputs(self.cfg, self.n_frames, seed)
        return {f: (depth[f:f + 1, sub.cams].contiguous().to(self.device), feat[f:f + 1, sub.cams].contiguous().to(self.device))
                for f, sub in self.subs.items()}

    @property
    def views_per_step(self):
        return sum(len(s.cams) for s in self.subs.values()) if self.cfg.render else 0

    # ---- HOA, sharded by frame ----------------------------------------------------------------------------------
    @torch.no_grad()
    def _hoa12(self, slot=0):
        """HOA-1/2 of the frames this rank has a part in -> {frame: (Y,X) opacity BEV} (empty on an idle rank).
        ``slot``: which output buffer set a REPLAYED segment writes — the pipelined step alternates two, because step k's
        HOA-3 gate reads these tensors on the communication stream while step k + 1's replay would already rewrite them on
        the caller's (a write-after-read race that constant test inputs hid)."""
        self.hoa_launch_frames = 0
        if self.base is None or not self.my_frames:
            return {}
        cfg = self.cfg
        X, Y, _ = cfg.bev_xyz
        opac, alpha, pos = self._hoa_in
        m = self.base.hoa_mods

        def body(rec):
            return m['v2b'](hoa.hoa1(m['dca'], opac, alpha, cfg.num_height, Y, X), pos)      # (len(my_frames), 1, Y, X)
        if self.device.type == 'cuda':
            ob = self._segment('hoa12', (opac.data_ptr(), alpha.data_ptr(), pos.data_ptr(), int(slot)),
                               [torch.cuda.current_stream(self.device)], body)
        else:
            ob = body(None)
        self.hoa_launch_frames = len(self.my_frames)
        return {f: ob[i, 0] for i, f in enumerate(self.my_frames)}

    def _gate(self, ex, ob):
        """HOA-3 on this rank's finished plane blocks, in place (``sharding.gate_blocks``)."""
        from . import sharding
        if self.base is None:
            return
        X, Y, _ = self.cfg.bev_xyz
        mask = self.base.hoa_mods['mask']

        def stats_fn(x):
            return hoa.channel_stats(x.unsqueeze(0))[0]

        def gate_fn(x, stats, opacity):
            mask.gate(x.unsqueeze(0), opacity.reshape(1, 1, Y, X), stats=stats.unsqueeze(0).contiguous(), in_place=True)
        def body(rec):
            with torch.no_grad():
                sharding.gate_blocks(ex, self.planes_lss, self.cfg.channels, None, ob, stats_fn, gate_fn,
                                     partial_ok=self.partial_statistics_ok)
        # a rank whose frames are all its own (no group to gather statistics from) gates without a collective inside:
        # one more recorded segment
        alone = all(len(self.plan.group_of_frame[f]) == 1 or not ex.active for f, _, _ in ex.my_blocks)
        if alone and self.device.type == 'cuda':
            key = (id(ex),) + tuple(t.data_ptr() for t in ob.values())
            self._segment('gate', key, [torch.cuda.current_stream(self.device)], body)
        else:
            body(None)
        # the frame's opacity BEV into its plane of the fused grid (the member whose block holds that plane): it travels
        # with the gather (a torch copy: not part of a recorded segment)
        with torch.no_grad():
            for f, p0, n, view in ex.block_views():
                if p0 <= self.opacity_plane < p0 + n:
                    view[self.opacity_plane - p0].copy_(ob[f])

    def _outputs(self, full, rendered):
        gated = opacity_bev = None
        if self.base is not None:
            gated = [full[f:f + 1, self.planes_lss:self.planes_pool] for f in range(self.n_frames)]
            opacity_bev = full[:, self.planes_pool:self.planes_pool + 1]
        return full, rendered, gated, opacity_bev

    @property
    def one_call(self):
        """The compute segments are replayed by one host call each (False once a recording was refused)."""
        return self._one_call and self._segments.refused is None

    @property
    def one_call_refused(self):
        return self._segments.refused

    def _segment(self, name, key, streams, fn):
        """``fn(rec)`` — library calls only, on ``streams`` (slot 0 = the caller's) — by ONE host call from the third time
        ``key`` (the pointers it works on) is seen (``_lib.StepCache``; no first-replay check: the ``gate`` segment works
        in place, so a second run is not comparable).  -> what ``fn`` returned (the same tensors every replay)."""
        if not self._one_call:
            return fn(None)
        return self._segments((name, key), streams, fn)

    def _pool_and_render(self, inputs, target_of):
        cur = torch.cuda.current_stream(self.device) if self._side is not None else None
        targets = {f: target_of(f) for f in self.subs}

        def body(rec):
            rendered = []
            if self._side is not None:
                self._set_busy(1)
                self._streams.bind(cur, rec).fork('main', 'render0')
                rendered = [sub.render([self._side]) for sub in self.subs.values()]
            for f, sub in self.subs.items():
                (depth, feat), tgt = inputs[f], targets[f]
                sub.pool(sub.lss, depth, feat, out=tgt[:self.planes_lss])
                sub.pool(sub.ht, depth, feat, out=tgt[self.planes_lss:self.planes_pool])
            return rendered
        if self.device.type != 'cuda' or not self.subs:
            return cur, body(None)
        key = tuple((f, inputs[f][0].data_ptr(), inputs[f][1].data_ptr(), targets[f].data_ptr()) for f in self.subs)
        streams = self._streams.bind(cur).streams if self._side is not None else [torch.cuda.current_stream(self.device)]
        return cur, self._segment('pool_render', key, streams, body)

    def _join_renders(self, cur, rendered):
        if self._side is not None:
            self._set_busy(0)
            self._streams.bind(cur).join('render0', 'main')      # (behind the gather: outside the recorded segment)
            for per_sub in rendered:
                consumed_on(per_sub, cur)

    def step(self, inputs):
        """-> (fused BEV (n_frames, Z*C + C [+ 1], Y, X) complete on every rank — LSS planes, GATED height-sampling planes,
        opacity BEV —, rendered list, gated (views of the fused grid, per frame), opacity_bev (view))."""
        if self.pipe is not None and self.pipe._pending is not None:
            raise _lib.OcrfHipError('a pipelined step is pending on the shared exchange buffers: flush_pipelined() first')
        ex = self.exchange
        cur, rendered = self._pool_and_render(inputs, ex.pool_target)
        works = ex.start()
        ob = self._hoa12()
        ex.finish_reduce(works)
        self._gate(ex, ob)
        full = ex.gather()
        self._join_renders(cur, rendered)
        return self._outputs(full, rendered)

    def step_pipelined(self, inputs):
        """The same step with the exchange taken off its critical path (``sharding.PipelinedExchange``): this call pools
        and renders step k, runs its HOA-1/2 and starts its exchange — step 1, the in-place HOA-3 of the own blocks, step 2
        — on a communication stream; it RETURNS step k - 1 (as ``step`` does; ``None`` for the first call), whose exchange
        ran under this call's poolings and renders.  ``flush_pipelined()`` hands out the last step.  A rank's throughput
        is then max(own compute, exchange) instead of their sum; the price is one step of latency, and the returned
        tensors of step k - 1 are overwritten two calls later.  The pipeline has two buffer sets of its own on the process
        groups of ``self.exchange``."""
        from . import sharding
        if self.pipe is None:
            ex0 = sharding.BevExchange(self.plan, self.rank, self.device, (self.exchange.Y, self.exchange.X),
                                       share=self.exchange)
            if self.exchange.touched:
                ex0.adopt_touched(self.exchange)
            self.pipe = sharding.PipelinedExchange(self.plan, self.rank, self.device, (self.exchange.Y, self.exchange.X),
                                                   first=ex0)
        pipe = self.pipe
        cur, rendered = self._pool_and_render(inputs, pipe.pool_target)
        self._pipe_k += 1
        ob = self._hoa12(slot=self._pipe_k % 2)
        if pipe._comm is not None:
            for t in ob.values():
                t.record_stream(pipe._comm)
        full_prev = pipe.submit(between=lambda ex: self._gate(ex, ob))      # step k's exchange starts; step k - 1's grid is complete
        held, self._held = self._held, rendered
        self._join_renders(cur, rendered)
        if full_prev is None or held is None:
            return None
        return self._outputs(full_prev, held)

    def flush_pipelined(self):
        """-> the last step submitted by ``step_pipelined`` (None if nothing is pending)."""
        if self.pipe is None:
            return None
        held, self._held = self._held, None
        full = self.pipe.flush()
        if full is None or held is None:
            return None
        return self._outputs(full, held)

    def _set_busy(self, value):
        if self._busy is not None:
            _lib.launch('ocrf_stream_write_value32', self.device, self._busy, int(value))

    @property
    def bev_voxels_per_step(self):
        return bev_voxels(self.cfg, self.n_frames)
