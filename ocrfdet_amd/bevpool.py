"""BEVPoolv2 voxel pooling — the MI355X op behind the reference's ``bev_pool_v2``.

Public surface (identical names / argument order / tensor conventions to
``mmdet3d/ops/bev_pool_v2/bev_pool.py`` so the reference's import line is the only edit):

``bev_pool_v2(depth, feat, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape, interval_starts,
interval_lengths)``  -> ``(B, C, Z, Y, X)`` contiguous fp32                     [bev_pool.py:86-92]
    depth ``(B,N,D,H,W)`` any float dtype, feat ``(B,N,H,W,C)`` channels-last, 1-D integer ranks,
    ``bev_feat_shape = (B,Z,Y,X,C)``.  Differentiable w.r.t. depth and feat.  Empty voxels are 0.
``QuickCumsumCuda``   the autograd Function (returns the pre-permute ``(B,Z,Y,X,C)`` tensor)
                                                                                [bev_pool.py:11-83]
``TRTBEVPoolv2``      export shim with the ``mmdeploy::bev_pool_v2`` symbolic   [bev_pool.py:95-142]
``bev_pool_v2_ext``   object with ``bev_pool_v2_forward`` / ``bev_pool_v2_backward`` taking the
                      pybind module's argument order — ``interval_lengths`` BEFORE
                      ``interval_starts``                               [src/bev_pool.cpp:30-39,74-85]

Beyond the reference's surface: ``bev_pool_v2_collapsed`` and ``bev_pool_v2_device_counts[_autograd]`` (the fused tile
kernel, the latter on rank vectors whose lengths stay on the device), ``DevicePoolPlan`` / ``MfmaPoolPlan`` with
``bev_pool_v2_planned`` / ``bev_pool_v2_mfma`` / ``bev_pool_v2_panel`` for cached rank vectors, and ``PoolPlan``, which owns
cached rank vectors and is the one place that says which of those pools them (``PoolPlan.pool``).  Stated once for all
of them: the operand prologue with the 2 GiB refusal (``_fp32_operands``), the ``out=`` contract (``_out_tensor``), the
panel channel counts (``PANEL_CHANNELS``) and the backward (``_pool_backward``, behind ``QuickCumsumCuda`` and
``_FusedPool``).

All compute is in ``csrc/bev_pool*.hip`` behind the C ABI of ``include/ocrf_hip.h``.  There is no
CPU path: CPU tensors raise ``OcrfHipError``.
"""
import os

import torch

from . import _lib

__all__ = ['bev_pool_v2_device_counts', 'bev_pool_v2', 'bev_pool_v2_collapsed', 'TRTBEVPoolv2', 'QuickCumsumCuda',
           'bev_pool_v2_ext', 'runs_of', 'dense_runs']


def _want(t, dtype, name):
    if t.dtype != dtype or not t.is_contiguous():
        raise _lib.OcrfHipError(f'{name}: expected contiguous {dtype}, got {t.dtype} '
                                f'contiguous={t.is_contiguous()}')


def runs_of(sorted_ranks):
    """(starts, lengths) int32 of the runs of equal values in a sorted 1-D tensor — what
    view_transformer.py:245-252 and bev_pool.py:50-57 build with a boolean mask."""
    _, counts = torch.unique_consecutive(sorted_ranks, return_counts=True)
    ends = torch.cumsum(counts, 0)
    return (ends - counts).int(), counts.int()


def dense_runs(sorted_ranks, n_values):
    """(starts, lengths) int32 of the run of EVERY value 0..n_values-1 in a sorted 1-D tensor (length 0 where
    a value is absent).  Same runs as ``runs_of`` plus empty ones, but of a size the host knows: no
    device -> host read (``unique_consecutive`` has to return its count), so the backward of ``bev_pool_v2``
    does not stall the autograd thread.  The gradient kernels skip empty runs."""
    edges = torch.searchsorted(sorted_ranks, torch.arange(n_values + 1, device=sorted_ranks.device,
                                                          dtype=sorted_ranks.dtype))
    return edges[:-1].int(), (edges[1:] - edges[:-1]).int()


class _ExtensionAPI:
    """Call-compatible stand-in for the reference's pybind module (src/bev_pool.cpp:106-111)."""

    @staticmethod
    def bev_pool_v2_forward(depth, feat, out, ranks_depth, ranks_feat, ranks_bev,
                            interval_lengths, interval_starts):
        _lib.require_cuda(depth, feat, out, ranks_depth, ranks_feat, ranks_bev, interval_lengths,
                          interval_starts)
        for name, t in (('depth', depth), ('feat', feat), ('out', out)):
            _want(t, torch.float32, name)
        for name, t in (('ranks_depth', ranks_depth), ('ranks_feat', ranks_feat),
                        ('ranks_bev', ranks_bev), ('interval_lengths', interval_lengths),
                        ('interval_starts', interval_starts)):
            _want(t, torch.int32, name)
        channels = feat.size(4)                       # `c = _feat.size(4)`, bev_pool.cpp:40
        n_iv = interval_lengths.size(0)
        n_pts = ranks_depth.numel()
        if ranks_feat.numel() != n_pts or ranks_bev.numel() != n_pts or interval_starts.numel() != n_iv:
            raise _lib.OcrfHipError('rank / interval vectors disagree in length')
        dev = depth.device                         # launch() is the OptionalCUDAGuard, bev_pool.cpp:42
        if os.environ.get('OCRF_CHECK_INTERVALS', '0') == '1':
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.launch('ocrf_bev_pool_v2_check_intervals', dev, n_iv, n_pts, interval_starts, interval_lengths, flag)
            bad = int(flag.item())
            if bad:
                raise _lib.OcrfHipError(
                    f'intervals are not an ascending non-overlapping cover (flag={bad}); the '
                    'C entry point bev_pool_v2() accepts arbitrary layouts')
        n_vox = out.numel() // max(channels, 1)
        scratch = _lib.workspace.get(dev, _lib.lib().ocrf_bev_pool_v2_workspace_bytes(channels, n_pts, n_vox), 'bev_pool')
        _lib.launch('ocrf_bev_pool_v2', dev, channels, n_iv, n_pts, n_vox, depth, feat, ranks_depth, ranks_feat, ranks_bev,
                    interval_starts, interval_lengths, out, scratch, scratch.numel())

    @staticmethod
    def bev_pool_v2_backward(out_grad, depth_grad, feat_grad, depth, feat, ranks_depth,
                             ranks_feat, ranks_bev, interval_lengths, interval_starts):
        _lib.require_cuda(out_grad, depth_grad, feat_grad, depth, feat, ranks_depth, ranks_feat,
                          ranks_bev, interval_lengths, interval_starts)
        for name, t in (('out_grad', out_grad), ('depth_grad', depth_grad),
                        ('feat_grad', feat_grad), ('depth', depth), ('feat', feat)):
            _want(t, torch.float32, name)
        for name, t in (('ranks_depth', ranks_depth), ('ranks_feat', ranks_feat),
                        ('ranks_bev', ranks_bev), ('interval_lengths', interval_lengths),
                        ('interval_starts', interval_starts)):
            _want(t, torch.int32, name)
        channels = out_grad.size(4)                   # `c = _out_grad.size(4)`, bev_pool.cpp:86
        _lib.launch('ocrf_bev_pool_v2_grad', out_grad.device, channels, interval_lengths.size(0), out_grad, depth, feat,
                    ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths, depth_grad, feat_grad)


bev_pool_v2_ext = _ExtensionAPI()


PANEL_CHANNELS = (64, 80, 96, 128)      # channel counts csrc/bev_pool_mfma.hip / bev_pool_panel.hip are instantiated for


def _fusable(channels):
    return channels % 4 == 0 and 32 <= channels <= 256


def _panel_channels(channels):
    return channels in PANEL_CHANNELS


def _check_32bit_offsets(*tensors):
    """The tile / MFMA / panel pooling kernels address their operands, as fp32, with 32-bit byte offsets (raw buffer loads
    whose resource covers 2^31 - 1 bytes: a load beyond returns 0 silently).  An operand of 2 GiB or more is refused here,
    on its size alone."""
    for t in tensors:
        if t is not None and t.numel() * 4 >= (1 << 31):
            raise _lib.OcrfHipError(f'a pooling operand of {t.numel() * 4} bytes exceeds the 2 GiB the '
                                    'kernels\' 32-bit offsets cover: split the batch')


def _fp32_operands(*tensors, channels=None, said_by='the plan was built for'):
    """The operand prologue of every wrapper of those kernels: 2 GiB refused (before anything asks for the device),
    contiguous fp32, on the GPU, and — with ``channels`` — the last one a ``feat`` of that many channels."""
    _check_32bit_offsets(*tensors)
    ops = [t.float().contiguous() for t in tensors]
    _lib.require_cuda(*ops)
    if channels is not None and ops[-1].size(-1) != channels:
        raise _lib.OcrfHipError(f'feat has {ops[-1].size(-1)} channels, {said_by} {channels}')
    return ops


def _int32(*ranks):
    """dtype / contiguity normalisation of rank and interval vectors as bev_pool.py:19-25."""
    return tuple(t.int().contiguous() for t in ranks)


def _out_tensor(out, shape, layout, dev):
    """The ``out=`` contract: a new (B,C,Z,Y,X) (layout 0) / (B,Z*C,Y,X) tensor, or the caller's once it is contiguous fp32
    of that many elements on ``dev`` (e.g. a slice of a fused multi-frame buffer)."""
    B, Z, Y, X, C = shape
    if out is None:
        return torch.empty((B, C, Z, Y, X) if layout == 0 else (B, Z * C, Y, X), dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * C * Z * Y * X or out.device != dev:
        raise _lib.OcrfHipError('out must be a contiguous fp32 tensor of B*C*Z*Y*X elements on the inputs\' device')
    return out


def _pool_backward(grad_rows, d32, f32, rd, rf, rb, n_live=None):
    """The backward of every autograd surface -> (depth_grad, feat_grad).  ``grad_rows``: the upstream gradient as contiguous
    fp32 (B,Z,Y,X,C) rows.  The point list is regrouped by feature pixel (bev_pool.py:47-57), stably, so that runs of
    equal ranks_feat keep their forward order.  ``n_live``: device-side point count of rank vectors at their capacity; the
    entries past it (uninitialised) get a feature index past the last pixel first, so the stable sort puts them behind
    every run and no run covers them — and nothing is read back from the device."""
    n_pixels = f32.numel() // f32.size(-1)
    if n_live is not None:
        live = torch.arange(rf.numel(), device=rf.device, dtype=torch.int32) < n_live
        rf = torch.where(live, rf, torch.full_like(rf, n_pixels))
    rf_sorted, perm = torch.sort(rf, stable=True)
    starts_bp, lengths_bp = dense_runs(rf_sorted, n_pixels)
    g_depth = torch.zeros_like(d32)
    g_feat = torch.zeros_like(f32)
    bev_pool_v2_ext.bev_pool_v2_backward(grad_rows, g_depth, g_feat, d32, f32, rd[perm].contiguous(), rf_sorted.contiguous(),
                                         rb[perm].contiguous(), lengths_bp, starts_bp)
    return g_depth, g_feat


class QuickCumsumCuda(torch.autograd.Function):
    """Autograd wrapper with the reference's name and call signature (bev_pool.py:11-83)."""

    @staticmethod
    def forward(ctx, depth, feat, ranks_depth, ranks_feat, ranks_bev,
                bev_feat_shape, interval_starts, interval_lengths):
        rb, rd, rf, starts, lengths = _int32(ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths)
        d32 = depth.float().contiguous()
        f32 = feat.float().contiguous()
        pooled = f32.new_zeros(tuple(int(s) for s in bev_feat_shape))    # bev_pool.py:27
        bev_pool_v2_ext.bev_pool_v2_forward(d32, f32, pooled, rd, rf, rb, lengths, starts)
        ctx.save_for_backward(rb, d32, f32, rf, rd)
        return pooled

    @staticmethod
    def backward(ctx, grad_pooled):
        rb, d32, f32, rf, rd = ctx.saved_tensors
        return _pool_backward(grad_pooled.contiguous(), d32, f32, rd, rf, rb) + (None,) * 6


@torch.no_grad()
def bev_pool_v2_device_counts(depth, feat, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape,
                              interval_starts, interval_lengths, counts, layout=1, scratch_tag='bev_pool_nchw'):
    """Forward-only pooling on rank vectors whose lengths live on the device: the five vectors are
    passed at their CAPACITY (as ``index_prep.*_hip(sync=False)`` returns them) together with
    ``counts`` = int32 device tensor [n_points, n_intervals], so that nothing between the index
    preparation and the pooling reads the device.  ``layout`` as in ``_FusedPool``.  ``scratch_tag``: the call's scratch
    (voxel table, unit list, slabs) is one buffer per tag — two poolings that run at the same time on two streams need
    two tags."""
    B, Z, Y, X, C = (int(v) for v in bev_feat_shape)
    if not _fusable(C):
        raise _lib.OcrfHipError(f'bev_pool_v2_device_counts needs C % 4 == 0 and C <= 256, got {C}')
    d32, f32 = _fp32_operands(depth, feat)
    _lib.require_cuda(ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths, counts)
    for t in (ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths, counts):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise _lib.OcrfHipError('rank / interval / count vectors must be contiguous int32')
    cap_pts, cap_iv = ranks_depth.numel(), interval_starts.numel()
    dev = d32.device
    out = _out_tensor(None, (B, Z, Y, X, C), layout, dev)
    need = _lib.lib().ocrf_bev_pool_v2_nchw_workspace_bytes(C, cap_iv, cap_pts, B, Z, Y, X)
    scratch = _lib.workspace.get(dev, need, scratch_tag)
    _lib.launch('ocrf_bev_pool_v2_nchw_dyn', dev, C, cap_iv, cap_pts, counts, d32, f32, ranks_depth, ranks_feat, ranks_bev,
                interval_starts, interval_lengths, out, B, Z, Y, X, int(layout), scratch, scratch.numel())
    return out


class _FusedPool(torch.autograd.Function):
    """bev_pool_v2 + the reference's layout passes in one go: ``layout`` 0 -> (B,C,Z,Y,X) (bev_pool.py:91), 1 ->
    (B,Z*C,Y,X) (view_transformer.py:194).  The output is written exactly once (no zero-fill, no permute, no cat).
    ``counts`` None: exact rank vectors (C ABI ``ocrf_bev_pool_v2_nchw``); otherwise rank vectors whose LENGTHS LIVE ON THE
    DEVICE (``bev_pool_v2_device_counts``), so that a training forward reads nothing back.  One backward for both."""

    @staticmethod
    def forward(ctx, depth, feat, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape, interval_starts, interval_lengths,
                layout, counts, scratch_tag):
        B, Z, Y, X, C = shape = tuple(int(v) for v in bev_feat_shape)
        if counts is None:
            d32, f32 = _fp32_operands(depth, feat, channels=C, said_by='bev_feat_shape says')
            rb, rd, rf, starts, lengths = _int32(ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths)
            _lib.require_cuda(rb, rd, rf, starts, lengths)
            n_iv, n_pts = starts.numel(), rd.numel()
            if rf.numel() != n_pts or rb.numel() != n_pts or lengths.numel() != n_iv:
                raise _lib.OcrfHipError('rank / interval vectors disagree in length')
            dev = d32.device
            out = _out_tensor(None, shape, layout, dev)
            need = _lib.lib().ocrf_bev_pool_v2_nchw_workspace_bytes(C, n_iv, n_pts, B, Z, Y, X)
            scratch = _lib.workspace.get(dev, need, scratch_tag)
            _lib.launch('ocrf_bev_pool_v2_nchw', dev, C, n_iv, n_pts, d32, f32, rd, rf, rb, starts, lengths, out, B, Z, Y, X,
                        int(layout), scratch, scratch.numel())
        else:
            d32, f32 = _fp32_operands(depth, feat)
            rb, rd, rf = ranks_bev, ranks_depth, ranks_feat
            out = bev_pool_v2_device_counts(d32, f32, rd, rf, rb, shape, interval_starts, interval_lengths, counts,
                                            layout=layout, scratch_tag=scratch_tag)
        ctx.save_for_backward(rb, d32, f32, rf, rd, counts)
        ctx.geom = shape + (int(layout),)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        rb, d32, f32, rf, rd, counts = ctx.saved_tensors
        B, Z, Y, X, C, layout = ctx.geom
        if layout == 0:
            g = grad_out.permute(0, 2, 3, 4, 1)                       # (B,Z,Y,X,C)
        else:
            g = grad_out.view(B, Z, C, Y, X).permute(0, 1, 3, 4, 2)
        return _pool_backward(g.contiguous().float(), d32, f32, rd, rf, rb,
                              n_live=None if counts is None else counts[0]) + (None,) * 9


def bev_pool_v2(depth, feat, ranks_depth, ranks_feat, ranks_bev,
                bev_feat_shape, interval_starts, interval_lengths):
    """The reference's op: -> (B, C, Z, Y, X) contiguous fp32 (bev_pool.py:86-92)."""
    if _fusable(int(bev_feat_shape[-1])):
        return _FusedPool.apply(depth, feat, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape,
                                interval_starts, interval_lengths, 0, None, 'bev_pool_nchw')
    pooled = QuickCumsumCuda.apply(depth, feat, ranks_depth, ranks_feat, ranks_bev,
                                   bev_feat_shape, interval_starts, interval_lengths)
    return pooled.permute(0, 4, 1, 2, 3).contiguous()        # (B,Z,Y,X,C) -> (B,C,Z,Y,X)


def bev_pool_v2_device_counts_autograd(depth, feat, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape, interval_starts,
                                       interval_lengths, counts, layout=1, scratch_tag='bev_pool_nchw'):
    """``bev_pool_v2_device_counts`` with autograd for ``depth`` and ``feat`` (``_FusedPool`` with ``counts``)."""
    return _FusedPool.apply(depth, feat, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape, interval_starts,
                            interval_lengths, int(layout), counts, scratch_tag)


class DevicePoolPlan:
    """The rank-only part of one pooling, built once for rank vectors that are cached across calls
    (C ABI ``ocrf_bev_pool_plan_build``): the dense voxel table, the list of work units (tiles, and slices
    of heavy tiles) and their split over the XCDs.  ``bev_pool_v2_planned`` is then ONE launch that needs
    only depth, feat, ranks_depth and ranks_feat.  Forward only; a plan serves one stream at a time (it
    holds the arrival counters of the cut tiles)."""

    def __init__(self, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape, interval_starts, interval_lengths):
        _lib.require_cuda(ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths)
        B, Z, Y, X, C = (int(v) for v in bev_feat_shape)
        if not _fusable(C):
            raise _lib.OcrfHipError(f'pool plans need C % 4 == 0 and C <= 256, got {C}')
        self.shape = (B, Z, Y, X, C)
        self.ranks_depth, self.ranks_feat, rb, st, ln = _int32(ranks_depth, ranks_feat, ranks_bev, interval_starts,
                                                               interval_lengths)
        self.n_points, self.n_intervals = self.ranks_depth.numel(), st.numel()
        dev = rb.device
        L = _lib.lib()
        self.plan = torch.empty(L.ocrf_bev_pool_plan_bytes(C, self.n_points, B, Z, Y, X), dtype=torch.uint8, device=dev)
        _lib.launch('ocrf_bev_pool_plan_build', dev, C, self.n_intervals, self.n_points, rb, st, ln, B, Z, Y, X, self.plan,
                    self.plan.numel())
        # the slabs of cut tiles: owned by the plan (its lifetime, not the process-wide grow-only workspace), so a
        # plan can run beside another plan's launch and a dropped plan returns its memory
        self.scratch = torch.empty(max(int(L.ocrf_bev_pool_planned_workspace_bytes(C, self.n_points)), 256),
                                   dtype=torch.uint8, device=dev)


@torch.no_grad()
def bev_pool_v2_planned(depth, feat, plan, layout=1, out=None):
    """``bev_pool_v2_collapsed`` (layout 1: (B, Z*C, Y, X)) or ``bev_pool_v2`` (layout 0: (B,C,Z,Y,X)) for the
    rank vectors a ``DevicePoolPlan`` was built from; bit-identical results.  ``out``: see ``_out_tensor``."""
    B, Z, Y, X, C = plan.shape
    d32, f32 = _fp32_operands(depth, feat, channels=C)
    dev = d32.device
    out = _out_tensor(out, plan.shape, layout, dev)
    _lib.launch('ocrf_bev_pool_v2_nchw_planned', dev, C, plan.n_points, d32, f32, plan.ranks_depth, plan.ranks_feat,
                plan.plan, out, B, Z, Y, X, int(layout), plan.scratch, plan.scratch.numel(), d32.numel() * 4,
                f32.numel() * 4)
    return out


class MfmaPoolPlan:
    """Rank-only part of the MFMA panel pooling (csrc/bev_pool_mfma.hip): per 64-voxel tile its UNIQUE feature rows in
    panels of 64, per panel its non-zero (voxel slot, row slot) cells with their points in summation order, and the
    unit list (a tile's panels in groups of at most ``group``; heaviest units first; tiles of several units reduce
    through slabs).  Built once per calibration from the rank vectors with device-side torch index algebra (sort /
    unique / searchsorted — plan time, not step time); every point of the rank vectors is pooled into
    ``ranks_bev[p]`` (what the reference's intervals amount to when they cover the point list: bev_pool.py:40-57).
    A non-finite value in a REFERENCED feature row or depth entry spreads over its whole tile in the dense W . F form
    (0 * inf = NaN), by construction; rows and entries that no kept point references are never read into a sum."""

    def __init__(self, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape, group=4, unit_cost=None):
        _lib.require_cuda(ranks_depth, ranks_feat, ranks_bev)
        B, Z, Y, X, C = (int(v) for v in bev_feat_shape)
        if not _panel_channels(C):
            raise _lib.OcrfHipError(f'the MFMA pooling takes C in {PANEL_CHANNELS}, got {C}')
        self.shape = (B, Z, Y, X, C)
        dev = ranks_bev.device
        L = _lib.lib()
        KP = int(L.ocrf_bev_pool_mfma_panel_rows())
        TS = int(L.ocrf_bev_pool_mfma_tile_side())
        YX, TV = Y * X, TS * TS
        tcx, tcy = (X + TS - 1) // TS, (Y + TS - 1) // TS
        tpp = tcx * tcy
        n_tiles = B * Z * tpp
        rb, rf, rd = ranks_bev.long(), ranks_feat.long(), ranks_depth.long()
        keep = (rb >= 0) & (rb < B * Z * YX)
        rb, rf, rd = rb[keep], rf[keep], rd[keep]
        self.n_points = int(rb.numel())
        i32 = lambda t: t.to(torch.int32).contiguous()  # noqa: E731
        if self.n_points:
            plane, inpl = rb // YX, rb % YX
            y, x = inpl // X, inpl % X
            tile, v = plane * tpp + (y // TS) * tcx + x // TS, (y % TS) * TS + x % TS
            n_rows = int(rf.max()) + 1
            key = (tile * n_rows + rf) * TV + v
            order = torch.argsort(key, stable=True)                 # points of a cell stay in list order
            key_s = key[order]
            first = torch.ones_like(key_s, dtype=torch.bool)
            first[1:] = key_s[1:] != key_s[:-1]
            cell_start = torch.nonzero(first).flatten()
            cell_key = key_s[cell_start]
            cell_pair, cell_v = cell_key // TV, cell_key % TV
            pfirst = torch.ones_like(cell_pair, dtype=torch.bool)
            pfirst[1:] = cell_pair[1:] != cell_pair[:-1]
            pair_of_cell = torch.cumsum(pfirst.long(), 0) - 1
            pair_key = cell_pair[pfirst]
            pair_tile, pair_rf = pair_key // n_rows, pair_key % n_rows
            tiles = torch.arange(n_tiles + 1, device=dev)
            tile_pair_start = torch.searchsorted(pair_tile, tiles)                # first pair of every tile
            rslot = torch.arange(pair_key.numel(), device=dev) - tile_pair_start[pair_tile]
            n_pan_tile = (tile_pair_start[1:] - tile_pair_start[:-1] + KP - 1) // KP
        else:
            n_pan_tile = torch.zeros(n_tiles, dtype=torch.long, device=dev)
        tile_panel_off = torch.cumsum(n_pan_tile, 0) - n_pan_tile
        n_panels = int(n_pan_tile.sum())
        if self.n_points:
            pair_panel = tile_panel_off[pair_tile] + rslot // KP
            pair_r = rslot % KP
            panel_rows = torch.zeros(max(n_panels, 1) * KP, dtype=torch.long, device=dev)
            panel_rows[pair_panel * KP + pair_r] = pair_rf
            panel_nrows = torch.bincount(pair_panel, minlength=max(n_panels, 1))
            cell_panel = pair_panel[pair_of_cell]
            panel_cell_off = torch.searchsorted(cell_panel, torch.arange(n_panels + 1, device=dev))
            rd_sorted = rd[order]
            cell_end = torch.cat((cell_start[1:], torch.tensor([self.n_points], device=dev)))
            npts = cell_end - cell_start
            code = cell_v | (pair_r[pair_of_cell] << 8)
            # cells of a panel voxel-major (v, then row slot): bev_pool_panel.hip walks a voxel's cells in row order —
            # the k order of the MFMA form, which itself does not depend on the order inside a panel
            vm = torch.argsort((cell_panel * TV + cell_v) * KP + pair_r[pair_of_cell])
            cell_start, cell_end, npts, code, cell_v = cell_start[vm], cell_end[vm], npts[vm], code[vm], cell_v[vm]
            # voxel slot v of panel p owns the cells [voff[p][v], voff[p][v + 1]) (relative to the panel's first cell)
            panel_voff = torch.searchsorted(cell_panel * TV + cell_v, torch.arange(n_panels * TV, device=dev)) - \
                torch.repeat_interleave(panel_cell_off[:-1], TV)
            cell_code = ((code >> 8) | ((code & 0xFF) << 8)).to(torch.int16).contiguous()      # row slot | voxel slot << 8 (< 2^14)
            last = self.n_points - 1
            inline = npts <= 3
            rd0 = rd_sorted[cell_start]
            rd1 = rd_sorted[torch.clamp(cell_start + 1, max=last)]
            rd2 = rd_sorted[torch.clamp(cell_start + 2, max=last)]
            cells = torch.stack((code | (torch.where(inline, npts, torch.full_like(npts, 0xFFFF)) << 16),
                                 torch.where(inline, rd0, cell_start), torch.where(inline, rd1, npts),
                                 torch.where(inline, rd2, torch.zeros_like(rd2))), 1)
        else:
            panel_rows = torch.zeros(KP, dtype=torch.long, device=dev)
            panel_nrows = torch.zeros(1, dtype=torch.long, device=dev)
            panel_cell_off = torch.zeros(2, dtype=torch.long, device=dev)
            panel_voff = torch.zeros(TV, dtype=torch.long, device=dev)
            cell_code = torch.zeros(1, dtype=torch.int16, device=dev)
            cells = torch.zeros(1, 4, dtype=torch.long, device=dev)
            rd_sorted = torch.zeros(1, dtype=torch.long, device=dev)
        # units: consecutive panels of a tile, at most `group` of them and — with `unit_cost` — about that much estimated
        # time (cost of a panel = 1 + its longest voxel run / 8: what a panel of bev_pool_panel.hip takes, its row fetch
        # plus one trip per cell of the longest run); a tile without points is one unit without panels.  The few
        # tiles beside the rig (hundreds of rows, runs of 30-48 cells) are cut finely, the ordinary ones not at all.
        G = max(1, min(int(group), int(L.ocrf_bev_pool_mfma_max_unit_panels())))
        tiles_i = torch.arange(n_tiles, device=dev)
        if self.n_points and n_panels:
            pan_tile = torch.repeat_interleave(tiles_i, n_pan_tile)
            pan_idx = torch.arange(n_panels, device=dev) - tile_panel_off[pan_tile]          # index of the panel in its tile
            if unit_cost is not None:
                ends = torch.cat((panel_voff.reshape(n_panels, TV), (panel_cell_off[1:] - panel_cell_off[:-1])[:, None]), 1)
                longest = (ends[:, 1:] - ends[:, :-1]).max(1).values
                cost = 1.0 + longest.double() / 8.0
                cum = torch.cumsum(cost, 0)
                excl = cum - cost
                excl = excl - excl[tile_panel_off[pan_tile]]                                   # exclusive prefix inside the tile
                bucket = torch.floor(excl / float(unit_cost)).long()
            else:
                bucket = torch.zeros(n_panels, dtype=torch.long, device=dev)
            # a new unit starts where the bucket changes, and every G panels inside a bucket
            bfirst = torch.ones(n_panels, dtype=torch.bool, device=dev)
            bfirst[1:] = (bucket[1:] != bucket[:-1]) | (pan_tile[1:] != pan_tile[:-1])
            bstart = torch.cummax(torch.where(bfirst, torch.arange(n_panels, device=dev), torch.zeros_like(pan_idx)), 0).values
            ufirst = bfirst | ((torch.arange(n_panels, device=dev) - bstart) % G == 0)
            unit_p0 = torch.nonzero(ufirst).flatten()
            unit_p1 = torch.cat((unit_p0[1:], torch.tensor([n_panels], device=dev)))
            unit_tile_np = pan_tile[unit_p0]
            n_unit_tile = torch.bincount(unit_tile_np, minlength=n_tiles)
            empty = n_unit_tile == 0
            # empty tiles: one unit without panels each
            e_tiles = tiles_i[empty]
            unit_tile = torch.cat((unit_tile_np, e_tiles))
            p0 = torch.cat((unit_p0, torch.zeros_like(e_tiles)))
            p1 = torch.cat((unit_p1, torch.zeros_like(e_tiles)))
            first_unit_of_tile = torch.searchsorted(unit_tile_np, tiles_i)
            slice_ = torch.cat((torch.arange(unit_p0.numel(), device=dev) - first_unit_of_tile[unit_tile_np], torch.zeros_like(e_tiles)))
            n_unit_tile = torch.clamp(n_unit_tile, min=1)
        else:
            n_unit_tile = torch.ones(n_tiles, dtype=torch.long, device=dev)
            unit_tile, p0, p1, slice_ = tiles_i, torch.zeros_like(tiles_i), torch.zeros_like(tiles_i), torch.zeros_like(tiles_i)
        multi = n_unit_tile > 1
        slab_first = torch.cumsum(torch.where(multi, n_unit_tile, torch.zeros_like(n_unit_tile)), 0) - \
            torch.where(multi, n_unit_tile, torch.zeros_like(n_unit_tile))
        self.n_slab_slices = int(torch.where(multi, n_unit_tile, torch.zeros_like(n_unit_tile)).sum())
        units = torch.stack((unit_tile, p0, p1, slice_ | (n_unit_tile[unit_tile] << 16)), 1)
        heavy_first = torch.argsort(p1 - p0, descending=True, stable=True)
        self.units = i32(units[heavy_first])
        self.unit_slab = i32(slab_first[unit_tile][heavy_first])
        self.n_units = int(self.units.size(0))
        self.panel_rows, self.panel_nrows, self.panel_cell_off = i32(panel_rows), i32(panel_nrows), i32(panel_cell_off)
        self.cells, self.rd_sorted = i32(cells), i32(rd_sorted)
        self.panel_voff, self.cell_code = i32(panel_voff), cell_code
        self.cw = torch.zeros(int(cells.size(0)), dtype=torch.float32, device=dev)      # bev_pool_cell_weights' output
        self.n_panels, self.n_cells, self.n_tiles = n_panels, int(cells.size(0)), n_tiles
        self.unique_rows = int(panel_nrows.sum()) if self.n_points else 0
        self.arrive = torch.zeros(n_tiles, dtype=torch.int32, device=dev)
        self.slabs = torch.empty(int(L.ocrf_bev_pool_mfma_slab_bytes(C, self.n_slab_slices)), dtype=torch.uint8, device=dev)


@torch.no_grad()
def bev_pool_v2_mfma(depth, feat, plan, layout=1, out=None):
    """The pooling of ``plan``'s rank vectors on the matrix cores: (B, Z*C, Y, X) (layout 1) or (B,C,Z,Y,X)
    (layout 0); same result as ``bev_pool_v2_planned`` up to the summation order."""
    B, Z, Y, X, C = plan.shape
    d32, f32 = _fp32_operands(depth, feat, channels=C)
    dev = d32.device
    out = _out_tensor(out, plan.shape, layout, dev)
    _lib.launch('ocrf_bev_pool_v2_nchw_mfma', dev, C, plan.n_units, plan.units, plan.unit_slab, plan.panel_rows,
                plan.panel_nrows, plan.panel_cell_off, plan.cells, plan.rd_sorted, d32, f32, out, B, Z, Y, X, int(layout),
                plan.arrive, plan.slabs)
    return out


@torch.no_grad()
def bev_pool_cell_weights(depth, plan, plan2=None):
    """Pre-pass of ``bev_pool_v2_panel``: the summed depth weight of every cell of ``plan`` (and of ``plan2`` — the LSS
    and the height-sampling plan of a step read the same depth tensor) in ONE launch -> ``plan.cw`` (``plan2.cw``)."""
    d32, = _fp32_operands(depth)
    n2 =plan2.n_cells if (plan2 is not None and plan2.n_points) else 0
    n1 = plan.n_cells if plan.n_points else 0
    _lib.launch('ocrf_bev_pool_cell_weights', d32.device, n1, plan.cells, plan.rd_sorted, plan.cw,
                n2, plan2.cells if n2 else None, plan2.rd_sorted if n2 else None, plan2.cw if n2 else None, d32)
    return d32


@torch.no_grad()
def bev_pool_v2_panel(depth, feat, plan, layout=1, out=None, weights_ready=False, stats=None):
    """The pooling of ``plan``'s rank vectors cell by cell out of LDS (csrc/bev_pool_panel.hip): same plan and same
    result as ``bev_pool_v2_mfma`` (bit for bit on finite inputs).  ``weights_ready``: ``bev_pool_cell_weights`` has
    already run for this ``depth`` on this stream (one launch for both poolings of a step).  ``stats``: contiguous fp32
    (B, 2, Y, X) tensor (Z == 1, layout 0 or 1) that the same launch fills with the output's channel mean and max, every
    pixel of it — the bits of ``hoa.channel_stats(out)`` without its pass over the BEV
    (``ocrf_bev_pool_v2_nchw_panel_stats``)."""
    B, Z, Y, X, C = plan.shape
    f32, = _fp32_operands(feat, channels=C)
    if not weights_ready:
        bev_pool_cell_weights(depth, plan)
    dev = f32.device
    out = _out_tensor(out, plan.shape, layout, dev)
    args =(C, plan.n_units, plan.units, plan.unit_slab, plan.panel_rows, plan.panel_nrows, plan.panel_cell_off,
            plan.panel_voff, plan.cell_code, plan.cw, f32, out, B, Z, Y, X, int(layout), plan.arrive, plan.slabs, f32.numel() * 4)
    if stats is None:
        _lib.launch('ocrf_bev_pool_v2_nchw_panel', dev, *args)
        return out
    if Z != 1 or int(layout) not in (0, 1):
        raise _lib.OcrfHipError('channel statistics come with a pooling of Z == 1 in layout 0 or 1')
    if (not torch.is_tensor(stats) or stats.dtype != torch.float32 or not stats.is_contiguous()
            or tuple(stats.shape) != (B, 2, Y, X) or stats.device != dev):
        raise _lib.OcrfHipError('stats must be a contiguous fp32 (B, 2, Y, X) tensor on the inputs\' device')
    _lib.launch('ocrf_bev_pool_v2_nchw_panel_stats', dev, *args, stats)
    return out


def bev_pool_v2_collapsed(depth, feat, ranks_depth, ranks_feat, ranks_bev,
                          bev_feat_shape, interval_starts, interval_lengths):
    """``torch.cat(bev_pool_v2(...).unbind(dim=2), 1)`` -> (B, Z*C, Y, X), the tensor
    ``voxel_pooling_v2`` / ``fast_sampling`` hand on (view_transformer.py:190-195,
    view_transformer_ocrf.py:776-782), produced without the intermediate copies."""
    if _fusable(int(bev_feat_shape[-1])):
        return _FusedPool.apply(depth, feat, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape,
                                interval_starts, interval_lengths, 1, None, 'bev_pool_nchw')
    x = bev_pool_v2(depth, feat, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape,
                    interval_starts, interval_lengths)
    return torch.cat(x.unbind(dim=2), 1)


def panel_plan_args(which, backend, lss_mfma_group=2):
    """``MfmaPoolPlan``'s unit arguments for the rank vectors of branch ``which`` ('lss' | 'ht').  The height-sampling ranks have
    no heavy tiles (11 points per feature row and 8 x 8 tile): units of up to 8 panels.  The LSS ranks do (the block
    beside the rig): units cut by estimated cost for the panel kernel, short units for the MFMA kernel, more slabs."""
    if which == 'ht':
        return dict(group=8)
    return dict(group=8, unit_cost=8.0) if backend == 'panel' else dict(group=lss_mfma_group)


class PoolPlan:
    """Rank vectors of one bev_pool_v2 call, cached on the device, and the one statement of how such vectors are pooled
    (``pool``): the rank-only half of the pooling is cached with them, built on first use."""

    def __init__(self, ranks_bev, ranks_depth, ranks_feat, starts, lengths, bev_shape):
        self.ranks_bev, self.ranks_depth, self.ranks_feat = ranks_bev, ranks_depth, ranks_feat
        self.starts, self.lengths = starts, lengths
        self.bev_shape = tuple(int(v) for v in bev_shape)      # (B, Z, Y, X, C)
        self.device_plan = None                                # DevicePoolPlan, built on first use
        self.mfma_plan = None                                  # MfmaPoolPlan, built on first use

    @property
    def n_points(self):
        return int(self.ranks_bev.numel())

    @property
    def n_intervals(self):
        return int(self.starts.numel())

    def algorithmic_bytes(self, depth_numel, feat_numel):
        """4*(depth + feat + 3*Np + 2*Nv + B*Z*Y*X*C)."""
        out = 1
        for v in self.bev_shape:
            out *= v
        return 4 * (depth_numel + feat_numel + 3 * self.n_points + 2 * self.n_intervals + out)

    def route(self, backend):
        """The kernel that pools these vectors when ``backend`` ('tile' | 'mfma' | 'panel') is asked for: 'unplanned'
        without points, the tile kernel where the channel count is not a panel count."""
        if not self.ranks_bev.numel():
            return 'unplanned'
        return backend if backend != 'tile' and _panel_channels(self.bev_shape[-1]) else 'tile'

    def writes_stats(self, backend, layout=1):
        """Whether that pooling can write the channel statistics (``bev_pool_v2_panel(..., stats=...)``)."""
        return self.route(backend) == 'panel' and self.bev_shape[1] == 1 and layout in (0, 1)

    def panel_plan(self, which, backend, lss_mfma_group=2):
        """The ``MfmaPoolPlan`` of the MFMA / panel kernels: built once, with the arguments in force at its first use."""
        if self.mfma_plan is None:
            self.mfma_plan = MfmaPoolPlan(self.ranks_depth, self.ranks_feat, self.ranks_bev, self.bev_shape,
                                          **panel_plan_args(which, backend, lss_mfma_group))
        return self.mfma_plan

    def pool(self, depth, feat, backend, which=None, lss_mfma_group=2, out=None, weights_ready=False, stats=None):
        """-> (B, Z*C, Y, X): pooled BEV with Z collapsed into channels (view_transformer.py:194).  ``which`` /
        ``lss_mfma_group``: see ``panel_plan_args``; ``out`` / ``weights_ready`` / ``stats`` as in ``bev_pool_v2_panel``.
        The panel plan: unique feature rows of an 8 x 8 tile in panels of 48, cells = (voxel, row) pairs.  'panel': cells
        walked out of LDS after a weight pre-pass (csrc/bev_pool_panel.hip); 'mfma': dense W . F panels on the matrix
        cores (csrc/bev_pool_mfma.hip)."""
        route = self.route(backend)
        if stats is not None and not self.writes_stats(backend):
            raise _lib.OcrfHipError('only the panel pooling (of Z == 1) writes channel statistics')
        if route == 'unplanned':
            res = bev_pool_v2_collapsed(depth, feat, self.ranks_depth, self.ranks_feat, self.ranks_bev, self.bev_shape,
                                        self.starts, self.lengths)
            if out is not None:
                out.view_as(res).copy_(res)
            return res
        if route == 'tile':
            if self.device_plan is None:
                self.device_plan = DevicePoolPlan(self.ranks_depth, self.ranks_feat, self.ranks_bev, self.bev_shape,
                                                  self.starts, self.lengths)
            return bev_pool_v2_planned(depth, feat, self.device_plan, out=out)
        plan = self.panel_plan(which, backend, lss_mfma_group)
        if route == 'mfma':
            return bev_pool_v2_mfma(depth, feat, plan, out=out)
        return bev_pool_v2_panel(depth, feat, plan, out=out, weights_ready=weights_ready, stats=stats)


class TRTBEVPoolv2(torch.autograd.Function):
    """Export shim (bev_pool.py:95-142): depth (N,D,H,W), feat (N,H,W,C) -> (1,Y,X,C)."""

    @staticmethod
    def symbolic(g, depth, feat, ranks_depth, ranks_feat, ranks_bev, interval_starts,
                 interval_lengths, out_height=128, out_width=128):
        return g.op('mmdeploy::bev_pool_v2', depth, feat, ranks_depth, ranks_feat, ranks_bev,
                    interval_starts, interval_lengths,
                    out_height_i=out_height, out_width_i=out_width)

    @staticmethod
    def forward(g, depth, feat, ranks_depth, ranks_feat, ranks_bev, interval_starts,
                interval_lengths, out_height=128, out_width=128):
        shape = (1, 1, out_height, out_width, feat.shape[-1])                  # (B,Z,Y,X,C)
        bev = bev_pool_v2(depth[None], feat[None], ranks_depth, ranks_feat, ranks_bev, shape,
                          interval_starts, interval_lengths)
        return bev.squeeze(2).permute(0, 2, 3, 1)
