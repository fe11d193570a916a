"""What ``OcRFViewTransformerFull`` derives from the calibration alone (``Geometry``, built by ``build_geometry`` in one of
four ``Mode``s), and how a forward's random camera choice reaches the device (``stage_cameras`` through a ``PinnedRing``)."""
import math
from typing import NamedTuple

import torch

from . import gaussian_renderer, index_prep
from .diff_gaussian_rasterization import pack_cameras

CALIB = (1, 2, 3, 4, 5, 6, 11)          # the seven calibration tensors among the 12 ``img_inputs``


def calib_on_device(input):
    return all(torch.is_tensor(input[i]) and input[i].is_cuda for i in CALIB)


def to_host(tensors):
    """float32 host copies of the calibration tensors.  Device tensors leave in ONE packed read-back (the reference reads
    them one by one, :1086-1088; each read is a device synchronisation); host tensors pass through untouched — a caller
    that still has the dataloader's host copies can hand those in and the forward does not synchronise at all."""
    ts = [t.detach().float() for t in tensors]
    on_dev = [t for t in ts if t.is_cuda]
    if len(on_dev) > 1:
        flat = torch.cat([t.reshape(-1) for t in on_dev]).cpu()
        parts = iter(flat.split([t.numel() for t in on_dev]))
        return [next(parts).view(t.shape) if t.is_cuda else t for t in ts]
    return [t.cpu() for t in ts]


class Mode(NamedTuple):
    """How the rank vectors of one ``Geometry`` are made."""
    sync: bool          # trimmed to host-known lengths (one device read); False: at capacity, lengths on the device
    lazy: bool          # left to ``geo.rank_vectors``: the eval schedule makes them on the poolings' own strand, behind
                        # the fork of the colour / NeRF strand (which needs only the projections) instead of in front of it
    persistent: bool    # written into the module's persistent ``_rank_bufs`` instead of tensors of this call
    # ``persistent`` is a soundness rule.  Synchronised ranks and a training forward's device-side ranks reach autograd
    # Functions that save them for the backward (``QuickCumsumCuda`` / ``_FusedPool``; ``.int().contiguous()`` is a no-op on
    # them): a later forward of the same module before that backward (adjacent frame, second view, eval hook) must not
    # overwrite them, and a cached geometry outlives every later forward.  Only forward-only ranks, which nobody keeps, may.


CACHED = Mode(sync=True, lazy=False, persistent=False)       # the cached geometry of ``accelerate`` (``pre_compute``)
AUTOGRAD = Mode(sync=True, lazy=False, persistent=False)     # host-synchronised ranks for autograd
FORWARD = Mode(sync=False, lazy=True, persistent=True)       # forward-only ranks at capacity
CAPACITY = Mode(sync=False, lazy=False, persistent=False)    # device-side ranks of a training forward


def choose_mode(accelerate, fused, device_geometry, on_device):
    """The mode of a geometry that ``view_transform_core`` has to build; with ``accelerate`` and a cached geometry it
    builds none.  ``fused``: eval mode with nothing recorded by autograd; ``on_device``: ``calib_on_device``.

        accelerate  fused  device_geometry, calibration     mode      calibration algebra
        False       yes    any                              FORWARD   device if on the GPU and not False, else host
        False       no     not False and on the GPU         CAPACITY  device
        False       no     False, or on the host            AUTOGRAD  host
        True        any    any (``pre_compute``)            CACHED    host
        True, core called before pre_compute: as with False, except that FORWARD becomes CAPACITY and CAPACITY AUTOGRAD

    The algebra runs on the device (``ocrf_geometry_blocks``: ~1 ulp from the host formulation, whose rank vectors are the
    reference's bit for bit) exactly when the mode does not synchronise, the calibration is on the GPU and
    ``device_geometry`` is not False: with the default ``None``, whenever the calibration arrives there."""
    if fused:
        return CAPACITY if accelerate else FORWARD
    return CAPACITY if (device_geometry is not False and on_device and not accelerate) else AUTOGRAD


class Geometry:
    """Everything ``view_transform_core`` derives from the calibration alone: both rank-vector sets,
    voxel centres, pillar projections and their validity (view_transformer.py:108-147,197-255;
    view_transformer_ocrf.py:651-740,785-852)."""

    def __init__(self):
        self.calib = self.c2w = None                # host formulation: the six host calibration tensors, cam2world
        self.cam_rows = {}                          # host cache: (sample, camera) -> packed (1,36) rasteriser row
        self.cam_rows_dev = None                    # device formulation: the (B,N,36) rows of every camera-frame
        self.pix = self.mask = self.voxel = None
        self.lss = self.ht = None                   # rank vectors; None until ``rank_vectors`` ran (lazy mode)
        self.rank_vectors = None                    # lazy mode: {'lss': f, 'ht': f}, f() -> that rank-vector set
        self.plans = {}                             # cached geometry: 'lss' / 'ht' -> bevpool.PoolPlan
        self.raster_plan = None                     # cached geometry: (RasterPlan, view offsets); False: not eligible

    def cam_row(self, bs, c, input_size, znear, zfar):
        """The rasteriser's packed host row of camera ``c`` of sample ``bs``, made once, from the ``data`` dict of the render call
        (:1135-1152), quirks included: unscaled intrinsics, network-input viewport, ``c2w`` where world->view is expected."""
        row = self.cam_rows.get((bs, c))
        if row is None:
            H, W = input_size
            cam = gaussian_renderer.camera_from_calibration(self.calib[2][bs, c].numpy(), self.c2w[bs, c].numpy(), H, W,
                                                            znear=znear, zfar=zfar)
            row = self.cam_rows[(bs, c)] = pack_cameras(
                cam['world_view_transform'][None], cam['full_proj_transform'][None],
                math.tan(float(cam['FovX']) * 0.5), math.tan(float(cam['FovY']) * 0.5), H, W, 'cpu')
        return row


def build_geometry(m, input, mode):
    """-> ``Geometry`` of the calibration in ``input`` for the neck ``m`` (its grid settings, templates and rank buffers)."""
    x, calib = input[0], [input[i] for i in CALIB]
    dev = x.device
    B, N, _, Hf, Wf = x.shape
    geo = Geometry()
    if m.device_geometry is not False and not mode.sync and calib_on_device(input):
        # the tiny per-camera algebra on the GPU too: nothing in the forward reads the device or waits for it
        lss_block, ht_block, geo.cam_rows_dev = index_prep.geometry_blocks_hip(*calib, m.input_size, m.znear, m.zfar)
    else:
        # the per-camera 3x3 algebra on the host, as the same torch calls the reference makes (a handful of (B,N,3,3)
        # tensors; the reference moves them to the host itself, :1086-1088)
        host = to_host(calib)
        geo.calib, geo.c2w = host[:6], host[6]
        lss_block = index_prep.lss_camera_block(*geo.calib).to(dev)
        lidar2img, img_aug, _, _ = index_prep.get_projection(*geo.calib)
        ht_block = index_prep.ht_camera_block(lidar2img, img_aug).to(dev)
    frustum, tmpl = m._templates(dev)
    lss_bufs, ht_bufs = m._rank_bufs if mode.persistent else (None, None)
    rank_vectors = dict(
        lss=lambda: index_prep.voxel_pooling_prepare_v2_hip(
            frustum, lss_block, B, N, m.grid_lower_bound, m.grid_interval, m.grid_size, buffers=lss_bufs, sync=mode.sync),
        ht=lambda: index_prep.fast_sample_prepare_hip(
            tmpl, ht_block, B, N, list(m.pc_range), m.input_size, m.grid_config['depth'], Wf, Hf, m.D, buffers=ht_bufs,
            sync=mode.sync))
    geo.pix, geo.mask, geo.voxel = index_prep.ht_project_hip(tmpl, ht_block, B, N, list(m.pc_range), m.input_size,
                                                             m.grid_config['depth'])
    if mode.lazy:
        geo.rank_vectors = rank_vectors
    else:
        geo.lss, geo.ht = rank_vectors['lss'](), rank_vectors['ht']()
    return geo


class PinnedRing:
    """``slots`` pinned host buffers of ``numel`` elements for small asynchronous host -> device copies (out of pageable memory
    such a copy blocks the host until the stream reaches it, or may still be reading a temporary that is gone), each guarded by
    an event so that it is not rewritten while its copy is in flight.  Never module state: see the two owners."""

    def __init__(self, slots, numel, dtype):
        self.slots = [[torch.empty(numel, dtype=dtype).pin_memory(), None] for _ in range(slots)]
        self.next = 0

    def put(self, host_values, device, out=None):
        """-> ``out`` (default: a fresh device tensor) with the copy of the 1-D ``host_values`` under way."""
        slot = self.slots[self.next]
        self.next = (self.next + 1) % len(self.slots)
        if slot[1] is not None:
            slot[1].synchronize()
        n = host_values.numel()
        slot[0][:n].copy_(host_values.reshape(-1))
        if out is None:
            out = torch.empty(n, dtype=slot[0].dtype, device=device)
        out.copy_(slot[0][:n], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(device))
        return out


def stage_cameras(m, geo, cam_idx_list, device, out=None):
    """``OcRFViewTransformerFull.stage_cameras``."""
    cam_idx_list = list(cam_idx_list)
    n = len(cam_idx_list)
    sel = torch.tensor(cam_idx_list, dtype=torch.int32)
    if geo.cam_rows_dev is not None:
        # device geometry: the rows of every camera-frame are already on the GPU; pick the chosen ones there
        sel_d = m._small_h2d(sel, device)
        packed = geo.cam_rows_dev[torch.arange(n, device=device), sel_d.long()].contiguous()
        if out is None:
            return dict(cam_sel=sel_d, packed=packed, cam_idx_list=cam_idx_list)
        out['cam_sel'].copy_(sel_d)
        out['packed'].copy_(packed)
    else:
        # ONE buffer behind both tensors (the n x 36 rows, then n int32 words): a refresh is one copy
        rows = [geo.cam_row(bs, c, m.input_size, m.znear, m.zfar) for bs, c in enumerate(cam_idx_list)]
        host = torch.empty(n * 37, dtype=torch.float32)
        host[:36 * n].copy_(torch.cat(rows, 0).reshape(-1))
        host[36 * n:].view(torch.int32).copy_(sel)
        if out is None:
            buf = torch.empty(n * 37, dtype=torch.float32, device=device)
            buf.copy_(host)
            return dict(cam_sel=buf[36 * n:].view(torch.int32), packed=buf[:36 * n].view(n, 36),
                        cam_idx_list=cam_idx_list, _buf=buf)
        # the static device tensors of a captured graph are refreshed through a ring that lives in their dict
        if '_ring' not in out:
            out['_ring'] = PinnedRing(4, n * 37, torch.float32)
        out['_ring'].put(host, device, out['_buf'])
    out['cam_idx_list'] = cam_idx_list
    return out
