"""Streaming inference of ``OcRFDet4D``: frames arrive one after another, and a step computes only what the new frame
adds.  The batch forward (``extract_img_feat``) runs the image encoder three times and the neck twice per call, because
it recomputes the adjacent frame and the extra stereo reference frame; here the adjacent frames' BEV maps and the
previous frame's stereo feature are the ones the earlier steps produced.

* ``key_frame_inputs``: frame 0 of every entry of a multi-frame ``img_inputs``, as ``prepare_inputs`` splits it;
* ``StreamState``: what is kept between the steps;
* ``stream_step``: one step, the body of ``OcRFDet4D.stream_step``.

Why the cached maps are the batch forward's.  The view transformer is fed ``rots[fid]`` / ``trans[fid]`` (sensor -> that
frame's own ego) and never ``sensor2keyego``.  So with ``align_after_view_transfromation=False`` the adjacent frame's BEV
map of the batch forward is the map the previous step produced as key frame, and with the flag set the same map is warped
by ``shift_feature``'s transform; the stereo cost volume of frame t needs the stereo feature and the raw poses of t - 1.
Step t of a sequence therefore reproduces the batch forward on the frames (t, max(t - 1, 0), ..., max(t - K - 1, 0)),
K = ``num_adj``: a sequence starts with its first frame repeated, the dataset's convention.

The one deliberate deviation: the cached adjacent map was computed with ITS OWN ``rots`` / ``trans`` / ``bda`` in
``mlp_input``, the batch forward uses the key frame's there (``get_mlp_input(rots[0], trans[0], ...)``).  The two agree
when the rig's calibration and the BEV augmentation do not change between the frames, as at test time.

``bf16=True`` streams in bfloat16 on fused kernels from the images to the BEV encoder: the step runs inside
``OcRFDet4D.bf16_inference()``, the ring is bfloat16 and aligned by ``ocrf_bev_stream_align_bf16``, and the stereo feature
is packed once per frame for ``ocrf_stereo_cost_volume_bf16``: the packed previous frame is the one the previous step
packed (``StreamState.stereo_packed``).

No device -> host read in a step.  A step whose ``new_sequence`` flags are mixed uploads them (B bytes, from pinned
memory, asynchronously); a step without a flag uploads nothing.
"""
import contextlib

import torch

from . import depthnet, temporal
from .detector import frame_poses, frame_split


def key_frame_inputs(img_inputs, num_frame):
    """The 12-entry list of ONE frame from the multi-frame ``img_inputs`` (images (B, N * num_frame, C, H, W)
    camera-major, poses (B, num_frame * N, ...) frame-major): frame 0 of each entry, views as ``prepare_inputs`` makes
    them, ``bda`` as it is."""
    B, N = frame_split(img_inputs, num_frame)
    image = lambda t: t.view(B, N, num_frame, *t.shape[2:])[:, :, 0]          # noqa: E731
    pose = lambda t: t.view(B, num_frame, N, *t.shape[2:])[:, 0]              # noqa: E731
    (imgs, rots, trans, intrins, post_rots, post_trans, bda, sensor2egos, ego2globals, imgs_wo_norm, imgs_wo_aug,
     c2w) = img_inputs
    return [image(imgs), pose(rots), pose(trans), pose(intrins), pose(post_rots), pose(post_trans), bda,
            pose(sensor2egos), pose(ego2globals), image(imgs_wo_norm), image(imgs_wo_aug), pose(c2w)]


class StreamState:
    """What ``stream_step`` keeps between the steps of B parallel sequences (K = ``num_adj``, S = K + 1):

    * ``ring`` (S, B, C, H, W): the last S key-frame BEV maps (``pre_process_net``'s output), slot ``head`` the newest;
    * ``sensor2ego0``, ``ego2global0`` (S, B, 4, 4), ``bda`` (S, B, 3, 3): camera 0's raw poses and the BEV augmentation
      at each slot's time, what ``temporal.stream_align`` evaluates its transforms from;
    * ``stereo``: the last key frame's stereo feature (B * N, ...), ``sensor2egos`` / ``ego2globals`` (B, N, 4, 4) its
      raw poses: the previous frame of the next step's cost volume; ``stereo_packed``: the same feature as
      ``depthnet.stereo_pack_bf16`` lays it out, (B * N, NB, H, W, 8) sample-major, kept only by bfloat16 steps whose
      cost volume takes the bfloat16 kernel (else None);
    * ``bf16``: the mode of the steps that made the state; a step of the other mode does not continue it;
    * ``valid`` (B) int32 on the device: the number of real history frames of each sample, ``valid_host`` its host
      mirror, kept by counting (never read back)."""

    def __init__(self, num_adj, bf16=False):
        self.num_adj = int(num_adj)
        self.bf16 = bool(bf16)
        self.head = 0
        self.ring = self.sensor2ego0 = self.ego2global0 = self.bda = None
        self.stereo = self.sensor2egos = self.ego2globals = None
        self.stereo_packed = None
        self.valid = None
        self.valid_host = None
        self.steps = 0

    @property
    def slots(self):
        return self.num_adj + 1

    def ring_dtype(self, bev_feat):
        """bfloat16 in a bf16 state (a float32 map is narrowed once by the copy into the ring), else the map's."""
        return torch.bfloat16 if self.bf16 else bev_feat.dtype

    def allocate(self, bev_feat, sensor2egos):
        """The buffers, from the first key-frame map (B, C, H, W) and its poses (B, N, 4, 4)."""
        S, B = self.slots, bev_feat.shape[0]
        self.ring = bev_feat.new_empty((S, *bev_feat.shape), dtype=self.ring_dtype(bev_feat))
        self.sensor2ego0 = sensor2egos.new_zeros(S, B, 4, 4)
        self.ego2global0 = sensor2egos.new_zeros(S, B, 4, 4)
        self.bda = sensor2egos.new_zeros(S, B, 3, 3)
        self.valid = torch.zeros(B, dtype=torch.int32, device=bev_feat.device)
        self.valid_host = [0] * B

    def matches(self, bev_feat):
        return self.ring is not None and self.ring.shape[1:] == bev_feat.shape \
            and self.ring.dtype == self.ring_dtype(bev_feat) and self.ring.device == bev_feat.device


def _flags(new_sequence, B, fresh):
    """``new_sequence`` as a list of B bools; a fresh state starts every sequence."""
    if fresh:
        return [True] * B
    if new_sequence is None:
        return [False] * B
    flags = [bool(f) for f in new_sequence]
    if len(flags) != B:
        raise ValueError(f'new_sequence has {len(flags)} entries for {B} samples')
    return flags


def _upload(flags, device):
    """(B) bool on ``device`` without a synchronisation: from pinned memory, asynchronously, on the GPU."""
    host = torch.tensor(flags, dtype=torch.bool)
    if device.type != 'cuda':
        return host.to(device)
    return host.pin_memory().to(device, non_blocking=True)


def _select(mask, own, cached):
    """Per sample ``own`` where ``mask`` (B) is set, else ``cached``; both (B, ...) or (B * n, ...) sample-major."""
    B, n = mask.shape[0], own.shape[0] // mask.shape[0]
    m = mask.view(B, 1).expand(B, n).reshape(B * n, *([1] * (own.dim() - 1)))
    return torch.where(m, own, cached)


def _packed_stereo(det, stereo_feat, B, N):
    """``stereo_feat`` packed for ``ocrf_stereo_cost_volume_bf16`` (one ``ocrf_stereo_pack_bf16`` launch), or None when
    the view transformer's cost volume would not take that kernel: the feature is not CUDA bfloat16, has fewer than 4
    channels or a map below 2 x 2, or the depth net's ``fused_cost_volume`` / ``fused_cost_volume_bf16`` is off."""
    vt = det.img_view_transformer
    depth_net = getattr(vt, 'depth_net', None)
    if not (getattr(depth_net, 'fused_cost_volume', False) and getattr(depth_net, 'fused_cost_volume_bf16', False)):
        return None
    if not (stereo_feat.is_cuda and stereo_feat.dtype == torch.bfloat16):
        return None
    H, W = vt.cv_frustum.shape[1:3]
    channels, rest = divmod(stereo_feat.numel(), B * N * H * W)
    if H < 2 or W < 2 or rest or channels < depthnet.GROUP:
        return None
    return depthnet.stereo_pack_bf16(stereo_feat.reshape(B * N, -1, H, W))


def stream_step(det, img_inputs, state=None, new_sequence=None, multi_frame=False, bf16=False):
    """One streaming step of ``det`` (an ``OcRFDet4D`` in eval mode) on ONE frame: ``img_inputs`` is the 12-entry list
    with images (B, N, 3, H, W) and poses (B, N, ...), or with ``multi_frame=True`` the multi-frame list, of which frame 0
    is taken (``key_frame_inputs``).  ``new_sequence``: a host sequence of B bools, the samples whose sequence starts with
    this frame; ``state=None`` (or a state of another shape) starts all of them.

    Returns ``(([x], depth, bev_mask), state)``, the first what ``extract_img_feat`` returns in eval mode.  The step:
    the frame poses of the (B, 2, N) stack [current, cached] in one ``frame_poses`` call (``curr2adjsensor`` and
    ``mlp_input``; ``det.fused_poses``), ``image_encoder(stereo=True)`` once, the view transformer once with
    ``cv_feat_list = [cached stereo feature, own]``, ``pre_process_net`` into ring slot ``head``,
    ``temporal.stream_align`` for the concatenation, ``bev_encoder``; then the cache advances.  For a sample with
    ``new_sequence`` the cached stereo feature and poses are its own (selected on the device) and ``valid = 0``.

    With ``det.with_prev`` False the step returns what the batch forward returns for the frame (zeros and the key frame)
    and keeps no state.

    ``bf16=True``: the step runs inside ``det.bf16_inference()``.  The ring is bfloat16 (a float32 ``bev_feat``, from a
    detector without ``pre_process``, is narrowed once by the copy into the ring) and ``temporal.stream_align`` keeps it
    (``keep_bf16=True``); the new stereo feature is packed once and the view transformer gets ``cv_feat_packed =
    [cached packed, own packed]``; ``[x]`` is what the BEV encoder returns under ``autocast_bf16``, ``depth`` and
    ``bev_mask`` come back as the neck returns them.  A state made by steps of the other mode is not continued: the step
    starts every sequence, as with ``state=None``.  CPU inputs raise ``ValueError`` before any module runs."""
    if det.training:
        raise RuntimeError('stream_step is a test mode: call eval() first (training takes extract_img_feat)')
    if multi_frame:
        img_inputs = key_frame_inputs(img_inputs, det.num_frame)
    if len(img_inputs) != 12:
        raise ValueError(f'img_inputs has 12 entries, got {len(img_inputs)}')
    (imgs, rots, trans, intrins, post_rots, post_trans, bda, sensor2egos, ego2globals, imgs_wo_norm, imgs_wo_aug,
     c2w) = img_inputs
    if imgs.dim() != 5 or sensor2egos.dim() != 4:
        raise ValueError(f'stream_step takes ONE frame: images (B, N, 3, H, W) and poses (B, N, 4, 4), got '
                         f'{tuple(imgs.shape)} and {tuple(sensor2egos.shape)}')
    bf16 = bool(bf16)
    if bf16 and not all(t.is_cuda for t in img_inputs if isinstance(t, torch.Tensor)):
        raise ValueError('stream_step(bf16=True) runs on the GPU only: the bfloat16 kernels have no CPU form; move '
                         'img_inputs to the GPU or stream with bf16=False')
    B, N = imgs.shape[:2]
    K = det.num_frame - det.extra_ref_frames - 1
    with torch.no_grad(), (det.bf16_inference() if bf16 else contextlib.nullcontext()):
        if not det.with_prev:
            return _step_without_history(det, img_inputs), None
        fresh = state is None or state.num_adj != K or state.ring is None or state.ring.shape[1] != B \
            or state.sensor2egos.shape != sensor2egos.shape or state.bf16 != bf16
        if fresh:
            state = StreamState(K, bf16=bf16)
        flags = _flags(new_sequence, B, fresh)
        mask = None if all(flags) or not any(flags) else _upload(flags, imgs.device)
        own = all(flags)

        x, stereo_feat = det.image_encoder(imgs, stereo=True)
        if own:
            prev_stereo, prev_s2e, prev_e2g = stereo_feat, sensor2egos, ego2globals
        elif mask is None:
            prev_stereo, prev_s2e, prev_e2g = state.stereo, state.sensor2egos, state.ego2globals
        else:
            prev_stereo = _select(mask, stereo_feat, state.stereo)
            prev_s2e = _select(mask, sensor2egos, state.sensor2egos)
            prev_e2g = _select(mask, ego2globals, state.ego2globals)
        packed = None
        own_packed = _packed_stereo(det, stereo_feat, B, N) if bf16 else None
        if own_packed is not None:
            cached = state.stereo_packed
            if own or cached is None or cached.shape != own_packed.shape:
                cached = own_packed if own else None              # None: the cost volume packs the previous feature
            elif mask is not None:
                cached = _select(mask, own_packed, cached)
            packed = [cached, own_packed]
        pair = lambda a, b: torch.stack([a, b], 1)                # noqa: E731  (B, 2, N, ...)
        _, curr2adj, mlp_input = frame_poses(pair(sensor2egos, prev_s2e), pair(ego2globals, prev_e2g), pair(rots, rots),
                                             pair(trans, trans), pair(intrins, intrins), pair(post_rots, post_rots),
                                             pair(post_trans, post_trans), bda, 1, fused=det.fused_poses)
        bev_feat, depth, bev_mask, _ = det.lift_to_bev(x, stereo_feat, imgs, rots, trans, intrins, post_rots,
                                                          post_trans, bda, mlp_input[0], prev_stereo, curr2adj[:, 0],
                                                          imgs_wo_norm, imgs_wo_aug, c2w, cv_feat_packed=packed)
        if not state.matches(bev_feat):
            state.allocate(bev_feat, sensor2egos)
        head = state.head
        state.ring[head].copy_(bev_feat)
        state.sensor2ego0[head].copy_(sensor2egos[:, 0])
        state.ego2global0[head].copy_(ego2globals[:, 0])
        state.bda[head].copy_(bda)
        if own:
            state.valid.zero_()
        elif mask is not None:
            state.valid.masked_fill_(mask, 0)
        state.valid_host = [0 if f else v for f, v in zip(flags, state.valid_host)]

        vt = det.img_view_transformer
        cat, _ = temporal.stream_align(state.ring, head, state.valid, state.sensor2ego0, state.ego2global0, state.bda,
                                       vt.grid_interval, vt.grid_lower_bound,
                                       align=bool(det.align_after_view_transfromation), fused=det.fused_align,
                                       keep_bf16=bf16)
        out = det.bev_encoder(cat)

        state.head = (head + 1) % state.slots
        state.stereo, state.sensor2egos, state.ego2globals = stereo_feat, sensor2egos, ego2globals
        state.stereo_packed = own_packed
        if K > 0:
            state.valid.add_(1).clamp_(max=K)
        state.valid_host = [min(v + 1, K) for v in state.valid_host]
        state.steps += 1
    return ([out], depth, bev_mask), state


def _step_without_history(det, img_inputs):
    """``with_prev=False``: the batch forward skips every frame but the key frame, hands the view transformer no previous
    stereo feature and fills the adjacent groups with zeros (``det.cat_history``).  ``k2s_sensor`` is the key frame onto
    itself: the step knows no other frame (the stereo DepthNet does not read it without a previous feature)."""
    (imgs, rots, trans, intrins, post_rots, post_trans, bda, sensor2egos, ego2globals, imgs_wo_norm, imgs_wo_aug,
     c2w) = img_inputs
    pair = lambda a: torch.stack([a, a], 1)                       # noqa: E731
    _, curr2adj, mlp_input = frame_poses(pair(sensor2egos), pair(ego2globals), pair(rots), pair(trans), pair(intrins),
                                         pair(post_rots), pair(post_trans), bda, 1, fused=det.fused_poses)
    x, stereo_feat = det.image_encoder(imgs, stereo=True)
    key, depth, bev_mask, _ = det.lift_to_bev(x, stereo_feat, imgs, rots, trans, intrins, post_rots, post_trans, bda,
                                                 mlp_input[0], None, curr2adj[:, 0], imgs_wo_norm, imgs_wo_aug, c2w)
    return [det.bev_encoder(det.cat_history([key]))], depth, bev_mask
