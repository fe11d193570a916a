"""The tail of a training iteration of the reference config (configs/ocrfdet/ocrfdet.py:258-274, 329-330): gradient
clipping by the global L2 norm, AdamW and the weight EMA, for all tensors of a model in three launches
(``csrc/optim.hip``: ``ocrf_optim_grad_sqnorm``, two kernels, and ``ocrf_optim_step``, one).

* ``FusedAdamW``: a ``torch.optim.Optimizer`` with AdamW's defaults, state under torch's names (``step``, ``exp_avg``,
  ``exp_avg_sq``) and ``max_grad_norm`` for ``clip_grad_norm_(params, max_norm, norm_type=2)`` inside the same step.
* ``ModelEMA``: mmdet3d/core/hook/ema.py:17-60 with the same signature and ``decay`` ramp; ``update(model)`` is one
  launch, and ``optimizer.attach_ema(ema)`` moves it into the optimizer's launch.
* ``paramwise_groups``: the ``custom_keys`` rule of mmcv's ``DefaultOptimizerConstructor``, one group per parameter.

How the kernels see the tensors is described in ``include/ocrf_hip.h``: a static device table (addresses, element
counts, modes, chunks of ``OCRF_OPTIM_CHUNK`` elements) built once and rebuilt lazily after ``load_state_dict``,
``add_param_group``, ``attach_ema`` or when a tensor has moved, and one small record per tensor and step (the
gradient's address and the scalars of the tensor's group and step count, computed here in float64 and rounded once to
f32).  The records travel through a ring of pinned staging buffers, each guarded by an event recorded after its copy, so
a step reads nothing back from the device and does not block the host while the ring has a free buffer.

There is no fallback: CPU tensors, dtypes other than float32, non-contiguous parameters or gradients, sparse
gradients and ``amsgrad`` / ``maximize`` / ``capturable`` raise ``OcrfHipError`` naming the parameter.  Deliberate
differences from the torch calls it replaces: the clipped gradient is used but NOT written back to ``p.grad``
(``clip_grad_norm_`` scales the gradients in place), and ``step()`` returns the norm as a device tensor without reading
it (mmcv's ``float(grad_norm)`` is the caller's to do, or to leave out).
"""
import copy
import math

import numpy as np
import torch

from . import _lib
from ._lib import OcrfHipError

CHUNK = _lib.OCRF_OPTIM_CHUNK
ADAM_EMA, ADAM, EMA_ONLY = _lib.OCRF_OPTIM_ADAM_EMA, _lib.OCRF_OPTIM_ADAM, _lib.OCRF_OPTIM_EMA_ONLY
RING_DEPTH = 4                                   # pinned staging buffers of the per-step records

# the three structs of include/ocrf_hip.h as numpy packs them (checked against the compiler: ``c_layout``)
TENSOR_DT = np.dtype([('p', '<u8'), ('exp_avg', '<u8'), ('exp_avg_sq', '<u8'), ('ema', '<u8'), ('n', '<i8'),
                      ('mode', '<i4'), ('reserved', '<i4')])
CHUNK_DT = np.dtype([('tensor', '<i4'), ('offset', '<i4')])
REC_DT = np.dtype([('grad', '<u8'), ('decay', '<f4'), ('one_minus_beta1', '<f4'), ('beta2', '<f4'),
                   ('one_minus_beta2', '<f4'), ('bc2_sqrt', '<f4'), ('eps', '<f4'), ('step_size', '<f4'),
                   ('reserved', '<i4')])


def c_layout():
    """``ocrf_optim_layout``: sizeof and field offsets of the three table structs as the compiler laid them out."""
    import ctypes
    out = (ctypes.c_int * _lib.OCRF_OPTIM_LAYOUT_INTS)()
    _lib.check(_lib.lib().ocrf_optim_layout(out), 'ocrf_optim_layout')
    return list(out)


def numpy_layout():
    """The same list from the numpy dtypes the tables are packed with."""
    out = []
    for dt in (TENSOR_DT, CHUNK_DT, REC_DT):
        out.append(dt.itemsize)
        out.extend(dt.fields[name][1] for name in dt.names if name != 'reserved')
    return out


def plan_chunks(sizes, chunk=None):
    """The chunk table (``CHUNK_DT``) for tensors of ``sizes`` elements: every tensor is cut at the multiples of
    ``chunk`` (default ``OCRF_OPTIM_CHUNK``), tensors in order, a tensor's chunks ascending; an empty tensor gets none."""
    chunk = CHUNK if chunk is None else int(chunk)
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    counts = (sizes + chunk - 1) // chunk
    first = np.cumsum(counts) - counts                         # index of each tensor's first chunk
    out = np.zeros(int(counts.sum()), dtype=CHUNK_DT)
    out['tensor'] = np.repeat(np.arange(len(sizes)), counts)
    out['offset'] = (np.arange(len(out)) - np.repeat(first, counts)) * chunk
    return out


def _check_tensor(t, what):
    """``t`` is something the kernels can address: strided, float32, contiguous, on a GPU (checked in this order)."""
    if t.layout is not torch.strided:
        raise OcrfHipError(f'{what} is a {t.layout} tensor: the fused optimizer step takes dense tensors only')
    if t.dtype is not torch.float32:
        raise OcrfHipError(f'{what} is {t.dtype}: the fused optimizer step is float32 only')
    if not t.is_contiguous():
        raise OcrfHipError(f'{what} is not contiguous (shape {tuple(t.shape)}, strides {t.stride()})')
    if t.numel() >= 1 << 29:
        raise OcrfHipError(f'{what} has {t.numel()} elements: the kernels index a tensor with int (below 2 GiB)')
    if not t.is_cuda:
        raise OcrfHipError(f'{what} is on {t.device}: the fused optimizer step runs on the GPU only (HIP kernels, no '
                           'CPU fallback)')


class _Table:
    """The device tables of one set of tensors.  ``entries``: (p, exp_avg, exp_avg_sq, ema, mode) with None where the
    mode uses no tensor; ``p`` is the LIVE parameter or buffer object (not a detached alias, which would keep pointing
    at the old storage after ``p.data = ...``), so that ``moved()`` sees it move.  Holds the tensors, so that the
    addresses it has packed stay allocated."""

    def __init__(self, entries):
        self.entries = entries
        devices = {t.device for e in entries for t in e[:4] if t is not None}
        if len(devices) != 1:
            raise OcrfHipError(f'the fused optimizer step needs all its tensors on one GPU, got {sorted(map(str, devices))}')
        self.device = dev = devices.pop()
        n = len(entries)
        tensors = np.zeros(n, dtype=TENSOR_DT)
        for k, name in enumerate(('p', 'exp_avg', 'exp_avg_sq', 'ema')):
            tensors[name] = [0 if e[k] is None or e[k].numel() == 0 else e[k].data_ptr() for e in entries]
        tensors['n'] = [e[0].numel() for e in entries]
        tensors['mode'] = [e[4] for e in entries]
        chunks = plan_chunks(tensors['n'])
        self.n_tensors, self.n_chunks = n, len(chunks)
        self.max_elements = int(tensors['n'].max()) if n else 0
        self.n_elements = int(tensors['n'].sum())
        self.sources = [e[0] for e in entries]
        self.source_ptrs = [t.data_ptr() for t in self.sources]
        # one allocation: tensors | chunks | step records | partials (doubles) | total_norm, each 16-byte aligned
        sizes = [tensors.nbytes, chunks.nbytes, n * REC_DT.itemsize, 8 * max(self.n_chunks, 1), 16]
        offs = np.cumsum([0] + [(s + 15) // 16 * 16 for s in sizes])
        self._static_bytes = int(offs[2])
        self.rec_bytes = sizes[2]
        self.buf = torch.zeros(int(offs[-1]), dtype=torch.uint8, device=dev)
        base = self.buf.data_ptr()
        self.p_tensors, self.p_chunks, self.p_recs, self.p_partials = (base + int(o) for o in offs[:4])
        self.recs_dev = self.buf[int(offs[2]):int(offs[2]) + self.rec_bytes]
        self.total_norm = self.buf[int(offs[4]):int(offs[4]) + 4].view(torch.float32).view(())
        # the static part goes through a pinned buffer of its own that is never written again: no blocking copy
        self._static_host = torch.zeros(max(self._static_bytes, 16), dtype=torch.uint8, pin_memory=True)
        host = self._static_host.numpy()
        host[:tensors.nbytes] = tensors.view(np.uint8)
        host[int(offs[1]):int(offs[1]) + chunks.nbytes] = chunks.view(np.uint8)
        if self._static_bytes:
            self.buf[:self._static_bytes].copy_(self._static_host[:self._static_bytes], non_blocking=True)
        self.recs = np.zeros(n, dtype=REC_DT)                  # packed anew every step
        self._ring = self._ring_np = None                      # pinned staging buffers, allocated at the first send
        self._events = [None] * RING_DEPTH
        self._slot = 0

    def moved(self):
        """A parameter or source buffer is no longer where the table says (``p.data = ...``, ``module.to(...)``).  Only
        ``p`` is watched: an ``exp_avg`` / ``exp_avg_sq`` replaced by hand in ``state[p]`` or a reassigned EMA tensor is
        not noticed (the table keeps updating the tensor it was built with) and needs ``invalidate()``."""
        return [t.data_ptr() for t in self.sources] != self.source_ptrs

    def send_recs(self):
        """``self.recs`` -> device, through the next pinned buffer of the ring.  A buffer is reused only after the event
        recorded behind its last copy has passed; the host waits for it only if the whole ring is still in flight."""
        if not self.rec_bytes:
            return
        if self._ring is None:
            self._ring = [torch.zeros(self.rec_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(RING_DEPTH)]
            self._ring_np = [r.numpy() for r in self._ring]
        k = self._slot
        self._slot = (k + 1) % RING_DEPTH
        ev = self._events[k]
        if ev is None:
            ev = self._events[k] = torch.cuda.Event()
        elif not ev.query():
            ev.synchronize()
        self._ring_np[k][:] = self.recs.view(np.uint8)
        self.recs_dev.copy_(self._ring[k], non_blocking=True)
        ev.record()

    def grad_sqnorm(self):
        _lib.launch('ocrf_optim_grad_sqnorm', self.device, self.p_tensors, self.n_tensors, self.p_chunks, self.n_chunks,
                    self.p_recs, self.max_elements, self.p_partials, self.total_norm)

    def step(self, norm, max_norm, d, one_minus_d):
        _lib.launch('ocrf_optim_step', self.device, self.p_tensors, self.n_tensors, self.p_chunks, self.n_chunks,
                    self.p_recs, self.max_elements, norm, float(max_norm), float(d), float(one_minus_d))


def _is_parallel(model):
    return isinstance(model, (torch.nn.parallel.DataParallel, torch.nn.parallel.DistributedDataParallel))


class ModelEMA:
    """mmdet3d/core/hook/ema.py:17-60: a moving average of everything floating in the model's ``state_dict``.
    ``ema`` is the deep copy (parameters frozen, ``.eval()``; ``ema_model`` names the same module), ``updates`` the
    counter, ``decay(x) = decay * (1 - exp(-x / 2000))`` the ramp.  ``update(model)``: ``updates += 1`` and, for every
    floating entry, ``v = v * d + (1 - d) * msd[k]`` with ``d = decay(updates)``, ``d`` and ``1 - d`` each rounded once
    to f32, in ONE launch (the reference: two launches and a temporary per entry).  Non-floating entries
    (``num_batches_tracked``) stay as copied, as in the reference.  Floating entries other than contiguous float32 GPU
    tensors raise ``OcrfHipError`` naming the entry.  The reference's ``update(trainer, model)`` ignores its trainer."""

    def __init__(self, model, decay=0.9999, updates=0):
        self.source = model.module if _is_parallel(model) else model
        self.ema = self.ema_model = copy.deepcopy(self.source).eval()
        self.updates = updates
        self.decay = lambda x: decay * (1 - math.exp(-x / 2000))
        for p in self.ema.parameters():
            p.requires_grad_(False)
        self._table = self._table_of = None

    def pairs(self, model=None):
        """[(key, averaged tensor, source tensor)] of the floating ``state_dict`` entries; the source is the model's own
        parameter or buffer object."""
        model = self.source if model is None else (model.module if _is_parallel(model) else model)
        msd = model.state_dict(keep_vars=True)
        out = []
        for k, v in self.ema.state_dict(keep_vars=True).items():
            if v.dtype.is_floating_point:
                src = msd[k]
                if src.shape != v.shape:
                    raise OcrfHipError(f'EMA entry {k}: shape {tuple(v.shape)} here, {tuple(src.shape)} in the model')
                _check_tensor(v, f'EMA entry {k}')
                _check_tensor(src, f'model entry {k}')
                out.append((k, v, src))
        return out

    def next_decay(self):
        """Advance ``updates`` and return (d, 1 - d) of this update as Python floats."""
        self.updates += 1
        d = self.decay(self.updates)
        return d, 1.0 - d

    def _peek_decay(self):
        """(updates + 1, d, 1 - d) of the next update; ``updates`` advances once its launch has been issued."""
        d = self.decay(self.updates + 1)
        return self.updates + 1, d, 1.0 - d

    @torch.no_grad()
    def update(self, model):
        model = model.module if _is_parallel(model) else model
        t = self._table
        if t is None or self._table_of is not model or t.moved():
            t = self._table = _Table([(src, None, None, v.detach(), EMA_ONLY) for _, v, src in self.pairs(model)])
            self._table_of = model
        updates, d, omd = self._peek_decay()
        if t.n_chunks:
            t.step(None, 0.0, d, omd)
        self.updates = updates                                 # a launch that raises leaves the counter where it was


class FusedAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` (its single-tensor formula, in f32, every operation rounded once) with gradient clipping
    and, after ``attach_ema``, the weight EMA in the same launch.

    ``step()`` = ``clip_grad_norm_(params, max_grad_norm)`` (when ``max_grad_norm`` is not None) + ``AdamW.step()`` +
    ``ema.update(model)`` (when an EMA is attached; ``ema.updates`` advances).  It returns the total gradient norm as a
    0-dim device tensor (the optimizer's own buffer, overwritten by the next step) or None without clipping, and never
    reads the device.  The clipped gradients are used, not written back to ``p.grad``.  A NaN or infinite norm
    propagates into every parameter as it does in torch.

    ``param_groups`` are read every step (LR hooks work unchanged); ``state[p]`` holds ``step`` (a CPU float32 scalar,
    as torch keeps it; here a view into one tensor for all parameters), ``exp_avg`` and ``exp_avg_sq``, so
    ``state_dict()`` loads into ``torch.optim.AdamW`` and back.  ``step(closure)`` evaluates the closure and still
    returns the norm, not the closure's loss.

    State is created when the tables are built, for every parameter that requires a gradient (torch: at a parameter's
    first gradient), and for one that does not when it first has a gradient.  A parameter without a gradient this step
    keeps ``p`` and its state bit for bit, its ``step`` does not advance, and its EMA still moves.  ``step`` counts and
    ``ema.updates`` advance after the launches have been issued: a step that raises leaves them where they were.

    The tables are rebuilt lazily after ``load_state_dict``, ``add_param_group``, ``attach_ema`` and when a parameter
    (or, with an EMA attached, a source buffer) has moved: their addresses are compared every step.  Nothing else is
    watched: after replacing ``state[p]['step']``, ``exp_avg`` or ``exp_avg_sq`` by hand, or reassigning a tensor of
    the EMA model, call ``invalidate()`` (or ``load_state_dict``).  All steps are expected on one stream."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None,
                 amsgrad=False, maximize=False, capturable=False):
        if lr < 0 or eps < 0 or weight_decay < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError(f'invalid AdamW hyper-parameters: lr {lr}, betas {betas}, eps {eps}, weight_decay {weight_decay}')
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f'max_grad_norm must be positive or None, got {max_grad_norm}')
        self.max_grad_norm = max_grad_norm
        self._ema = self._ema_model = None
        self._table = None
        # the keys torch.optim.AdamW keeps in a group, so that a state_dict travels both ways
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=None, capturable=capturable, differentiable=False, fused=None,
                        decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self._check_groups()

    # ------------------------------------------------------------------------------------------------ bookkeeping
    def invalidate(self):
        """Rebuild the device tables at the next ``step()``."""
        self._table = None

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._table = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._table = None

    def attach_ema(self, ema, model=None):
        """From now on ``step()`` also does ``ema.update(model)`` (``model``: default the one ``ema`` was built from):
        the EMA of a parameter this optimizer owns is taken in the pass that updates it, every other floating
        ``state_dict`` entry (BN running statistics, parameters of other optimizers) as an EMA-only entry of the same
        launch.  ``attach_ema(None)`` detaches."""
        self._ema, self._ema_model = ema, model
        self._table = None

    def _name(self, gi, pi, p):
        g = self.param_groups[gi]
        names = g.get('param_names')
        name = names[pi] if names else (g.get('name') if len(g['params']) == 1 else None)
        where = f'parameter {pi} of group {gi}'
        return f'{where} ({name}, shape {tuple(p.shape)})' if name else f'{where} (shape {tuple(p.shape)})'

    def _check_groups(self):
        for gi, g in enumerate(self.param_groups):
            for flag in ('amsgrad', 'maximize', 'capturable'):
                if g.get(flag):
                    who = ', '.join(self._name(gi, pi, p) for pi, p in enumerate(g['params'][:3]))
                    raise OcrfHipError(f'{flag}=True is not implemented by the fused optimizer step (group {gi}: {who})')

    def _rebuild(self, with_grad):
        """State for the parameters that need it, then the tables.  ``with_grad``: ids of parameters that have a
        gradient right now."""
        self._params, self._group_index, entries = [], [], []
        ema_of = {}
        extra = []
        if self._ema is not None:
            owned = {id(p) for g in self.param_groups for p in g['params']}
            for k, v, src in self._ema.pairs(self._ema_model):
                if id(src) in owned:
                    ema_of[id(src)] = v.detach()
                else:
                    extra.append((src, None, None, v.detach(), EMA_ONLY))
        steps, has_state = [], []
        for gi, g in enumerate(self.param_groups):
            for pi, p in enumerate(g['params']):
                what = self._name(gi, pi, p)
                _check_tensor(p, what)
                st = self.state[p]
                if not st and (p.requires_grad or id(p) in with_grad):
                    st['step'] = torch.tensor(0.0, dtype=torch.float32)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m = v = None
                if st:
                    m, v = st['exp_avg'], st['exp_avg_sq']
                    for t, key in ((m, 'exp_avg'), (v, 'exp_avg_sq')):
                        _check_tensor(t, f'{key} of {what}')
                        if t.shape != p.shape or t.device != p.device:
                            raise OcrfHipError(f'{key} of {what} has shape {tuple(t.shape)} on {t.device}')
                    steps.append(float(st['step']))
                else:
                    steps.append(0.0)
                has_state.append(bool(st))
                e = ema_of.get(id(p))
                entries.append((p, m, v, e, ADAM if e is None else ADAM_EMA))
                self._params.append(p)
                self._group_index.append(gi)
        self._n_own = len(self._params)
        self._group_index = np.asarray(self._group_index, dtype=np.int64)
        # every state[p]['step'] is a 0-dim view into ONE CPU float32 tensor (torch keeps a CPU float32 scalar per
        # parameter): a step advances all of them with one numpy addition, and there is no second copy to keep in sync
        store = torch.tensor(steps, dtype=torch.float32)
        self._steps = store.numpy()
        for k, p in enumerate(self._params):
            if has_state[k]:
                self.state[p]['step'] = store[k]
        self._has_state = has_state
        self._table = _Table(entries + extra) if entries or extra else None

    # ------------------------------------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:                                # evaluated as torch does; what comes back is the norm
            with torch.enable_grad():
                closure()
        self._check_groups()
        # this step's gradients: checked before anything is built or launched
        grads, with_grad = [], set()
        for gi, g in enumerate(self.param_groups):
            for pi, p in enumerate(g['params']):
                gr = p.grad
                if gr is not None:
                    if gr.layout is not torch.strided or gr.dtype is not torch.float32 or not gr.is_cuda \
                            or not gr.is_contiguous() or gr.shape != p.shape:
                        _check_tensor(gr, f'the gradient of {self._name(gi, pi, p)}')
                        raise OcrfHipError(f'the gradient of {self._name(gi, pi, p)} has shape {tuple(gr.shape)}')
                    with_grad.add(id(p))
                grads.append(gr)
        t = self._table
        if t is None or len(grads) != self._n_own or t.moved() \
                or any(gr is not None and not hs for gr, hs in zip(grads, self._has_state)):
            self._rebuild(with_grad)
            t = self._table
        if t is None:
            return None
        n = self._n_own
        recs = t.recs
        addr = np.fromiter((0 if gr is None or gr.numel() == 0 else gr.data_ptr() for gr in grads), dtype=np.uint64,
                           count=n)
        has = np.fromiter((gr is not None for gr in grads), dtype=bool, count=n)
        groups = self.param_groups
        gidx = self._group_index
        lr = np.asarray([g['lr'] for g in groups], dtype=np.float64)[gidx]
        wd = np.asarray([g['weight_decay'] for g in groups], dtype=np.float64)[gidx]
        b1 = np.asarray([g['betas'][0] for g in groups], dtype=np.float64)[gidx]
        b2 = np.asarray([g['betas'][1] for g in groups], dtype=np.float64)[gidx]
        eps = np.asarray([g['eps'] for g in groups], dtype=np.float64)[gidx]
        step = np.where(has, self._steps + 1.0, 1.0).astype(np.float64)   # no gradient: scalars unused, kept finite
        recs['grad'][:n] = addr
        recs['decay'][:n] = 1.0 - lr * wd
        recs['one_minus_beta1'][:n] = 1.0 - b1
        recs['beta2'][:n] = b2
        recs['one_minus_beta2'][:n] = 1.0 - b2
        recs['bc2_sqrt'][:n] = np.sqrt(1.0 - b2 ** step)
        recs['eps'][:n] = eps
        recs['step_size'][:n] = lr / (1.0 - b1 ** step)
        t.send_recs()
        clip = self.max_grad_norm is not None
        updates, d, omd = self._ema._peek_decay() if self._ema is not None else (None, 1.0, 0.0)
        if t.n_chunks:
            if clip:
                t.grad_sqnorm()
            t.step(t.total_norm if clip else None, self.max_grad_norm if clip else 0.0, d, omd)
        # issued: now the counters advance (a launch that raises leaves them where they were)
        self._steps[has] += 1.0                                # the state's step tensors are views of this array
        if self._ema is not None:
            self._ema.updates = updates
        return t.total_norm if clip else None


def paramwise_groups(model, lr, weight_decay, custom_keys):
    """The ``custom_keys`` rule of mmcv 1.x ``DefaultOptimizerConstructor.add_params`` restated: one param group per
    parameter of ``model`` (``named_parameters()`` order), ``lr`` and ``weight_decay`` set in every group.  A key matches
    a parameter when it is a substring of the parameter's dotted name; the keys are tried longest first, keys of one
    length alphabetically, and the first match wins: the group gets ``lr * lr_mult`` and ``weight_decay * decay_mult``
    (each multiplier 1 when absent).  Each group also carries the parameter's ``name``, which ``FusedAdamW`` quotes in
    its errors.  mmcv's other rules (``bias_lr_mult``, ``norm_decay_mult``, ``dwconv_decay_mult``, ...) are not used by
    the reference config and are not restated.  mmcv is not installed where this package is developed, so the rule is
    restated from its source text and is not tested against mmcv itself."""
    keys = sorted(sorted(custom_keys), key=len, reverse=True)
    groups = []
    for name, p in model.named_parameters():
        group = dict(params=[p], lr=lr, weight_decay=weight_decay, name=name)
        for key in keys:
            if key in name:
                group['lr'] = lr * custom_keys[key].get('lr_mult', 1.0)
                group['weight_decay'] = weight_decay * custom_keys[key].get('decay_mult', 1.0)
                break
        groups.append(group)
    return groups
