"""Loader for ``libocrf_hip.so`` — the C-ABI HIP library behind every op in this package.

``lib()`` never falls back: if the library cannot be loaded it raises, and so does every op that
launches through it.  Its entry points are declared from ``include/ocrf_hip.h`` itself, and ``launch()``
is how the ops call them.  ``build()`` compiles it in-tree with hipcc for gfx950 (cross-compiles
without a GPU); the built ``.so`` is git-ignored but travels with the source tree.
"""
import collections
import contextlib
import ctypes
import os
import re
import subprocess

import torch

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# OCRF_HIP_SO: another build of the same library (A/B of kernel versions in diagnostics); default: the in-tree one
_SO = os.environ.get("OCRF_HIP_SO") or os.path.join(_CSRC, "libocrf_hip.so")
_LIB = None


class OcrfHipError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Compile every ``csrc/*.hip`` into ``csrc/libocrf_hip.so`` (``--offload-arch=gfx950``)."""
    args = ["make", "-C", _CSRC, "-j4", "libocrf_hip.so"]
    if force:
        subprocess.check_call(["make", "-C", _CSRC, "clean"], stdout=subprocess.DEVNULL)
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(args, stdout=out)
    return _SO


def lib():
    """The loaded library, its entry points declared from ``include/ocrf_hip.h``.  Raises ``OcrfHipError`` if it is
    missing — never falls back."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            raise OcrfHipError(
                f"{_SO} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C ocrfdet_amd/csrc` (hipcc, gfx950). ocrfdet_amd has no fallback path.")
        protos = prototypes()
        try:
            L = ctypes.CDLL(_SO)
        except OSError as e:  # pragma: no cover
            raise OcrfHipError(f"cannot load {_SO}: {e}") from e
        for name, (restype, argtypes) in protos.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _LIB = L
    rec = getattr(_RECORDER, 'rec', None)
    if rec is not None:
        return _RecordingLib(_LIB, rec)
    return _LIB


# ---------------------------------------------------------------------------------------------------------------
# The C ABI as include/ocrf_hip.h states it: the ctypes declarations, kernel ids and constants are read from there.
# ---------------------------------------------------------------------------------------------------------------
_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ocrf_hip.h')
_SCALARS = {'int': ctypes.c_int, 'long': ctypes.c_long, 'long long': ctypes.c_longlong, 'size_t': ctypes.c_size_t,
            'float': ctypes.c_float, 'double': ctypes.c_double, 'ocrf_stream_t': ctypes.c_void_p}
# what a pointer may point at; every pointer is passed as c_void_p (device buffers, host out-parameters, handles)
_POINTEES = set(_SCALARS) | {'void', 'char', 'unsigned', 'unsigned char', 'unsigned short', 'unsigned long long',
                             'uint32_t', 'uint64_t', 'ocrf_step'}
_PROTO = re.compile(r'^[ \t]*(\w[\w \t*]*?)\s*\b((?:ocrf_|bev_pool_v2)\w*)\s*\(([^()]*)\)\s*;', re.M)


def _header_text(path=_HEADER):
    """The header without its ``/* */`` and ``//`` comments."""
    with open(path) as f:
        text = re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)
    return re.sub(r'//[^\n]*', '', text)


def _ctype(spelling, proto, ret=False):
    """ctypes type of one C type spelling (``const float *const *``, ``size_t`` ...)."""
    words = spelling.replace('*', ' * ').split()
    base = ' '.join(w for w in words if w not in ('const', '*'))
    stars = words.count('*')
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 0 and base == 'void' and ret:
        return None
    if stars == 1 and base == 'char':
        return ctypes.c_char_p
    if stars and base in _POINTEES:
        return ctypes.c_void_p
    raise OcrfHipError(f'ocrf_hip.h: no ctypes type for {spelling.strip()!r} in {proto!r}')


def _declarations(text):
    """(return type, name, prototype, [parameter types]) of every ``ocrf_*`` / ``bev_pool_v2*`` prototype in C source
    ``text`` (comments already stripped), the types as they are spelled."""
    for m in _PROTO.finditer(text):
        ret, name, params = m.groups()
        params = [] if params.strip() in ('', 'void') else params.split(',')
        # a parameter's name is its last identifier; what is in front of it is its type
        yield ret, name, ' '.join(m.group(0).split()), [' '.join(re.sub(r'\b\w+\s*$', '', p).split()) for p in params]


def parse_prototypes(text):
    """{name: (restype, [argtypes])} of every prototype in ``text`` (``_declarations``).  A type without a mapping raises
    ``OcrfHipError`` naming the prototype."""
    return {name: (_ctype(ret, proto, ret=True), [_ctype(p, proto) for p in params])
            for ret, name, proto, params in _declarations(text)}


def parse_enqueueing(text):
    """Names of the prototypes in ``text`` that enqueue work: exactly those whose last parameter is an ``ocrf_stream_t``."""
    return frozenset(name for _, name, _, params in _declarations(text) if params[-1:] == ['ocrf_stream_t'])


def prototypes():
    """The declarations of the library's entry points, from include/ocrf_hip.h."""
    return parse_prototypes(_header_text())


def _constants(text):
    """``#define OCRF_X <int>`` as ``OCRF_X`` and the kernel ids ``OCRF_K_X = <int>`` as ``K_X``."""
    consts = {k: int(v) for k, v in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(OCRF_\w+)[ \t]+(-?\d+)[ \t]*$', text, re.M)}
    consts.update((k[len('OCRF_'):], int(v)) for k, v in re.findall(r'\b(OCRF_K_\w+)\s*=\s*(\d+)', text))
    return consts


globals().update(_constants(_header_text()))      # K_BEV_POOL_FWD, OCRF_CD_MAX_TASKS, ...
_ENQUEUEING = parse_enqueueing(_header_text())    # what a step being recorded logs (``_RecordingLib``)


# passed as they are without the isinstance(a, torch.Tensor) check (~70 ns each): scalars, NULL, pre-built pointers
_PLAIN = frozenset((int, float, type(None), ctypes.c_void_p))
_Tensor = torch.Tensor


def launch(name, device, *args, stream=None):
    """Call the enqueueing entry point ``name`` on ``device``: a tensor is passed as its data pointer (0 when empty),
    anything else as it is (scalars as Python numbers), then ``stream`` (default: torch's current stream of ``device``).
    A non-zero hipError_t raises.  ``name`` is looked up through ``lib()`` on every call, so that a step being recorded
    (``StepRecorder``) sees the call."""
    with on_device(device):
        err = getattr(lib(), name)(*[a if type(a) in _PLAIN else (a.data_ptr() if a.numel() > 0 else 0)
                                     if isinstance(a, _Tensor) else a for a in args],
                                   stream_ptr(device) if stream is None else stream)
    if err != 0:
        raise OcrfHipError(f'{name} failed with hipError_t {err}')


# ---------------------------------------------------------------------------------------------------------------
# One host call per step (csrc/step.hip): the library calls of a step are recorded once, while the step runs eagerly,
# and replayed from C afterwards.
# ---------------------------------------------------------------------------------------------------------------
import threading  # noqa: E402

_RECORDER = threading.local()      # .rec: the StepRecorder of THIS thread (another thread calling lib()
                                   # while a step is recorded must not get its calls spliced into that step)


class StepNotRecordable(OcrfHipError):
    pass


class StepRecorder:
    """Records the library calls of ONE step while it is issued eagerly: ``with recorder: step()``.  ``streams``: the
    torch streams of the step in slot order (slot 0 = the caller's); a call on any other stream, or of an entry point
    ``ocrf_step_fn_id`` does not know, makes the step not recordable (``ok`` False — keep issuing it call by call).
    The owner marks the fork / join points itself (``fork`` / ``join``: it is the one that issues the torch events).
    ``build()`` -> a ``CompiledStep``.  Everything a recorded call points at has to stay alive and in place."""

    def __init__(self, streams):
        self.slots = {int(st.cuda_stream): i for i, st in enumerate(streams)}
        self.items = []
        self.names = []                  # every enqueueing entry point the step called, recordable or not
        self.ok = True
        self.why = None

    def __enter__(self):
        if getattr(_RECORDER, 'rec', None) is not None:
            raise OcrfHipError('a step is already being recorded')
        lib()
        _RECORDER.rec = self
        return self

    def __exit__(self, *exc):
        _RECORDER.rec = None
        return False

    def fail(self, why):
        if self.ok:
            self.ok, self.why = False, why

    def fork(self, frm, to):
        self.items.append(('fork', frm, to))

    def join(self, frm, to):
        self.items.append(('join', frm, to))

    def on_call(self, name, fn, args):
        L = _LIB
        self.names.append(name)
        fid = L.ocrf_step_fn_id(name.encode())
        if fid < 0:
            return self.fail(f'{name} cannot be held by a step object')
        types = fn.argtypes
        if types is None or len(types) != len(args) or L.ocrf_step_fn_args(fid) != len(args) - 1:
            return self.fail(f'{name}: argument list does not match its declaration')
        raw = args[-1]
        raw = raw.value if isinstance(raw, ctypes._SimpleCData) else raw
        slot = self.slots.get(int(raw or 0))
        if slot is None:
            return self.fail(f'{name} was issued on a stream the step does not know')
        words = []
        for a, t in zip(args[:-1], types[:-1]):
            v = a.value if isinstance(a, ctypes._SimpleCData) else a
            if t is ctypes.c_float:
                import struct
                words.append(struct.unpack('<I', struct.pack('<f', float(v)))[0])
            else:
                words.append((0 if v is None else int(v)) & 0xFFFFFFFFFFFFFFFF)
        self.items.append(('call', fid, slot, words))

    def build(self):
        if not self.ok:
            raise StepNotRecordable(self.why)
        return CompiledStep(self.items, self.names)


class StepStreams:
    """The streams of a step by name, in slot order (slot 0, ``'main'``, is the caller's), and the hand-overs between
    them.  ``fork`` / ``join`` issue the ordering edge — an event recorded on ``frm`` that ``to`` then waits for — and mark
    it for the recorder of a step that is being recorded, in that order: a recorded step holds the edges that were issued.
    Each edge's event is created once and reused (``wait_stream`` creates one per call, ~5 us of host time); ``bind``
    takes the caller's stream and the recorder of the next step and keeps the events.  ``event``: the event type."""

    def __init__(self, streams, names, rec=None, event=None):
        assert len(streams) == len(names) == len(set(names)) and names[0] == 'main'
        self.streams, self.names, self.rec = list(streams), tuple(names), rec
        self.slot = {name: i for i, name in enumerate(names)}
        self._event, self._events = event or torch.cuda.Event, {}

    def bind(self, cur, rec=None):
        self.streams[0], self.rec = cur, rec
        return self

    def __getitem__(self, name):
        return self.streams[self.slot[name]]

    def _edge(self, frm, to):
        a, b = self.slot[frm], self.slot[to]
        if (a, b) not in self._events:
            self._events[a, b] = self._event()
        self._events[a, b].record(self.streams[a])
        self.streams[b].wait_event(self._events[a, b])
        return a, b

    def fork(self, frm, to):
        """``to`` starts behind everything issued on ``frm`` so far."""
        a, b = self._edge(frm, to)
        if self.rec is not None:
            self.rec.fork(a, b)

    def join(self, frm, to):
        """What ``to`` gets next is ordered behind everything issued on ``frm`` so far."""
        a, b = self._edge(frm, to)
        if self.rec is not None:
            self.rec.join(a, b)


class _RecordingLib:
    """What ``lib()`` hands out while a step is recorded: every entry point that enqueues work (its last parameter is an
    ``ocrf_stream_t``, ``_ENQUEUEING``) is logged, then called; every other one is passed through."""

    def __init__(self, L, rec):
        self._L, self._rec = L, rec

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if name not in _ENQUEUEING:
            return fn
        rec = self._rec

        def logged(*args):
            rec.on_call(name, fn, args)
            return fn(*args)
        return logged


class CompiledStep:
    """The calls of one step inside the library (``ocrf_step``): ``run(main, side, ...)`` issues all of them with one
    host call."""

    def __init__(self, items, names=()):
        L = lib()
        self.names = tuple(names)        # the entry points it holds, in call order
        self._h = ctypes.c_void_p()
        check(L.ocrf_step_create(ctypes.byref(self._h)), 'ocrf_step_create')
        self.n_calls = 0
        for it in items:
            if it[0] == 'call':
                _, fid, slot, words = it
                arr = (ctypes.c_uint64 * len(words))(*words)
                check(L.ocrf_step_add_call(self._h, fid, slot, len(words), arr), 'ocrf_step_add_call')
                self.n_calls += 1
            elif it[0] == 'fork':
                check(L.ocrf_step_add_fork(self._h, it[1], it[2]), 'ocrf_step_add_fork')
            else:
                check(L.ocrf_step_add_join(self._h, it[1], it[2]), 'ocrf_step_add_join')
        self._run2 = L.ocrf_hotpath_step
        self._runn = L.ocrf_step_run

    def run(self, *raw_streams):
        """``raw_streams``: hipStream_t values (ints) in slot order."""
        if len(raw_streams) == 2:
            err = self._run2(self._h, raw_streams[0], raw_streams[1])
        else:
            arr = (ctypes.c_void_p * len(raw_streams))(*raw_streams)
            err = self._runn(self._h, arr, len(raw_streams))
        if err != 0:
            raise OcrfHipError(f'ocrf_hotpath_step failed with hipError_t {err}')

    def __del__(self):
        try:
            if self._h:
                _LIB.ocrf_step_destroy(self._h)
                self._h = None
        except Exception:
            pass


_Recorded = collections.namedtuple('_Recorded', 'step outputs pool generation')
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _same_bits(a, b):
    """``a`` and ``b`` hold the same bits (a NaN equals the same NaN, 0.0 differs from -0.0)."""
    as_int = _BITS[a.element_size()]
    return torch.equal(a.view(as_int), b.view(as_int))


class StepCache:
    """Recorded steps (``CompiledStep``) by key: whatever decides a step's launches and pointers.  ``cache(key, streams,
    fn)``, where ``fn(rec)`` issues the step eagerly on ``streams`` (slot 0 = the caller's) and returns its outputs: the
    first sighting of a key runs eagerly (plans and scratch get built), the second is recorded (``StepRecorder``) with its
    allocations in a memory pool of its own, from the third the recording is replayed and returns the same outputs.

    A recording holds while ``workspace.generation`` stays where it was before recording: a replaced scratch buffer
    means stale pointers, and the key is recorded anew.  ``check(outputs)``, if given, yields the tensors the first replay
    must reproduce bit for bit: the recorder sees the library's calls only, so a torch kernel inside the step would be
    missing from the replay.  A step that cannot be recorded or does not reproduce itself is refused
    (``refused``: why) and every later call runs eagerly.  At most ``size`` recordings and ``seen_size`` first sightings
    are kept: a caller that hands over new tensors every step never repeats a key."""

    def __init__(self, device, size, seen_size, check=None):
        self.device, self.size, self.seen_size, self.check = device, int(size), int(seen_size), check
        self._recorded = {}                    # key -> _Recorded
        self._seen = set()
        self.refused = None

    def __len__(self):
        return len(self._recorded)

    def values(self):
        return self._recorded.values()

    def clear(self):
        self._recorded.clear()
        self._seen.clear()

    def __call__(self, key, streams, fn):
        if self.refused is not None or torch.cuda.is_current_stream_capturing():
            return fn(None)
        generation = workspace.generation(self.device)
        hit = self._recorded.get(key)
        if hit is not None:
            if hit.generation == generation:
                hit.step.run(*[st.cuda_stream for st in streams])
                return hit.outputs
            del self._recorded[key]            # a scratch buffer it baked in was replaced since: record anew
        elif key not in self._seen:
            if len(self._seen) >= self.seen_size:
                self._seen.clear()
            self._seen.add(key)
            return fn(None)
        return self._record(key, streams, fn, generation)

    def _record(self, key, streams, fn, generation):
        rec, pool = StepRecorder(streams), torch.cuda.MemPool()
        with torch.cuda.use_mem_pool(pool, self.device), rec:
            out = fn(rec)
        if not rec.ok:
            self.refused = rec.why
            return out
        if workspace.generation(self.device) != generation:
            return out                         # a scratch buffer was replaced while recording: record again next time
        step = rec.build()
        if self.check is not None:
            got = list(self.check(out))
            want = [t.clone() for t in got]
            step.run(*[st.cuda_stream for st in streams])
            torch.cuda.synchronize(self.device)
            if not all(_same_bits(a, b) for a, b in zip(got, want)):
                self.refused = 'the first replay of the recorded step did not reproduce the step issued call by call'
                return fn(None)
        while len(self._recorded) >= self.size:
            self._recorded.pop(next(iter(self._recorded)))
        self._recorded[key] = _Recorded(step, out, pool, generation)
        return out


def check(err, what):
    if err != 0:
        raise OcrfHipError(f"{what} failed with hipError_t {err}")


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream_ptr(device=None):
    """hipStream_t of torch's current stream on ``device`` as an integer for ctypes."""
    if _raw_stream is not None:
        idx = device.index if isinstance(device, torch.device) else device
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device() if idx is None else idx))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_NO_SWITCH = contextlib.nullcontext()


def on_device(device):
    """``torch.cuda.device(device)`` when the current device differs, else a no-op: the context manager costs
    ~10 us per call, more than the launch it guards (the reference's OptionalCUDAGuard, bev_pool.cpp:42)."""
    idx = device.index if isinstance(device, torch.device) else device
    if idx is None or idx == torch.cuda.current_device():
        return _NO_SWITCH
    return torch.cuda.device(idx)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise OcrfHipError(
                "ocrfdet_amd ops run on the GPU only (HIP kernels, no CPU fallback); got a "
                f"{t.device} tensor")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() > 0 else 0)


def graph_census(cuda_graph):
    """{kernel, memset, memcpy, other} node counts of a ``torch.cuda.CUDAGraph`` built with ``keep_graph=True``."""
    k, ms, mc, o = (ctypes.c_int(0) for _ in range(4))
    check(lib().ocrf_graph_node_census(ctypes.c_void_p(int(cuda_graph.raw_cuda_graph())), ctypes.byref(k), ctypes.byref(ms),
                                       ctypes.byref(mc), ctypes.byref(o)), 'ocrf_graph_node_census')
    return dict(kernel=k.value, memset=ms.value, memcpy=mc.value, other=o.value)


def masked_stream(device, cu_bits=None, priority=0):
    """A torch stream object over a HIP stream limited to the compute units whose bits are set in ``cu_bits`` (an
    iterable of CU indices; None: every CU, with HIP ``priority``).  The HIP stream lives for the process."""
    h = ctypes.c_void_p()
    with torch.cuda.device(device):
        if cu_bits is None:
            check(lib().ocrf_stream_create(None, 0, int(priority), ctypes.byref(h)), 'ocrf_stream_create')
        else:
            bits = sorted(set(int(b) for b in cu_bits))
            n_words = (max(bits) // 32) + 1
            words = (ctypes.c_uint32 * n_words)()
            for b in bits:
                words[b // 32] |= 1 << (b % 32)
            check(lib().ocrf_stream_create(words, n_words, 0, ctypes.byref(h)), 'ocrf_stream_create')
    return torch.cuda.ExternalStream(h.value, device=device)


def diag_stamp(stamps, index):
    """Diagnostic: store the device clock (100 MHz) into ``stamps[index]`` (int64, cuda) when torch's current
    stream reaches this point — works inside a captured graph (``ocrf_diag_stamp``)."""
    require_cuda(stamps)
    launch('ocrf_diag_stamp', stamps.device, stamps.data_ptr() + 8 * index)


class Workspace:
    """Per-device grow-only scratch buffers (torch uint8 tensors, one per tag), so that steady-state calls
    allocate nothing.  Reuse is stream-ordered: a tag is meant for one stream at a time (the side streams of
    ``HotPath`` / ``_core_fused`` use tags of their own).

    Two hazards of replacing a buffer when a larger request arrives are handled here:
    * a captured hipGraph has the raw pointers of the buffers it used baked in — ``hold(device)`` returns
      strong references to every buffer of the device; whoever owns a graph keeps that object for the
      graph's lifetime (``GraphedNeck``), so a later, larger eager request gets a NEW buffer while the
      graph keeps replaying on its own, still allocated one;
    * the caching allocator may hand a freed block to the next allocation on the allocating stream while
      another stream that used the buffer is still running — every stream that asked for the tag is
      recorded on the old buffer (``Tensor.record_stream``) before it is dropped."""

    def __init__(self):
        self._bufs = {}
        self._users = {}                       # key -> raw hipStream_t values that asked for the tag
        self._generation = {}                  # device index -> number of buffers REPLACED so far

    def get(self, device, nbytes, tag="default"):
        idx = device.index if device.index is not None else torch.cuda.current_device()
        key = (idx, tag)
        buf = self._bufs.get(key)
        if _raw_stream is not None:
            users = self._users.get(key)
            if users is None:
                users = self._users[key] = set()
            users.add(_raw_stream(idx))
        if buf is None or buf.numel() < nbytes:
            if buf is not None:
                # whoever baked the old buffer's address into a recorded step (StepCache: HotPath._compiled,
                # ShardedHotPath._segments) sees the generation move and records anew instead of replaying into freed
                # memory
                self._generation[idx] = self._generation.get(idx, 0) + 1
                for raw in self._users.get(key, ()):
                    if raw:                    # 0 = the legacy default stream, the allocator's own
                        buf.record_stream(torch.cuda.ExternalStream(raw, device=buf.device))
                self._users[key] = {_raw_stream(idx)} if _raw_stream is not None else set()
            buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
            self._bufs[key] = buf
        return buf

    def generation(self, device):
        """Number of scratch buffers of ``device`` replaced so far: a recorded step (raw pointers baked in) is valid
        while this has not moved since it was recorded."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        return self._generation.get(idx, 0)

    def hold(self, device):
        """Strong references to every scratch buffer of ``device`` as of now (see the class docstring)."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        return [b for (d, _), b in self._bufs.items() if d == idx]


workspace = Workspace()


class KernelTimer:
    """Device duration of every launch of ONE kernel of the library while armed (HIP events on
    the launch stream, ``ocrf_timer_*`` in include/ocrf_hip.h).  Used by bench.py's roofline leg."""

    def __init__(self, kernel_id, capacity):
        self.kernel_id, self.capacity = kernel_id, int(capacity)
        self._h = ctypes.c_void_p()
        check(lib().ocrf_timer_create(self.capacity, ctypes.byref(self._h)), 'ocrf_timer_create')

    @property
    def kernel_name(self):
        return lib().ocrf_kernel_name(self.kernel_id).decode()

    def arm(self):
        """Several timers (different kernel ids) may be armed at once."""
        check(lib().ocrf_timer_arm(self._h, self.kernel_id), 'ocrf_timer_arm')

    def disarm(self):
        check(lib().ocrf_timer_arm(None, 0), 'ocrf_timer_arm')

    @staticmethod
    def disarm_all():
        check(lib().ocrf_timer_arm(None, 0), 'ocrf_timer_arm')

    def mean_ms(self):
        v = self.read_ms()
        self._count = len(v)
        return sum(v) / len(v) if v else None

    def count(self):
        return getattr(self, '_count', 0)

    def read_ms(self):
        buf = (ctypes.c_float * self.capacity)()
        n = ctypes.c_int(0)
        check(lib().ocrf_timer_read(self._h, buf, self.capacity, ctypes.byref(n)), 'ocrf_timer_read')
        return [float(buf[i]) for i in range(n.value)]

    def close(self):
        if self._h:
            lib().ocrf_timer_destroy(self._h)
            self._h = ctypes.c_void_p()
