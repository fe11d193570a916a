// One host call per step: a recorded list of this library's own C-ABI calls, replayed from C.
//
// The reference launches one pybind call per op (mmdet3d/ops/bev_pool_v2/src/bev_pool.cpp:30-57); a step of the hot
// path here is ~18 kernel launches behind 7 entry points on two HIP streams, and issued from Python (ctypes argument
// conversion, torch stream / event objects) it costs the host 225 us — as long as the device needs to run it.  A step
// object holds the calls of one step (entry point + argument values, recorded once by ocrfdet_amd._lib.StepRecorder
// while the step ran eagerly) and the fork / join points of its streams; ocrf_hotpath_step replays them: the same
// entry points, the same arguments, the caller's streams.  Nothing is captured into a hipGraph (replaying the step as a
// graph was measured slower: 0.28 vs 0.23 ms) — the launches are issued eagerly, only without the interpreter.
//
// Which entry points a step can hold is one list (kFns); how many argument words each takes and how each word is
// converted back to its parameter's type are derived from the prototypes in ocrf_hip.h at compile time (Signature).
//
// Every pointer argument is used as recorded: the caller keeps the tensors alive and in place (persistent inputs,
// outputs and scratch), exactly as for a captured graph.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "ocrf_hip.h"

namespace {

constexpr int kMaxArgs = 40;
constexpr int kMaxStreams = 8;

// A recorded argument word as the declared type of its parameter: a pointer from its address, a float from its bit
// pattern (the low 32 bits), an integer from its 64-bit two's complement.  Any other parameter type does not compile.
template <typename T>
T word_as(uint64_t w) {
  if constexpr (std::is_pointer_v<T>) {
    return reinterpret_cast<T>(static_cast<uintptr_t>(w));
  } else if constexpr (std::is_same_v<T, float>) {
    const uint32_t b = static_cast<uint32_t>(w);
    float f;
    std::memcpy(&f, &b, 4);
    return f;
  } else {
    static_assert(std::is_integral_v<T>, "a step argument is a pointer, a float or an integer");
    return static_cast<T>(static_cast<int64_t>(w));
  }
}

// What a step needs of an entry point, derived from its prototype: how many argument words it takes (the trailing
// stream excluded) and how to call it with them.
template <typename F>
struct Signature;
template <typename R, typename... A>
struct Signature<R (*)(A...)> {
  static constexpr int n_args = int(sizeof...(A)) - 1;
  static_assert(std::is_same_v<R, int>, "an entry point a step holds returns its hipError_t as int");
  static_assert(std::is_same_v<std::tuple_element_t<sizeof...(A), std::tuple<void, A...>>, ocrf_stream_t>,
                "an entry point a step holds takes its ocrf_stream_t last");
  static_assert(n_args <= kMaxArgs, "raise kMaxArgs");

  template <R (*fn)(A...), size_t... I>
  static int call(const uint64_t* a, ocrf_stream_t s, std::index_sequence<I...>) {
    return fn(word_as<std::tuple_element_t<I, std::tuple<A...>>>(a[I])..., s);
  }
};

template <auto fn>
int invoke(const uint64_t* a, ocrf_stream_t s) {
  using Sig = Signature<decltype(fn)>;
  return Sig::template call<fn>(a, s, std::make_index_sequence<Sig::n_args>{});
}

struct FnInfo {
  const char* name;
  int n_args;          // without the trailing stream
  int (*invoke)(const uint64_t* args, ocrf_stream_t stream);
};

#define OCRF_STEP_FN(fn) FnInfo{#fn, Signature<decltype(&fn)>::n_args, &invoke<&fn>}

// The entry points a step can hold; a position in this list is the id ocrf_step_fn_id returns.  The per-sample step
// (nothing calibration- or pose-dependent cached) adds the index preparation, pooling on device-side counts and the
// per-call render; their host-pointer arguments (grid bounds, pc_range) are read at replay like at the call: the caller
// keeps them alive (ocrfdet_amd.index_prep._host_floats).
const FnInfo kFns[] = {
    OCRF_STEP_FN(ocrf_bev_pool_v2_nchw_planned), OCRF_STEP_FN(ocrf_bev_pool_v2_nchw_mfma),
    OCRF_STEP_FN(ocrf_bev_pool_cell_weights),    OCRF_STEP_FN(ocrf_bev_pool_v2_nchw_panel),
    OCRF_STEP_FN(ocrf_rasterize_planned),        OCRF_STEP_FN(ocrf_hoa1_forward),
    OCRF_STEP_FN(ocrf_hoa_v2b_forward),          OCRF_STEP_FN(ocrf_hoa_channel_stats),
    OCRF_STEP_FN(ocrf_hoa_opacity_mask_gate),    OCRF_STEP_FN(ocrf_stream_write_value32),
    OCRF_STEP_FN(ocrf_raster_plan_build),        OCRF_STEP_FN(ocrf_rasterize_forward),
    OCRF_STEP_FN(ocrf_bev_pool_v2_nchw_dyn),     OCRF_STEP_FN(ocrf_lss_prepare),
    OCRF_STEP_FN(ocrf_ht_prepare),               OCRF_STEP_FN(ocrf_geometry_blocks),
    OCRF_STEP_FN(ocrf_rasterize_forward_sets),   OCRF_STEP_FN(ocrf_bev_pool_v2_nchw_panel_stats),
};
#undef OCRF_STEP_FN
constexpr int kFnCount = int(sizeof(kFns) / sizeof(kFns[0]));

struct Cmd {
  int kind;            // 0: call, 1: fork (from -> to), 2: join (`to` waits for `from`)
  int fn, slot, from, to;
  uint64_t a[kMaxArgs];      // ints / pointers / sizes as 64-bit words, floats as their bit pattern
};

}  // namespace

struct ocrf_step {
  std::vector<Cmd> cmds;
  hipEvent_t events[2 * kMaxStreams * kMaxStreams];      // one per (fork | join, from, to), created on first use
  int device;
};

extern "C" {

// id of an entry point a step can hold, or -1
int ocrf_step_fn_id(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < kFnCount; ++i)
    if (std::strcmp(name, kFns[i].name) == 0) return i;
  return -1;
}
// number of arguments (without the trailing stream) the entry point takes, or -1
int ocrf_step_fn_args(int fn) { return (fn >= 0 && fn < kFnCount) ? kFns[fn].n_args : -1; }

int ocrf_step_create(ocrf_step** out) {
  if (!out) return (int)hipErrorInvalidValue;
  ocrf_step* s = new ocrf_step();
  for (auto& e : s->events) e = nullptr;
  s->device = -1;
  *out = s;
  return 0;
}

void ocrf_step_destroy(ocrf_step* s) {
  if (!s) return;
  for (auto& e : s->events)
    if (e) (void)hipEventDestroy(e);
  delete s;
}

// a call of entry point `fn` on stream slot `slot` with `n_args` argument words (the stream argument is not among them)
int ocrf_step_add_call(ocrf_step* s, int fn, int slot, int n_args, const uint64_t* args) {
  if (!s || fn < 0 || fn >= kFnCount || slot < 0 || slot >= kMaxStreams || n_args != kFns[fn].n_args || !args)
    return (int)hipErrorInvalidValue;
  Cmd c;
  std::memset(&c, 0, sizeof(c));
  c.kind = 0; c.fn = fn; c.slot = slot;
  std::memcpy(c.a, args, sizeof(uint64_t) * (size_t)n_args);
  s->cmds.push_back(c);
  return 0;
}

// stream `to` continues only after everything issued to `from` so far (kind 1: a fork of `to` off `from`; kind 2: `to`
// joins `from`) — the same event record + wait either way; the two kinds keep their own events
static int add_edge(ocrf_step* s, int kind, int from, int to) {
  if (!s || from < 0 || from >= kMaxStreams || to < 0 || to >= kMaxStreams || from == to) return (int)hipErrorInvalidValue;
  Cmd c;
  std::memset(&c, 0, sizeof(c));
  c.kind = kind; c.from = from; c.to = to;
  s->cmds.push_back(c);
  return 0;
}
int ocrf_step_add_fork(ocrf_step* s, int from, int to) { return add_edge(s, 1, from, to); }
int ocrf_step_add_join(ocrf_step* s, int from, int to) { return add_edge(s, 2, from, to); }

int ocrf_step_size(const ocrf_step* s) { return s ? (int)s->cmds.size() : -1; }

// Replay: every call on the stream of its slot, in recorded order.
int ocrf_step_run(ocrf_step* s, const ocrf_stream_t* streams, int n_streams) {
  if (!s || !streams || n_streams <= 0 || n_streams > kMaxStreams) return (int)hipErrorInvalidValue;
  for (const Cmd& c : s->cmds) {
    if (c.kind == 0) {
      if (c.slot >= n_streams) return (int)hipErrorInvalidValue;
      const int e = kFns[c.fn].invoke(c.a, streams[c.slot]);
      if (e != 0) return e;
    } else {
      if (c.from >= n_streams || c.to >= n_streams) return (int)hipErrorInvalidValue;
      hipEvent_t& ev = s->events[((c.kind - 1) * kMaxStreams + c.from) * kMaxStreams + c.to];
      if (!ev) {
        const hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) return (int)e;
      }
      hipError_t e = hipEventRecord(ev, static_cast<hipStream_t>(streams[c.from]));
      if (e != hipSuccess) return (int)e;
      e = hipStreamWaitEvent(static_cast<hipStream_t>(streams[c.to]), ev, 0);
      if (e != hipSuccess) return (int)e;
    }
  }
  return 0;
}

// The two-stream form the hot path uses: slot 0 = the caller's stream, slot 1 = the render stream
int ocrf_hotpath_step(ocrf_step* s, ocrf_stream_t main_stream, ocrf_stream_t side_stream) {
  const ocrf_stream_t streams[2] = {main_stream, side_stream};
  return ocrf_step_run(s, streams, 2);
}

}  // extern "C"
