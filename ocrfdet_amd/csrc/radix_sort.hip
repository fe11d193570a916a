// Stable LSD radix sort of 32-bit keys, one 9-bit digit per pass (histogram -> exclusive scan of the [digit][workgroup]
// table -> stable scatter), and the in-place exclusive scan of ints (radix_sort.h).  One workspace layout and one driver
// of the passes serve both users: the LSS index preparation (index_prep.hip: voxel keys, 1-3 passes into the rank vectors)
// and the render-plan build (raster_plan.hip: view | depth keys, 4 passes into the plan's lists; three scans).
#include <hip/hip_runtime.h>

#include "launch.h"
#include "lookback_scan.h"
#include "radix_sort.h"

namespace {

using ocrf::kBins;
using ocrf::kRadixBits;
static_assert(kChunk == ocrf::kSortChunk, "a workgroup sorts kItems keys per thread");

__global__ __launch_bounds__(kBlock) void radix_hist_kernel(const unsigned* __restrict__ keys, int n, int shift,
                                                            int n_wg, int* __restrict__ table) {
  __shared__ int s_hist[kBins];
  for (int i = threadIdx.x; i < kBins; i += kBlock) s_hist[i] = 0;
  __syncthreads();
  const int base = blockIdx.x * kChunk;
  // the thread's keys in ONE round trip (clamped addresses; `if (i < n) load` per key was a branch and a wait per key)
  unsigned key[kItems];
#pragma unroll
  for (int it = 0; it < kItems; ++it) key[it] = keys[min(base + it * kBlock + (int)threadIdx.x, n - 1)];
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const int i = base + it * kBlock + threadIdx.x;
    if (i < n) atomicAdd(&s_hist[(key[it] >> shift) & (kBins - 1)], 1);
  }
  __syncthreads();
  for (int d = threadIdx.x; d < kBins; d += kBlock) table[(long)d * n_wg + blockIdx.x] = s_hist[d];
}

// Stable scatter of one pass.  A wave owns 512 consecutive keys of the workgroup's chunk and walks
// them 64 at a time in order; the rank of a key among equal digits of its step is a ballot match,
// running per-digit positions live in LDS (LDS operations of one wave execute in order).
// EMIT 1 / 2 (the LAST pass of the LSS preparation's / a render-plan build's sort): the consumer's own arrays leave with
// the sorted keys (radix_emit.h); the launch that read the pairs back to write them is gone.
struct ScatterExtra {
  ocrf::RadixRankEmit lss;
  ocrf::RadixPlanEmit plan;
};
template <bool IMPLICIT_VALS, int EMIT = 0>
__global__ __launch_bounds__(kBlock) void radix_scatter_kernel(
    const unsigned* __restrict__ keys_in, const int* __restrict__ vals_in, int n, int shift, int n_wg,
    const int* __restrict__ table, unsigned* __restrict__ keys_out, int* __restrict__ vals_out, ScatterExtra x) {
  __shared__ int s_pos[kBlock / 64][kBins];
  const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
  for (int i = tid; i < (kBlock / 64) * kBins; i += kBlock) (&s_pos[0][0])[i] = 0;
  __syncthreads();
  const int wbase = blockIdx.x * kChunk + wave * (kChunk / (kBlock / 64));
  unsigned key[kItems];
  int val[kItems];
  bool ok[kItems];
  // keys (and values) of the thread in ONE round trip, at clamped addresses
#pragma unroll
  for (int s = 0; s < kItems; ++s) {
    const int i = wbase + s * 64 + lane;
    ok[s] = i < n;
    key[s] = keys_in[min(i, n - 1)];
    val[s] = IMPLICIT_VALS ? i : vals_in[min(i, n - 1)];
  }
  // EMIT 2: what the value points at, requested now (a gather per key inside the ordered walk below would be a round
  // trip per step)
  int e_id[EMIT == 2 ? kItems : 1];
  float2 e_pix[EMIT == 2 ? kItems : 1];
  if constexpr (EMIT == 2) {
#pragma unroll
    for (int s = 0; s < kItems; ++s) {
      const int e = val[s];
      e_id[s] = x.plan.rec_id[e];
      const float4 q1 = x.plan.e_q1[e];
      e_pix[s] = make_float2(q1.z, q1.w);
    }
  }
#pragma unroll
  for (int s = 0; s < kItems; ++s) {
    if (!ok[s]) key[s] = 0u;
    if (ok[s]) atomicAdd(&s_pos[wave][(key[s] >> shift) & (kBins - 1)], 1);
  }
  __syncthreads();
  // per digit: global base of this workgroup, then the waves in order
  for (int d = tid; d < kBins; d += kBlock) {
    int run = table[(long)d * n_wg + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
      const int c = s_pos[w][d];
      s_pos[w][d] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < kItems; ++s) {
    const int digit = (int)((key[s] >> shift) & (kBins - 1));
    unsigned long long same = __ballot(ok[s]);
#pragma unroll
    for (int b = 0; b < kRadixBits; ++b) {
      const unsigned long long m = __ballot((digit >> b) & 1);
      same &= ((digit >> b) & 1) ? m : ~m;
    }
    if (ok[s]) {
      const int rank = __popcll(same & ((1ull << lane) - 1ull));
      const int pos = s_pos[wave][digit] + rank;
      keys_out[pos] = key[s];
      if constexpr (EMIT != 2) vals_out[pos] = val[s];
      if constexpr (EMIT == 1) x.lss.ranks_feat[pos] = (val[s] / x.lss.DHW) * x.lss.HW + val[s] % x.lss.HW;
      if constexpr (EMIT == 2) {
        x.plan.s_e[pos] = (unsigned)val[s];
        x.plan.s_id[pos] = (unsigned)e_id[s];
        x.plan.s_key[pos] = (key[s] & x.plan.depth_mask) + x.plan.key_base;
        x.plan.s_pix[pos] = e_pix[s];
      }
      if (rank == 0) s_pos[wave][digit] = pos + __popcll(same);      // leader advances the digit
    }
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace

namespace ocrf {

SortLayout radix_sort_layout(long n, bool keys_a_inside, size_t tail_state_bytes) {
  SortLayout w{};
  auto take = [&](size_t b) { size_t o = w.bytes; w.bytes += align_up(b, 256); return o; };
  w.n_wg = (int)((n + kChunk - 1) / kChunk);
  w.keys_a = keys_a_inside ? take((size_t)n * 4) : 0;
  w.keys_b = take((size_t)n * 4);
  w.vals_a = take((size_t)n * 4);
  w.vals_b = take((size_t)n * 4);
  w.table = take((size_t)kBins * w.n_wg * 4);
  const size_t pass_state = lb_state_bytes(((long)kBins * w.n_wg + kChunk - 1) / kChunk);
  w.st_words = (long)(pass_state / 8);
  w.state = take(4 * pass_state + tail_state_bytes);
  w.state_bytes = w.bytes - w.state;
  return w;
}

hipError_t radix_sort_passes(unsigned* keys, int n, int passes, bool hist0_ready, void* workspace, const SortLayout& w,
                             const RadixRankEmit* ranks, const RadixPlanEmit* plan, unsigned** keys_out, int** vals_out,
                             hipStream_t stream) {
  if (passes < 1 || passes > 4 || (ranks && plan) || (plan && passes == 1)) return hipErrorInvalidValue;
  char* base = static_cast<char*>(workspace);
  unsigned* kbuf[2] = {keys, reinterpret_cast<unsigned*>(base + w.keys_b)};
  int* vbuf[2] = {reinterpret_cast<int*>(base + w.vals_a), reinterpret_cast<int*>(base + w.vals_b)};
  int* table = reinterpret_cast<int*>(base + w.table);
  auto* state = reinterpret_cast<unsigned long long*>(base + w.state);
  if (!hist0_ready)
    if (hipError_t e = zero_async(state, w.state_bytes, stream); e != hipSuccess) return e;
  const int n_wg = w.n_wg;
  const ScatterExtra x{ranks ? *ranks : RadixRankEmit{}, plan ? *plan : RadixPlanEmit{}};
  // [pass 0: a key's value is its position][what the pass emits]; EMIT 2 still writes the sorted keys
  static constexpr decltype(&radix_scatter_kernel<false, 0>) kScatter[2][3] = {
      {radix_scatter_kernel<false, 0>, radix_scatter_kernel<false, 1>, radix_scatter_kernel<false, 2>},
      {radix_scatter_kernel<true, 0>, radix_scatter_kernel<true, 1>, nullptr}};
  int cur = 0;
  for (int pass = 0; pass < passes; ++pass) {
    const int shift = pass * kRadixBits;
    const bool last = pass == passes - 1;
    if (pass > 0 || !hist0_ready)
      launch(OCRF_K_RADIX_HIST, radix_hist_kernel, dim3(n_wg), dim3(kBlock), 0, stream,
             static_cast<const unsigned*>(kbuf[cur]), n, shift, n_wg, table);
    scan_exclusive_lookback(table, (long)kBins * n_wg, (int*)nullptr, state + pass * w.st_words, stream);
    if (last && *keys_out) kbuf[cur ^ 1] = *keys_out;
    if (last && *vals_out) vbuf[cur ^ 1] = *vals_out;
    launch(OCRF_K_RADIX_SCATTER, kScatter[pass == 0][!last ? 0 : ranks ? 1 : plan ? 2 : 0], dim3(n_wg), dim3(kBlock), 0,
           stream, static_cast<const unsigned*>(kbuf[cur]), static_cast<const int*>(pass == 0 ? nullptr : vbuf[cur]), n,
           shift, n_wg, static_cast<const int*>(table), kbuf[cur ^ 1], vbuf[cur ^ 1], x);
    cur ^= 1;
  }
  *keys_out = kbuf[cur];
  *vals_out = plan ? nullptr : vbuf[cur];
  return hipGetLastError();
}

size_t radix_sort_ids_bytes(int n) { return n > 0 ? radix_sort_layout(n, false, 0).bytes : 0; }

hipError_t radix_sort_ids(unsigned* keys, int n, int key_bits, void* scratch, size_t scratch_bytes,
                          const unsigned** sorted_keys, const int** sorted_ids, hipStream_t stream,
                          const RadixPlanEmit* plan_emit) {
  if (n <= 0 || key_bits <= 0 || key_bits > 32 || !keys || !scratch) return hipErrorInvalidValue;
  const SortLayout w = radix_sort_layout(n, false, 0);
  if (scratch_bytes < w.bytes) return hipErrorInvalidValue;
  unsigned* k = nullptr;
  int* v = nullptr;
  const hipError_t e = radix_sort_passes(keys, n, radix_passes_of_bits(key_bits), false, scratch, w, nullptr, plan_emit,
                                         &k, &v, stream);
  *sorted_keys = k;
  *sorted_ids = v;
  return e;
}

void radix_sort_states(void* scratch, int n, int key_bits, const unsigned long long** states, int* n_states,
                       long* stride_words) {
  const SortLayout w = radix_sort_layout(n, false, 0);
  *states = reinterpret_cast<const unsigned long long*>(static_cast<char*>(scratch) + w.state);
  *n_states = radix_passes_of_bits(key_bits);
  *stride_words = w.st_words;
}

size_t exclusive_scan_bytes(long n) { return n > 0 ? align_up(lb_state_bytes((n + kChunk - 1) / kChunk), 256) : 0; }

hipError_t exclusive_scan_ints(int* data, long n, int* total, void* scratch, size_t scratch_bytes, hipStream_t stream) {
  if (n <= 0 || !data || !scratch || scratch_bytes < exclusive_scan_bytes(n)) return hipErrorInvalidValue;
  hipError_t e = zero_async(scratch, exclusive_scan_bytes(n), stream);
  if (e != hipSuccess) return e;
  scan_exclusive_lookback<int>(data, n, total, static_cast<unsigned long long*>(scratch), stream);
  return hipGetLastError();
}

}  // namespace ocrf

extern "C" {

size_t ocrf_diag_radix_sort_workspace_bytes(int n) { return ocrf::radix_sort_ids_bytes(n); }

int ocrf_diag_radix_sort_states(void* workspace, int n, int key_bits, size_t* offset_bytes, int* n_states,
                                long* stride_words) {
  if (!workspace || n <= 0 || key_bits <= 0 || key_bits > 32 || !offset_bytes || !n_states || !stride_words)
    return (int)hipErrorInvalidValue;
  const unsigned long long* states = nullptr;
  ocrf::radix_sort_states(workspace, n, key_bits, &states, n_states, stride_words);
  *offset_bytes = (size_t)(reinterpret_cast<const char*>(states) - static_cast<const char*>(workspace));
  return 0;
}

int ocrf_diag_radix_sort(unsigned* keys, int n, int key_bits, unsigned* out_keys, int* out_ids, void* workspace,
                         size_t workspace_bytes, ocrf_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!out_keys || !out_ids) return (int)hipErrorInvalidValue;
  const unsigned* sk = nullptr;
  const int* si = nullptr;
  hipError_t e = ocrf::radix_sort_ids(keys, n, key_bits, workspace, workspace_bytes, &sk, &si, stream);
  if (e != hipSuccess) return (int)e;
  e = hipMemcpyAsync(out_keys, sk, (size_t)n * 4, hipMemcpyDeviceToDevice, stream);
  if (e != hipSuccess) return (int)e;
  return (int)hipMemcpyAsync(out_ids, si, (size_t)n * 4, hipMemcpyDeviceToDevice, stream);
}

}  // extern "C"
