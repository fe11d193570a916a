// Single-launch prefix sums: the decoupled look-back as device functions a kernel folds into its own work
// (lss_intervals_kernel) and as a ready-made in-place exclusive scan.  Internal to the units that launch such kernels
// (index_prep.hip, radix_sort.hip): all in the unnamed namespace, each unit instantiates what it uses and no more.
#pragma once
#include <hip/hip_runtime.h>

#include "launch.h"

namespace {

constexpr int kBlock = 256;
constexpr int kItems = 8;                     // values per thread of a scan (keys per thread and radix pass)
constexpr int kChunk = kBlock * kItems;       // 2048 values per workgroup

// exclusive prefix of v over the 256 threads of the workgroup (each thread of a scan owns 8 consecutive
// values, so a wave touches 2 KB of contiguous memory per load)
template <typename T>
__device__ __forceinline__ T block_exclusive(T v, T* s_wave, T* block_total) {
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  T inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) {
    const T c = s_wave[w];
    if (w < wave) base += c;
    tot += c;
  }
  if (block_total) *block_total = tot;
  return base + inc - v;
}

// ---------------------------------------------------------------------------------------------
// Single-launch prefix sums: decoupled look-back over TICKET-ordered tiles.  state[0] is the ticket
// counter, state[1 + t] the 64-bit word of tile t: bits 63:62 = 0 nothing yet | 1 the tile's own sum |
// 2 its inclusive prefix, bits 61:0 the value — one word, written and read with agent-scope atomics,
// so a reader never sees a value without its status.  A workgroup takes the next ticket before it
// does anything else: the tiles it may wait for hold smaller tickets, i.e. are already running —
// every wave reaches its exit whatever the scheduling order.  `state` must be zero before the launch.
// ---------------------------------------------------------------------------------------------
constexpr unsigned long long kLbValue = (1ull << 62) - 1;

__device__ __forceinline__ void lb_publish(unsigned long long* state, int tile, unsigned status, unsigned long long v) {
  __hip_atomic_store(state + 1 + tile, ((unsigned long long)status << 62) | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ticket of this workgroup (uniform); contains a barrier
__device__ __forceinline__ int lb_ticket(unsigned long long* state, int* s_tile) {
  if (threadIdx.x == 0) *s_tile = (int)atomicAdd(reinterpret_cast<unsigned*>(state), 1u);
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(*s_tile);      // known-uniform: what depends on it stays in SGPRs
}

template <int NW = kBlock / 64>
struct LbShared {
  unsigned long long inc[NW], none[NW], sum[NW], run;
};

// exclusive prefix of this tile given its own sum `tot` (uniform).  All 64 NW threads call; contains barriers.
// The look-back reads 64 NW predecessors per round (thread i reads tile hi - i): an agent-scope load is a
// round trip to memory, and while every tile still holds only its own sum a tile t needs ~t / (2 kBlock) rounds.
template <int NW>
__device__ __forceinline__ unsigned long long lb_tile_prefix(unsigned long long* state, int tile, unsigned long long tot,
                                                             LbShared<NW>* sh) {
  constexpr int kThreads = NW * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {
    lb_publish(state, tile, tile == 0 ? 2u : 1u, tot);
    sh->run = 0;
  }
  int hi = tile - 1;
  int spins = 0;
  while (hi >= 0) {                                   // uniform: hi, and the decisions below, are the same everywhere
    const int j = hi - tid;
    const unsigned long long w = j >= 0 ? __hip_atomic_load(state + 1 + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                        : (2ull << 62);                 // before tile 0: inclusive prefix 0
    const unsigned status = (unsigned)(w >> 62);
    const unsigned long long inc = __ballot(status == 2), none = __ballot(status == 0);
    if (lane == 0) { sh->inc[wave] = inc; sh->none[wave] = none; }
    __syncthreads();
    // nearest predecessor with a full prefix, as a thread index; everything nearer must at least hold its sum
    int first = kThreads;
    bool wait = false;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      if (first < kThreads) break;
      const unsigned long long i = sh->inc[k], n = sh->none[k];
      const int f = i ? __ffsll((long long)i) - 1 : 64;
      const unsigned long long need = f >= 63 ? ~0ull : ((2ull << f) - 1ull);
      wait = wait || (n & need) != 0;
      if (f < 64) first = k * 64 + f;
    }
    __syncthreads();                                  // sh->inc / none are rewritten by the next round
    if (wait) {
      // Every tile this one waits for holds a smaller ticket and is running, so the wait ends within microseconds —
      // unless the state words are being overwritten, e.g. by a second call sharing this scratch on another stream.
      // A wave must not spin on a shared GPU for ever, and a trap would take the whole process down: after ~a second
      // the tile gives up, raises the error bit of the state block (bit 63 of word 0; the ticket counter is the low
      // half) and carries on with what it has — the call's last kernel turns the bit into counts = -1, which the
      // poolings read as "no points" and the host wrappers as an OcrfHipError.
      if (++spins > (1 << 20)) {
        if (tid == 0) atomicOr(state, 1ull << 63);
        break;
      }
      __builtin_amdgcn_s_sleep(2);
      continue;                                       // something nearer than `first` is unpublished: read again
    }
    unsigned long long v = tid <= first ? (w & kLbValue) : 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) sh->sum[wave] = v;
    __syncthreads();
    if (tid == 0) {
      unsigned long long r = sh->run;
#pragma unroll
      for (int k = 0; k < NW; ++k) r += sh->sum[k];
      sh->run = r;
    }
    if (first < kThreads) break;
    hi -= kThreads;
  }
  __syncthreads();
  const unsigned long long prefix = sh->run;
  if (tid == 0 && tile > 0) lb_publish(state, tile, 2u, prefix + tot);
  return prefix;
}

inline size_t lb_state_bytes(long n_tiles) { return ((size_t)n_tiles + 1) * 8; }

// in-place exclusive scan of n non-negative values (sums < 2^62), one launch of ceil(n / kChunk) workgroups
template <typename T>
__global__ __launch_bounds__(kBlock) void scan_lookback_kernel(T* __restrict__ data, long n, T* __restrict__ total,
                                                               unsigned long long* __restrict__ state) {
  __shared__ T s_wave[kBlock / 64];
  __shared__ int s_tile;
  __shared__ LbShared<> s_lb;
  const int tile = lb_ticket(state, &s_tile);
  const long base = (long)tile * kChunk + (long)threadIdx.x * kItems;
  T v[kItems];
  T sum = 0;
#pragma unroll
  for (int i = 0; i < kItems; ++i) {
    v[i] = base + i < n ? data[base + i] : (T)0;
    sum += v[i];
  }
  T tot;
  const T local = block_exclusive<T>(sum, s_wave, &tot);
  const unsigned long long prefix = lb_tile_prefix(state, tile, (unsigned long long)tot, &s_lb);
  T run = (T)prefix + local;
#pragma unroll
  for (int i = 0; i < kItems; ++i) {
    if (base + i < n) data[base + i] = run;
    run += v[i];
  }
  if (total && tile == (int)gridDim.x - 1 && threadIdx.x == 0) *total = (T)prefix + tot;
}

template <typename T>
inline void scan_exclusive_lookback(T* data, long n, T* total, unsigned long long* zeroed_state, hipStream_t stream) {
  const int nb = (int)((n + kChunk - 1) / kChunk);
  ocrf::launch(OCRF_K_SCAN, scan_lookback_kernel<T>, dim3(nb), dim3(kBlock), 0, stream, data, n, total, zeroed_state);
}

}  // namespace
