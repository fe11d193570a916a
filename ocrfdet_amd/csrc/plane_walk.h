// What the memory-bound plane kernels (resnet_fuse.hip, upsample_cat.hip) share: their constants, the access width, the
// host's shape check and launch geometry, and the forward walk over a destination plane.
//
// Layout.  A forward kernel sees every (b, c) destination plane as a flat run of P = Hout * Wout floats and cuts it into
// chunks of kThreads x kGroups x V floats: a workgroup takes (plane, chunk) units in a grid-stride loop (the grid is
// capped at kMaxBlocks), a thread kGroups groups of V consecutive floats per unit, kThreads * V floats apart.  V = 4
// when P is a multiple of 4 and the pointers the kernel accesses by groups are 16-byte aligned: a group is then one
// 16-byte access, a wave touches 1 KiB contiguously, and a group may straddle two rows (the width need not be a
// multiple of 4: the column wraps inside the group).  V = 1 otherwise: the same code with 4-byte accesses.  The kernels
// index with int, so every operand stays below 2 GiB, and they keep one table entry per row and per column in LDS, so
// Hout + Wout stays within kMaxAxisSum.
//
// The width of an access is counted in bytes: with 16-bit elements (bf16, passed as unsigned short) a 16-byte group is
// V = 8 elements, P has to be a multiple of 8 for it, and the narrow form is a 2-byte access.  Walk<V> counts in
// elements and does not care what they are.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace plane {

constexpr int kThreads = 256;
constexpr int kGroups = 4;                         // groups of V floats per thread and unit
constexpr int kMaxBlocks = 2048;                   // 8 workgroups per CU; the rest of the work is grid-strided
constexpr int kMaxAxisSum = 8192;                  // Hout + Wout: the tables take up to 8 bytes per entry of 64 KiB LDS
constexpr long long kTwoGiB = 1LL << 31;

template <int V>
struct Vec;
template <>
struct Vec<4> {
  using type = float4;
};
template <>
struct Vec<1> {
  using type = float;
};

// the same for 16-bit elements: 8 of them in one 16-byte access, or one
template <int V>
struct Vec16;
template <>
struct Vec16<8> {
  using type = uint4;
};
template <>
struct Vec16<1> {
  using type = unsigned short;
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// `planes` destination planes of Hout x Wout elements of `elem_bytes` each: the tables fit, and the destination-sized
// operands (the largest) stay below 2 GiB
inline bool planes_ok(long long planes, long long Hout, long long Wout, long long elem_bytes = sizeof(float)) {
  if (Hout + Wout > kMaxAxisSum) return false;
  return planes < kTwoGiB && planes * Hout * Wout * elem_bytes < kTwoGiB;
}

inline unsigned capped_grid(long long blocks) { return (unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks); }

// launch geometry of a forward walk over `planes` planes of P elements in groups of V
struct Units {
  int chunks;                                      // per plane
  long long units;                                 // planes * chunks, < 2^29 + planes
  unsigned grid;
};

inline Units units_of(long long planes, long long P, int V) {
  const int per_unit = kThreads * kGroups * V;
  Units n;
  n.chunks = (int)((P + per_unit - 1) / per_unit);
  n.units = planes * n.chunks;
  n.grid = capped_grid(n.units);
  return n;
}

// One thread's part of the walk over a plane of Wout columns.  groups(first(chunk), P, f) calls f(idx, y, x) for each
// of the thread's kGroups groups of that chunk that lies inside the plane (P % V == 0: a group is inside or outside),
// idx its first float and (y, x) that float's row and column; values(v, y, x, f) fills v[k] = f(row, column) for the V
// floats of a group that starts at (y, x).
template <int V>
struct Walk {
  static constexpr int kStep = kThreads * V;       // floats between a thread's groups
  int Wout, step_y, step_x;

  __device__ __forceinline__ explicit Walk(int Wout_) : Wout(Wout_) {
    step_y = kStep / Wout;
    step_x = kStep - step_y * Wout;
  }

  // the first float of the thread's first group in `chunk`
  __device__ __forceinline__ int first(int chunk) const { return chunk * (kStep * kGroups) + (int)threadIdx.x * V; }

  template <typename F>
  __device__ __forceinline__ void groups(int first, int P, F&& f) const {
    int oy = first / Wout, ox = first - oy * Wout;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
      const int idx = first + g * kStep;
      if (idx < P) f(idx, oy, ox);
      oy += step_y;
      ox += step_x;
      if (ox >= Wout) {
        ox -= Wout;
        ++oy;
      }
    }
  }

  template <typename F>
  __device__ __forceinline__ void values(float (&v)[V], int y, int x, F&& f) const {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      v[k] = f(y, x);
      if (++x == Wout) {
        x = 0;
        ++y;                                       // past the last row only behind the group's last element
      }
    }
  }
};

}  // namespace plane
