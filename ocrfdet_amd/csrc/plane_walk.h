// What the memory-bound plane kernels (resnet_fuse.hip, upsample_cat.hip, bev_align.hip) share: their constants, the
// access width, the host's shape check and launch geometry, the forward walk over a destination plane, and the bf16
// arithmetic of their *_bf16 forms.
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

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---------------------------------------------------------------------------------------------- bf16 arithmetic
// What every bf16 form of these kernels does: widen its operands to float32 (a shift: exact), compute in float32, round
// once to nearest even.
using bf16_t = unsigned short;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float widen(bf16_t h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ float widen_lo(unsigned w) { return __uint_as_float(w << 16); }          // element 0 of a word
__device__ __forceinline__ float widen_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }  // element 1
// float32 -> bf16, to nearest even; a NaN stays a NaN
__device__ __forceinline__ bf16_t round_one(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }
__device__ __forceinline__ unsigned round_pair(float lo, float hi) {
  const f32x2 f = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2));
}

// One element as float32 and back, for a kernel body that serves both element types: the float32 form moves the value,
// the bf16 form widens it and rounds it once.
__device__ __forceinline__ float load_f32(const float* p) { return *p; }
__device__ __forceinline__ float load_f32(const bf16_t* p) { return widen(*p); }
__device__ __forceinline__ void store_f32(float* p, float v) { *p = v; }
__device__ __forceinline__ void store_f32(bf16_t* p, float v) { *p = round_one(v); }

// The same for a group of V consecutive elements, one access (load_group / store_group): 16 bytes for the wide form
// (4 floats, 8 bf16), one element for V = 1.  kWide<T> is the wide form's V, GroupOf<T, V> the type that moves a group
// untouched.
template <typename T>
constexpr int kWide = 16 / (int)sizeof(T);
template <typename T, int V>
struct GroupOf {
  static_assert(V == 1, "a group is one 16-byte access or one element");
  using type = T;
};
template <>
struct GroupOf<float, 4> {
  using type = float4;
};
template <>
struct GroupOf<bf16_t, 8> {
  using type = uint4;
};

// a group as it was loaded -> its V elements as float32
__device__ __forceinline__ void unpack(float t, float (&v)[1]) { v[0] = t; }
__device__ __forceinline__ void unpack(float4 t, float (&v)[4]) { v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w; }
__device__ __forceinline__ void unpack(bf16_t t, float (&v)[1]) { v[0] = widen(t); }
__device__ __forceinline__ void unpack(uint4 t, float (&v)[8]) {
  v[0] = widen_lo(t.x), v[1] = widen_hi(t.x), v[2] = widen_lo(t.y), v[3] = widen_hi(t.y);
  v[4] = widen_lo(t.z), v[5] = widen_hi(t.z), v[6] = widen_lo(t.w), v[7] = widen_hi(t.w);
}
template <int V, typename T>
__device__ __forceinline__ void load_group(const T* p, float (&v)[V]) {
  unpack(*reinterpret_cast<const typename GroupOf<T, V>::type*>(p), v);
}

template <int V>
__device__ __forceinline__ void store_group(float* p, const float (&v)[V]) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    static_assert(V == 1, "a group of floats is 4 or 1");
    *p = v[0];
  }
}
template <int V>
__device__ __forceinline__ void store_group(bf16_t* p, const float (&v)[V]) {
  if constexpr (V == 8) {
    *reinterpret_cast<uint4*>(p) = make_uint4(round_pair(v[0], v[1]), round_pair(v[2], v[3]), round_pair(v[4], v[5]),
                                              round_pair(v[6], v[7]));
  } else {
    static_assert(V == 1, "a group of bf16 is 8 or 1");
    *p = round_one(v[0]);
  }
}

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
