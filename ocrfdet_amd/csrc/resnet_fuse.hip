// The memory-bound passes between the image encoder's convolutions (ocrfdet_amd/image_encoder.py), each as ONE launch:
//
//   add_relu forward       out  = relu(a + b)                 the residual tail of every ResNet block
//   add_relu backward      grad = out <= 0 ? 0 : grad_out     the gradient of both addends
//   upsample_add forward   out  = dst + nearest(src)          CustomFPN's top-down step
//                                                             (mmdet3d/models/necks/fpn.py:190-196)
//   upsample_add backward  grad_src = the transpose of nearest() as a gather; the gradient of dst is grad_out itself
//
// No atomics, no workspace, no host synchronisation; repeated runs are bit-identical.  All four are HBM-bound: eager
// torch makes two launches and five tensor passes of the tail (a + b -> t; t -> relu_ -> t), this file one launch and
// three passes.
//
// Arithmetic.  a + b is one float32 addition, rounded once; the ReLU is `s < 0 ? 0 : s`, so that a NaN sum stays NaN
// (torch's clamp_min) and -0 stays a zero.  The backward is torch's threshold_backward: `out <= 0 ? 0 : grad_out`, so
// that a NaN `out` passes the gradient.  nearest() restates torch's mode='nearest', per axis, for destination index d of
// `out` points over `in` source points:
//   i = min((int)floorf(d * ((float)in / (float)out)), in - 1)
// which is non-decreasing in d with steps of at most 1 for out >= in: the destinations of a source index form one
// contiguous run, and every source index has one.
//
// Layout.  The element-wise kernels see their operands as flat runs of n floats cut into chunks of 256 threads x 4
// groups x V floats: a workgroup takes chunks in a grid-stride loop (the grid is capped), a thread 4 groups of V
// consecutive floats per chunk, 256 V floats apart, all loads of a chunk issued before its first store.  V = 4 when
// every pointer is 16-byte aligned: a group is one 16-byte access, a wave touches 1 KiB contiguously, and the n % 4
// floats behind the last whole group are handled by the first lanes of workgroup 0 with 4-byte accesses.  V = 1
// otherwise (a view that starts off a 16-byte boundary): the same code with 4-byte accesses.
// upsample_add forward walks every (b, c) destination plane of Hout * Wout floats as plane_walk.h describes.  Both
// axes' source indices sit in LDS (Hout + Wout ints, built once per workgroup).  The source plane is a quarter of the
// destination's or less and is read through L1 / L2: HBM sees it once.
// upsample_add backward: one thread per source pixel, the lanes of a wave neighbouring pixels of a source row.  The
// first destination of every source index sits in LDS (Hin + 1 + Win + 1 ints); a thread sums its run of rows, and
// inside a row its run of columns, in ascending order into one float32 accumulator.  The lanes of a wave read
// neighbouring runs of the same destination rows, so every fetched line is used in full.
//
// bfloat16 (the *_bf16 entry points, for the encoder under bf16 autocast).  Every kernel is a template on the element
// type, float or bf16 (as unsigned short), with ONE body: load_group / unpack / load_f32 widen the operands to float32 (a
// shift: exact), the op is the float32 expression above, store_group / store_f32 round once to bf16 to nearest even (the
// compiler's float -> __bf16 conversion: v_cvt_pk_bf16_f32 on gfx950, two values per instruction).  The ReLU tests the
// float32 sum, whose sign is the rounded sum's: a sum of two bf16 values is a multiple of the smallest bf16 denormal,
// so a negative one does not round to zero.  The threshold's result is an element of grad_out or zero and is stored as
// that element's bits, never through the rounding (store_result).  The layout is the same with the access width
// counted in bytes: a 16-byte group is V = 8 elements, the tail is n % 8 elements, the narrow form a 2-byte access;
// upsample_add's wide path needs P % 8 == 0.  The backward keeps one thread per source pixel and one float32
// accumulator, and rounds once.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "ocrf_hip.h"
#include "plane_walk.h"

namespace {

using namespace plane;

// The numbers of the layout comment above are plane_walk.h's, which the element-wise kernels use too:
//   constexpr int kThreads = 256;  constexpr int kGroups = 4;  constexpr int kMaxBlocks = 2048;
static_assert(kThreads == 256 && kGroups == 4 && kMaxBlocks == 2048, "the comments of this file state these values");

// The ops of the element-wise passes, on float32 values.  kSelects: the result is the first operand or zero.
struct AddRelu {                                   // (a, b) -> relu(a + b)
  static constexpr bool kSelects = false;
  __device__ __forceinline__ float operator()(float a, float b) const {
    const float s = a + b;
    return s < 0.0f ? 0.0f : s;                    // NaN < 0 is false: a NaN sum stays NaN
  }
};
struct Threshold {                                 // (grad_out, out) -> grad
  static constexpr bool kSelects = true;
  __device__ __forceinline__ float operator()(float g, float o) const {
    return o <= 0.0f ? 0.0f : g;                   // NaN <= 0 is false: a NaN out passes the gradient
  }
};

// A group of results to memory: rounded once, or, for an op that selects among widened bf16 operands, their upper
// halves, which are the operands' bits (a rounding would quiet a signalling NaN).
template <typename Op, int V>
__device__ __forceinline__ void store_result(float* p, const float (&v)[V]) {
  store_group<V>(p, v);
}
template <typename Op, int V>
__device__ __forceinline__ void store_result(bf16_t* p, const float (&v)[V]) {
  if constexpr (!Op::kSelects) {
    store_group<V>(p, v);
  } else if constexpr (V == 8) {
    auto word = [](float lo, float hi) { return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u); };
    *reinterpret_cast<uint4*>(p) = make_uint4(word(v[0], v[1]), word(v[2], v[3]), word(v[4], v[5]), word(v[6], v[7]));
  } else {
    static_assert(V == 1, "a group of bf16 is 8 or 1");
    *p = (bf16_t)(__float_as_uint(v[0]) >> 16);
  }
}

// out[i] = op(p[i], q[i]) for i in [0, n): groups = n / V whole groups, chunks of kThreads * kGroups of them
template <typename T, int V, typename Op>
__global__ void __launch_bounds__(kThreads) binary_kernel(int n, int groups, int chunks, const T* __restrict__ p,
                                                           const T* __restrict__ q, T* __restrict__ out) {
  using VT = typename GroupOf<T, V>::type;
  const Op op;
  const VT* pv = reinterpret_cast<const VT*>(p);
  const VT* qv = reinterpret_cast<const VT*>(q);
  VT* ov = reinterpret_cast<VT*>(out);
  for (int c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int first = c * (kThreads * kGroups) + (int)threadIdx.x;
    VT x[kGroups], y[kGroups];                     // as loaded: widened only where they are used
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
      const int idx = first + g * kThreads;
      if (idx < groups) {
        x[g] = pv[idx];
        y[g] = qv[idx];
      }
    }
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
      const int idx = first + g * kThreads;
      if (idx < groups) {
        float a[V], b[V];
        unpack(x[g], a);
        unpack(y[g], b);
#pragma unroll
        for (int k = 0; k < V; ++k) a[k] = op(a[k], b[k]);
        store_result<Op, V>(reinterpret_cast<T*>(ov + idx), a);
      }
    }
  }
  if constexpr (V > 1) {                           // the n % V elements behind the last whole group
    const int i = groups * V + (int)threadIdx.x;
    if (blockIdx.x == 0 && i < n) {
      const float r[1] = {op(load_f32(p + i), load_f32(q + i))};
      store_result<Op, 1>(out + i, r);
    }
  }
}

// torch's mode='nearest' source index of destination index d
__device__ __forceinline__ int nearest_index(int d, int in, int out) {
  const float scale = (float)in / (float)out;
  return min((int)floorf((float)d * scale), in - 1);
}

template <typename T, int V>
__global__ void __launch_bounds__(kThreads) upsample_add_kernel(int Hin, int Win, int Hout, int Wout, int chunks,
                                                                 int units, const T* __restrict__ dst,
                                                                 const T* __restrict__ src, T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  int* tab_y = reinterpret_cast<int*>(lds_raw);    // [0, Hout): source row times Win; [Hout, Hout + Wout): source column
  int* tab_x = tab_y + Hout;
  for (int i = threadIdx.x; i < Hout + Wout; i += kThreads) {
    tab_y[i] = i < Hout ? nearest_index(i, Hin, Hout) * Win : nearest_index(i - Hout, Win, Wout);
  }
  __syncthreads();
  const int P = Hout * Wout, Pin = Hin * Win;
  const Walk<V> walk(Wout);
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int plane = u / chunks, chunk = u - plane * chunks;
    const int first = walk.first(chunk);
    const T* d = dst + (size_t)plane * P;
    const T* s = src + (size_t)plane * Pin;
    T* o = out + (size_t)plane * P;
    walk.groups(first, P, [&](int idx, int y, int x) {
      float v[V];
      if constexpr (V == 8) {                      // word by word: timed faster than adding in a widened group
        const uint4 dv = *reinterpret_cast<const uint4*>(d + idx);
        walk.values(v, y, x, [&](int yy, int xx) { return load_f32(s + (tab_y[yy] + tab_x[xx])); });
        *reinterpret_cast<uint4*>(o + idx) = make_uint4(round_pair(widen_lo(dv.x) + v[0], widen_hi(dv.x) + v[1]),
                                                        round_pair(widen_lo(dv.y) + v[2], widen_hi(dv.y) + v[3]),
                                                        round_pair(widen_lo(dv.z) + v[4], widen_hi(dv.z) + v[5]),
                                                        round_pair(widen_lo(dv.w) + v[6], widen_hi(dv.w) + v[7]));
      } else {
        float dv[V];
        load_group<V>(d + idx, dv);
        walk.values(v, y, x, [&](int yy, int xx) { return load_f32(s + (tab_y[yy] + tab_x[xx])); });
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = dv[k] + v[k];
        store_group<V>(o + idx, v);
      }
    });
  }
}

// start[i], i in [0, in]: the first destination index whose source index is >= i (start[in] = out), so that the
// destinations of source index i are [start[i], start[i + 1])
__device__ __forceinline__ void build_starts(int* start, int in, int out) {
  for (int d = threadIdx.x; d <= out; d += kThreads) {
    const int lo = d == 0 ? 0 : nearest_index(d - 1, in, out) + 1;
    const int hi = d == out ? in : nearest_index(d, in, out);
    for (int i = lo; i <= hi; ++i) start[i] = d;
  }
}

template <typename T>
__global__ void __launch_bounds__(kThreads) upsample_add_backward_kernel(int Hin, int Win, int Hout, int Wout,
                                                                          int total, const T* __restrict__ grad_out,
                                                                          T* __restrict__ grad_src) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  int* start_y = reinterpret_cast<int*>(lds_raw);  // Hin + 1 entries
  int* start_x = start_y + Hin + 1;                // Win + 1 entries
  build_starts(start_y, Hin, Hout);
  build_starts(start_x, Win, Wout);
  __syncthreads();
  const int P = Hout * Wout, Pin = Hin * Win;
  for (int i = blockIdx.x * kThreads + (int)threadIdx.x; i < total; i += gridDim.x * kThreads) {
    const int plane = i / Pin, pix = i - plane * Pin;
    const int iy = pix / Win, ix = pix - iy * Win;
    const T* g = grad_out + (size_t)plane * P;
    const int y0 = start_y[iy], y1 = start_y[iy + 1], x0 = start_x[ix], x1 = start_x[ix + 1];
    float acc = 0.0f;
    for (int oy = y0; oy < y1; ++oy) {
      const T* row = g + oy * Wout;
      for (int ox = x0; ox < x1; ++ox) acc += load_f32(row + ox);
    }
    store_f32(grad_src + i, acc);                  // bf16: the one rounding
  }
}

// the wide form (groups of kWide<T> elements, 16 bytes) when every pointer allows it, else one element per access
template <typename Op, typename T>
int binary(int kernel_id, long long n, const T* p, const T* q, T* out, ocrf_stream_t stream) {
  // every operand below 2 GiB: the kernels index with int
  if (n <= 0 || n * (long long)sizeof(T) >= kTwoGiB) return (int)hipErrorInvalidValue;
  if (!p || !q || !out) return (int)hipErrorInvalidValue;
  const bool vec = aligned16(p) && aligned16(q) && aligned16(out);
  const int V = vec ? kWide<T> : 1;
  const int groups = (int)(n / V);
  const int per_chunk = kThreads * kGroups;
  const int chunks = (groups + per_chunk - 1) / per_chunk;         // 0 for n < V on the wide path: the tail lanes alone
  const unsigned grid = capped_grid(chunks < 1 ? 1 : chunks);
  if (vec) {
    ocrf::launch(kernel_id, binary_kernel<T, kWide<T>, Op>, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, (int)n,
                 groups, chunks, p, q, out);
  } else {
    ocrf::launch(kernel_id, binary_kernel<T, 1, Op>, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, (int)n, groups,
                 chunks, p, q, out);
  }
  return (int)hipGetLastError();
}

// the shapes the upsample_add entry points accept; *P / *Pin: elements (of elem_bytes) per destination / source plane
bool shapes_ok(int B, int C, int Hin, int Win, int Hout, int Wout, long long elem_bytes, long long* P, long long* Pin) {
  if (B <= 0 || C <= 0 || Hin <= 0 || Win <= 0 || Hout < Hin || Wout < Win) return false;
  if (!planes_ok((long long)B * C, Hout, Wout, elem_bytes)) return false;
  *P = (long long)Hout * Wout;
  *Pin = (long long)Hin * Win;
  return true;
}

template <typename T>
int upsample_add_forward(int kernel_id, int B, int C, int Hin, int Win, int Hout, int Wout, const T* dst, const T* src,
                         T* out, ocrf_stream_t stream) {
  long long P, Pin;
  if (!shapes_ok(B, C, Hin, Win, Hout, Wout, sizeof(T), &P, &Pin)) return (int)hipErrorInvalidValue;
  if (!dst || !src || !out) return (int)hipErrorInvalidValue;
  constexpr int W = kWide<T>;
  const size_t lds = (size_t)(Hout + Wout) * sizeof(int);
  const bool vec = P % W == 0 && aligned16(dst) && aligned16(out);
  const Units n = units_of((long long)B * C, P, vec ? W : 1);
  if (n.units >= kTwoGiB) return (int)hipErrorInvalidValue;
  if (vec) {
    ocrf::launch(kernel_id, upsample_add_kernel<T, W>, dim3(n.grid), dim3(kThreads), lds, (hipStream_t)stream, Hin, Win,
                 Hout, Wout, n.chunks, (int)n.units, dst, src, out);
  } else {
    ocrf::launch(kernel_id, upsample_add_kernel<T, 1>, dim3(n.grid), dim3(kThreads), lds, (hipStream_t)stream, Hin, Win,
                 Hout, Wout, n.chunks, (int)n.units, dst, src, out);
  }
  return (int)hipGetLastError();
}

template <typename T>
int upsample_add_backward(int kernel_id, int B, int C, int Hin, int Win, int Hout, int Wout, const T* grad_out,
                          T* grad_src, ocrf_stream_t stream) {
  long long P, Pin;
  if (!shapes_ok(B, C, Hin, Win, Hout, Wout, sizeof(T), &P, &Pin)) return (int)hipErrorInvalidValue;
  if (!grad_out || !grad_src) return (int)hipErrorInvalidValue;
  // Hin <= Hout and Win <= Wout (shapes_ok), so this is at most (kMaxAxisSum + 2) ints: within the forward's LDS limit
  const size_t lds = (size_t)(Hin + Win + 2) * sizeof(int);
  const long long total = (long long)B * C * Pin;                 // <= B C P < 2^29
  const unsigned grid = capped_grid((total + kThreads - 1) / kThreads);
  ocrf::launch(kernel_id, upsample_add_backward_kernel<T>, dim3(grid), dim3(kThreads), lds, (hipStream_t)stream, Hin,
               Win, Hout, Wout, (int)total, grad_out, grad_src);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int ocrf_add_relu_forward(long long n, const float* a, const float* b, float* out, ocrf_stream_t stream) {
  return binary<AddRelu>(OCRF_K_ADD_RELU, n, a, b, out, stream);
}

int ocrf_add_relu_backward(long long n, const float* grad_out, const float* out, float* grad, ocrf_stream_t stream) {
  return binary<Threshold>(OCRF_K_ADD_RELU_BWD, n, grad_out, out, grad, stream);
}

int ocrf_upsample_add_forward(int B, int C, int Hin, int Win, int Hout, int Wout, const float* dst, const float* src,
                              float* out, ocrf_stream_t stream) {
  return upsample_add_forward(OCRF_K_UPSAMPLE_ADD, B, C, Hin, Win, Hout, Wout, dst, src, out, stream);
}

int ocrf_upsample_add_backward(int B, int C, int Hin, int Win, int Hout, int Wout, const float* grad_out,
                               float* grad_src, ocrf_stream_t stream) {
  return upsample_add_backward(OCRF_K_UPSAMPLE_ADD_BWD, B, C, Hin, Win, Hout, Wout, grad_out, grad_src, stream);
}

int ocrf_add_relu_forward_bf16(long long n, const unsigned short* a, const unsigned short* b, unsigned short* out,
                               ocrf_stream_t stream) {
  return binary<AddRelu>(OCRF_K_ADD_RELU_BF16, n, a, b, out, stream);
}

int ocrf_add_relu_backward_bf16(long long n, const unsigned short* grad_out, const unsigned short* out,
                                unsigned short* grad, ocrf_stream_t stream) {
  return binary<Threshold>(OCRF_K_ADD_RELU_BWD_BF16, n, grad_out, out, grad, stream);
}

int ocrf_upsample_add_forward_bf16(int B, int C, int Hin, int Win, int Hout, int Wout, const unsigned short* dst,
                                   const unsigned short* src, unsigned short* out, ocrf_stream_t stream) {
  return upsample_add_forward(OCRF_K_UPSAMPLE_ADD_BF16, B, C, Hin, Win, Hout, Wout, dst, src, out, stream);
}

int ocrf_upsample_add_backward_bf16(int B, int C, int Hin, int Win, int Hout, int Wout, const unsigned short* grad_out,
                                    unsigned short* grad_src, ocrf_stream_t stream) {
  return upsample_add_backward(OCRF_K_UPSAMPLE_ADD_BWD_BF16, B, C, Hin, Win, Hout, Wout, grad_out, grad_src, stream);
}

}  // extern "C"
