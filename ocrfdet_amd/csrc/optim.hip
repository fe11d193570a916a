// The tail of a training iteration: gradient clipping by the global L2 norm (torch.nn.utils.clip_grad_norm_), AdamW
// (torch.optim.AdamW's single-tensor formula) and the weight EMA of mmdet3d/core/hook/ema.py:48-60, for ALL tensors of
// a model in a fixed number of launches: two for the norm, one for the update.
//
// Multi-tensor layout.  The tensors are cut into chunks of at most OCRF_OPTIM_CHUNK elements that start at multiples of
// it inside their tensor; a static device table names every tensor (addresses, element count, mode) and every chunk
// (tensor, first element), and a per-step record per tensor carries this step's gradient address and the scalars of
// the tensor's param group and step count (ocrf_hip.h: the three structs).  A workgroup takes chunks in a grid-stride
// loop; all decisions about a chunk (mode, gradient or none, access width) are uniform over the workgroup.
//
// Access.  A thread handles groups of 4 consecutive elements, kThreads groups apart: one 16-byte access per array when
// every address the chunk touches is 16-byte aligned (chunks start at multiples of 16 bytes inside their tensor, so that
// is a property of the tensor's base addresses), four 4-byte accesses otherwise; the last n % 4 elements of a tensor
// are a scalar tail.  Both widths do the same arithmetic on the same elements in the same order, so results do not
// depend on where an allocation happens to lie.  The update pass moves 36 bytes per element (g, p, m, v, ema read; p,
// m, v, ema written), the norm pass 4.
//
// Determinism.  The norm has no float atomics: a thread adds the squares of its elements in element order (double), the
// workgroup reduces the 256 sums in a fixed tree, one double per chunk goes to `partials`, and a second launch of one
// workgroup adds the partials (thread t those at t, t + 256, ..., ascending, then the same tree).  Reruns give the same
// bits.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "launch.h"
#include "ocrf_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kMaxBlocks = 2048;                   // 8 workgroups per CU; the rest of the chunks is grid-strided
constexpr long long kTwoGiB = 1LL << 31;

static_assert(OCRF_OPTIM_CHUNK % 4 == 0, "chunks start at multiples of 16 bytes inside their tensor");
static_assert(sizeof(ocrf_optim_tensor) == 48 && sizeof(ocrf_optim_chunk) == 8 && sizeof(ocrf_optim_step_rec) == 40,
              "the tables are packed by the host with these sizes");

__device__ __forceinline__ bool aligned16(unsigned long long a) { return (a & 15ull) == 0; }

// sum of the 256 per-thread values in a fixed order: inside each wave by halving distances, then the waves in index
// order; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d, kWave);
  const int wave = (int)threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) lds[wave] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kThreads / kWave; ++w) s += lds[w];
  }
  __syncthreads();                                 // lds is reused by the next chunk
  return s;
}

template <bool VEC>
__device__ __forceinline__ void load4(const float* a, int i, float (&v)[4]) {
  if constexpr (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(a + i);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = a[i + k];
  }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* a, int i, const float (&v)[4]) {
  if constexpr (VEC) {
    *reinterpret_cast<float4*>(a + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) a[i + k] = v[k];
  }
}

// partials[chunk] = sum of g * g over the chunk's elements (0 for a chunk without a gradient)
template <bool VEC>
__device__ __forceinline__ double chunk_sqsum(const float* g, int len) {
  const int groups = len >> 2;
  double acc = 0.0;
  for (int q = (int)threadIdx.x; q < groups; q += kThreads) {
    float v[4];
    load4<VEC>(g, q * 4, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double d = (double)v[k];
      acc += d * d;
    }
  }
  const int tail = (groups << 2) + (int)threadIdx.x;
  if (tail < len) {
    const double d = (double)g[tail];
    acc += d * d;
  }
  return acc;
}

__global__ void __launch_bounds__(kThreads) optim_grad_sqnorm_kernel(const ocrf_optim_tensor* __restrict__ tensors,
                                                                     int n_tensors,
                                                                     const ocrf_optim_chunk* __restrict__ chunks,
                                                                     int n_chunks,
                                                                     const ocrf_optim_step_rec* __restrict__ recs,
                                                                     double* __restrict__ partials) {
  __shared__ double lds[kThreads / kWave];
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const ocrf_optim_chunk ch = chunks[c];
    double acc = 0.0;
    if (ch.tensor >= 0 && ch.tensor < n_tensors) {
      const ocrf_optim_tensor t = tensors[ch.tensor];
      const unsigned long long ga = recs[ch.tensor].grad;
      if (ga != 0 && t.mode != OCRF_OPTIM_EMA_ONLY && ch.offset >= 0 && ch.offset < t.n) {
        const long long rest = t.n - ch.offset;
        const int len = (int)(rest < OCRF_OPTIM_CHUNK ? rest : OCRF_OPTIM_CHUNK);
        const float* g = reinterpret_cast<const float*>(ga) + ch.offset;
        acc = aligned16(ga) ? chunk_sqsum<true>(g, len) : chunk_sqsum<false>(g, len);
      }
    }
    const double s = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[c] = s;
  }
}

// total_norm = sqrt(sum of the partials), rounded once to f32
__global__ void __launch_bounds__(kThreads) optim_norm_final_kernel(const double* __restrict__ partials, int n_chunks,
                                                                    float* __restrict__ total_norm) {
  __shared__ double lds[kThreads / kWave];
  double acc = 0.0;
  for (int c = (int)threadIdx.x; c < n_chunks; c += kThreads) acc += partials[c];
  const double s = block_sum(acc, lds);
  if (threadIdx.x == 0) *total_norm = (float)sqrt(s);
}

struct StepScalars {
  float decay, one_minus_beta1, beta2, one_minus_beta2, bc2_sqrt, eps, step_size;
};

// torch.optim.adamw._single_tensor_adamw, every operation rounded once (the library builds with -ffp-contract=off)
__device__ __forceinline__ void adamw(float g, float coef, const StepScalars& s, float& p, float& m, float& v) {
  g = g * coef;
  p = p * s.decay;
  m = m + s.one_minus_beta1 * (g - m);
  v = v * s.beta2 + s.one_minus_beta2 * g * g;
  p = p - s.step_size * (m / (sqrtf(v) / s.bc2_sqrt + s.eps));
}

template <bool VEC, bool ADAM, bool EMA>
__device__ __forceinline__ void chunk_update(const float* g, float* p, float* m, float* v, float* e, int len, float coef,
                                             const StepScalars& s, float d, float one_minus_d) {
  const int groups = len >> 2;
  for (int q = (int)threadIdx.x; q < groups; q += kThreads) {
    const int i = q * 4;
    float pv[4];
    load4<VEC>(p, i, pv);
    if constexpr (ADAM) {
      float gv[4], mv[4], vv[4];
      load4<VEC>(g, i, gv);
      load4<VEC>(m, i, mv);
      load4<VEC>(v, i, vv);
#pragma unroll
      for (int k = 0; k < 4; ++k) adamw(gv[k], coef, s, pv[k], mv[k], vv[k]);
      store4<VEC>(p, i, pv);
      store4<VEC>(m, i, mv);
      store4<VEC>(v, i, vv);
    }
    if constexpr (EMA) {
      float ev[4];
      load4<VEC>(e, i, ev);
#pragma unroll
      for (int k = 0; k < 4; ++k) ev[k] = ev[k] * d + one_minus_d * pv[k];
      store4<VEC>(e, i, ev);
    }
  }
  const int i = (groups << 2) + (int)threadIdx.x;
  if (i < len) {
    float pv = p[i];
    if constexpr (ADAM) {
      float mv = m[i], vv = v[i];
      adamw(g[i], coef, s, pv, mv, vv);
      p[i] = pv;
      m[i] = mv;
      v[i] = vv;
    }
    if constexpr (EMA) e[i] = e[i] * d + one_minus_d * pv;
  }
}

template <bool ADAM, bool EMA>
__device__ __forceinline__ void chunk_update_width(bool vec, const float* g, float* p, float* m, float* v, float* e,
                                                   int len, float coef, const StepScalars& s, float d,
                                                   float one_minus_d) {
  if (vec) {
    chunk_update<true, ADAM, EMA>(g, p, m, v, e, len, coef, s, d, one_minus_d);
  } else {
    chunk_update<false, ADAM, EMA>(g, p, m, v, e, len, coef, s, d, one_minus_d);
  }
}

__global__ void __launch_bounds__(kThreads) optim_step_kernel(const ocrf_optim_tensor* __restrict__ tensors,
                                                              int n_tensors,
                                                              const ocrf_optim_chunk* __restrict__ chunks, int n_chunks,
                                                              const ocrf_optim_step_rec* __restrict__ recs,
                                                              const float* __restrict__ total_norm, float max_norm,
                                                              float d, float one_minus_d) {
  float coef = 1.0f;
  if (total_norm) {
    // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0); a NaN stays a NaN
    const float c = max_norm / (*total_norm + 1e-6f);
    coef = c > 1.0f ? 1.0f : c;
  }
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const ocrf_optim_chunk ch = chunks[c];
    if (ch.tensor < 0 || ch.tensor >= n_tensors) continue;
    const ocrf_optim_tensor t = tensors[ch.tensor];
    if (ch.offset < 0 || ch.offset >= t.n || !t.p) continue;
    const ocrf_optim_step_rec r = recs[ch.tensor];
    const bool adam = t.mode != OCRF_OPTIM_EMA_ONLY && r.grad != 0 && t.exp_avg && t.exp_avg_sq;
    const bool ema = t.mode != OCRF_OPTIM_ADAM && t.ema != 0;
    if (!adam && !ema) continue;
    const long long rest = t.n - ch.offset;
    const int len = (int)(rest < OCRF_OPTIM_CHUNK ? rest : OCRF_OPTIM_CHUNK);
    bool vec = aligned16(t.p);
    if (adam) vec = vec && aligned16(r.grad) && aligned16(t.exp_avg) && aligned16(t.exp_avg_sq);
    if (ema) vec = vec && aligned16(t.ema);
    // an address the chunk does not use may be 0: pointers are formed only from the addresses it does use
    float* p = reinterpret_cast<float*>(t.p) + ch.offset;
    const float* g = nullptr;
    float *m = nullptr, *v = nullptr, *e = nullptr;
    if (adam) {
      g = reinterpret_cast<const float*>(r.grad) + ch.offset;
      m = reinterpret_cast<float*>(t.exp_avg) + ch.offset;
      v = reinterpret_cast<float*>(t.exp_avg_sq) + ch.offset;
    }
    if (ema) e = reinterpret_cast<float*>(t.ema) + ch.offset;
    StepScalars s;
    s.decay = r.decay, s.one_minus_beta1 = r.one_minus_beta1, s.beta2 = r.beta2, s.one_minus_beta2 = r.one_minus_beta2;
    s.bc2_sqrt = r.bc2_sqrt, s.eps = r.eps, s.step_size = r.step_size;
    if (adam && ema) {
      chunk_update_width<true, true>(vec, g, p, m, v, e, len, coef, s, d, one_minus_d);
    } else if (adam) {
      chunk_update_width<true, false>(vec, g, p, m, v, e, len, coef, s, d, one_minus_d);
    } else {
      chunk_update_width<false, true>(vec, g, p, m, v, e, len, coef, s, d, one_minus_d);
    }
  }
}

unsigned capped_grid(int blocks) { return (unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks); }

}  // namespace

extern "C" {

int ocrf_optim_layout(int* out) {
  if (!out) return (int)hipErrorInvalidValue;
  int k = 0;
  out[k++] = (int)sizeof(ocrf_optim_tensor);
  out[k++] = (int)offsetof(ocrf_optim_tensor, p);
  out[k++] = (int)offsetof(ocrf_optim_tensor, exp_avg);
  out[k++] = (int)offsetof(ocrf_optim_tensor, exp_avg_sq);
  out[k++] = (int)offsetof(ocrf_optim_tensor, ema);
  out[k++] = (int)offsetof(ocrf_optim_tensor, n);
  out[k++] = (int)offsetof(ocrf_optim_tensor, mode);
  out[k++] = (int)sizeof(ocrf_optim_chunk);
  out[k++] = (int)offsetof(ocrf_optim_chunk, tensor);
  out[k++] = (int)offsetof(ocrf_optim_chunk, offset);
  out[k++] = (int)sizeof(ocrf_optim_step_rec);
  out[k++] = (int)offsetof(ocrf_optim_step_rec, grad);
  out[k++] = (int)offsetof(ocrf_optim_step_rec, decay);
  out[k++] = (int)offsetof(ocrf_optim_step_rec, one_minus_beta1);
  out[k++] = (int)offsetof(ocrf_optim_step_rec, beta2);
  out[k++] = (int)offsetof(ocrf_optim_step_rec, one_minus_beta2);
  out[k++] = (int)offsetof(ocrf_optim_step_rec, bc2_sqrt);
  out[k++] = (int)offsetof(ocrf_optim_step_rec, eps);
  out[k++] = (int)offsetof(ocrf_optim_step_rec, step_size);
  static_assert(OCRF_OPTIM_LAYOUT_INTS == 19, "ocrf_optim_layout writes this many ints");
  return 0;
}

int ocrf_optim_grad_sqnorm(const void* tensors, int n_tensors, const void* chunks, int n_chunks, const void* step_recs,
                           long long max_elements, double* partials, float* total_norm, ocrf_stream_t stream) {
  if (!tensors || !chunks || !step_recs || !partials || !total_norm) return (int)hipErrorInvalidValue;
  if (n_tensors <= 0 || n_chunks <= 0 || max_elements <= 0) return (int)hipErrorInvalidValue;
  if (max_elements >= kTwoGiB / (long long)sizeof(float)) return (int)hipErrorInvalidValue;
  ocrf::launch(OCRF_K_OPTIM_SQNORM, optim_grad_sqnorm_kernel, dim3(capped_grid(n_chunks)), dim3(kThreads), 0,
               (hipStream_t)stream, static_cast<const ocrf_optim_tensor*>(tensors), n_tensors,
               static_cast<const ocrf_optim_chunk*>(chunks), n_chunks,
               static_cast<const ocrf_optim_step_rec*>(step_recs), partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  ocrf::launch(OCRF_K_OPTIM_NORM_FINAL, optim_norm_final_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream,
               static_cast<const double*>(partials), n_chunks, total_norm);
  return (int)hipGetLastError();
}

int ocrf_optim_step(const void* tensors, int n_tensors, const void* chunks, int n_chunks, const void* step_recs,
                    long long max_elements, const float* total_norm, float max_norm, float ema_decay,
                    float ema_one_minus_decay, ocrf_stream_t stream) {
  if (!tensors || !chunks || !step_recs) return (int)hipErrorInvalidValue;
  if (n_tensors <= 0 || n_chunks <= 0 || max_elements <= 0) return (int)hipErrorInvalidValue;
  if (max_elements >= kTwoGiB / (long long)sizeof(float)) return (int)hipErrorInvalidValue;
  ocrf::launch(OCRF_K_OPTIM_STEP, optim_step_kernel, dim3(capped_grid(n_chunks)), dim3(kThreads), 0,
               (hipStream_t)stream, static_cast<const ocrf_optim_tensor*>(tensors), n_tensors,
               static_cast<const ocrf_optim_chunk*>(chunks), n_chunks,
               static_cast<const ocrf_optim_step_rec*>(step_recs), total_norm, max_norm, ema_decay,
               ema_one_minus_decay);
  return (int)hipGetLastError();
}

}  // extern "C"
