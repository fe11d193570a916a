// Batch norm fused with what follows it in the residual blocks (ocrfdet_amd/norm_ops.py): relu(bn(x)) and
// relu(bn(x) + residual), forward and backward, over (N, C, H, W) contiguous tensors.
//
//   stats            (channel, chunk) -> (count, mean, M2) of the chunk's values          1 read
//   finalize         per channel: merge the chunks; mean, invstd, scale, shift; the running statistics
//   forward          out = [relu](fmaf(x, scale[c], shift[c]) [+ residual])               2 or 3 reads, 1 write
//   backward reduce  (channel, chunk) -> (sum g, sum g x^)                                2 or 3 reads
//   backward         merge the sums; dx, dresidual, dweight, dbias                        2 or 3 reads, 1 or 2 writes
//
// No kernel waits for another workgroup: there are no flags, counters or atomics.  A reduction that spans workgroups
// is two launches with a workspace between them, and every sum has one fixed shape (below), so repeated runs are
// bit-identical.
//
// Chunks.  The N * H * W values of channel c, sample after sample, form one logical run; it is cut into chunks of
// kChunk = 4096 values, the last one ragged.  The number of chunks is ceil(N * H * W / kChunk): a function of the shape
// alone.  A chunk is made of segments, the pieces of it that lie in one (n, c) plane; a plane smaller than a chunk
// gives a chunk that crosses from one sample's plane into the next.  Workgroup b of a C * chunks grid owns
// (channel, chunk) = (b / chunks, b % chunks).
//
// Access width.  A segment starts wherever its plane does: at a multiple of the element size, not of 16 bytes (H * W
// = 63).  With every tensor's base 16-byte aligned a segment is walked as a ragged head of single elements up to the
// next 16-byte boundary, a body of 16-byte groups (4 floats, 8 bf16) and a ragged tail of single elements; all tensors
// of a kernel have the same shape, so one split serves them all.  With a base off a 16-byte boundary the whole segment
// is "head".
//
// Sums.  The reducing kernels stage their chunk in LDS at its logical position (value q of the chunk at word q), so
// that the sum's shape does not depend on how the values were fetched: thread t owns values t, t + 256, ... (16 of
// them), reduces them in that order, the 64 lanes of a wave combine in a fixed tree (lane l takes lane l + 32, 16, ...,
// 1), and thread 0 combines the 4 waves in order.  This is also why the bf16 forms give, bit for bit, the statistics
// and parameter gradients of the float32 forms on the widened tensor.
//
// Statistics do not cancel.  A mean is held as anchor + offset, two floats: a thread takes its first value as anchor K,
// offset = sum(v - K) / count, M2 = sum((v - K - offset)^2) over its values in registers (a constant channel gives M2 =
// 0 exactly).  Partial results are combined with the pairwise update of (count, mean, M2) (Chan, Golub, LeVeque), in
// which the difference of two means is (K_b - K_a) + (offset_b - offset_a) and the result keeps K_a: with a mean of
// 100 and a deviation of 0.1 the anchors differ by exactly representable amounts and the offsets are small, where a
// mean rounded to one float32 would carry an error of 2^-24 * 100 into a difference of 0.1 / sqrt(count).  Across
// chunks finalize combines tiles of 64 chunks in the same lane tree and the tiles in index order, and rounds anchor +
// offset once.
//
// bfloat16 (the *_bf16 entry points): x, residual, out, grad_out, dx and dresidual are bf16 (unsigned short); they are
// widened to float32 (exact), every computation and every per-channel vector is float32, and each result element is
// rounded once to nearest even.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "ocrf_hip.h"
#include "plane_walk.h"

namespace {

using namespace plane;

constexpr int kChunk = 4096;                       // values of one channel per workgroup
constexpr int kPerThread = kChunk / kThreads;      // 16
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
static_assert(kThreads == 256 && kPerThread == 16 && kWaves == 4, "the comments of this file state these values");

// The workgroup's (channel, chunk) and the walk over the chunk's segments.  one(off, q) handles the single element at
// tensor offset `off`, value q of the chunk; wide(off, q) the V consecutive elements from there, `off` a multiple of V.
struct Chunk {
  int c, P, C, first, len;                         // first: the chunk's first value in the channel's run of N * P

  __device__ __forceinline__ Chunk(int C_, int P_, int chunks, int total) : P(P_), C(C_) {
    c = (int)blockIdx.x / chunks;
    first = ((int)blockIdx.x - c * chunks) * kChunk;
    len = min(kChunk, total - first);
  }

  template <int V, typename One, typename Wide>
  __device__ __forceinline__ void walk(One&& one, Wide&& wide) const {
    int n = first / P, p = first - n * P;
    for (int q = 0; q < len;) {
      const int seg = min(P - p, len - q);
      const int off = (n * C + c) * P + p;
      const int head = V == 1 ? seg : min(seg, (V - (off & (V - 1))) & (V - 1));
      const int groups = (seg - head) / V;
      const int tail = seg - head - groups * V;    // 0 for V == 1
      for (int i = threadIdx.x; i < head; i += kThreads) one(off + i, q + i);
      for (int g = threadIdx.x; g < groups; g += kThreads) wide(off + head + g * V, q + head + g * V);
      const int done = head + groups * V;
      for (int i = threadIdx.x; i < tail; i += kThreads) one(off + done + i, q + done + i);
      q += seg;
      p = 0;
      ++n;
    }
  }
};

// ---------------------------------------------------------------------------------------------- (count, mean, M2)
struct Moments {
  int n;
  float anchor, off, m2;                           // the mean is anchor + off
};

// the pairwise update; an empty side leaves the other untouched
__device__ __forceinline__ Moments merge(Moments a, Moments b) {
  if (b.n == 0) return a;
  if (a.n == 0) return b;
  Moments r;
  r.n = a.n + b.n;
  const float f = (float)b.n / (float)r.n;
  const float d = (b.anchor - a.anchor) + (b.off - a.off);
  r.anchor = a.anchor;
  r.off = a.off + d * f;
  r.m2 = a.m2 + b.m2 + d * d * ((float)a.n * f);
  return r;
}

// lane 0 gets the 64 lanes' moments combined in the fixed tree
__device__ __forceinline__ Moments wave_merge(Moments m) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    Moments o;
    o.n = __shfl_down(m.n, d, kWave);
    o.anchor = __shfl_down(m.anchor, d, kWave);
    o.off = __shfl_down(m.off, d, kWave);
    o.m2 = __shfl_down(m.m2, d, kWave);
    m = merge(m, o);
  }
  return m;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d, kWave);
  return v;
}

// ---------------------------------------------------------------------------------------------- stats
// partials: (C, chunks, 4) floats: count, anchor, offset, M2
template <typename T, int V>
__global__ void __launch_bounds__(kThreads) bn_stats_kernel(int C, int P, int chunks, int total,
                                                             const T* __restrict__ x, float* __restrict__ partials) {
  __shared__ float vals[kChunk];
  __shared__ Moments per_wave[kWaves];
  const Chunk ch(C, P, chunks, total);
  ch.walk<V>([&](int off, int q) { vals[q] = load_f32(x + off); },
             [&](int off, int q) {
               float v[V];
               load_group<V>(x + off, v);
#pragma unroll
               for (int k = 0; k < V; ++k) vals[q + k] = v[k];
             });
  __syncthreads();
  const int t = threadIdx.x;
  float v[kPerThread];
  Moments m = {0, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int q = t + k * kThreads;
    v[k] = q < ch.len ? vals[q] : 0.0f;
    m.n += q < ch.len ? 1 : 0;
  }
  if (m.n > 0) {                                   // the thread's values are v[0 .. m.n)
    m.anchor = v[0];
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      v[k] -= m.anchor;
      s += k > 0 && k < m.n ? v[k] : 0.0f;
    }
    m.off = s / (float)m.n;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      const float d = v[k] - m.off;
      m.m2 += k < m.n ? d * d : 0.0f;
    }
  }
  m = wave_merge(m);
  if ((t & (kWave - 1)) == 0) per_wave[t / kWave] = m;
  __syncthreads();
  if (t == 0) {
    m = per_wave[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) m = merge(m, per_wave[w]);
    float* slot = partials + (size_t)blockIdx.x * 4;
    slot[0] = (float)m.n;
    slot[1] = m.anchor;
    slot[2] = m.off;
    slot[3] = m.m2;
  }
}

// ---------------------------------------------------------------------------------------------- finalize
// One wave per channel.  from_running == 0: the statistics of the batch from `partials`, and the running statistics
// updated where there are any; 1: mean and invstd from the running statistics.
__global__ void __launch_bounds__(kWave) bn_finalize_kernel(int chunks, int from_running,
                                                             const float* __restrict__ partials,
                                                             const float* __restrict__ weight,
                                                             const float* __restrict__ bias,
                                                             float* __restrict__ running_mean,
                                                             float* __restrict__ running_var,
                                                             const long long* __restrict__ num_batches_tracked,
                                                             float momentum, float eps, float* __restrict__ mean,
                                                             float* __restrict__ invstd, float* __restrict__ scale,
                                                             float* __restrict__ shift) {
  const int c = blockIdx.x, lane = threadIdx.x;
  float mu, var;
  if (from_running) {
    if (lane != 0) return;
    mu = running_mean[c];
    var = running_var[c];
  } else {
    Moments all = {0, 0.0f, 0.0f, 0.0f};
    for (int base = 0; base < chunks; base += kWave) {
      Moments m = {0, 0.0f, 0.0f, 0.0f};
      if (base + lane < chunks) {
        const float* slot = partials + ((size_t)c * chunks + base + lane) * 4;
        m.n = (int)slot[0];
        m.anchor = slot[1];
        m.off = slot[2];
        m.m2 = slot[3];
      }
      all = merge(all, wave_merge(m));             // lane 0's is the one that counts
    }
    if (lane != 0) return;
    mu = all.anchor + all.off;
    var = all.m2 / (float)all.n;
    if (running_mean) {
      const float m = momentum >= 0.0f ? momentum : 1.0f / (float)*num_batches_tracked;
      running_mean[c] = (1.0f - m) * running_mean[c] + m * mu;
      running_var[c] = (1.0f - m) * running_var[c] + m * (all.m2 / (float)(all.n - 1));
    }
  }
  const float is = 1.0f / sqrtf(var + eps);
  const float sc = weight[c] * is;
  mean[c] = mu;
  invstd[c] = is;
  scale[c] = sc;
  shift[c] = bias[c] - mu * sc;
}

// ---------------------------------------------------------------------------------------------- forward
__device__ __forceinline__ float bn_act_value(float x, float sc, float sh, bool has_res, float res, bool relu) {
  float v = fmaf(x, sc, sh);
  if (has_res) v = v + res;
  return relu && v < 0.0f ? 0.0f : v;              // NaN < 0 is false: a NaN stays NaN
}

template <typename T, int V>
__global__ void __launch_bounds__(kThreads) bn_act_forward_kernel(int C, int P, int chunks, int total, int relu,
                                                                   const T* __restrict__ x,
                                                                   const T* __restrict__ residual,
                                                                   const float* __restrict__ scale,
                                                                   const float* __restrict__ shift,
                                                                   T* __restrict__ out) {
  const Chunk ch(C, P, chunks, total);
  const float sc = scale[ch.c], sh = shift[ch.c];
  const bool has_res = residual != nullptr, act = relu != 0;
  ch.walk<V>(
      [&](int off, int) {
        const float r = has_res ? load_f32(residual + off) : 0.0f;
        store_f32(out + off, bn_act_value(load_f32(x + off), sc, sh, has_res, r, act));
      },
      [&](int off, int) {
        float a[V], r[V], o[V];
        load_group<V>(x + off, a);
        if (has_res) load_group<V>(residual + off, r);
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = bn_act_value(a[k], sc, sh, has_res, has_res ? r[k] : 0.0f, act);
        store_group<V>(out + off, o);
      });
}

// ---------------------------------------------------------------------------------------------- backward
// torch's threshold_backward: a NaN `out` passes the gradient
__device__ __forceinline__ float gate(float out, float g) { return out <= 0.0f ? 0.0f : g; }

// the 256 threads' `a` and `b` summed in the fixed shape; thread 0 holds the result
__device__ __forceinline__ void block_sum2(float& a, float& b, float (*per_wave)[2]) {
  const int t = threadIdx.x;
  a = wave_sum(a);
  b = wave_sum(b);
  if ((t & (kWave - 1)) == 0) per_wave[t / kWave][0] = a, per_wave[t / kWave][1] = b;
  __syncthreads();
  if (t == 0) {
    a = per_wave[0][0], b = per_wave[0][1];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) a += per_wave[w][0], b += per_wave[w][1];
  }
}

// partials: (C, chunks, 2) floats: sum g, sum g x^
template <typename T, int V>
__global__ void __launch_bounds__(kThreads) bn_act_backward_reduce_kernel(int C, int P, int chunks, int total,
                                                                           const T* __restrict__ grad_out,
                                                                           const T* __restrict__ x,
                                                                           const T* __restrict__ out,
                                                                           const float* __restrict__ mean,
                                                                           const float* __restrict__ invstd,
                                                                           float* __restrict__ partials) {
  __shared__ float gs[kChunk];
  __shared__ float gxs[kChunk];
  __shared__ float per_wave[kWaves][2];
  const Chunk ch(C, P, chunks, total);
  const float mu = mean[ch.c], is = invstd[ch.c];
  const bool act = out != nullptr;
  ch.walk<V>(
      [&](int off, int q) {
        float g = load_f32(grad_out + off);
        if (act) g = gate(load_f32(out + off), g);
        gs[q] = g;
        gxs[q] = g * ((load_f32(x + off) - mu) * is);
      },
      [&](int off, int q) {
        float g[V], a[V], o[V];
        load_group<V>(grad_out + off, g);
        load_group<V>(x + off, a);
        if (act) load_group<V>(out + off, o);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float gk = act ? gate(o[k], g[k]) : g[k];
          gs[q + k] = gk;
          gxs[q + k] = gk * ((a[k] - mu) * is);
        }
      });
  __syncthreads();
  float sg = 0.0f, sgx = 0.0f;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int q = (int)threadIdx.x + k * kThreads;
    sg += q < ch.len ? gs[q] : 0.0f;
    sgx += q < ch.len ? gxs[q] : 0.0f;
  }
  block_sum2(sg, sgx, per_wave);
  if (threadIdx.x == 0) {
    partials[(size_t)blockIdx.x * 2] = sg;
    partials[(size_t)blockIdx.x * 2 + 1] = sgx;
  }
}

// batch_stats != 0: dx = weight invstd (g - sum g / n - x^ sum(g x^) / n); 0: dx = weight invstd g.  Every workgroup
// of a channel merges the channel's partials itself, in the same shape: lane l of wave 0 adds chunks l, l + 64, ... in
// order, then the lane tree.  The workgroup of chunk 0 writes dweight and dbias.  With dx and dresidual both null the
// grid is one workgroup per channel (chunks_grid == 1) and nothing else is done.
template <typename T, int V>
__global__ void __launch_bounds__(kThreads) bn_act_backward_kernel(int C, int P, int chunks, int chunks_grid, int total,
                                                                    int batch_stats, const T* __restrict__ grad_out,
                                                                    const T* __restrict__ x, const T* __restrict__ out,
                                                                    const float* __restrict__ mean,
                                                                    const float* __restrict__ invstd,
                                                                    const float* __restrict__ weight,
                                                                    const float* __restrict__ partials,
                                                                    T* __restrict__ dx, T* __restrict__ dresidual,
                                                                    float* __restrict__ dweight,
                                                                    float* __restrict__ dbias) {
  __shared__ float sums[2];
  const Chunk ch(C, P, chunks_grid, total);
  if (partials) {
    if (threadIdx.x < kWave) {
      float sg = 0.0f, sgx = 0.0f;
      for (int i = threadIdx.x; i < chunks; i += kWave) {
        sg += partials[((size_t)ch.c * chunks + i) * 2];
        sgx += partials[((size_t)ch.c * chunks + i) * 2 + 1];
      }
      sg = wave_sum(sg);
      sgx = wave_sum(sgx);
      if (threadIdx.x == 0) {
        sums[0] = sg, sums[1] = sgx;
        if (ch.first == 0) {
          if (dbias) dbias[ch.c] = sg;
          if (dweight) dweight[ch.c] = sgx;
        }
      }
    }
    __syncthreads();
  }
  if (!dx && !dresidual) return;
  const float mu = mean[ch.c], is = invstd[ch.c];
  const float a = weight[ch.c] * is;
  const bool stats = batch_stats != 0, act = out != nullptr;
  const float mg = stats ? sums[0] / (float)total : 0.0f;
  const float mgx = stats ? sums[1] / (float)total : 0.0f;
  auto dx_of = [&](float g, float xv) { return stats ? a * (g - mg - ((xv - mu) * is) * mgx) : a * g; };
  ch.walk<V>(
      [&](int off, int) {
        float g = load_f32(grad_out + off);
        if (act) g = gate(load_f32(out + off), g);
        if (dresidual) store_f32(dresidual + off, g);
        if (dx) store_f32(dx + off, dx_of(g, load_f32(x + off)));
      },
      [&](int off, int) {
        float g[V], xv[V], o[V], r[V];
        load_group<V>(grad_out + off, g);
        if (act) load_group<V>(out + off, o);
#pragma unroll
        for (int k = 0; k < V; ++k) g[k] = act ? gate(o[k], g[k]) : g[k];
        if (dresidual) store_group<V>(dresidual + off, g);
        if (dx) {
          load_group<V>(x + off, xv);
#pragma unroll
          for (int k = 0; k < V; ++k) r[k] = dx_of(g[k], xv[k]);
          store_group<V>(dx + off, r);
        }
      });
}

// ---------------------------------------------------------------------------------------------- host
struct Shape {
  int P, chunks, total;
  long long blocks;
};

// fewer than 2^31 elements (the kernels index with int), and at least one
bool shape_of(int N, int C, int H, int W, Shape* s) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return false;
  const long long P = (long long)H * W, total = (long long)N * P;
  if (P >= kTwoGiB || total >= kTwoGiB || total * C >= kTwoGiB) return false;
  s->P = (int)P;
  s->total = (int)total;
  s->chunks = (int)((total + kChunk - 1) / kChunk);
  s->blocks = (long long)C * s->chunks;            // < 2^31 / kChunk + C
  return s->blocks < kTwoGiB;
}

template <typename T>
int stats(int N, int C, int H, int W, const T* x, float* partials, ocrf_stream_t stream, int id) {
  Shape s;
  if (!shape_of(N, C, H, W, &s) || !x || !partials) return (int)hipErrorInvalidValue;
  if (aligned16(x)) {
    ocrf::launch(id, bn_stats_kernel<T, kWide<T>>, dim3((unsigned)s.blocks), dim3(kThreads), 0, (hipStream_t)stream, C,
                 s.P, s.chunks, s.total, x, partials);
  } else {
    ocrf::launch(id, bn_stats_kernel<T, 1>, dim3((unsigned)s.blocks), dim3(kThreads), 0, (hipStream_t)stream, C, s.P,
                 s.chunks, s.total, x, partials);
  }
  return (int)hipGetLastError();
}

template <typename T>
int forward(int N, int C, int H, int W, const T* x, const T* residual, const float* scale, const float* shift, int relu,
            T* out, ocrf_stream_t stream, int id) {
  Shape s;
  if (!shape_of(N, C, H, W, &s) || !x || !scale || !shift || !out) return (int)hipErrorInvalidValue;
  if (aligned16(x) && aligned16(residual) && aligned16(out)) {
    ocrf::launch(id, bn_act_forward_kernel<T, kWide<T>>, dim3((unsigned)s.blocks), dim3(kThreads), 0,
                 (hipStream_t)stream, C, s.P, s.chunks, s.total, relu, x, residual, scale, shift, out);
  } else {
    ocrf::launch(id, bn_act_forward_kernel<T, 1>, dim3((unsigned)s.blocks), dim3(kThreads), 0, (hipStream_t)stream, C,
                 s.P, s.chunks, s.total, relu, x, residual, scale, shift, out);
  }
  return (int)hipGetLastError();
}

template <typename T>
int backward_reduce(int N, int C, int H, int W, const T* grad_out, const T* x, const T* out, const float* mean,
                    const float* invstd, float* partials, ocrf_stream_t stream, int id) {
  Shape s;
  if (!shape_of(N, C, H, W, &s) || !grad_out || !x || !mean || !invstd || !partials) return (int)hipErrorInvalidValue;
  if (aligned16(grad_out) && aligned16(x) && aligned16(out)) {
    ocrf::launch(id, bn_act_backward_reduce_kernel<T, kWide<T>>, dim3((unsigned)s.blocks), dim3(kThreads), 0,
                 (hipStream_t)stream, C, s.P, s.chunks, s.total, grad_out, x, out, mean, invstd, partials);
  } else {
    ocrf::launch(id, bn_act_backward_reduce_kernel<T, 1>, dim3((unsigned)s.blocks), dim3(kThreads), 0,
                 (hipStream_t)stream, C, s.P, s.chunks, s.total, grad_out, x, out, mean, invstd, partials);
  }
  return (int)hipGetLastError();
}

template <typename T>
int backward(int N, int C, int H, int W, const T* grad_out, const T* x, const T* out, const float* mean,
             const float* invstd, const float* weight, const float* partials, int batch_stats, T* dx, T* dresidual,
             float* dweight, float* dbias, ocrf_stream_t stream, int id) {
  Shape s;
  if (!shape_of(N, C, H, W, &s) || !grad_out || !x || !mean || !invstd || !weight) return (int)hipErrorInvalidValue;
  const bool maps = dx || dresidual;
  // the sums are needed by dx with the batch's statistics and by the parameter gradients
  if (!partials && ((dx && batch_stats) || dweight || dbias)) return (int)hipErrorInvalidValue;
  if (!maps && !dweight && !dbias) return (int)hipErrorInvalidValue;
  const int chunks_grid = maps ? s.chunks : 1;
  const dim3 grid((unsigned)((long long)C * chunks_grid));
  if (aligned16(grad_out) && aligned16(x) && aligned16(out) && aligned16(dx) && aligned16(dresidual)) {
    ocrf::launch(id, bn_act_backward_kernel<T, kWide<T>>, grid, dim3(kThreads), 0, (hipStream_t)stream, C, s.P, s.chunks,
                 chunks_grid, s.total, batch_stats, grad_out, x, out, mean, invstd, weight, partials, dx, dresidual,
                 dweight, dbias);
  } else {
    ocrf::launch(id, bn_act_backward_kernel<T, 1>, grid, dim3(kThreads), 0, (hipStream_t)stream, C, s.P, s.chunks,
                 chunks_grid, s.total, batch_stats, grad_out, x, out, mean, invstd, weight, partials, dx, dresidual,
                 dweight, dbias);
  }
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int ocrf_bn_chunks(int N, int C, int H, int W) {
  Shape s;
  return shape_of(N, C, H, W, &s) ? s.chunks : 0;
}

int ocrf_bn_stats(int N, int C, int H, int W, const float* x, float* partials, ocrf_stream_t stream) {
  return stats(N, C, H, W, x, partials, stream, OCRF_K_BN_STATS);
}

int ocrf_bn_stats_bf16(int N, int C, int H, int W, const unsigned short* x, float* partials, ocrf_stream_t stream) {
  return stats(N, C, H, W, x, partials, stream, OCRF_K_BN_STATS_BF16);
}

int ocrf_bn_finalize(int N, int C, int H, int W, int from_running, const float* partials, const float* weight,
                     const float* bias, float* running_mean, float* running_var, const long long* num_batches_tracked,
                     float momentum, float eps, float* mean, float* invstd, float* scale, float* shift,
                     ocrf_stream_t stream) {
  Shape s;
  if (!shape_of(N, C, H, W, &s) || !weight || !bias || !mean || !invstd || !scale || !shift) {
    return (int)hipErrorInvalidValue;
  }
  if (from_running ? (!running_mean || !running_var) : !partials) return (int)hipErrorInvalidValue;
  if (!from_running && running_mean) {
    if (!running_var || s.total < 2 || (momentum < 0.0f && !num_batches_tracked)) return (int)hipErrorInvalidValue;
  }
  ocrf::launch(OCRF_K_BN_FINALIZE, bn_finalize_kernel, dim3((unsigned)C), dim3(kWave), 0, (hipStream_t)stream, s.chunks,
               from_running, partials, weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps, mean,
               invstd, scale, shift);
  return (int)hipGetLastError();
}

int ocrf_bn_act_forward(int N, int C, int H, int W, const float* x, const float* residual, const float* scale,
                        const float* shift, int relu, float* out, ocrf_stream_t stream) {
  return forward(N, C, H, W, x, residual, scale, shift, relu, out, stream, OCRF_K_BN_ACT_FWD);
}

int ocrf_bn_act_forward_bf16(int N, int C, int H, int W, const unsigned short* x, const unsigned short* residual,
                             const float* scale, const float* shift, int relu, unsigned short* out,
                             ocrf_stream_t stream) {
  return forward(N, C, H, W, x, residual, scale, shift, relu, out, stream, OCRF_K_BN_ACT_FWD_BF16);
}

int ocrf_bn_act_backward_reduce(int N, int C, int H, int W, const float* grad_out, const float* x, const float* out,
                                const float* mean, const float* invstd, float* partials, ocrf_stream_t stream) {
  return backward_reduce(N, C, H, W, grad_out, x, out, mean, invstd, partials, stream, OCRF_K_BN_ACT_BWD_REDUCE);
}

int ocrf_bn_act_backward_reduce_bf16(int N, int C, int H, int W, const unsigned short* grad_out,
                                     const unsigned short* x, const unsigned short* out, const float* mean,
                                     const float* invstd, float* partials, ocrf_stream_t stream) {
  return backward_reduce(N, C, H, W, grad_out, x, out, mean, invstd, partials, stream, OCRF_K_BN_ACT_BWD_REDUCE_BF16);
}

int ocrf_bn_act_backward(int N, int C, int H, int W, const float* grad_out, const float* x, const float* out,
                         const float* mean, const float* invstd, const float* weight, const float* partials,
                         int batch_stats, float* dx, float* dresidual, float* dweight, float* dbias,
                         ocrf_stream_t stream) {
  return backward(N, C, H, W, grad_out, x, out, mean, invstd, weight, partials, batch_stats, dx, dresidual, dweight,
                  dbias, stream, OCRF_K_BN_ACT_BWD);
}

int ocrf_bn_act_backward_bf16(int N, int C, int H, int W, const unsigned short* grad_out, const unsigned short* x,
                              const unsigned short* out, const float* mean, const float* invstd, const float* weight,
                              const float* partials, int batch_stats, unsigned short* dx, unsigned short* dresidual,
                              float* dweight, float* dbias, ocrf_stream_t stream) {
  return backward(N, C, H, W, grad_out, x, out, mean, invstd, weight, partials, batch_stats, dx, dresidual, dweight,
                  dbias, stream, OCRF_K_BN_ACT_BWD_BF16);
}

}  // extern "C"
