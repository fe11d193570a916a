// Geometry distillation of OcRFDet4DVGGT (mmdet3d/models/detectors/ocrfdet_vggt.py:175-230, :476-480): the group-wise
// correlation volume over a camera pair, and the two losses between the teacher's and the student's volume.
//
// Volume.  out[b][g][d][h][w] = sum_{c < Cg} L[b][g Cg + c][h][w] * R[b][g Cg + c][h][max(w - d, 0)],  d = 0 .. D - 1.
// The reference expands both operands to (B, G, D, Cg, H, W), gathers, multiplies and sums.  Here a workgroup takes one
// (sample, group, 256 pixels of the H x W plane); its threads are neighbouring pixels of the plane, so the loads of L are
// coalesced, and the D shifted reads of R come from LDS: per step of kCh channels the workgroup stages the pixels
// [p0 - (D - 1), p0 + 256) of those channels of R once (pixel p reads plane index p - min(d, w), which never leaves its
// row, so the back halo of D - 1 pixels covers every shift).  Every feature element is read from global memory once, up
// to the halo; every output element is written once by the thread that owns it: no atomics, no memset, and the sum
// runs over c ascending with one fmaf per term, so reruns are bit-identical.
//
// Backward.  Two gathers, one launch each, the same workgroup shape:
//   gL[b][c][h][w]  = sum_d g[b][g][d][h][w] * R[b][c][h][max(w - d, 0)]          (d ascending; R staged as in the forward)
//   gR[b][c][h][w'] = sum over (w, d) with max(w - d, 0) = w' of g[b][g][d][h][w] * L[b][c][h][w]
//     w' > 0: w = w' + d < W, d ascending;  w' = 0: every w <= min(d, W - 1), d ascending and w ascending inside a d.
//   g and L are staged with a FORWARD halo of D - 1 pixels (pixel p reads plane indices p .. p + D - 1 of its own row).
//
// Losses, for s, t (B, n):  smooth = 0.1 mean(smooth_l1(s - t, beta = 1)),
//   cos = 1 - mean_b(s_b . t_b / (max(|s_b|, 1e-8) max(|t_b|, 1e-8))).
// kd_partial_kernel: workgroup (j, b) sums its share of sample b in double (smooth-L1, s.t, s.s, t.t), reduces over the
// workgroup by a fixed tree in LDS and stores four doubles into the workspace.  kd_final_kernel: one workgroup adds the
// partials of each sample by the same tree, forms the two results in double, rounds each once to float32 and keeps
// (s.t, s.s, t.t) per sample for the backward.  No float atomics, no host read.  kd_backward_kernel: elementwise, the
// per-sample coefficients from the saved sums, in double, rounded once.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "ocrf_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxD = 16;
constexpr int kRow = kThreads + kMaxD - 1;     // a staged row: the workgroup's pixels and a halo of up to kMaxD - 1
constexpr int kCh = 8;                         // channels staged per step
constexpr long long kTwoGi = 1ll << 31;

// tile[k][i] = src[k * P + q], q = p0 - back + i, for i < span and k < nrows; 0 where q lies outside the plane
template <int ROWS>
__device__ __forceinline__ void stage(float (*tile)[kRow], const float* __restrict__ src, int nrows, int P, int p0,
                                      int back, int span) {
  for (int i = threadIdx.x; i < span; i += kThreads) {
    const int q = p0 - back + i;
    const bool in = q >= 0 && q < P;
#pragma unroll
    for (int k = 0; k < ROWS; ++k)
      if (k < nrows) tile[k][i] = in ? src[(size_t)k * P + q] : 0.0f;
  }
}

// what a unit is: (sample, group, chunk of 256 pixels)
struct Unit {
  int b, g, p0;
};

__device__ __forceinline__ Unit unit_of(int u, int chunks, int G) {
  const int bg = u / chunks;
  Unit r;
  r.p0 = (u - bg * chunks) * kThreads;
  r.b = bg / G;
  r.g = bg - r.b * G;
  return r;
}

template <int DT>
__global__ void __launch_bounds__(kThreads) group_corr_forward_kernel(int Cg, int G, int W, int P, int D, int chunks,
                                                                       int units, const float* __restrict__ left,
                                                                       const float* __restrict__ right,
                                                                       long long batch_stride, float* __restrict__ out) {
  __shared__ float rt[kCh][kRow];
  const int tid = threadIdx.x, back = D - 1, span = kThreads + back;
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const Unit un = unit_of(u, chunks, G);
    const int p = un.p0 + tid;
    const bool valid = p < P;
    const int w = valid ? p % W : 0;
    const size_t base = (size_t)un.b * batch_stride + (size_t)un.g * Cg * P;
    const float* Lg = left + base;
    const float* Rg = right + base;
    float acc[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) acc[d] = 0.0f;
    for (int c0 = 0; c0 < Cg; c0 += kCh) {
      const int nch = min(kCh, Cg - c0);
      float l[kCh];
#pragma unroll
      for (int k = 0; k < kCh; ++k) l[k] = (k < nch && valid) ? Lg[(size_t)(c0 + k) * P + p] : 0.0f;
      stage<kCh>(rt, Rg + (size_t)c0 * P, nch, P, un.p0, back, span);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kCh; ++k) {
        if (k < nch) {
#pragma unroll
          for (int d = 0; d < DT; ++d)
            if (d < D) acc[d] = fmaf(l[k], rt[k][tid + back - min(d, w)], acc[d]);
        }
      }
      __syncthreads();
    }
    if (valid) {
      float* o = out + ((size_t)un.b * G + un.g) * D * P + p;
#pragma unroll
      for (int d = 0; d < DT; ++d)
        if (d < D) o[(size_t)d * P] = acc[d];
    }
  }
}

template <int DT>
__global__ void __launch_bounds__(kThreads) group_corr_grad_left_kernel(int Cg, int G, int W, int P, int D, int chunks,
                                                                         int units, const float* __restrict__ grad_out,
                                                                         const float* __restrict__ right,
                                                                         long long batch_stride,
                                                                         float* __restrict__ grad_left,
                                                                         long long grad_batch_stride) {
  __shared__ float rt[kCh][kRow];
  const int tid = threadIdx.x, back = D - 1, span = kThreads + back;
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const Unit un = unit_of(u, chunks, G);
    const int p = un.p0 + tid;
    const bool valid = p < P;
    const int w = valid ? p % W : 0;
    const float* Rg = right + (size_t)un.b * batch_stride + (size_t)un.g * Cg * P;
    float* gl = grad_left + (size_t)un.b * grad_batch_stride + (size_t)un.g * Cg * P;
    const float* go = grad_out + ((size_t)un.b * G + un.g) * D * P + p;
    float gv[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) gv[d] = (d < D && valid) ? go[(size_t)d * P] : 0.0f;
    for (int c0 = 0; c0 < Cg; c0 += kCh) {
      const int nch = min(kCh, Cg - c0);
      stage<kCh>(rt, Rg + (size_t)c0 * P, nch, P, un.p0, back, span);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kCh; ++k) {
        if (k < nch) {
          float s = 0.0f;
#pragma unroll
          for (int d = 0; d < DT; ++d)
            if (d < D) s = fmaf(gv[d], rt[k][tid + back - min(d, w)], s);
          if (valid) gl[(size_t)(c0 + k) * P + p] = s;
        }
      }
      __syncthreads();
    }
  }
}

template <int DT>
__global__ void __launch_bounds__(kThreads) group_corr_grad_right_kernel(int Cg, int G, int W, int P, int D, int chunks,
                                                                          int units, const float* __restrict__ grad_out,
                                                                          const float* __restrict__ left,
                                                                          long long batch_stride,
                                                                          float* __restrict__ grad_right,
                                                                          long long grad_batch_stride) {
  __shared__ float gt[DT][kRow];
  __shared__ float lt[kCh][kRow];
  const int tid = threadIdx.x, span = kThreads + D - 1;
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const Unit un = unit_of(u, chunks, G);
    const int p = un.p0 + tid;
    const bool valid = p < P;
    const int w = valid ? p % W : 0;
    const float* Lg = left + (size_t)un.b * batch_stride + (size_t)un.g * Cg * P;
    float* gr = grad_right + (size_t)un.b * grad_batch_stride + (size_t)un.g * Cg * P;
    stage<DT>(gt, grad_out + ((size_t)un.b * G + un.g) * D * P, D, P, un.p0, 0, span);
    for (int c0 = 0; c0 < Cg; c0 += kCh) {
      const int nch = min(kCh, Cg - c0);
      stage<kCh>(lt, Lg + (size_t)c0 * P, nch, P, un.p0, 0, span);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kCh; ++k) {
        if (k < nch) {
          float s = 0.0f;
          if (w > 0) {
#pragma unroll
            for (int d = 0; d < DT; ++d)
              if (d < D && w + d < W) s = fmaf(gt[d][tid + d], lt[k][tid + d], s);
          } else {                                   // column 0 collects every clamped read of its row
            for (int d = 0; d < D; ++d) {
              const int last = min(d, W - 1);
              for (int x = 0; x <= last; ++x) s = fmaf(gt[d][tid + x], lt[k][tid + x], s);
            }
          }
          if (valid) gr[(size_t)(c0 + k) * P + p] = s;
        }
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------------------ the two losses
constexpr int kKdThreads = 256;
constexpr int kKdMaxBlocks = 64;       // partials per sample; kd_final_kernel reduces them with one 64-thread tree
constexpr int kKdPerThread = 8;

int kd_blocks(long long n) {
  const long long per = (long long)kKdThreads * kKdPerThread;
  const long long want = (n + per - 1) / per;
  return (int)(want < 1 ? 1 : (want > kKdMaxBlocks ? kKdMaxBlocks : want));
}

// v[0 .. 4) of every thread summed over the workgroup into thread 0's v, by a tree whose shape depends on N alone
template <int N>
__device__ __forceinline__ void tree_sum4(double (*red)[N], double* v) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) red[q][tid] = v[q];
  __syncthreads();
  for (int half = N / 2; half > 0; half >>= 1) {
    if (tid < half) {
#pragma unroll
      for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + half];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = red[q][0];
  __syncthreads();
}

__global__ void __launch_bounds__(kKdThreads) kd_partial_kernel(int n, const float* __restrict__ s,
                                                                 const float* __restrict__ t,
                                                                 double* __restrict__ partial) {
  __shared__ double red[4][kKdThreads];
  const int b = blockIdx.y, j = blockIdx.x, nblk = gridDim.x;
  const float* sb = s + (size_t)b * n;
  const float* tb = t + (size_t)b * n;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = j * kKdThreads + (int)threadIdx.x; i < n; i += nblk * kKdThreads) {
    const double x = (double)sb[i], y = (double)tb[i];
    const double a = fabs(x - y);
    v[0] += a < 1.0 ? 0.5 * a * a : a - 0.5;
    v[1] += x * y;
    v[2] += x * x;
    v[3] += y * y;
  }
  tree_sum4<kKdThreads>(red, v);
  if (threadIdx.x == 0) {
    double* o = partial + ((size_t)b * nblk + j) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = v[q];
  }
}

__global__ void __launch_bounds__(kKdMaxBlocks) kd_final_kernel(int B, int n, int nblk,
                                                                 const double* __restrict__ partial,
                                                                 float* __restrict__ loss_smooth,
                                                                 float* __restrict__ loss_cos,
                                                                 double* __restrict__ sums) {
  __shared__ double red[4][kKdMaxBlocks];
  const int tid = threadIdx.x;
  double smooth = 0.0, cosine = 0.0;
  for (int b = 0; b < B; ++b) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (tid < nblk) {
      const double* src = partial + ((size_t)b * nblk + tid) * 4;
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = src[q];
    }
    tree_sum4<kKdMaxBlocks>(red, v);
    if (tid == 0) {
      const double eps = 1e-8;
      smooth += v[0];
      cosine += v[1] / (fmax(sqrt(v[2]), eps) * fmax(sqrt(v[3]), eps));
      sums[b * 3 + 0] = v[1];
      sums[b * 3 + 1] = v[2];
      sums[b * 3 + 2] = v[3];
    }
  }
  if (tid == 0) {
    *loss_smooth = (float)(0.1 * smooth / ((double)B * (double)n));
    *loss_cos = (float)(1.0 - cosine / (double)B);
  }
}

__global__ void __launch_bounds__(kKdThreads) kd_backward_kernel(int B, int n, const float* __restrict__ s,
                                                                  const float* __restrict__ t,
                                                                  const double* __restrict__ sums,
                                                                  const float* __restrict__ grad_smooth,
                                                                  const float* __restrict__ grad_cos,
                                                                  float* __restrict__ grad_s) {
  const int b = blockIdx.y;
  const double eps = 1e-8;
  const double st = sums[b * 3 + 0], ns = sqrt(sums[b * 3 + 1]), nt = sqrt(sums[b * 3 + 2]);
  const double hs = fmax(ns, eps), ht = fmax(nt, eps);
  const double gc = (double)*grad_cos / (double)B;
  const double ct = gc / (hs * ht);                                        // times t
  const double cs = ns > eps ? gc * st / (hs * hs * ht * ns) : 0.0;        // times s: the clamp passes no gradient
  const double gs = (double)*grad_smooth * 0.1 / ((double)B * (double)n);
  const float* sb = s + (size_t)b * n;
  const float* tb = t + (size_t)b * n;
  float* o = grad_s + (size_t)b * n;
  for (int i = blockIdx.x * kKdThreads + (int)threadIdx.x; i < n; i += gridDim.x * kKdThreads) {
    const double x = (double)sb[i], y = (double)tb[i];
    const double diff = fmin(fmax(x - y, -1.0), 1.0);
    o[i] = (float)(gs * diff - (ct * y - cs * x));
  }
}

// the shapes the volume's entry points accept; *P: pixels of a plane, *units: (sample, group, chunk) triples
bool corr_shapes_ok(int B, int C, int H, int W, int G, int D, long long batch_stride, long long grad_batch_stride, int* P,
                    int* chunks, int* units) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || G <= 0 || D < 1 || D > kMaxD || C % G != 0) return false;
  const long long plane = (long long)H * W;
  if (plane >= kTwoGi) return false;
  const long long sample = (long long)C * plane;
  if (sample >= kTwoGi || batch_stride < sample || grad_batch_stride < sample) return false;
  if (batch_stride >= kTwoGi || grad_batch_stride >= kTwoGi) return false;
  // the features of both views, the volume, and the farthest element either stride reaches
  if (2 * (long long)B * sample >= kTwoGi || (long long)B * G * D * plane >= kTwoGi) return false;
  if ((B - 1) * batch_stride + sample >= kTwoGi || (B - 1) * grad_batch_stride + sample >= kTwoGi) return false;
  *P = (int)plane;
  *chunks = (int)((plane + kThreads - 1) / kThreads);
  *units = B * G * *chunks;                                  // <= B * G * plane < 2^31
  return true;
}

unsigned corr_grid(int units) { return (unsigned)(units < 8192 ? units : 8192); }

}  // namespace

extern "C" {

int ocrf_group_corr_forward(int B, int C, int H, int W, int G, int D, const float* left, const float* right,
                            long long batch_stride, float* out, ocrf_stream_t stream) {
  int P, chunks, units;
  if (!corr_shapes_ok(B, C, H, W, G, D, batch_stride, batch_stride, &P, &chunks, &units)) return (int)hipErrorInvalidValue;
  if (!left || !right || !out) return (int)hipErrorInvalidValue;
  const dim3 grid(corr_grid(units)), block(kThreads);
  if (D <= 5) {
    ocrf::launch(OCRF_K_GROUP_CORR, group_corr_forward_kernel<5>, grid, block, 0, (hipStream_t)stream, C / G, G, W, P, D,
                 chunks, units, left, right, batch_stride, out);
  } else {
    ocrf::launch(OCRF_K_GROUP_CORR, group_corr_forward_kernel<kMaxD>, grid, block, 0, (hipStream_t)stream, C / G, G, W, P,
                 D, chunks, units, left, right, batch_stride, out);
  }
  return (int)hipGetLastError();
}

int ocrf_group_corr_backward(int B, int C, int H, int W, int G, int D, const float* grad_out, const float* left,
                             const float* right, long long batch_stride, float* grad_left, float* grad_right,
                             long long grad_batch_stride, ocrf_stream_t stream) {
  int P, chunks, units;
  if (!corr_shapes_ok(B, C, H, W, G, D, batch_stride, grad_batch_stride, &P, &chunks, &units))
    return (int)hipErrorInvalidValue;
  if (!grad_out || !left || !right || !grad_left || !grad_right) return (int)hipErrorInvalidValue;
  const dim3 grid(corr_grid(units)), block(kThreads);
  if (D <= 5) {
    ocrf::launch(OCRF_K_GROUP_CORR_GRAD_LEFT, group_corr_grad_left_kernel<5>, grid, block, 0, (hipStream_t)stream, C / G,
                 G, W, P, D, chunks, units, grad_out, right, batch_stride, grad_left, grad_batch_stride);
    ocrf::launch(OCRF_K_GROUP_CORR_GRAD_RIGHT, group_corr_grad_right_kernel<5>, grid, block, 0, (hipStream_t)stream,
                 C / G, G, W, P, D, chunks, units, grad_out, left, batch_stride, grad_right, grad_batch_stride);
  } else {
    ocrf::launch(OCRF_K_GROUP_CORR_GRAD_LEFT, group_corr_grad_left_kernel<kMaxD>, grid, block, 0, (hipStream_t)stream,
                 C / G, G, W, P, D, chunks, units, grad_out, right, batch_stride, grad_left, grad_batch_stride);
    ocrf::launch(OCRF_K_GROUP_CORR_GRAD_RIGHT, group_corr_grad_right_kernel<kMaxD>, grid, block, 0, (hipStream_t)stream,
                 C / G, G, W, P, D, chunks, units, grad_out, left, batch_stride, grad_right, grad_batch_stride);
  }
  return (int)hipGetLastError();
}

size_t ocrf_kd_losses_workspace_bytes(int B, long long n) {
  if (B <= 0 || n <= 0 || (long long)B * n >= kTwoGi) return 0;
  return (size_t)B * kd_blocks(n) * 4 * sizeof(double);
}

int ocrf_kd_losses_forward(int B, long long n, const float* s, const float* t, float* loss_smooth, float* loss_cos,
                           double* sums, void* workspace, size_t workspace_bytes, ocrf_stream_t stream) {
  const size_t need = ocrf_kd_losses_workspace_bytes(B, n);
  if (need == 0 || B > 65535) return (int)hipErrorInvalidValue;
  if (!s || !t || !loss_smooth || !loss_cos || !sums || !workspace || workspace_bytes < need ||
      ((size_t)workspace & 7) != 0)
    return (int)hipErrorInvalidValue;
  const int nblk = kd_blocks(n);
  double* partial = static_cast<double*>(workspace);
  ocrf::launch(OCRF_K_KD_PARTIAL, kd_partial_kernel, dim3(nblk, B), dim3(kKdThreads), 0, (hipStream_t)stream, (int)n, s,
               t, partial);
  ocrf::launch(OCRF_K_KD_FINAL, kd_final_kernel, dim3(1), dim3(kKdMaxBlocks), 0, (hipStream_t)stream, B, (int)n, nblk,
               (const double*)partial, loss_smooth, loss_cos, sums);
  return (int)hipGetLastError();
}

int ocrf_kd_losses_backward(int B, long long n, const float* s, const float* t, const double* sums,
                            const float* grad_smooth, const float* grad_cos, float* grad_s, ocrf_stream_t stream) {
  if (B <= 0 || B > 65535 || n <= 0 || (long long)B * n >= kTwoGi) return (int)hipErrorInvalidValue;
  if (!s || !t || !sums || !grad_smooth || !grad_cos || !grad_s) return (int)hipErrorInvalidValue;
  const long long want = (n + kKdThreads - 1) / kKdThreads;
  const unsigned gx = (unsigned)(want > 1024 ? 1024 : want);
  ocrf::launch(OCRF_K_KD_BWD, kd_backward_kernel, dim3(gx, B), dim3(kKdThreads), 0, (hipStream_t)stream, B, (int)n, s, t,
               sums, grad_smooth, grad_cos, grad_s);
  return (int)hipGetLastError();
}

}  // extern "C"
