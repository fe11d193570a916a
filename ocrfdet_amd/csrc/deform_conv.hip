// Deformable convolution, DCN v1 (mmcv 1.x deform_conv2d): the deformable im2col and its transpose.  The sampling rule
// is in deform_taps.h; the contract of the entry points in include/ocrf_hip.h.  The dense products around these kernels
// are GEMMs and stay with the caller (ocrfdet_amd/deform_conv.py).
//
// im2col.  A thread owns one (image, deformable group, chunk of kChunk channels, tap, position), the position fastest:
// the lanes of a wave read neighbouring offsets and write neighbouring columns.  It forms the coordinates, the range
// test and the four weights once and walks its channels: four 4-byte loads of the map (neighbouring lanes read
// neighbouring addresses of two rows as long as the offsets vary smoothly) and one store per channel.  Every element of
// col is written exactly once, a zero where nothing is sampled.
//
// col2im.  A thread owns one (image, deformable group, tap, position) and walks ALL channels of the group in ascending
// order, so that the two offset gradients are summed in registers in a fixed order and each grad_offset element is
// written once: deterministic.  grad_x is a scatter whose targets depend on the offsets, so there is no gather form
// with a bounded candidate set (bev_align.hip has one because its map is affine): the four corner terms are added with
// float atomicAdd, which compiles to the hardware's no-return global float add (no compare-and-swap loop), and grad_x
// is reproducible only to rounding.  A corner with weight 0 issues no atomic.
#include <hip/hip_runtime.h>

#include "deform_taps.h"
#include "launch.h"
#include "ocrf_hip.h"

namespace {

using namespace deform;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 4096;                   // 16 workgroups per CU; the rest of the work is grid-strided
constexpr int kChunk = 32;                         // channels per im2col thread
constexpr long long kTwoGiB = 1LL << 31;
constexpr int kMaxExtent = 1 << 20;                // H, W, pad, dil * (k - 1): coordinates stay exact floats

struct Geometry {
  int C, H, W, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, dg;
  int Ho, Wo, K, P, cpg;                           // cpg: channels per deformable group
};

// the tap of flat index k at flat position p, offsets read from `off` (this image's and group's 2K planes of P floats)
__device__ __forceinline__ Taps tap_of(const Geometry& q, const float* __restrict__ off, int k, int p) {
  const int i = k / q.kw, j = k - i * q.kw;
  const int ho = p / q.Wo, wo = p - ho * q.Wo;
  const float off_h = off[(2 * k) * q.P + p], off_w = off[(2 * k + 1) * q.P + p];
  return taps_at(ho * q.stride_h - q.pad_h + i * q.dil_h, wo * q.stride_w - q.pad_w + j * q.dil_w, off_h, off_w, q.H, q.W);
}

__global__ void __launch_bounds__(kThreads) deform_im2col_kernel(Geometry q, int n0, int chunks, long long total,
                                                                 const float* __restrict__ x,
                                                                 const float* __restrict__ offset,
                                                                 float* __restrict__ col) {
  const int HW = q.H * q.W;
  for (long long u = (long long)blockIdx.x * kThreads + threadIdx.x; u < total; u += (long long)gridDim.x * kThreads) {
    int rest = (int)(u / q.P);
    const int p = (int)(u - (long long)rest * q.P);
    const int k = rest % q.K;
    rest /= q.K;
    const int chunk = rest % chunks;
    rest /= chunks;
    const int g = rest % q.dg, b = rest / q.dg;    // b: image within [n0, n1)
    const int img = n0 + b;
    const Taps t = tap_of(q, offset + ((size_t)img * q.dg + g) * (2 * q.K) * q.P, k, p);
    const Weights wt = weights_of(t);
    const int i00 = t.r0 * q.W + t.c0, i01 = t.r0 * q.W + t.c1, i10 = t.r1 * q.W + t.c0, i11 = t.r1 * q.W + t.c1;
    const int c_first = g * q.cpg + chunk * kChunk;
    const int nc = min(kChunk, q.cpg - chunk * kChunk);
    const float* xs = x + ((size_t)img * q.C + c_first) * HW;
    float* d = col + (((size_t)b * q.C + c_first) * q.K + k) * q.P + p;
    const size_t step = (size_t)q.K * q.P;
    for (int c = 0; c < nc; ++c) {
      const float v00 = t.v00 != 0.0f ? xs[i00] : 0.0f, v01 = t.v01 != 0.0f ? xs[i01] : 0.0f;
      const float v10 = t.v10 != 0.0f ? xs[i10] : 0.0f, v11 = t.v11 != 0.0f ? xs[i11] : 0.0f;
      *d = (wt.w00 * v00 + wt.w01 * v01) + (wt.w10 * v10 + wt.w11 * v11);
      xs += HW;
      d += step;
    }
  }
}

__global__ void __launch_bounds__(kThreads) deform_col2im_kernel(Geometry q, int n0, long long total,
                                                                 const float* __restrict__ gcol,
                                                                 const float* __restrict__ x,
                                                                 const float* __restrict__ offset,
                                                                 float* __restrict__ grad_x,
                                                                 float* __restrict__ grad_offset) {
  const int HW = q.H * q.W;
  for (long long u = (long long)blockIdx.x * kThreads + threadIdx.x; u < total; u += (long long)gridDim.x * kThreads) {
    int rest = (int)(u / q.P);
    const int p = (int)(u - (long long)rest * q.P);
    const int k = rest % q.K;
    rest /= q.K;
    const int g = rest % q.dg, b = rest / q.dg;
    const int img = n0 + b;
    const size_t off_base = ((size_t)img * q.dg + g) * (2 * q.K) * q.P;
    const Taps t = tap_of(q, offset + off_base, k, p);
    const Weights wt = weights_of(t);
    const float mh = 1.0f - t.lh, mw = 1.0f - t.lw;
    const int i00 = t.r0 * q.W + t.c0, i01 = t.r0 * q.W + t.c1, i10 = t.r1 * q.W + t.c0, i11 = t.r1 * q.W + t.c1;
    const int c_first = g * q.cpg;
    const float* xs = x + ((size_t)img * q.C + c_first) * HW;
    float* gx = grad_x + ((size_t)img * q.C + c_first) * HW;
    const float* gc = gcol + (((size_t)b * q.C + c_first) * q.K + k) * q.P + p;
    const size_t step = (size_t)q.K * q.P;
    float goh = 0.0f, gow = 0.0f;
    const bool any = t.v00 + t.v01 + t.v10 + t.v11 != 0.0f;
    if (any) {
      for (int c = 0; c < q.cpg; ++c) {
        const float go = *gc;
        const float v00 = t.v00 != 0.0f ? xs[i00] : 0.0f, v01 = t.v01 != 0.0f ? xs[i01] : 0.0f;
        const float v10 = t.v10 != 0.0f ? xs[i10] : 0.0f, v11 = t.v11 != 0.0f ? xs[i11] : 0.0f;
        goh += go * (mw * (v10 - v00) + t.lw * (v11 - v01));
        gow += go * (mh * (v01 - v00) + t.lh * (v11 - v10));
        if (wt.w00 != 0.0f) atomicAdd(gx + i00, go * wt.w00);
        if (wt.w01 != 0.0f) atomicAdd(gx + i01, go * wt.w01);
        if (wt.w10 != 0.0f) atomicAdd(gx + i10, go * wt.w10);
        if (wt.w11 != 0.0f) atomicAdd(gx + i11, go * wt.w11);
        xs += HW;
        gx += HW;
        gc += step;
      }
    }
    grad_offset[off_base + (size_t)(2 * k) * q.P + p] = goh;
    grad_offset[off_base + (size_t)(2 * k + 1) * q.P + p] = gow;
  }
}

// The shapes the entry points accept (include/ocrf_hip.h: Limits).  Fills *q; *col_elems: floats of col / gcol
bool geometry_ok(int n, int C, int H, int W, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                 int dil_w, int dg, int n0, int n1, Geometry* q, long long* col_elems) {
  if (n <= 0 || C <= 0 || H <= 0 || W <= 0 || kh <= 0 || kw <= 0 || dg <= 0) return false;
  if (stride_h <= 0 || stride_w <= 0 || dil_h <= 0 || dil_w <= 0 || pad_h < 0 || pad_w < 0) return false;
  if (C % dg != 0 || n0 < 0 || n0 >= n1 || n1 > n) return false;
  if (H >= kMaxExtent || W >= kMaxExtent || pad_h >= kMaxExtent || pad_w >= kMaxExtent) return false;
  if (kh >= kMaxExtent || kw >= kMaxExtent) return false;
  const long long eh = (long long)dil_h * (kh - 1), ew = (long long)dil_w * (kw - 1);
  if (eh >= kMaxExtent || ew >= kMaxExtent) return false;
  const long long Ho = (H + 2LL * pad_h - eh - 1) / stride_h + 1, Wo = (W + 2LL * pad_w - ew - 1) / stride_w + 1;
  if (H + 2LL * pad_h - eh - 1 < 0 || W + 2LL * pad_w - ew - 1 < 0 || Ho < 1 || Wo < 1) return false;
  const long long limit = kTwoGiB / (long long)sizeof(float);
  const long long K = (long long)kh * kw, P = Ho * Wo;                           // each below 2^42
  if (K >= limit || P >= limit || K * P >= limit) return false;
  const long long planes = (long long)n * C, HW = (long long)H * W;
  if (planes >= limit || planes * HW >= limit) return false;                     // x, grad_x
  const long long off_planes = (long long)n * dg * 2;
  if (off_planes >= limit || off_planes * K >= limit || off_planes * K * P >= limit) return false;   // offset
  const long long col_planes = (long long)(n1 - n0) * C;
  if (col_planes * K * P >= limit) return false;                                 // col, gcol (K * P < 2^29, planes < 2^29)
  q->C = C, q->H = H, q->W = W, q->kh = kh, q->kw = kw, q->stride_h = stride_h, q->stride_w = stride_w;
  q->pad_h = pad_h, q->pad_w = pad_w, q->dil_h = dil_h, q->dil_w = dil_w, q->dg = dg;
  q->Ho = (int)Ho, q->Wo = (int)Wo, q->K = (int)K, q->P = (int)P, q->cpg = C / dg;
  *col_elems = col_planes * K * P;
  return true;
}

inline unsigned grid_of(long long total) {
  const long long blocks = (total + kThreads - 1) / kThreads;
  return (unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

}  // namespace

extern "C" {

int ocrf_deform_im2col(int n, int C, int H, int W, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w,
                       int dil_h, int dil_w, int dg, int n0, int n1, const float* x, const float* offset, float* col,
                       ocrf_stream_t stream) {
  Geometry q;
  long long col_elems;
  if (!geometry_ok(n, C, H, W, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, dg, n0, n1, &q, &col_elems) ||
      !x || !offset || !col) {
    return (int)hipErrorInvalidValue;
  }
  const int chunks = (q.cpg + kChunk - 1) / kChunk;
  // at most col_elems threads: (n1 - n0) * dg * chunks * K * P with dg * chunks <= C
  const long long total = (long long)(n1 - n0) * dg * chunks * q.K * q.P;
  ocrf::launch(OCRF_K_DEFORM_IM2COL, deform_im2col_kernel, dim3(grid_of(total)), dim3(kThreads), 0, (hipStream_t)stream,
               q, n0, chunks, total, x, offset, col);
  return (int)hipGetLastError();
}

int ocrf_deform_col2im(int n, int C, int H, int W, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w,
                       int dil_h, int dil_w, int dg, int n0, int n1, const float* gcol, const float* x,
                       const float* offset, float* grad_x, float* grad_offset, ocrf_stream_t stream) {
  Geometry q;
  long long col_elems;
  if (!geometry_ok(n, C, H, W, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, dg, n0, n1, &q, &col_elems) ||
      !gcol || !x || !offset || !grad_x || !grad_offset) {
    return (int)hipErrorInvalidValue;
  }
  const size_t image = (size_t)C * H * W;
  hipError_t e = hipMemsetAsync(grad_x + (size_t)n0 * image, 0, (size_t)(n1 - n0) * image * sizeof(float),
                                (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  const long long total = (long long)(n1 - n0) * dg * q.K * q.P;
  ocrf::launch(OCRF_K_DEFORM_COL2IM, deform_col2im_kernel, dim3(grid_of(total)), dim3(kThreads), 0, (hipStream_t)stream,
               q, n0, total, gcol, x, offset, grad_x, grad_offset);
  return (int)hipGetLastError();
}

int ocrf_deform_taps(int H, int W, int base_h, int base_w, float off_h, float off_w, float* weights, int* index,
                     float* frac) {
  if (H <= 0 || W <= 0 || H >= kMaxExtent || W >= kMaxExtent || !weights || !index || !frac) {
    return (int)hipErrorInvalidValue;
  }
  if ((long long)H * W >= kTwoGiB / (long long)sizeof(float)) return (int)hipErrorInvalidValue;   // as a map of x
  if (base_h <= -2 * kMaxExtent || base_h >= 2 * kMaxExtent || base_w <= -2 * kMaxExtent || base_w >= 2 * kMaxExtent) {
    return (int)hipErrorInvalidValue;
  }
  const Taps t = taps_at(base_h, base_w, off_h, off_w, H, W);
  const Weights wt = weights_of(t);
  weights[0] = wt.w00, weights[1] = wt.w01, weights[2] = wt.w10, weights[3] = wt.w11;
  index[0] = t.r0 * W + t.c0, index[1] = t.r0 * W + t.c1, index[2] = t.r1 * W + t.c0, index[3] = t.r1 * W + t.c1;
  frac[0] = t.lh, frac[1] = t.lw;
  return 0;
}

}  // extern "C"
