// Training losses of the neck (view_transformer_ocrf.py get_loss :1354-1417 and its helpers :1203-1314, SSIM of
// MVSGaussian/lib/train/losses/ssim_loss.py): the soft depth labels, the depth / semantic BCE and the per-sample render
// losses (masked MSE, 1 - SSIM, depth L1) for all samples and their three renders, forward and backward.
//
// Every reduction is per-block partials in a fixed order followed by a fixed-order final sum in one block: no float
// atomics, the same inputs give bit-identical outputs.  The box mask of Box2dtoMask (:1337-1352) is evaluated in the
// kernels from the packed boxes; the range zeroing of the gt depth (:1204-1207) is applied on read, so the caller's
// tensors are never written.
//
// SSIM: 11-tap Gaussian (sigma 1.5) as two separable passes through LDS over a 16 x 64 output tile (halo 5, zero outside
// the image = conv2d's zero padding).  The forward saves, per pixel and render, dS/dmu2, dS/dsigma2^2 and dS/dsigma12 with
// the mu terms chained through the sigmas; the backward filters them with the (symmetric) window again:
//   dS/dy[p] = sum_q w(q - p) (G_mu(q) + 2 y[p] G_yy(q) + x[p] G_xy(q)).
#include <hip/hip_runtime.h>

#include <cmath>

#include "launch.h"
#include "ocrf_hip.h"

namespace {

constexpr int kR = 5;                   // window radius (window 11)
constexpr int kTW = 64, kTH = 16;       // output tile
constexpr int kHW = kTW + 2 * kR;       // halo tile width 74
constexpr int kHH = kTH + 2 * kR;       // halo tile height 26
constexpr int kThreads = 256;
constexpr int kMaxBoxes = 256;
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;
constexpr int kL1Pixels = 8192;         // pixels per block of the depth-L1 pass

struct Taps {
  float w[2 * kR + 1];
};

struct RenderArgs {
  int B, K, C, H, W, N;
  const float* gt;                      // (>= B, C, H, W)
  const float* r[3];                    // (B, C, H, W) each
  const float* boxes;                   // (B, n_max, 4)
  const int* meta;                      // [0, B): box counts, [B, 2B): camera index per sample
  int n_max, use_mask;
  const float* gt_depth;                // (B, N, H, W) or null
  const float* rd[3];                   // (B, 1, H, W) each
  float d_min, d_max;
  Taps taps;
  int tiles_x, tiles_y;
};

__device__ __forceinline__ float bce(float p, float t) {
  // torch's binary_cross_entropy: the logs clamped at -100
  return -(t * fmaxf(logf(p), -100.0f) + (1.0f - t) * fmaxf(log1pf(-p), -100.0f));
}

__device__ __forceinline__ float bce_grad(float p, float t) { return (p - t) / fmaxf(p * (1.0f - p), 1e-12f); }

// Python slice normalisation of one axis of length L
__device__ __forceinline__ int slice_bound(long long v, int L) {
  if (v < 0) v += L;
  if (v < 0) v = 0;
  if (v > L) v = L;
  return (int)v;
}

__device__ __forceinline__ long long trunc_ll(float v) {
  const float t = truncf(v);
  if (!(t > -9.0e18f)) return (long long)-9e18;            // NaN / huge: behaves as an empty or clamped bound
  if (t > 9.0e18f) return (long long)9e18;
  return (long long)t;
}

// Box2dtoMask's integer bounds of sample b's boxes into LDS: {y0, y1, x0, x1}; returns the number of boxes
__device__ int load_boxes(const RenderArgs& a, int b, int (*sb)[4]) {
  if (!a.use_mask) return 0;
  const int n = min(a.meta[b], a.n_max);
  const float scale = (float)((double)a.W / 1600.0);
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float* bx = a.boxes + ((size_t)b * a.n_max + i) * 4;
    sb[i][0] = slice_bound(trunc_ll(bx[1] * scale) - 158, a.H);
    sb[i][1] = slice_bound(trunc_ll(bx[3] * scale) - 158, a.H);
    sb[i][2] = slice_bound(trunc_ll(bx[0] * scale), a.W);
    sb[i][3] = slice_bound(trunc_ll(bx[2] * scale), a.W);
  }
  return n;
}

__device__ __forceinline__ float mask_at(const RenderArgs& a, int n, const int (*sb)[4], int y, int x) {
  if (!a.use_mask) return 1.0f;
  for (int i = 0; i < n; ++i)
    if (y >= sb[i][0] && y < sb[i][1] && x >= sb[i][2] && x < sb[i][3]) return 1.0f;
  return 0.0f;
}

// the sample's camera, clamped into [0, N) (the Python layer checks host indices; device ones cannot be read there)
__device__ __forceinline__ int cam_of(const RenderArgs& a, int b) { return min(max(a.meta[a.B + b], 0), a.N - 1); }

__device__ __forceinline__ float range_zeroed(float g, float d_min, float d_max) {
  return (g < d_min || g > d_max) ? 0.0f : g;
}

// fixed-order block sum (blockDim.x == kThreads)
__device__ float block_sum(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// ------------------------------------------------------------------------------------------------ depth labels
// One wave per ds x ds patch, four patches per workgroup.  Histogram of the patch's depth * semantic bins in LDS with
// integer atomics (order-free); min / max by exact wave reductions.
__global__ __launch_bounds__(256) void depth_labels_kernel(int R, int h, int w, int H, int W, int ds, int D, float d_min,
                                                           float d_max, float c0, float step,
                                                           const float* __restrict__ gt_depth,
                                                           const float* __restrict__ gt_sem, float* __restrict__ labels,
                                                           float* __restrict__ sem_labels) {
  extern __shared__ int hist[];                 // [4][D + 1]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + wave;
  int* hw = hist + wave * (D + 1);
  for (int i = lane; i < D + 1; i += 64) hw[i] = 0;
  __syncthreads();
  float smax = 0.0f, dmin = 1e5f;
  if (r < R) {
    const int bn = r / (h * w), py = (r / w) % h, px = r % w;
    const size_t base = (size_t)bn * H * W + (size_t)py * ds * W + (size_t)px * ds;
    for (int i = lane; i < ds * ds; i += 64) {
      const size_t o = base + (size_t)(i / ds) * W + (i % ds);
      float d = gt_depth[o], s = gt_sem[o];
      if (d < d_min || d > d_max) d = 0.0f, s = 0.0f;
      smax = fmaxf(smax, s);
      dmin = fminf(dmin, d == 0.0f ? 1e5f : d);
      float sd = d * s;
      sd = sd == 0.0f ? 1e5f : sd;
      const float bin = (sd - c0) / step;
      const int ib = (bin < (float)(D + 1) && bin >= 0.0f) ? (int)bin : 0;
      atomicAdd(&hw[ib], 1);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    smax = fmaxf(smax, __shfl_xor(smax, o));
    dmin = fminf(dmin, __shfl_xor(dmin, o));
  }
  __syncthreads();
  if (r >= R) return;
  const int cls = (int)smax;                    // one_hot(max.long()) over 2 classes; the inputs are 0 / 1
  if (lane == 0) {
    sem_labels[2 * (size_t)r] = cls == 0 ? 1.0f : 0.0f;
    sem_labels[2 * (size_t)r + 1] = cls == 1 ? 1.0f : 0.0f;
  }
  float* row = labels + (size_t)r * D;
  if (cls == 1) {
    int cnt = 0;
    for (int i = 1 + lane; i < D + 1; i += 64) cnt += hw[i];
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    const float sum = (float)cnt;
    for (int i = lane; i < D; i += 64) row[i] = (float)hw[i + 1] / sum;     // 0 / 0 = NaN, as the reference
  } else {
    const float bin = (dmin - c0) / step;
    const int ib = (bin < (float)(D + 1) && bin >= 0.0f) ? (int)bin : 0;
    for (int i = lane; i < D; i += 64) row[i] = (i + 1 == ib) ? 1.0f : 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------ depth / semantic BCE
// One thread per label row; NCHW predictions read in place.  Partials per block: {depth numerator, weight sum,
// semantic numerator, rows in the mask}.
__device__ __forceinline__ bool row_in_mask(const float* lab, int D) {
  float m = -INFINITY;
  bool nan = false;
  for (int d = 0; d < D; ++d) {
    const float v = lab[d];
    nan |= v != v;
    m = fmaxf(m, v);
  }
  return !nan && m > 0.0f;
}

__global__ __launch_bounds__(256) void ds_loss_partial_kernel(int R, int HW, int D, const float* __restrict__ labels,
                                                              const float* __restrict__ sem_labels,
                                                              const float* __restrict__ depth,
                                                              const float* __restrict__ sem, float* __restrict__ part) {
  __shared__ float red[kThreads];
  const int r = blockIdx.x * kThreads + threadIdx.x;
  float dn = 0.0f, ws = 0.0f, sn = 0.0f, cnt = 0.0f;
  if (r < R) {
    const float* lab = labels + (size_t)r * D;
    if (row_in_mask(lab, D)) {
      const int bn = r / HW, pix = r % HW;
      const float w = sem_labels[2 * (size_t)r + 1] > 0.0f ? 0.9f : 0.1f;
      const float* p = depth + (size_t)bn * D * HW + pix;
      for (int d = 0; d < D; ++d) dn += bce(p[(size_t)d * HW], lab[d]) * w;
      ws = w;
      for (int c = 0; c < 2; ++c) {
        const float q = sem[((size_t)bn * 2 + c) * HW + pix], t = sem_labels[2 * (size_t)r + c];
        const float pt = (1.0f - q) * t + q * (1.0f - t);
        const float fw = (0.25f * t + 0.75f * (1.0f - t)) * (pt * pt);
        sn += bce(q, t) * fw;
      }
      cnt = 1.0f;
    }
  }
  const float v0 = block_sum(dn, red), v1 = block_sum(ws, red), v2 = block_sum(sn, red), v3 = block_sum(cnt, red);
  if (threadIdx.x == 0) {
    float* o = part + 4 * (size_t)blockIdx.x;
    o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v3;
  }
}

__global__ __launch_bounds__(256) void ds_loss_final_kernel(int n_blocks, const float* __restrict__ part, float w_depth,
                                                            float w_sem, float* __restrict__ out,
                                                            float* __restrict__ denoms) {
  __shared__ float red[kThreads];
  float v[4];
  for (int j = 0; j < 4; ++j) {
    float s = 0.0f;
    for (int i = threadIdx.x; i < n_blocks; i += kThreads) s += part[4 * (size_t)i + j];
    v[j] = block_sum(s, red);
  }
  if (threadIdx.x == 0) {
    const float den_d = fmaxf(0.1f, v[1]), den_s = fmaxf(1.0f, v[3]);
    out[0] = w_depth * (v[0] / den_d);
    out[1] = w_sem * (v[2] / den_s);
    denoms[0] = den_d;
    denoms[1] = den_s;
  }
}

__global__ __launch_bounds__(256) void ds_loss_backward_kernel(int R, int HW, int D, const float* __restrict__ labels,
                                                               const float* __restrict__ sem_labels,
                                                               const float* __restrict__ depth,
                                                               const float* __restrict__ sem, float w_depth, float w_sem,
                                                               const float* __restrict__ denoms,
                                                               const float* __restrict__ grad_out,
                                                               float* __restrict__ gdepth, float* __restrict__ gsem) {
  const int r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= R) return;
  const int bn = r / HW, pix = r % HW;
  const float* lab = labels + (size_t)r * D;
  const bool in = row_in_mask(lab, D);
  const float* p = depth + (size_t)bn * D * HW + pix;
  float* g = gdepth + (size_t)bn * D * HW + pix;
  const float w = sem_labels[2 * (size_t)r + 1] > 0.0f ? 0.9f : 0.1f;
  const float kd = in ? grad_out[0] * w_depth / denoms[0] * w : 0.0f;
  for (int d = 0; d < D; ++d) g[(size_t)d * HW] = in ? kd * bce_grad(p[(size_t)d * HW], lab[d]) : 0.0f;
  const float ks = in ? grad_out[1] * w_sem / denoms[1] : 0.0f;
  for (int c = 0; c < 2; ++c) {
    const size_t o = ((size_t)bn * 2 + c) * HW + pix;
    float v = 0.0f;
    if (in) {
      const float q = sem[o], t = sem_labels[2 * (size_t)r + c];
      const float pt = (1.0f - q) * t + q * (1.0f - t);
      const float a = 0.25f * t + 0.75f * (1.0f - t);
      const float fw = a * (pt * pt);
      v = ks * (bce_grad(q, t) * fw + bce(q, t) * (a * 2.0f * pt * (1.0f - 2.0f * t)));
    }
    gsem[o] = v;
  }
}

// ------------------------------------------------------------------------------------------------ render losses
// Tile of (b, c): per render k the five window moments, the SSIM map, the saved partials and the MSE terms.  Blocks with
// c == 0 also reduce the min / max of the range-zeroed gt depth of the sample's camera over their tile.
// part: [(b * C + c) * tiles + tile][6] = {ssim_k, mse_k}, mm: [b * tiles + tile][2]
__global__ __launch_bounds__(256) void render_tile_kernel(RenderArgs a, float* __restrict__ saved, float* __restrict__ part,
                                                          float* __restrict__ mm) {
  __shared__ int sb[kMaxBoxes][4];
  __shared__ float sin_[2][kHH][kHW];
  __shared__ float sh[5][kHH][kTW];
  __shared__ float red[kThreads];
  const int b = blockIdx.z / a.C, c = blockIdx.z % a.C;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const int tile = blockIdx.y * a.tiles_x + blockIdx.x, tiles = a.tiles_x * a.tiles_y;
  const int nb = load_boxes(a, b, sb);
  __syncthreads();
  const size_t plane = (size_t)a.H * a.W;
  const float* gx = a.gt + ((size_t)b * a.C + c) * plane;
  // x = masked gt over the halo tile (shared by the K renders)
  for (int i = threadIdx.x; i < kHH * kHW; i += kThreads) {
    const int yy = y0 - kR + i / kHW, xx = x0 - kR + i % kHW;
    float v = 0.0f;
    if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) v = gx[(size_t)yy * a.W + xx] * mask_at(a, nb, sb, yy, xx);
    sin_[0][i / kHW][i % kHW] = v;
  }
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int k = 0; k < a.K; ++k) {
    const float* gy = a.r[k] + ((size_t)b * a.C + c) * plane;
    for (int i = threadIdx.x; i < kHH * kHW; i += kThreads) {
      const int yy = y0 - kR + i / kHW, xx = x0 - kR + i % kHW;
      float v = 0.0f;
      if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) v = gy[(size_t)yy * a.W + xx] * mask_at(a, nb, sb, yy, xx);
      sin_[1][i / kHW][i % kHW] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kHH * kTW; i += kThreads) {
      const int row = i / kTW, col = i % kTW;
      float m1 = 0.0f, m2 = 0.0f, e11 = 0.0f, e22 = 0.0f, e12 = 0.0f;
#pragma unroll
      for (int t = 0; t < 2 * kR + 1; ++t) {
        const float wt = a.taps.w[t], u = sin_[0][row][col + t], v = sin_[1][row][col + t];
        m1 += wt * u; m2 += wt * v; e11 += wt * (u * u); e22 += wt * (v * v); e12 += wt * (u * v);
      }
      sh[0][row][col] = m1; sh[1][row][col] = m2; sh[2][row][col] = e11; sh[3][row][col] = e22; sh[4][row][col] = e12;
    }
    __syncthreads();
    float* sv = saved + ((((size_t)b * a.C + c) * a.K + k) * 3) * plane;
    for (int j = 0; j < kTH / 4; ++j) {
      const int oy = ty + 4 * j, yy = y0 + oy, xx = x0 + tx;
      if (yy >= a.H || xx >= a.W) continue;
      float mu1 = 0.0f, mu2 = 0.0f, e11 = 0.0f, e22 = 0.0f, e12 = 0.0f;
#pragma unroll
      for (int t = 0; t < 2 * kR + 1; ++t) {
        const float wt = a.taps.w[t];
        mu1 += wt * sh[0][oy + t][tx]; mu2 += wt * sh[1][oy + t][tx]; e11 += wt * sh[2][oy + t][tx];
        e22 += wt * sh[3][oy + t][tx]; e12 += wt * sh[4][oy + t][tx];
      }
      const float mu1mu2 = mu1 * mu2, mu1sq = mu1 * mu1, mu2sq = mu2 * mu2;
      const float s1 = e11 - mu1sq, s2 = e22 - mu2sq, s12 = e12 - mu1mu2;
      const float A1 = 2.0f * mu1mu2 + kC1, A2 = 2.0f * s12 + kC2, B1 = mu1sq + mu2sq + kC1, B2 = s1 + s2 + kC2;
      const float den = B1 * B2;
      const float s = (A1 * A2) / den;
      const float d_s2 = -s / B2, d_s12 = 2.0f * A1 / den;
      const float d_mu2 = 2.0f * mu1 * A2 / den - 2.0f * mu2 * s / B1 - 2.0f * mu2 * d_s2 - mu1 * d_s12;
      const size_t o = (size_t)yy * a.W + xx;
      sv[o] = d_mu2;
      sv[plane + o] = d_s2;
      sv[2 * plane + o] = d_s12;
      const float dxy = sin_[0][oy + kR][tx + kR] - sin_[1][oy + kR][tx + kR];
      acc[k] += s;
      acc[3 + k] += dxy * dxy;
    }
    __syncthreads();
  }
  float tot[6];
  for (int j = 0; j < 6; ++j) tot[j] = block_sum(acc[j], red);
  if (threadIdx.x == 0) {
    float* o = part + ((size_t)blockIdx.z * tiles + tile) * 6;
    for (int j = 0; j < 6; ++j) o[j] = tot[j];
  }
  if (c == 0 && a.gt_depth) {
    const float* g = a.gt_depth + ((size_t)b * a.N + cam_of(a, b)) * plane;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < kTH * kTW; i += kThreads) {
      const int yy = y0 + i / kTW, xx = x0 + i % kTW;
      if (yy >= a.H || xx >= a.W) continue;
      const float v = range_zeroed(g[(size_t)yy * a.W + xx], a.d_min, a.d_max);
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
    red[threadIdx.x] = lo;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] = fminf(red[threadIdx.x], red[threadIdx.x + s]);
      __syncthreads();
    }
    if (threadIdx.x == 0) mm[((size_t)b * tiles + tile) * 2] = red[0];
    __syncthreads();
    red[threadIdx.x] = hi;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
      __syncthreads();
    }
    if (threadIdx.x == 0) mm[((size_t)b * tiles + tile) * 2 + 1] = red[0];
  }
}

// min / max of sample b from the tile partials (exact whatever the order); den = (max - min + 0.01) in double, once
// rounded, as the reference's host arithmetic on the two .item() values
__device__ void depth_range(const RenderArgs& a, int b, const float* mm, float* red, float* lo_out, float* den_out) {
  const int tiles = a.tiles_x * a.tiles_y;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < tiles; i += kThreads) {
    lo = fminf(lo, mm[((size_t)b * tiles + i) * 2]);
    hi = fmaxf(hi, mm[((size_t)b * tiles + i) * 2 + 1]);
  }
  red[threadIdx.x] = lo;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fminf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  lo = red[0];
  __syncthreads();
  red[threadIdx.x] = hi;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  hi = red[0];
  __syncthreads();
  *lo_out = lo;
  *den_out = (float)((double)hi - (double)lo + 0.01);
}

// depth L1 partials: grid (blocks of kL1Pixels, B); stats[b] = {min, den}
__global__ __launch_bounds__(256) void render_depth_kernel(RenderArgs a, const float* __restrict__ mm,
                                                           float* __restrict__ l1part, float* __restrict__ stats) {
  __shared__ float red[kThreads];
  const int b = blockIdx.y;
  float lo, den;
  depth_range(a, b, mm, red, &lo, &den);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    stats[2 * b] = lo;
    stats[2 * b + 1] = den;
  }
  const size_t plane = (size_t)a.H * a.W;
  const float* g = a.gt_depth + ((size_t)b * a.N + cam_of(a, b)) * plane;
  const size_t p0 = (size_t)blockIdx.x * kL1Pixels, p1 = min(plane, p0 + kL1Pixels);
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for (size_t p = p0 + threadIdx.x; p < p1; p += kThreads) {
    const float t = (range_zeroed(g[p], a.d_min, a.d_max) - lo) / den;
    for (int k = 0; k < a.K; ++k) acc[k] += fabsf(a.rd[k][(size_t)b * plane + p] - t);
  }
  for (int k = 0; k < 3; ++k) {
    const float s = block_sum(acc[k], red);
    if (threadIdx.x == 0) l1part[((size_t)b * gridDim.x + blockIdx.x) * 3 + k] = s;
  }
}

// one block: per (b, k) the fixed-order sums of the partials, then the reference's averages
__global__ __launch_bounds__(256) void render_final_kernel(RenderArgs a, const float* __restrict__ part,
                                                           const float* __restrict__ l1part, int l1_blocks, float w_color,
                                                           float w_ssim, float w_depth, float* __restrict__ out) {
  __shared__ float red[kThreads];
  const int tiles = a.tiles_x * a.tiles_y;
  const float n_img = (float)a.C * (float)a.H * (float)a.W, n_dep = (float)a.H * (float)a.W;
  float color = 0.0f, ssim = 0.0f, depth = 0.0f;
  for (int b = 0; b < a.B; ++b) {
    float cs = 0.0f, ss = 0.0f, ds = 0.0f;
    for (int k = 0; k < a.K; ++k) {
      float s_ssim = 0.0f, s_mse = 0.0f, s_l1 = 0.0f;
      for (int i = threadIdx.x; i < a.C * tiles; i += kThreads) {
        const float* o = part + ((size_t)b * a.C * tiles + i) * 6;
        s_ssim += o[k];
        s_mse += o[3 + k];
      }
      if (a.gt_depth)
        for (int i = threadIdx.x; i < l1_blocks; i += kThreads) s_l1 += l1part[((size_t)b * l1_blocks + i) * 3 + k];
      s_ssim = block_sum(s_ssim, red);
      s_mse = block_sum(s_mse, red);
      s_l1 = block_sum(s_l1, red);
      cs += s_mse / n_img;
      ss += 1.0f - s_ssim / n_img;
      ds += s_l1 / n_dep;
    }
    color += cs / (float)a.K;
    ssim += ss / (float)a.K;
    depth += ds / (float)a.K;
  }
  if (threadIdx.x == 0) {
    out[0] = color / (float)a.B * w_color;
    out[1] = ssim / (float)a.B * w_ssim;
    out[2] = a.gt_depth ? depth / (float)a.B * w_depth : 0.0f;
  }
}

// backward: per tile of (b, c) and render k, the saved partials filtered by the window, chained with the masked image
// values, plus the MSE term; blocks with c == 0 also write the depth-L1 gradients
struct RenderGrads {
  float* gr[3];
  float* grd[3];
  float w_color, w_ssim, w_depth;
};

__global__ __launch_bounds__(256) void render_backward_kernel(RenderArgs a, RenderGrads o, const float* __restrict__ saved,
                                                              const float* __restrict__ stats,
                                                              const float* __restrict__ grad_out) {
  __shared__ int sb[kMaxBoxes][4];
  __shared__ float sg[3][kHH][kHW];
  __shared__ float sh[3][kHH][kTW];
  const int b = blockIdx.z / a.C, c = blockIdx.z % a.C;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const int nb = load_boxes(a, b, sb);
  __syncthreads();
  const size_t plane = (size_t)a.H * a.W;
  const float n_all = (float)a.B * (float)a.K;
  const float k_ssim = -grad_out[1] * o.w_ssim / n_all / ((float)a.C * (float)a.H * (float)a.W);
  const float k_mse = grad_out[0] * o.w_color / n_all / ((float)a.C * (float)a.H * (float)a.W);
  const float* gx = a.gt + ((size_t)b * a.C + c) * plane;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int k = 0; k < a.K; ++k) {
    const float* sv = saved + ((((size_t)b * a.C + c) * a.K + k) * 3) * plane;
    for (int i = threadIdx.x; i < kHH * kHW; i += kThreads) {
      const int yy = y0 - kR + i / kHW, xx = x0 - kR + i % kHW;
      const bool in = yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
      const size_t q = in ? (size_t)yy * a.W + xx : 0;
      for (int j = 0; j < 3; ++j) sg[j][i / kHW][i % kHW] = in ? sv[j * plane + q] : 0.0f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kHH * kTW; i += kThreads) {
      const int row = i / kTW, col = i % kTW;
      float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
#pragma unroll
      for (int t = 0; t < 2 * kR + 1; ++t) {
        const float wt = a.taps.w[t];
        f0 += wt * sg[0][row][col + t]; f1 += wt * sg[1][row][col + t]; f2 += wt * sg[2][row][col + t];
      }
      sh[0][row][col] = f0; sh[1][row][col] = f1; sh[2][row][col] = f2;
    }
    __syncthreads();
    if (o.gr[k]) {
      const float* gy = a.r[k] + ((size_t)b * a.C + c) * plane;
      float* go = o.gr[k] + ((size_t)b * a.C + c) * plane;
      for (int j = 0; j < kTH / 4; ++j) {
        const int oy = ty + 4 * j, yy = y0 + oy, xx = x0 + tx;
        if (yy >= a.H || xx >= a.W) continue;
        float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
#pragma unroll
        for (int t = 0; t < 2 * kR + 1; ++t) {
          const float wt = a.taps.w[t];
          f0 += wt * sh[0][oy + t][tx]; f1 += wt * sh[1][oy + t][tx]; f2 += wt * sh[2][oy + t][tx];
        }
        const size_t p = (size_t)yy * a.W + xx;
        const float m = mask_at(a, nb, sb, yy, xx);
        const float x = gx[p] * m, y = gy[p] * m;
        const float dS = f0 + 2.0f * y * f1 + x * f2;
        go[p] = m * (k_ssim * dS + k_mse * 2.0f * (y - x));
      }
    }
    __syncthreads();
  }
  if (c != 0 || !a.gt_depth) return;
  const float k_l1 = grad_out[2] * o.w_depth / n_all / ((float)a.H * (float)a.W);
  const float lo = stats[2 * b], den = stats[2 * b + 1];
  const float* g = a.gt_depth + ((size_t)b * a.N + cam_of(a, b)) * plane;
  for (int i = threadIdx.x; i < kTH * kTW; i += kThreads) {
    const int yy = y0 + i / kTW, xx = x0 + i % kTW;
    if (yy >= a.H || xx >= a.W) continue;
    const size_t p = (size_t)yy * a.W + xx;
    const float t = (range_zeroed(g[p], a.d_min, a.d_max) - lo) / den;
    for (int k = 0; k < a.K; ++k) {
      if (!o.grd[k]) continue;
      const float d = a.rd[k][(size_t)b * plane + p] - t;
      o.grd[k][(size_t)b * plane + p] = d > 0.0f ? k_l1 : (d < 0.0f ? -k_l1 : 0.0f);
    }
  }
}

Taps gaussian_taps() {
  // the reference's window: exp(-(x - 5)^2 / (2 sigma^2)) in double, stored as float32, normalised in float32
  Taps t;
  float f[2 * kR + 1], sum = 0.0f;
  for (int i = 0; i < 2 * kR + 1; ++i) {
    f[i] = (float)std::exp(-(double)((i - kR) * (i - kR)) / (2.0 * 1.5 * 1.5));
    sum += f[i];
  }
  for (int i = 0; i < 2 * kR + 1; ++i) t.w[i] = f[i] / sum;
  return t;
}

constexpr size_t kMaxElems = (size_t)1 << 31;

bool render_shape_ok(int B, int K, int C, int H, int W, int n_max) {
  return B > 0 && K >= 1 && K <= 3 && C > 0 && H > 0 && W > 0 && n_max >= 0 && n_max <= kMaxBoxes &&
         (size_t)B * C * K * 3 * H * W < kMaxElems;
}

void render_grid(int H, int W, int* tx, int* ty) {
  *tx = (W + kTW - 1) / kTW;
  *ty = (H + kTH - 1) / kTH;
}

int l1_blocks(int H, int W) { return (int)(((size_t)H * W + kL1Pixels - 1) / kL1Pixels); }

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

void render_ws_layout(int B, int C, int H, int W, size_t* off_mm, size_t* off_l1, size_t* total) {
  int tx, ty;
  render_grid(H, W, &tx, &ty);
  const size_t tiles = (size_t)tx * ty;
  const size_t part = align256((size_t)B * C * tiles * 6 * sizeof(float));
  const size_t mm = align256((size_t)B * tiles * 2 * sizeof(float));
  const size_t l1 = align256((size_t)B * l1_blocks(H, W) * 3 * sizeof(float));
  *off_mm = part;
  *off_l1 = part + mm;
  *total = part + mm + l1;
}

bool fill_args(RenderArgs* a, int B, int K, int C, int H, int W, const float* gt, const float* r0, const float* r1,
               const float* r2, const float* boxes, const int* meta, int n_max, int use_mask, const float* gt_depth,
               int n_cams, const float* rd0, const float* rd1, const float* rd2, float d_min, float d_max) {
  if (!render_shape_ok(B, K, C, H, W, n_max) || !gt || ((use_mask || gt_depth) && !meta)) return false;
  const float* r[3] = {r0, r1, r2};
  const float* rd[3] = {rd0, rd1, rd2};
  for (int k = 0; k < 3; ++k) {
    if (k < K && (!r[k] || (gt_depth && !rd[k]))) return false;
    a->r[k] = k < K ? r[k] : nullptr;
    a->rd[k] = (k < K && gt_depth) ? rd[k] : nullptr;
  }
  if (use_mask && n_max > 0 && !boxes) return false;
  if (gt_depth && n_cams <= 0) return false;
  a->B = B; a->K = K; a->C = C; a->H = H; a->W = W; a->N = n_cams;
  a->gt = gt; a->boxes = boxes; a->meta = meta; a->n_max = n_max; a->use_mask = use_mask ? 1 : 0;
  a->gt_depth = gt_depth; a->d_min = d_min; a->d_max = d_max;
  a->taps = gaussian_taps();
  render_grid(H, W, &a->tiles_x, &a->tiles_y);
  return true;
}

}  // namespace

extern "C" {

int ocrf_depth_labels(int BN, int H, int W, int ds, int D, double d_min, double d_max, double d_step,
                      const float* gt_depth, const float* gt_semantic, float* depth_labels, float* semantic_labels,
                      ocrf_stream_t stream) {
  if (BN <= 0 || ds <= 0 || H <= 0 || W <= 0 || H % ds || W % ds || D <= 0 || D > 4096 || !(d_step > 0.0))
    return (int)hipErrorInvalidValue;
  if (!gt_depth || !gt_semantic || !depth_labels || !semantic_labels) return (int)hipErrorInvalidValue;
  const int h = H / ds, w = W / ds;
  const size_t R = (size_t)BN * h * w;
  if ((size_t)BN * H * W >= kMaxElems || R * D >= kMaxElems) return (int)hipErrorInvalidValue;
  // (d - (d0 - s)) / s of the reference: the scalar d0 - s evaluated in double, both scalars rounded to float32
  const float c0 = (float)(d_min - d_step), step = (float)d_step;
  ocrf::launch(OCRF_K_LOSS_DEPTH_LABELS, depth_labels_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256),
               4 * (size_t)(D + 1) * sizeof(int), (hipStream_t)stream, (int)R, h, w, H, W, ds, D, (float)d_min,
               (float)d_max, c0, step, gt_depth, gt_semantic, depth_labels, semantic_labels);
  return (int)hipGetLastError();
}

size_t ocrf_depth_semantic_loss_workspace_bytes(int rows) {
  if (rows <= 0) return 0;
  return (size_t)((rows + kThreads - 1) / kThreads) * 4 * sizeof(float);
}

int ocrf_depth_semantic_loss(int BN, int HW, int D, const float* depth_labels, const float* semantic_labels,
                             const float* depth, const float* semantic, float w_depth, float w_semantic, float* out,
                             float* denoms, void* workspace, size_t workspace_bytes, ocrf_stream_t stream) {
  if (BN <= 0 || HW <= 0 || D <= 0 || (size_t)BN * HW * D >= kMaxElems) return (int)hipErrorInvalidValue;
  const int R = BN * HW;
  if (!depth_labels || !semantic_labels || !depth || !semantic || !out || !denoms || !workspace ||
      workspace_bytes < ocrf_depth_semantic_loss_workspace_bytes(R))
    return (int)hipErrorInvalidValue;
  const int nb = (R + kThreads - 1) / kThreads;
  float* part = (float*)workspace;
  ocrf::launch(OCRF_K_LOSS_DS, ds_loss_partial_kernel, dim3(nb), dim3(kThreads), 0, (hipStream_t)stream, R, HW, D,
               depth_labels, semantic_labels, depth, semantic, part);
  ocrf::launch(OCRF_K_LOSS_FINAL, ds_loss_final_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, nb,
               (const float*)part, w_depth, w_semantic, out, denoms);
  return (int)hipGetLastError();
}

int ocrf_depth_semantic_loss_backward(int BN, int HW, int D, const float* depth_labels, const float* semantic_labels,
                                      const float* depth, const float* semantic, float w_depth, float w_semantic,
                                      const float* denoms, const float* grad_out, float* grad_depth,
                                      float* grad_semantic, ocrf_stream_t stream) {
  if (BN <= 0 || HW <= 0 || D <= 0 || (size_t)BN * HW * D >= kMaxElems) return (int)hipErrorInvalidValue;
  if (!depth_labels || !semantic_labels || !depth || !semantic || !denoms || !grad_out || !grad_depth || !grad_semantic)
    return (int)hipErrorInvalidValue;
  const int R = BN * HW;
  ocrf::launch(OCRF_K_LOSS_DS_BWD, ds_loss_backward_kernel, dim3((R + kThreads - 1) / kThreads), dim3(kThreads), 0,
               (hipStream_t)stream, R, HW, D, depth_labels, semantic_labels, depth, semantic, w_depth, w_semantic, denoms,
               grad_out, grad_depth, grad_semantic);
  return (int)hipGetLastError();
}

size_t ocrf_render_losses_workspace_bytes(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  size_t a, b, total;
  render_ws_layout(B, C, H, W, &a, &b, &total);
  return total;
}

int ocrf_render_losses(int B, int K, int C, int H, int W, const float* gt, const float* r0, const float* r1,
                       const float* r2, const float* boxes, const int* meta, int n_max, int use_mask,
                       const float* gt_depth, int n_cams, const float* rd0, const float* rd1, const float* rd2,
                       float d_min, float d_max, float w_color, float w_ssim, float w_depth, float* out, float* saved,
                       float* depth_stats, void* workspace, size_t workspace_bytes, ocrf_stream_t stream) {
  RenderArgs a;
  if (!fill_args(&a, B, K, C, H, W, gt, r0, r1, r2, boxes, meta, n_max, use_mask, gt_depth, n_cams, rd0, rd1, rd2, d_min,
                 d_max))
    return (int)hipErrorInvalidValue;
  size_t off_mm, off_l1, total;
  render_ws_layout(B, C, H, W, &off_mm, &off_l1, &total);
  if (!out || !saved || (gt_depth && !depth_stats) || !workspace || workspace_bytes < total)
    return (int)hipErrorInvalidValue;
  char* ws = (char*)workspace;
  float *part = (float*)ws, *mm = (float*)(ws + off_mm), *l1 = (float*)(ws + off_l1);
  hipStream_t s = (hipStream_t)stream;
  ocrf::launch(OCRF_K_LOSS_RENDER, render_tile_kernel, dim3(a.tiles_x, a.tiles_y, B * C), dim3(kThreads), 0, s, a, saved,
               part, mm);
  const int nl1 = l1_blocks(H, W);
  if (gt_depth)
    ocrf::launch(OCRF_K_LOSS_RENDER_DEPTH, render_depth_kernel, dim3(nl1, B), dim3(kThreads), 0, s, a, (const float*)mm,
                 l1, depth_stats);
  ocrf::launch(OCRF_K_LOSS_FINAL, render_final_kernel, dim3(1), dim3(kThreads), 0, s, a, (const float*)part,
               (const float*)l1, nl1, w_color, w_ssim, w_depth, out);
  return (int)hipGetLastError();
}

int ocrf_render_losses_backward(int B, int K, int C, int H, int W, const float* gt, const float* r0, const float* r1,
                                const float* r2, const float* boxes, const int* meta, int n_max, int use_mask,
                                const float* gt_depth, int n_cams, const float* rd0, const float* rd1, const float* rd2,
                                float d_min, float d_max, float w_color, float w_ssim, float w_depth, const float* saved,
                                const float* depth_stats, const float* grad_out, float* grad_r0, float* grad_r1,
                                float* grad_r2, float* grad_rd0, float* grad_rd1, float* grad_rd2,
                                ocrf_stream_t stream) {
  RenderArgs a;
  if (!fill_args(&a, B, K, C, H, W, gt, r0, r1, r2, boxes, meta, n_max, use_mask, gt_depth, n_cams, rd0, rd1, rd2, d_min,
                 d_max))
    return (int)hipErrorInvalidValue;
  if (!saved || !grad_out || (gt_depth && !depth_stats)) return (int)hipErrorInvalidValue;
  RenderGrads o;
  float* gr[3] = {grad_r0, grad_r1, grad_r2};
  float* grd[3] = {grad_rd0, grad_rd1, grad_rd2};
  for (int k = 0; k < 3; ++k) {
    o.gr[k] = k < K ? gr[k] : nullptr;
    o.grd[k] = (k < K && gt_depth) ? grd[k] : nullptr;
  }
  o.w_color = w_color; o.w_ssim = w_ssim; o.w_depth = w_depth;
  ocrf::launch(OCRF_K_LOSS_RENDER_BWD, render_backward_kernel, dim3(a.tiles_x, a.tiles_y, B * C), dim3(kThreads), 0,
               (hipStream_t)stream, a, o, saved, depth_stats, grad_out);
  return (int)hipGetLastError();
}

}  // extern "C"
