// HOA-1 under autograd (view_transformer_ocrf.py:1159-1161 + mmdet3d/ops/cross_attention_2d.py:142-220) for the fixed
// configuration of hoa1_common.h: the forward of hoa.hip with an optional dropout keep-mask on the attention weights,
// keeping the kv buffer and every query token's softmax maximum and sum, and a backward of six launches that
// recomputes everything else.  No float atomics: every scatter of the graph is written as a gather, and the weight
// gradients are per-workgroup partial rows summed in a fixed order by the last launch, so reruns are bit-identical.
//
//   forward   hoa1_kv_kernel (hoa.hip) -> hoa1_attention_train_kernel            kv | (m, l) kept
//   backward  (1) hoa1_up_grad_kernel      d att[t][c]: gather over the <= 17 x 17 pixels that interpolate from token t
//             (2) hoa1_attn_grad_kernel    8 lanes per query token: to_out, softmax + dropout, q k^T, CPB; writes per
//                                          (token, key) pair {d sim, dropped weight, d grid x, d grid y} and per token
//                                          q, d o, d q; partial rows of to_out and CPB
//             (3) hoa1_kv_grad_kernel      one workgroup per kv token: gathers its pairs over all query tokens, then
//                                          to_k / to_v, grid_sample (input and grid), normalisation, tanh, 1x1, GELU,
//                                          depthwise 6x6; partial rows of to_k, to_v, to_offsets
//             (4) hoa1_token_grad_kernel   per query token: d q from <= 2 x 2 offset windows, to_q, and the alpha
//                                          token's gather over the <= nkv samples that tap it; partial rows of to_q
//             (5) hoa1_pixel_grad_kernel   per pixel: a pixel is a corner tap of at most one token per axis
//             (6) hoa1_weight_sum_kernel   partial rows -> grad_weights
#include <hip/hip_runtime.h>

#include "hoa1_common.h"
#include "launch.h"
#include "ocrf_hip.h"

namespace {

using namespace ocrf::hoa1;

constexpr int kB = kHoaBlock;
constexpr int kTokWg = kB / kAttSplit;          // query tokens per workgroup of launches (2) and (4)
constexpr int kCpbW = kHoaWeights - oC0W;       // 25 CPB weights, contiguous at the end of the packed vector
constexpr int kUpLanes = 16;                    // lanes per (token, channel) of launch (1)

__global__ __launch_bounds__(kB) void hoa1_attention_train_kernel(
    const float* __restrict__ opacity, const float* __restrict__ kvbuf, const float* __restrict__ wts, int Y, int X,
    int hq, int wq, int nkv, float* __restrict__ out, const unsigned char* __restrict__ mask, float dscale,
    float* __restrict__ ml) {
  attention_upsample_body<true>(opacity, kvbuf, wts, Y, X, hq, wq, nkv, out, mask, dscale, ml);
}

// weight of token index `tk` in the align-corners upsample of output position p (n tokens, d = (n - 1) / (size - 1)),
// as the forward mixes it: (1 - l) for the lower tap, l for the upper one (both when they coincide at the border)
__device__ __forceinline__ float up_weight(float d, int p, int n, int tk) {
  const float s = d * (float)p;
  const int i0 = min((int)s, n - 1), i1 = min(i0 + 1, n - 1);
  const float l = s - (float)i0;
  return (i0 == tk ? 1.f - l : 0.f) + (i1 == tk ? l : 0.f);
}

// (1) gatt[b][t][c] = sum over pixels of up_weight_y * up_weight_x * gout[b][c][y][x]; kUpLanes lanes (columns) per item
__global__ __launch_bounds__(kB) void hoa1_up_grad_kernel(const float* __restrict__ gout, int B, int Y, int X, int hq,
                                                          int wq, float* __restrict__ gatt) {
  const int tid = threadIdx.x, lane = tid % kUpLanes;
  const int ntok = hq * wq;
  const long n_items = (long)B * ntok * kHD;
  const long item = (long)blockIdx.x * (kB / kUpLanes) + tid / kUpLanes;
  const long it = min(item, n_items - 1);
  const int c = (int)(it % kHD);
  const long bt = it / kHD;
  const int t = (int)(bt % ntok), b = (int)(bt / ntok);
  const int ty = t / wq, tx = t % wq;
  const float dy = (float)(hq - 1) / (float)(Y - 1), dx = (float)(wq - 1) / (float)(X - 1);
  const float ry = (float)(Y - 1) / (float)(hq - 1), rx = (float)(X - 1) / (float)(wq - 1);
  // pixels whose source coordinate lies in [tk - 1, tk + 1), one more on either side for the rounding
  const int ylo = max((int)(ry * (float)(ty - 1)) - 1, 0), yhi = min((int)(ry * (float)(ty + 1)) + 2, Y - 1);
  const int xlo = max((int)(rx * (float)(tx - 1)) - 1, 0), xhi = min((int)(rx * (float)(tx + 1)) + 2, X - 1);
  const float* g = gout + ((long)b * kHD + c) * Y * X;
  float acc = 0.f;
  for (int x = xlo + lane; x <= xhi; x += kUpLanes) {
    const float wx = up_weight(dx, x, wq, tx);
    if (wx == 0.f) continue;
    float col = 0.f;
    for (int y = ylo; y <= yhi; ++y) col = fmaf(up_weight(dy, y, hq, ty), g[(long)y * X + x], col);
    acc = fmaf(wx, col, acc);
  }
#pragma unroll
  for (int off = kUpLanes / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kUpLanes);
  if (lane == 0 && item < n_items) gatt[item] = acc;
}

// score of one (query, key) pair as the forward computes it, with what CPB's backward needs of it
struct PairState { float px, py, bx, by, z0[3], h0[3], z1[3], h1[3]; };
__device__ __forceinline__ float pair_score(const float* q, const float* kv, float qx, float qy, const float* s_w,
                                            PairState& s) {
  float sc = 0.f;
#pragma unroll
  for (int d = 0; d < kHI; ++d) sc = fmaf(q[d], kv[d], sc);
  s.px = qx - kv[16];
  s.py = qy - kv[17];
  s.bx = copysignf(__logf(fabsf(s.px) + 1.f), s.px);
  s.by = copysignf(__logf(fabsf(s.py) + 1.f), s.py);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    s.z0[i] = fmaf(s_w[oC0W + i * 2], s.bx, fmaf(s_w[oC0W + i * 2 + 1], s.by, s_w[oC0B + i]));
    s.h0[i] = fmaxf(s.z0[i], 0.f);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    s.z1[i] = s_w[oC1B + i] + s_w[oC1W + i * 3] * s.h0[0] + s_w[oC1W + i * 3 + 1] * s.h0[1] + s_w[oC1W + i * 3 + 2] * s.h0[2];
    s.h1[i] = fmaxf(s.z1[i], 0.f);
  }
  sc += s_w[oC2B] + s_w[oC2W] * s.h1[0] + s_w[oC2W + 1] * s.h1[1] + s_w[oC2W + 2] * s.h1[2];
  return sc;
}

// (2) grid (ceil(ntok / kTokWg), B).  pair[(b, t, j)] = {d sim, dropped attention weight, d grid_x, d grid_y (CPB)};
// qbuf / gobuf / gqabuf (B, ntok, 8) = q (unscaled), d o, d q of the attention branch; rows (B * gridDim.x, kHoaWeights):
// the to_out, to_out bias and CPB entries are written.
__global__ __launch_bounds__(kB) void hoa1_attn_grad_kernel(
    const float* __restrict__ opacity, const float* __restrict__ kvbuf, const float* __restrict__ wts,
    const float* __restrict__ ml, const float* __restrict__ gatt, const unsigned char* __restrict__ mask, float dscale,
    int Y, int X, int hq, int wq, int nkv, float* __restrict__ qbuf, float* __restrict__ gobuf,
    float* __restrict__ gqabuf, float4* __restrict__ pair, float* __restrict__ rows) {
  __shared__ float s_w[kHoaWLds];
  __shared__ __attribute__((aligned(8))) float s_kv[kKvLoads * kB * 2];
  __shared__ float s_tok[kTokWg * kHD];
  __shared__ float s_ga[kTokWg * kHD];            // d att of the workgroup's tokens (0 beyond the last token)
  __shared__ float s_o[kTokWg * kHI];
  __shared__ float s_cpb[kB * kCpbW];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int ntok = hq * wq, t0 = blockIdx.x * kTokWg;
  const long plane = (long)Y * X;
  const float* op = opacity + (long)b * kHD * plane;
  const float ry = (float)(Y - 1) / (float)(hq - 1), rx = (float)(X - 1) / (float)(wq - 1);
  // ---- all global loads before the first barrier: weights, kv tokens, the tokens' samples, d att ----
  float wv[kHoaWLoads];
#pragma unroll
  for (int i = 0; i < kHoaWLoads; ++i) wv[i] = wts[min(tid + i * kB, kHoaWeights - 1)];
  float2 kvv[kKvLoads];
  {
    const float2* kv2 = reinterpret_cast<const float2*>(kvbuf + (long)b * nkv * 18);
#pragma unroll
    for (int i = 0; i < kKvLoads; ++i) kvv[i] = kv2[min(tid + i * kB, nkv * 9 - 1)];
  }
  float p00[2], p01[2], p10[2], p11[2], sly[2], slx[2], gav[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int it = min(tid + i * kB, kTokWg * kHD - 1);
    const int wi = it / kHD, c = it % kHD;
    const int t = min(t0 + wi, ntok - 1);
    const AcTaps a = ac_taps(Y, X, ry * (float)(t / wq), rx * (float)(t % wq));
    const float* p = op + c * plane;
    p00[i] = p[(long)a.y0 * X + a.x0]; p01[i] = p[(long)a.y0 * X + a.x1];
    p10[i] = p[(long)a.y1 * X + a.x0]; p11[i] = p[(long)a.y1 * X + a.x1];
    sly[i] = a.ly; slx[i] = a.lx;
    gav[i] = gatt[((long)b * ntok + t) * kHD + c];
  }
  const int tl = tid / kAttSplit, part = tid % kAttSplit;
  const bool has = t0 + tl < ntok;
  const int t = min(t0 + tl, ntok - 1);
  const int ty = t / wq, tx = t % wq;
  const float m = ml[((long)b * ntok + t) * 2], l = ml[((long)b * ntok + t) * 2 + 1];
#pragma unroll
  for (int i = 0; i < kHoaWLoads; ++i) s_w[tid + i * kB] = wv[i];
#pragma unroll
  for (int i = 0; i < kKvLoads; ++i) reinterpret_cast<float2*>(s_kv)[tid + i * kB] = kvv[i];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int it = min(tid + i * kB, kTokWg * kHD - 1);
    s_tok[it] = ac_mix(p00[i], p01[i], p10[i], p11[i], sly[i], slx[i]);
    s_ga[it] = (t0 + it / kHD < ntok) ? gav[i] : 0.f;
  }
  __syncthreads();
  float q[kHI], qs[kHI], go[kHI];
#pragma unroll
  for (int d = 0; d < kHI; ++d) q[d] = 0.f;
#pragma unroll
  for (int c = 0; c < kHD; ++c) {
    const float tk = s_tok[tl * kHD + c];
#pragma unroll
    for (int d = 0; d < kHI; ++d) q[d] = fmaf(s_w[oQ + d * kHD + c], tk, q[d]);
  }
#pragma unroll
  for (int d = 0; d < kHI; ++d) qs[d] = q[d] * kHoaScale;
#pragma unroll
  for (int d = 0; d < kHI; ++d) go[d] = 0.f;
#pragma unroll
  for (int c = 0; c < kHD; ++c) {
    const float g = s_ga[tl * kHD + c];
#pragma unroll
    for (int d = 0; d < kHI; ++d) go[d] = fmaf(s_w[oO + c * kHI + d], g, go[d]);
  }
  const float qx = 2.0f * (float)tx / (float)max(hq - 1, 1) - 1.0f, qy = 2.0f * (float)ty / (float)max(wq - 1, 1) - 1.0f;
  const float inv = 1.f / l;
  const unsigned char* mrow = mask ? mask + ((long)b * ntok + t) * nkv : nullptr;
  // ---- pass 1: o = sum_j dropped weight * v_j (to_out's weight gradient) and delta = sum_j p_j d p_j / sum_j p_j.
  // d sim_j = p_j (d p_j - delta) sums to 0 over a row analytically; in float32 the recomputed weights sum to 1 only to
  // 1e-7 and the row sum comes out as a residue of that size, which is all there is of the gradient of anything the
  // row's scores share.  delta is summed in double from the very products pass 2 subtracts it from, over the weights'
  // own sum: a one-key row has d sim = 0 exactly and a row's d sim cancel to double rounding before they are rounded ----
  float o[kHI];
  double delta = 0.0, psum = 0.0;
#pragma unroll
  for (int d = 0; d < kHI; ++d) o[d] = 0.f;
  for (int j = part; j < nkv; j += kAttSplit) {
    const float* kv = s_kv + j * 18;
    PairState ps;
    const float sc = pair_score(qs, kv, qx, qy, s_w, ps);
    const float p = __expf(sc - m) * inv;
    const float ms = mrow ? (float)mrow[j] * dscale : 1.f;
    const float ad = mrow ? p * ms : p;
    float gad = 0.f;
#pragma unroll
    for (int d = 0; d < kHI; ++d) {
      o[d] = fmaf(ad, kv[8 + d], o[d]);
      gad = fmaf(go[d], kv[8 + d], gad);
    }
    delta += (double)p * (double)(gad * ms);
    psum += (double)p;
  }
#pragma unroll
  for (int off = 1; off < kAttSplit; off <<= 1) {
#pragma unroll
    for (int d = 0; d < kHI; ++d) o[d] += __shfl_xor(o[d], off, kAttSplit);
    delta += __shfl_xor(delta, off, kAttSplit);
    psum += __shfl_xor(psum, off, kAttSplit);
  }
  delta /= psum;
  // ---- pass 2: d sim, d q, CPB ----
  float gq[kHI], cw[kCpbW];
#pragma unroll
  for (int d = 0; d < kHI; ++d) gq[d] = 0.f;
#pragma unroll
  for (int k = 0; k < kCpbW; ++k) cw[k] = 0.f;
  for (int j = part; j < nkv; j += kAttSplit) {
    const float* kv = s_kv + j * 18;
    PairState ps;
    const float sc = pair_score(qs, kv, qx, qy, s_w, ps);
    const float p = __expf(sc - m) * inv;
    const float ms = mrow ? (float)mrow[j] * dscale : 1.f;
    const float ad = mrow ? p * ms : p;
    float gad = 0.f;
#pragma unroll
    for (int d = 0; d < kHI; ++d) gad = fmaf(go[d], kv[8 + d], gad);
    const float gs = (float)((double)p * ((double)(gad * ms) - delta));
#pragma unroll
    for (int d = 0; d < kHI; ++d) gq[d] = fmaf(gs, kv[d], gq[d]);
    // CPB backwards: Linear(3,1) <- ReLU <- Linear(3,3) <- ReLU <- Linear(2,3) <- sign(p) log(|p| + 1).  The last bias
    // is one constant added to every score of a softmax row: its gradient is 0 identically, for any input and mask, and
    // is written as that (cw[24] stays 0) instead of as the rounding residue of the row sums.
    float gz1[3], gh0[3], gz0[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      cw[21 + i] = fmaf(gs, ps.h1[i], cw[21 + i]);
      gz1[i] = ps.z1[i] > 0.f ? gs * s_w[oC2W + i] : 0.f;
      cw[18 + i] += gz1[i];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) gh0[k] = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        cw[9 + i * 3 + k] = fmaf(gz1[i], ps.h0[k], cw[9 + i * 3 + k]);
        gh0[k] = fmaf(gz1[i], s_w[oC1W + i * 3 + k], gh0[k]);
      }
    }
    float gbx = 0.f, gby = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      gz0[i] = ps.z0[i] > 0.f ? gh0[i] : 0.f;
      cw[i * 2] = fmaf(gz0[i], ps.bx, cw[i * 2]);
      cw[i * 2 + 1] = fmaf(gz0[i], ps.by, cw[i * 2 + 1]);
      cw[6 + i] += gz0[i];
      gbx = fmaf(gz0[i], s_w[oC0W + i * 2], gbx);
      gby = fmaf(gz0[i], s_w[oC0W + i * 2 + 1], gby);
    }
    // d/dp sign(p) log(|p| + 1) = 1 / (|p| + 1), 0 at p == 0 (torch: sign' = 0, abs'(0) = 0)
    const float gpx = ps.px == 0.f ? 0.f : gbx / (fabsf(ps.px) + 1.f);
    const float gpy = ps.py == 0.f ? 0.f : gby / (fabsf(ps.py) + 1.f);
    if (has) pair[((long)b * ntok + t) * nkv + j] = make_float4(gs, ad, -gpx, -gpy);       // p = grid_q - grid_kv
  }
#pragma unroll
  for (int off = 1; off < kAttSplit; off <<= 1) {
#pragma unroll
    for (int d = 0; d < kHI; ++d) gq[d] += __shfl_xor(gq[d], off, kAttSplit);
  }
  if (part == 0) {
#pragma unroll
    for (int d = 0; d < kHI; ++d) s_o[tl * kHI + d] = o[d];
    if (has) {
      const long base = ((long)b * ntok + t) * kHI;
#pragma unroll
      for (int d = 0; d < kHI; ++d) {
        qbuf[base + d] = q[d];
        gobuf[base + d] = go[d];
        gqabuf[base + d] = gq[d] * kHoaScale;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kCpbW; ++k) s_cpb[tid * kCpbW + k] = cw[k];
  __syncthreads();
  // ---- this workgroup's row of the weight gradients, every sum in a fixed order ----
  float* row = rows + ((long)b * gridDim.x + blockIdx.x) * kHoaWeights;
  if (tid < kHD * kHI) {                              // to_out.weight[c][d] = sum_t d att[t][c] * o[t][d]
    const int c = tid / kHI, d = tid % kHI;
    float s = 0.f;
    for (int i = 0; i < kTokWg; ++i) s = fmaf(s_ga[i * kHD + c], s_o[i * kHI + d], s);
    row[oO + tid] = s;
  } else if (tid < kHD * kHI + kHD) {                 // to_out.bias
    const int c = tid - kHD * kHI;
    float s = 0.f;
    for (int i = 0; i < kTokWg; ++i) s += s_ga[i * kHD + c];
    row[oOB + c] = s;
  } else if (tid >= 128 && tid < 128 + kCpbW) {       // CPB
    const int k = tid - 128;
    float s = 0.f;
    for (int i = 0; i < kB; ++i) s += s_cpb[i * kCpbW + k];
    row[oC0W + k] = s;
  }
}

// (3) grid (nkv, B): kv token j of sample b.  gabuf (B, nkv, 8): d of the offset conv's output (before GELU);
// gkvin (B, nkv, 16): d of the sampled alpha token [13] | fx | fy | -.  rows (B * nkv, kHoaWeights): the depthwise /
// pointwise offset weights and to_k / to_v are written.
__global__ __launch_bounds__(kB) void hoa1_kv_grad_kernel(
    const float* __restrict__ opacity, const float* __restrict__ alpha, const float* __restrict__ wts,
    const float* __restrict__ kvbuf, const float* __restrict__ qbuf, const float* __restrict__ gobuf,
    const float4* __restrict__ pair, int Y, int X, int hq, int wq, int hk, int wk, float offset_scale,
    float* __restrict__ gabuf, float* __restrict__ gkvin, float* __restrict__ rows) {
  __shared__ float s_w[kHoaWLds];
  __shared__ float s_tok[36 * kHD];
  __shared__ float s_q[36 * kHI];
  __shared__ float s_a[kHI], s_gl[kHI], s_gact[kHI];
  __shared__ float s_f[4];                          // ox, oy, fx, fy
  __shared__ float s_tap[kHD * 16];
  __shared__ float s_kvin[kHD];
  __shared__ float s_red[kB / 64][18];
  __shared__ float s_g[18];                         // d k[8] | d v[8] | d grid (CPB)[2]
  __shared__ float s_gf[kHD * 2];
  __shared__ float s_go[2];
  const int tid = threadIdx.x, j = blockIdx.x, b = blockIdx.y;
  const int ky = j / wk, kx = j % wk, nkv = hk * wk, ntok = hq * wq;
  const long plane = (long)Y * X;
  const float* op = opacity + (long)b * kHD * plane;
  const float* al = alpha + (long)b * kHD * plane;
  const float* kvt = kvbuf + ((long)b * nkv + j) * 18;
  const float ry = (float)(Y - 1) / (float)(hq - 1), rx = (float)(X - 1) / (float)(wq - 1);
  float wv[kHoaWLoads];
#pragma unroll
  for (int i = 0; i < kHoaWLoads; ++i) wv[i] = wts[min(tid + i * kB, kHoaWeights - 1)];
  float p00[2], p01[2], p10[2], p11[2], sly[2], slx[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int it = min(tid + i * kB, 36 * kHD - 1);
    const int wi = it / kHD, c = it % kHD;
    const int qy = min(max(ky * 4 - 1 + wi / 6, 0), hq - 1), qx = min(max(kx * 4 - 1 + wi % 6, 0), wq - 1);
    const AcTaps a = ac_taps(Y, X, ry * (float)qy, rx * (float)qx);
    const float* p = op + c * plane;
    p00[i] = p[(long)a.y0 * X + a.x0]; p01[i] = p[(long)a.y0 * X + a.x1];
    p10[i] = p[(long)a.y1 * X + a.x0]; p11[i] = p[(long)a.y1 * X + a.x1];
    sly[i] = a.ly; slx[i] = a.lx;
  }
  const float grid_x = kvt[16], grid_y = kvt[17];
  // ---- the token's pairs over all query tokens: d k = scale * sum d sim * q, d v = sum weight * d o, d grid ----
  float acc[18];
#pragma unroll
  for (int k = 0; k < 18; ++k) acc[k] = 0.f;
  for (int t = tid; t < ntok; t += kB) {
    const float4 pr = pair[((long)b * ntok + t) * nkv + j];
    const float* qq = qbuf + ((long)b * ntok + t) * kHI;
    const float* gg = gobuf + ((long)b * ntok + t) * kHI;
#pragma unroll
    for (int d = 0; d < kHI; ++d) {
      acc[d] = fmaf(pr.x, qq[d], acc[d]);
      acc[8 + d] = fmaf(pr.y, gg[d], acc[8 + d]);
    }
    acc[16] += pr.z;
    acc[17] += pr.w;
  }
#pragma unroll
  for (int k = 0; k < 18; ++k) {
    float v = acc[k];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((tid & 63) == 0) s_red[tid >> 6][k] = v;
  }
#pragma unroll
  for (int i = 0; i < kHoaWLoads; ++i) s_w[tid + i * kB] = wv[i];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int it = min(tid + i * kB, 36 * kHD - 1);
    s_tok[it] = ac_mix(p00[i], p01[i], p10[i], p11[i], sly[i], slx[i]);
  }
  __syncthreads();
  if (tid < 18) {
    float v = s_red[0][tid];
    for (int w = 1; w < kB / 64; ++w) v += s_red[w][tid];
    s_g[tid] = tid < kHI ? v * kHoaScale : v;
  }
  // ---- the forward's chain again (hoa1_kv_kernel): to_q of the window, offset conv, GELU, 1x1 ----
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int it = tid + i * kB;
    if (it < 36 * kHI) {
      const int wi = it / kHI, d = it % kHI;
      float qv = 0.f;
#pragma unroll
      for (int c = 0; c < kHD; ++c) qv = fmaf(s_w[oQ + d * kHD + c], s_tok[wi * kHD + c], qv);
      s_q[it] = qv;
    }
  }
  __syncthreads();
  if (tid < kHI) {
    const int d = tid;
    float a = s_w[oDB + d];
#pragma unroll
    for (int u = 0; u < 6; ++u) {
      const int yy = ky * 4 - 1 + u;
      const bool yin = yy >= 0 && yy < hq;
#pragma unroll
      for (int v = 0; v < 6; ++v) {
        const int xx = kx * 4 - 1 + v;
        const bool in = yin && xx >= 0 && xx < wq;
        const float w = in ? s_w[oDW + d * 36 + u * 6 + v] : 0.f;
        a = fmaf(w, s_q[(u * 6 + v) * kHI + d], a);
      }
    }
    s_a[d] = a;
    s_gl[d] = 0.5f * a * (1.f + erff(a * 0.70710678118654752f));
  }
  __syncthreads();
  if (tid == 0) {
    float ox = 0.f, oy = 0.f;
#pragma unroll
    for (int d = 0; d < kHI; ++d) {
      ox = fmaf(s_w[oPW + d], s_gl[d], ox);
      oy = fmaf(s_w[oPW + 8 + d], s_gl[d], oy);
    }
    s_f[0] = ox;
    s_f[1] = oy;
    s_f[2] = ((grid_x + 1.f) * (float)wq - 1.f) * 0.5f;        // from the SAVED grid: the forward's cell
    s_f[3] = ((grid_y + 1.f) * (float)hq - 1.f) * 0.5f;
  }
  __syncthreads();
  const float fx = s_f[2], fy = s_f[3];
  const int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
  {
    const int it = min(tid, kHD * 16 - 1);
    const int c = it >> 4, tp = (it >> 2) & 3, cr = it & 3;
    const int xi = min(max(x0 + (tp & 1), 0), wq - 1), yi = min(max(y0 + (tp >> 1), 0), hq - 1);
    const AcTaps a = ac_taps(Y, X, ry * (float)yi, rx * (float)xi);
    const float v = al[c * plane + (long)((cr >> 1) ? a.y1 : a.y0) * X + ((cr & 1) ? a.x1 : a.x0)];
    if (tid < kHD * 16) s_tap[tid] = v;
  }
  __syncthreads();
  // ---- grid_sample (bilinear, zeros, align_corners=False): value, and d of it w.r.t. fx / fy; to_k / to_v ----
  if (tid < kHD) {
    const int c = tid;
    float kvin = 0.f, dfx = 0.f, dfy = 0.f;
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {
      const int xi = x0 + (tp & 1), yi = y0 + (tp >> 1);
      const bool in = xi >= 0 && xi < wq && yi >= 0 && yi < hq;
      const float wxx = 1.f - fabsf(fx - (float)xi), wyy = 1.f - fabsf(fy - (float)yi);
      const AcTaps a = ac_taps(Y, X, ry * (float)min(max(yi, 0), hq - 1), rx * (float)min(max(xi, 0), wq - 1));
      const float* qp = s_tap + c * 16 + tp * 4;
      const float val = ac_mix(qp[0], qp[1], qp[2], qp[3], a.ly, a.lx);
      if (in) {
        kvin = fmaf(val, wxx * wyy, kvin);
        dfx = fmaf(val, (tp & 1) ? wyy : -wyy, dfx);
        dfy = fmaf(val, (tp >> 1) ? wxx : -wxx, dfy);
      }
    }
    float g = 0.f;
#pragma unroll
    for (int d = 0; d < kHI; ++d) g = fmaf(s_w[oK + d * kHD + c], s_g[d], g);
#pragma unroll
    for (int d = 0; d < kHI; ++d) g = fmaf(s_w[oV + d * kHD + c], s_g[8 + d], g);
    s_kvin[c] = kvin;
    s_gf[c * 2] = g * dfx;
    s_gf[c * 2 + 1] = g * dfy;
    gkvin[((long)b * nkv + j) * 16 + c] = g;
  }
  __syncthreads();
  if (tid == 0) {
    float gfx = 0.f, gfy = 0.f;
#pragma unroll
    for (int c = 0; c < kHD; ++c) {
      gfx += s_gf[c * 2];
      gfy += s_gf[c * 2 + 1];
    }
    // fx = ((gx + 1) wq - 1) / 2, gx = 2 vx / max(hk - 1, 1) - 1, vx = kx + tanh(ox) * offset_scale  (y: hq, wk)
    const float ggx = s_g[16] + gfx * (0.5f * (float)wq), ggy = s_g[17] + gfy * (0.5f * (float)hq);
    const float gvx = ggx * (2.0f / (float)max(hk - 1, 1)), gvy = ggy * (2.0f / (float)max(wk - 1, 1));
    const float tx = tanhf(s_f[0]), ty = tanhf(s_f[1]);
    s_go[0] = gvx * offset_scale * (1.f - tx * tx);
    s_go[1] = gvy * offset_scale * (1.f - ty * ty);
    gkvin[((long)b * nkv + j) * 16 + 13] = fx;
    gkvin[((long)b * nkv + j) * 16 + 14] = fy;
    gkvin[((long)b * nkv + j) * 16 + 15] = 0.f;
  }
  __syncthreads();
  float* row = rows + ((long)b * nkv + j) * kHoaWeights;
  if (tid < kHI) {
    const int d = tid;
    const float gox = s_go[0], goy = s_go[1];
    const float ggl = s_w[oPW + d] * gox + s_w[oPW + 8 + d] * goy;
    const float a = s_a[d];
    const float cdf = 0.5f * (1.f + erff(a * 0.70710678118654752f));
    const float pdf = 0.3989422804014327f * expf(-0.5f * a * a);
    const float ga = ggl * (cdf + a * pdf);                       // exact GELU'
    s_gact[d] = ga;
    gabuf[((long)b * nkv + j) * kHI + d] = ga;
    row[oDB + d] = ga;
    row[oPW + d] = gox * s_gl[d];
    row[oPW + 8 + d] = goy * s_gl[d];
  } else if (tid >= 16 && tid < 16 + 2 * kHI * kHD) {             // to_k / to_v [d][c] = d k[d] * sampled[c]
    const int i = tid - 16;
    const int which = i / (kHI * kHD), r = i % (kHI * kHD);
    row[(which ? oV : oK) + r] = s_g[which * 8 + r / kHD] * s_kvin[r % kHD];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {                                   // depthwise weights [d][u][v], 0 outside the map
    const int it = tid + i * kB;
    if (it < kHI * 36) {
      const int d = it / 36, uv = it % 36;
      const int yy = ky * 4 - 1 + uv / 6, xx = kx * 4 - 1 + uv % 6;
      const bool in = yy >= 0 && yy < hq && xx >= 0 && xx < wq;
      row[oDW + it] = in ? s_gact[d] * s_q[uv * kHI + d] : 0.f;
    }
  }
}

// (4) grid (ceil(ntok / kTokWg), B): d q (attention branch + the offset windows the token lies in), to_q, and the
// gather of the alpha token's gradient over the samples whose bilinear cell has it as a corner.
// gtok / gatok (B, ntok, 13); rows (B * gridDim.x, kHoaWeights): to_q is written.
__global__ __launch_bounds__(kB) void hoa1_token_grad_kernel(
    const float* __restrict__ opacity, const float* __restrict__ wts, const float* __restrict__ gqabuf,
    const float* __restrict__ gabuf, const float* __restrict__ gkvin, int Y, int X, int hq, int wq, int hk, int wk,
    float* __restrict__ gtok, float* __restrict__ gatok, float* __restrict__ rows) {
  __shared__ float s_w[kHoaWLds];
  __shared__ float s_tok[kTokWg * kHD];
  __shared__ float s_gq[kTokWg * kHI];
  __shared__ float s_gk[kHMaxKV * 16];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int ntok = hq * wq, nkv = hk * wk, t0 = blockIdx.x * kTokWg;
  const long plane = (long)Y * X;
  const float* op = opacity + (long)b * kHD * plane;
  const float ry = (float)(Y - 1) / (float)(hq - 1), rx = (float)(X - 1) / (float)(wq - 1);
  float wv[kHoaWLoads];
#pragma unroll
  for (int i = 0; i < kHoaWLoads; ++i) wv[i] = wts[min(tid + i * kB, kHoaWeights - 1)];
  float p00[2], p01[2], p10[2], p11[2], sly[2], slx[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int it = min(tid + i * kB, kTokWg * kHD - 1);
    const int wi = it / kHD, c = it % kHD;
    const int t = min(t0 + wi, ntok - 1);
    const AcTaps a = ac_taps(Y, X, ry * (float)(t / wq), rx * (float)(t % wq));
    const float* p = op + c * plane;
    p00[i] = p[(long)a.y0 * X + a.x0]; p01[i] = p[(long)a.y0 * X + a.x1];
    p10[i] = p[(long)a.y1 * X + a.x0]; p11[i] = p[(long)a.y1 * X + a.x1];
    sly[i] = a.ly; slx[i] = a.lx;
  }
  float gkv[kHMaxKV * 16 / kB];
#pragma unroll
  for (int i = 0; i < kHMaxKV * 16 / kB; ++i) gkv[i] = gkvin[(long)b * nkv * 16 + min(tid + i * kB, nkv * 16 - 1)];
  const int tl = tid / kHI, d = tid % kHI;
  const bool has = t0 + tl < ntok;
  const int t = min(t0 + tl, ntok - 1);
  const int ty = t / wq, tx = t % wq;
  float gq = gqabuf[((long)b * ntok + t) * kHI + d];
#pragma unroll
  for (int i = 0; i < kHoaWLoads; ++i) s_w[tid + i * kB] = wv[i];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int it = min(tid + i * kB, kTokWg * kHD - 1);
    s_tok[it] = ac_mix(p00[i], p01[i], p10[i], p11[i], sly[i], slx[i]);
  }
#pragma unroll
  for (int i = 0; i < kHMaxKV * 16 / kB; ++i) s_gk[tid + i * kB] = gkv[i];
  __syncthreads();
  // window (ky, kx) covers query rows 4 ky - 1 .. 4 ky + 4: a token lies in at most 2 x 2 of them
  const int kylo = ty <= 4 ? 0 : (ty - 1) / 4, kyhi = min((ty + 1) / 4, hk - 1);
  const int kxlo = tx <= 4 ? 0 : (tx - 1) / 4, kxhi = min((tx + 1) / 4, wk - 1);
  for (int ky = kylo; ky <= kyhi; ++ky)
    for (int kx = kxlo; kx <= kxhi; ++kx) {
      const int u = ty - (4 * ky - 1), v = tx - (4 * kx - 1);
      if (u < 0 || u > 5 || v < 0 || v > 5) continue;
      gq = fmaf(s_w[oDW + d * 36 + u * 6 + v], gabuf[((long)b * nkv + ky * wk + kx) * kHI + d], gq);
    }
  s_gq[tid] = has ? gq : 0.f;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int it = tid + i * kB;
    const int wi = it / kHD, c = it % kHD;
    if (it < kTokWg * kHD && t0 + wi < ntok) {
      const int tt = t0 + wi;
      float g = 0.f;
#pragma unroll
      for (int dd = 0; dd < kHI; ++dd) g = fmaf(s_w[oQ + dd * kHD + c], s_gq[wi * kHI + dd], g);
      gtok[((long)b * ntok + tt) * kHD + c] = g;
      const int yy = tt / wq, xx = tt % wq;
      float ga = 0.f;
      for (int j = 0; j < nkv; ++j) {
        const float fx = s_gk[j * 16 + 13], fy = s_gk[j * 16 + 14];
        const int ddx = xx - (int)floorf(fx), ddy = yy - (int)floorf(fy);
        if (ddx >= 0 && ddx <= 1 && ddy >= 0 && ddy <= 1)
          ga = fmaf((1.f - fabsf(fx - (float)xx)) * (1.f - fabsf(fy - (float)yy)), s_gk[j * 16 + c], ga);
      }
      gatok[((long)b * ntok + tt) * kHD + c] = ga;
    }
  }
  if (tid < kHI * kHD) {                             // to_q.weight[d][c] = sum_t d q[t][d] * tok[t][c]
    const int dd = tid / kHD, c = tid % kHD;
    float s = 0.f;
    for (int i = 0; i < kTokWg; ++i) s = fmaf(s_gq[i * kHI + dd], s_tok[i * kHD + c], s);
    rows[((long)b * gridDim.x + blockIdx.x) * kHoaWeights + oQ + tid] = s;
  }
}

// the token (of n) that has position p (of size) as a corner tap of its align-corners sample, and p's weight in it
__device__ __forceinline__ void down_weight(int size, int n, int p, int& tk, float& w) {
  const float r = (float)(size - 1) / (float)(n - 1);
  const int cand = (int)((float)p / r);
  tk = 0;
  w = 0.f;
  for (int k = max(cand - 1, 0); k <= min(cand + 1, n - 1); ++k) {
    const float s = r * (float)k;
    const int i0 = min((int)s, size - 1), i1 = min(i0 + 1, size - 1);
    const float l = s - (float)i0;
    if (p == i0 || p == i1) {
      tk = k;
      w = (p == i0 ? 1.f - l : 0.f) + (p == i1 ? l : 0.f);
    }
  }
}

// (5) grad_opacity = grad_out + w * gtok[token], grad_alpha = w * gatok[token]: one pixel per thread
__global__ __launch_bounds__(kB) void hoa1_pixel_grad_kernel(const float* __restrict__ gout, const float* __restrict__ gtok,
                                                             const float* __restrict__ gatok, int Y, int X, int hq, int wq,
                                                             float* __restrict__ gop, float* __restrict__ gal) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
  if (x >= X || y >= Y) return;
  int ty, tx;
  float wy, wx;
  down_weight(Y, hq, y, ty, wy);
  down_weight(X, wq, x, tx, wx);
  const float w = wy * wx;
  const long plane = (long)Y * X, pix = (long)y * X + x;
  const long tb = ((long)b * hq * wq + (long)ty * wq + tx) * kHD;
  float g[kHD], a[kHD], o[kHD];
#pragma unroll
  for (int c = 0; c < kHD; ++c) {
    g[c] = gout[((long)b * kHD + c) * plane + pix];
    a[c] = gtok[tb + c];
    o[c] = gatok[tb + c];
  }
#pragma unroll
  for (int c = 0; c < kHD; ++c) {
    gop[((long)b * kHD + c) * plane + pix] = w != 0.f ? fmaf(w, a[c], g[c]) : g[c];
    gal[((long)b * kHD + c) * plane + pix] = w != 0.f ? w * o[c] : 0.f;
  }
}

// (6) grad_weights[i] = sum of the partial rows that own entry i, in row order
__global__ __launch_bounds__(kB) void hoa1_weight_sum_kernel(const float* __restrict__ rows_attn, int n_attn,
                                                             const float* __restrict__ rows_kv, int n_kv,
                                                             const float* __restrict__ rows_tok, int n_tok,
                                                             float* __restrict__ gw) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= kHoaWeights) return;
  const float* rows = i < oDW ? rows_tok : (i < oO ? rows_kv : rows_attn);
  const int n = i < oDW ? n_tok : (i < oO ? n_kv : n_attn);
  float s = 0.f;
#pragma unroll 8
  for (int r = 0; r < n; ++r) s += rows[(long)r * kHoaWeights + i];
  gw[i] = s;
}

// the workspace, in floats; every section starts on a 16-byte boundary
struct Layout {
  int hq, wq, hk, wk, ntok, nkv, n_wg;
  size_t kv, ml, gatt, q, go, gqa, pair, ga, gkvin, gtok, gatok, rows_attn, rows_kv, rows_tok, total;
};
bool make_layout(int B, int Y, int X, Layout& L) {
  if (B <= 0 || Y <= 0 || X <= 0) return false;
  L.hq = Y / 6; L.wq = X / 6;
  if (L.hq < 6 || L.wq < 6) return false;
  L.hk = (L.hq + 2 - 6) / 4 + 1; L.wk = (L.wq + 2 - 6) / 4 + 1;
  L.ntok = L.hq * L.wq; L.nkv = L.hk * L.wk;
  if (L.ntok > kHMaxTok || L.nkv > kHMaxKV || B > 65535) return false;
  L.n_wg = (L.ntok + kTokWg - 1) / kTokWg;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += (n + 3) / 4 * 4; return at; };
  const size_t bt = (size_t)B * L.ntok, bk = (size_t)B * L.nkv;
  L.kv = take(bk * 18); L.ml = take(bt * 2); L.gatt = take(bt * kHD); L.q = take(bt * kHI); L.go = take(bt * kHI);
  L.gqa = take(bt * kHI); L.pair = take(bt * L.nkv * 4); L.ga = take(bk * kHI); L.gkvin = take(bk * 16);
  L.gtok = take(bt * kHD); L.gatok = take(bt * kHD);
  L.rows_attn = take((size_t)B * L.n_wg * kHoaWeights); L.rows_kv = take(bk * kHoaWeights);
  L.rows_tok = take((size_t)B * L.n_wg * kHoaWeights);
  L.total = o;
  return true;
}

}  // namespace

extern "C" {

size_t ocrf_hoa1_train_workspace_floats(int B, int Y, int X) {
  Layout L;
  return make_layout(B, Y, X, L) ? L.total : 0;
}

int ocrf_hoa1_forward_train(const float* opacity, const float* alpha, const float* weights, int B, int Y, int X,
                            float offset_scale, const unsigned char* dropout_mask, float dropout_scale, float* workspace,
                            float* out, ocrf_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  Layout L;
  if (!opacity || !alpha || !weights || !workspace || !out || !make_layout(B, Y, X, L)) return (int)hipErrorInvalidValue;
  float* kvbuf = workspace + L.kv;
  launch_kv(stream, opacity, alpha, weights, B, Y, X, L.hq, L.wq, L.hk, L.wk, offset_scale, kvbuf);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  ocrf::launch(OCRF_K_HOA1_ATTN_TRAIN, hoa1_attention_train_kernel, dim3((X + kTP - 1) / kTP, (Y + kTP - 1) / kTP, B),
               dim3(kB), 0, stream, opacity, static_cast<const float*>(kvbuf), weights, Y, X, L.hq, L.wq, L.nkv, out,
               dropout_mask, dropout_scale, workspace + L.ml);
  return (int)hipGetLastError();
}

int ocrf_hoa1_backward(const float* grad_out, const float* opacity, const float* alpha, const float* weights, int B, int Y,
                       int X, float offset_scale, const unsigned char* dropout_mask, float dropout_scale,
                       float* workspace, float* grad_opacity, float* grad_alpha, float* grad_weights,
                       ocrf_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  Layout L;
  if (!grad_out || !opacity || !alpha || !weights || !workspace || !grad_opacity || !grad_alpha || !grad_weights ||
      !make_layout(B, Y, X, L))
    return (int)hipErrorInvalidValue;
  float* ws = workspace;
  const float* kvbuf = ws + L.kv;
  const long n_items = (long)B * L.ntok * kHD;
  ocrf::launch(OCRF_K_HOA1_UP_GRAD, hoa1_up_grad_kernel, dim3((unsigned)((n_items + kB / kUpLanes - 1) / (kB / kUpLanes))),
               dim3(kB), 0, stream, grad_out, B, Y, X, L.hq, L.wq, ws + L.gatt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  ocrf::launch(OCRF_K_HOA1_ATTN_GRAD, hoa1_attn_grad_kernel, dim3(L.n_wg, B), dim3(kB), 0, stream, opacity, kvbuf, weights,
               static_cast<const float*>(ws + L.ml), static_cast<const float*>(ws + L.gatt), dropout_mask, dropout_scale, Y,
               X, L.hq, L.wq, L.nkv, ws + L.q, ws + L.go, ws + L.gqa, reinterpret_cast<float4*>(ws + L.pair),
               ws + L.rows_attn);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  ocrf::launch(OCRF_K_HOA1_KV_GRAD, hoa1_kv_grad_kernel, dim3(L.nkv, B), dim3(kB), 0, stream, opacity, alpha, weights, kvbuf,
               static_cast<const float*>(ws + L.q), static_cast<const float*>(ws + L.go),
               reinterpret_cast<const float4*>(ws + L.pair), Y, X, L.hq, L.wq, L.hk, L.wk, offset_scale, ws + L.ga,
               ws + L.gkvin, ws + L.rows_kv);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  ocrf::launch(OCRF_K_HOA1_TOKEN_GRAD, hoa1_token_grad_kernel, dim3(L.n_wg, B), dim3(kB), 0, stream, opacity, weights,
               static_cast<const float*>(ws + L.gqa), static_cast<const float*>(ws + L.ga),
               static_cast<const float*>(ws + L.gkvin), Y, X, L.hq, L.wq, L.hk, L.wk, ws + L.gtok, ws + L.gatok,
               ws + L.rows_tok);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  ocrf::launch(OCRF_K_HOA1_PIXEL_GRAD, hoa1_pixel_grad_kernel, dim3((X + 63) / 64, (Y + 3) / 4, B), dim3(kB), 0, stream,
               grad_out, static_cast<const float*>(ws + L.gtok), static_cast<const float*>(ws + L.gatok), Y, X, L.hq, L.wq,
               grad_opacity, grad_alpha);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  ocrf::launch(OCRF_K_HOA1_WEIGHT_SUM, hoa1_weight_sum_kernel, dim3((kHoaWeights + kB - 1) / kB), dim3(kB), 0, stream,
               static_cast<const float*>(ws + L.rows_attn), B * L.n_wg, static_cast<const float*>(ws + L.rows_kv),
               B * L.nkv, static_cast<const float*>(ws + L.rows_tok), B * L.n_wg, grad_weights);
  return (int)hipGetLastError();
}

}  // extern "C"
