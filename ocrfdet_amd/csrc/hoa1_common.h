// What the eval kernels of HOA-1 (hoa.hip) and its training kernels (hoa1_train.hip) share: the fixed configuration,
// the packed-weight layout, the align-corners bilinear taps, the DPP merge, and the attention + upsample kernel's body
// for the training forward: the eval kernel's arithmetic, operation for operation (tests hold the two to each other bit
// for bit), plus the dropout keep-mask and the saved softmax state.  The eval kernel itself stays in hoa.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "launch.h"
#include "ocrf_hip.h"

namespace ocrf {
namespace hoa1 {

constexpr int kHoaBlock = 256;
constexpr int kHD = 13, kHI = 8, kHMaxTok = 1600, kHMaxKV = 128;
// Packed weights (floats): to_q[8][13] | off_dw[8][36] | off_db[8] | off_pw[2][8] | to_k[8][13] | to_v[8][13] |
//   to_out[13][8] | to_out_b[13] | cpb0_w[3][2] | cpb0_b[3] | cpb1_w[3][3] | cpb1_b[3] | cpb2_w[3] | cpb2_b[1]
constexpr int oQ = 0, oDW = oQ + 8 * 13, oDB = oDW + 8 * 36, oPW = oDB + 8, oK = oPW + 16, oV = oK + 104,
              oO = oV + 104, oOB = oO + 104, oC0W = oOB + 13, oC0B = oC0W + 6, oC1W = oC0B + 3, oC1B = oC1W + 9,
              oC2W = oC1B + 3, oC2B = oC2W + 3, kHoaWeights = oC2B + 1;
constexpr float kHoaScale = 0.35355339059327373f;               // dim_head ** -0.5

// F.interpolate(..., mode='bilinear', align_corners=True) sample of one channel plane at (sy, sx): the four corner taps
// and their mix, separately — corner q of a sample is one load, the mix happens once they are all back
struct AcTaps { int y0, y1, x0, x1; float ly, lx; };
__device__ __forceinline__ AcTaps ac_taps(int H, int W, float sy, float sx) {
  AcTaps a;
  a.y0 = min((int)sy, H - 1); a.x0 = min((int)sx, W - 1);
  a.y1 = min(a.y0 + 1, H - 1); a.x1 = min(a.x0 + 1, W - 1);
  a.ly = sy - (float)a.y0; a.lx = sx - (float)a.x0;
  return a;
}
__device__ __forceinline__ float ac_mix(float p00, float p01, float p10, float p11, float ly, float lx) {
  const float top = p00 * (1.f - lx) + p01 * lx;
  const float bot = p10 * (1.f - lx) + p11 * lx;
  return top * (1.f - ly) + bot * ly;
}

constexpr int kHoaWLoads = (kHoaWeights + kHoaBlock - 1) / kHoaBlock;      // 3
constexpr int kHoaWLds = kHoaWLoads * kHoaBlock;    // LDS copy of the packed weights: every thread stores every word it loaded

constexpr int kAttSplit = 8, kTP = 16, kTT = 5;
constexpr int kKvLoads = (kHMaxKV * 9 + kHoaBlock - 1) / kHoaBlock;       // 8-byte words of the kv tokens per thread (5)
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppMirror8 = 0x141;   // quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror
template <int CTRL>
__device__ __forceinline__ float hoa_dpp(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}

// hoa.hip: the launch of hoa1_kv_kernel (grid (nkv, B)), for the training forward, which keeps the same kv buffer
void launch_kv(hipStream_t stream, const float* opacity, const float* alpha, const float* wts, int B, int Y, int X, int hq,
               int wq, int hk, int wk, float offset_scale, float* kvbuf);

// attention + to_out + bilinear upsample + residual of one 16x16 output tile.  The tile's pixels interpolate between
// at most kTT x kTT tokens of the (hq, wq) attention map ((hq - 1) / (Y - 1) < 1/6: 15 pixels span < 2.5 tokens); the
// workgroup rebuilds q for those tokens from the opacity volume, runs their attention over the sample's kv tokens
// (LDS, online softmax, kAttSplit lanes per token merged by a fixed DPP butterfly) and keeps the 13 output channels
// in LDS for the interpolation: no q / attention buffers and no separate upsample launch.  Tokens shared by
// neighbouring tiles are recomputed (a token's attention is ~6 k flops).  The kernel is a latency chain on a chip
// it cannot fill (338 workgroups at 2 x 200 x 200), so every global load — the token's 52 bilinear taps, the pixel's
// 13 residual values, weights and kv tokens — is issued before the first barrier.
// TRAIN: `mask` (B, ntok, nkv) bytes or NULL and `dscale` = 1 / (1 - p): a pair's softmax weight is multiplied by
// mask * dscale after the normalisation (nn.Dropout on attn: the sum l stays the sum of ALL weights); ml (B, ntok, 2)
// receives every token's softmax maximum and sum (tiles that share a token store the same bits).
template <bool TRAIN>
__device__ __forceinline__ void attention_upsample_body(
    const float* __restrict__ opacity, const float* __restrict__ kvbuf, const float* __restrict__ wts, int Y, int X,
    int hq, int wq, int nkv, float* __restrict__ out, const unsigned char* __restrict__ mask, float dscale,
    float* __restrict__ ml) {
  constexpr int kBlock = kHoaBlock;
  __shared__ float s_w[kHoaWLds];
  __shared__ __attribute__((aligned(8))) float s_kv[kKvLoads * kBlock * 2];      // [nkv][18], padded to whole trips
  __shared__ float s_tok[kTT * kTT * kHD];
  __shared__ float s_att[kTT * kTT * kHD];
  const int tid = threadIdx.x, b = blockIdx.z;
  const long plane = (long)Y * X;
  const float* op = opacity + (long)b * kHD * plane;
  // token window of the tile: the bilinear_ac taps of its first and last pixel
  const float dy = Y > 1 ? (float)(hq - 1) / (float)(Y - 1) : 0.f, dx = X > 1 ? (float)(wq - 1) / (float)(X - 1) : 0.f;
  const int py0 = blockIdx.y * kTP, px0 = blockIdx.x * kTP;
  const int py1 = min(py0 + kTP, Y) - 1, px1 = min(px0 + kTP, X) - 1;
  const int ty0 = min((int)(dy * (float)py0), hq - 1), tx0 = min((int)(dx * (float)px0), wq - 1);
  const int ty1 = min(min((int)(dy * (float)py1), hq - 1) + 1, hq - 1), tx1 = min(min((int)(dx * (float)px1), wq - 1) + 1, wq - 1);
  const int nty = ty1 - ty0 + 1, ntx = tx1 - tx0 + 1;       // <= kTT each
  const int tl = tid / kAttSplit, part = tid % kAttSplit;
  const bool has = tl < nty * ntx;
  const int lt = has ? tl : 0;                               // idle lanes of a live wave run token 0
  const int ty = ty0 + lt / ntx, tx = tx0 + lt % ntx;
  const float ry = hq > 1 ? (float)(Y - 1) / (float)(hq - 1) : 0.f, rx = wq > 1 ? (float)(X - 1) / (float)(wq - 1) : 0.f;
  // ---- all global loads, unconditional (clamped), before the first wait: weights, kv tokens, the window tokens'
  // bilinear samples — one (token, channel) sample of four corner taps per thread and trip instead of every one of
  // a token's eight lanes loading all 52 — and the pixel's residual ----
  float wv[kHoaWLoads];
#pragma unroll
  for (int i = 0; i < kHoaWLoads; ++i) wv[i] = wts[min(tid + i * kBlock, kHoaWeights - 1)];
  float2 kvv[kKvLoads];
  {
    const float2* kv2 = reinterpret_cast<const float2*>(kvbuf + (long)b * nkv * 18);      // 18 floats per token: 8-byte aligned
#pragma unroll
    for (int i = 0; i < kKvLoads; ++i) kvv[i] = kv2[min(tid + i * kBlock, nkv * 9 - 1)];
  }
  float p00[2], p01[2], p10[2], p11[2], sly[2], slx[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int it = min(tid + i * kBlock, nty * ntx * kHD - 1);
    const int wi = it / kHD, c = it % kHD;
    const AcTaps a = ac_taps(Y, X, ry * (float)(ty0 + wi / ntx), rx * (float)(tx0 + wi % ntx));
    const float* p = op + c * plane;
    p00[i] = p[(long)a.y0 * X + a.x0]; p01[i] = p[(long)a.y0 * X + a.x1];
    p10[i] = p[(long)a.y1 * X + a.x0]; p11[i] = p[(long)a.y1 * X + a.x1];
    sly[i] = a.ly; slx[i] = a.lx;
  }
  const int y = py0 + tid / kTP, x = px0 + tid % kTP;
  const bool inside = y < Y && x < X;
  const long pix = (long)min(y, Y - 1) * X + min(x, X - 1);
  float res[kHD];
#pragma unroll
  for (int c = 0; c < kHD; ++c) res[c] = op[c * plane + pix];
#pragma unroll
  for (int i = 0; i < kHoaWLoads; ++i) s_w[tid + i * kBlock] = wv[i];
#pragma unroll
  for (int i = 0; i < kKvLoads; ++i) reinterpret_cast<float2*>(s_kv)[tid + i * kBlock] = kvv[i];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int it = min(tid + i * kBlock, nty * ntx * kHD - 1);    // (clamped duplicates store the same value)
    s_tok[it] = ac_mix(p00[i], p01[i], p10[i], p11[i], sly[i], slx[i]);
  }
  __syncthreads();
  float tok[kHD];
#pragma unroll
  for (int c = 0; c < kHD; ++c) tok[c] = s_tok[lt * kHD + c];
  // ---- attention of the window's tokens: kAttSplit adjacent lanes per token ----
  if (tl < kTT * kTT) {          // wave-uniform up to the last wave
    const float scale = kHoaScale;
    float q[kHI];
#pragma unroll
    for (int d = 0; d < kHI; ++d) q[d] = 0.f;
#pragma unroll
    for (int c = 0; c < kHD; ++c) {
#pragma unroll
      for (int d = 0; d < kHI; ++d) q[d] = fmaf(s_w[oQ + d * kHD + c], tok[c], q[d]);
    }
#pragma unroll
    for (int d = 0; d < kHI; ++d) q[d] *= scale;
    // query grid: create_grid_like(x_kv) normalised with dim=0 -> x over (h-1), y over (w-1)
    const float qx = 2.0f * (float)tx / (float)max(hq - 1, 1) - 1.0f, qy = 2.0f * (float)ty / (float)max(wq - 1, 1) - 1.0f;
    float m = -INFINITY, l = 0.f, acc[kHI];
#pragma unroll
    for (int d = 0; d < kHI; ++d) acc[d] = 0.f;
    const unsigned char* mrow = nullptr;
    if constexpr (TRAIN) {
      if (mask) mrow = mask + ((long)b * hq * wq + (long)ty * wq + tx) * nkv;
    }
#pragma unroll 2
    for (int j = part; j < nkv; j += kAttSplit) {
      const float* kv = s_kv + j * 18;
      float sc = 0.f;
#pragma unroll
      for (int d = 0; d < kHI; ++d) sc = fmaf(q[d], kv[d], sc);
      // CPB (cross_attention_2d.py:74-89)
      const float px = qx - kv[16], py = qy - kv[17];
      const float bx = copysignf(__logf(fabsf(px) + 1.f), px), by = copysignf(__logf(fabsf(py) + 1.f), py);
      float h0[3], h1[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) h0[i] = fmaxf(fmaf(s_w[oC0W + i * 2], bx, fmaf(s_w[oC0W + i * 2 + 1], by, s_w[oC0B + i])), 0.f);
#pragma unroll
      for (int i = 0; i < 3; ++i)
        h1[i] = fmaxf(s_w[oC1B + i] + s_w[oC1W + i * 3] * h0[0] + s_w[oC1W + i * 3 + 1] * h0[1] + s_w[oC1W + i * 3 + 2] * h0[2], 0.f);
      sc += s_w[oC2B] + s_w[oC2W] * h1[0] + s_w[oC2W + 1] * h1[1] + s_w[oC2W + 2] * h1[2];
      const float mn = fmaxf(m, sc);
      const float corr = __expf(m - mn), p = __expf(sc - mn);
      l = l * corr + p;
      float pv = p;
      if constexpr (TRAIN) {
        if (mrow) pv = p * ((float)mrow[j] * dscale);        // (mask 1, scale 1: p itself)
      }
#pragma unroll
      for (int d = 0; d < kHI; ++d) acc[d] = fmaf(pv, kv[8 + d], acc[d] * corr);
      m = mn;
    }
    // merge the kAttSplit partial softmax states: fixed butterfly over the 8 lanes (lane ^ 1, lane ^ 2, 7 - lane)
    auto merge = [&](auto perm) {
      const float mo = perm(m), lo = perm(l);
      const float mn = fmaxf(m, mo);
      const float c1 = (m == -INFINITY) ? 0.f : __expf(m - mn), c2 = (mo == -INFINITY) ? 0.f : __expf(mo - mn);
      l = l * c1 + lo * c2;
#pragma unroll
      for (int d = 0; d < kHI; ++d) acc[d] = acc[d] * c1 + perm(acc[d]) * c2;
      m = mn;
    };
    merge([](float v) { return hoa_dpp<kDppXor1>(v); });
    merge([](float v) { return hoa_dpp<kDppXor2>(v); });
    merge([](float v) { return hoa_dpp<kDppMirror8>(v); });
    if (has) {
      const float inv = 1.f / l;
      for (int c = part; c < kHD; c += kAttSplit) {          // the output projection's channels are shared out too
        float o = s_w[oOB + c];
#pragma unroll
        for (int d = 0; d < kHI; ++d) o = fmaf(s_w[oO + c * kHI + d], acc[d] * inv, o);
        s_att[lt * kHD + c] = o;
      }
      if constexpr (TRAIN) {
        if (part == 0) {
          float* dst = ml + ((long)b * hq * wq + (long)ty * wq + tx) * 2;
          dst[0] = m;
          dst[1] = l;
        }
      }
    }
  }
  __syncthreads();
  // ---- upsample (bilinear, align_corners) + residual: one pixel per thread, 13 channels ----
  if (!inside) return;
  const float sy = dy * (float)y, sx = dx * (float)x;
  const int y0 = min((int)sy, hq - 1), x0 = min((int)sx, wq - 1);
  const int y1 = min(y0 + 1, hq - 1), x1 = min(x0 + 1, wq - 1);
  const float ly = sy - (float)y0, lx = sx - (float)x0;
  const int i00 = ((y0 - ty0) * ntx + (x0 - tx0)) * kHD, i01 = ((y0 - ty0) * ntx + (x1 - tx0)) * kHD;
  const int i10 = ((y1 - ty0) * ntx + (x0 - tx0)) * kHD, i11 = ((y1 - ty0) * ntx + (x1 - tx0)) * kHD;
#pragma unroll
  for (int c = 0; c < kHD; ++c) {
    const float top = s_att[i00 + c] * (1.f - lx) + s_att[i01 + c] * lx;
    const float bot = s_att[i10 + c] * (1.f - lx) + s_att[i11 + c] * lx;
    out[((long)b * kHD + c) * plane + pix] = (top * (1.f - ly) + bot * ly) + res[c];
  }
}

}  // namespace hoa1
}  // namespace ocrf
