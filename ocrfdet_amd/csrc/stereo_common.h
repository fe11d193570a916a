// What the two stereo cost volume kernels (stereo.hip: float32 planar features; stereo_bf16.hip: bfloat16 features packed
// 8 channels per pixel) compute identically, written once: the camera's matrices, the projection of a frustum cell, the
// bilinear taps, the per-channel expression, the online softmax over depth and its second pass.  The semantics are the
// ones listed at the top of stereo.hip.  Every expression here is float32 and is evaluated in the order it is written
// (the library is built with -ffp-contract=off), so both kernels give the same bits for the same feature values.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace ocrf {
namespace stereo {

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kJ = 8;                   // depth bins per chunk held in registers

struct Cam {
  float pri[9];                         // inv(post_rot)
  float comb[9];                        // R_k2s . inv(K)
  float K[9];
  float t[3], pt[3];                    // t_k2s, post_trans
  float pr2[4];                         // post_rot[:2, :2]
};

__device__ __forceinline__ void inv3(const float* m, float* r) {
  const float c00 = m[4] * m[8] - m[5] * m[7];
  const float c01 = m[5] * m[6] - m[3] * m[8];
  const float c02 = m[3] * m[7] - m[4] * m[6];
  const float det = m[0] * c00 + m[1] * c01 + m[2] * c02;
  const float id = 1.0f / det;
  r[0] = c00 * id;
  r[1] = (m[2] * m[7] - m[1] * m[8]) * id;
  r[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  r[3] = c01 * id;
  r[4] = (m[0] * m[8] - m[2] * m[6]) * id;
  r[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  r[6] = c02 * id;
  r[7] = (m[1] * m[6] - m[0] * m[7]) * id;
  r[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

__device__ __forceinline__ void load_cam(int cam, const float* k2s, const float* intrins, const float* post_rots,
                                         const float* post_trans, Cam* c) {
  const float* S = k2s + cam * 16;
  const float* Kp = intrins + cam * 9;
  const float* P = post_rots + cam * 9;
  float Ki[9];
  for (int i = 0; i < 9; ++i) c->K[i] = Kp[i];
  inv3(c->K, Ki);
  float Pm[9];
  for (int i = 0; i < 9; ++i) Pm[i] = P[i];
  inv3(Pm, c->pri);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      c->comb[i * 3 + j] = S[i * 4 + 0] * Ki[0 * 3 + j] + S[i * 4 + 1] * Ki[1 * 3 + j] + S[i * 4 + 2] * Ki[2 * 3 + j];
    c->t[i] = S[i * 4 + 3];
    c->pt[i] = post_trans[cam * 3 + i];
  }
  c->pr2[0] = Pm[0];
  c->pr2[1] = Pm[1];
  c->pr2[2] = Pm[3];
  c->pr2[3] = Pm[4];
}

// Normalised grid coordinate of frustum cell (u, v, dep): gen_grid's steps 1-6 and the normalisation
__device__ __forceinline__ void grid_point(const Cam& c, float u, float v, float dep, float wi1, float hi1, float* px,
                                           float* py) {
  const float a0 = u - c.pt[0], a1 = v - c.pt[1], a2 = dep - c.pt[2];
  float p0 = c.pri[0] * a0 + c.pri[1] * a1 + c.pri[2] * a2;
  float p1 = c.pri[3] * a0 + c.pri[4] * a1 + c.pri[5] * a2;
  const float p2 = c.pri[6] * a0 + c.pri[7] * a1 + c.pri[8] * a2;
  p0 = p0 * p2;
  p1 = p1 * p2;
  const float q0 = c.comb[0] * p0 + c.comb[1] * p1 + c.comb[2] * p2 + c.t[0];
  const float q1 = c.comb[3] * p0 + c.comb[4] * p1 + c.comb[5] * p2 + c.t[1];
  const float q2 = c.comb[6] * p0 + c.comb[7] * p1 + c.comb[8] * p2 + c.t[2];
  const bool neg = !(q2 >= 1e-3f);       // neg_mask (NaN included: such a cell samples nothing)
  const float r0 = c.K[0] * q0 + c.K[1] * q1 + c.K[2] * q2;
  const float r1 = c.K[3] * q0 + c.K[4] * q1 + c.K[5] * q2;
  const float r2 = c.K[6] * q0 + c.K[7] * q1 + c.K[8] * q2;
  const float x = r0 / r2, y = r1 / r2;
  const float s0 = c.pr2[0] * x + c.pr2[1] * y + c.pt[0];
  const float s1 = c.pr2[2] * x + c.pr2[3] * y + c.pt[1];
  *px = neg ? -2.0f : s0 / wi1 * 2.0f - 1.0f;
  *py = neg ? -2.0f : s1 / hi1 * 2.0f - 1.0f;
}

// grid_sample's bilinear taps (align_corners=True, zeros padding) as clamped in-plane offsets and masked weights:
// an out-of-range corner keeps weight 0 and reads an in-range address, so every load is in bounds.  Offsets are in
// bytes within one plane of kPixelBytes per pixel (4: a float32 channel plane; 16: a block of 8 packed bfloat16
// channels): the voffset of a buffer load whose soffset selects the plane.
template <unsigned kPixelBytes>
__device__ __forceinline__ void taps(float px, float py, int H, int W, unsigned* o, float* w) {
  const float ix = ((px + 1.0f) / 2.0f) * (float)(W - 1);
  const float iy = ((py + 1.0f) / 2.0f) * (float)(H - 1);
  // both corners of an axis outside (or NaN): nothing is sampled
  const bool ok = ix > -1.0f && ix < (float)W && iy > -1.0f && iy < (float)H;
  const float fx = ok ? floorf(ix) : 0.0f, fy = ok ? floorf(iy) : 0.0f;
  const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
  const float nw = (fx + 1.0f - ix) * (fy + 1.0f - iy);
  const float ne = (ix - fx) * (fy + 1.0f - iy);
  const float sw = (fx + 1.0f - ix) * (iy - fy);
  const float se = (ix - fx) * (iy - fy);
  const bool bx0 = ok && x0 >= 0, bx1 = ok && x1 <= W - 1, by0 = ok && y0 >= 0, by1 = ok && y1 <= H - 1;
  const int cx0 = bx0 ? x0 : 0, cx1 = bx1 ? x1 : W - 1, cy0 = by0 ? y0 : 0, cy1 = by1 ? y1 : H - 1;
  o[0] = kPixelBytes * (unsigned)(cy0 * W + cx0);
  o[1] = kPixelBytes * (unsigned)(cy0 * W + cx1);
  o[2] = kPixelBytes * (unsigned)(cy1 * W + cx0);
  o[3] = kPixelBytes * (unsigned)(cy1 * W + cx1);
  w[0] = (bx0 && by0) ? nw : 0.0f;
  w[1] = (bx1 && by0) ? ne : 0.0f;
  w[2] = (bx0 && by1) ? sw : 0.0f;
  w[3] = (bx1 && by1) ? se : 0.0f;
}

// The taps of kN consecutive samples of the lane's pixel from bin d0 on (bins past D - 1 repeat the last one; they are
// never written)
template <unsigned kPixelBytes, int kN>
__device__ __forceinline__ void chunk_taps(const Cam& cm, float u, float v, const float* fd, long long sd, int d0, int D,
                                           float wi1, float hi1, int H, int W, unsigned (*o)[4], float (*wt)[4]) {
#pragma unroll
  for (int j = 0; j < kN; ++j) {
    const int d = min(d0 + j, D - 1);
    float px, py;
    grid_point(cm, u, v, fd[(long long)d * sd], wi1, hi1, &px, &py);
    taps<kPixelBytes>(px, py, H, W, o[j], wt[j]);
  }
}

// One channel of one sample: the warped value of prev from its four corner values (grid_sample's order nw, ne, sw, se)
__device__ __forceinline__ float warp_value(float t0, float t1, float t2, float t3, const float* w) {
  float s = t0 * w[0];
  s = s + t1 * w[1];
  s = s + t2 * w[2];
  s = s + t3 * w[3];
  return s;
}

// ... and what it adds to its group's sum
__device__ __forceinline__ float group_add(float grp, float cur, float s) {
  const float a = fabsf(cur - s);
  return grp + a;
}

// Pass 1's end for kN consecutive bins from d0 on, in ascending order: raw = -(cost + bias [bit j of zero]) is written
// (live lanes) and enters the lane's online max / sum
template <int kN>
__device__ __forceinline__ void chunk_emit(const float* cost, unsigned zero, float bias, int d0, int D, bool live,
                                           float* out_px, int HW, float* run_max, float* run_sum) {
#pragma unroll
  for (int j = 0; j < kN; ++j) {
    if (d0 + j < D) {
      const float r = -(((zero >> j) & 1u) ? cost[j] + bias : cost[j]);
      if (live) out_px[(size_t)(d0 + j) * HW] = r;
      const float m = fmaxf(*run_max, r);
      *run_sum = *run_sum * expf(*run_max - m) + expf(r - m);
      *run_max = m;
    }
  }
}

// The 4 waves' max / sum combined through LDS, then pass 2: the lane rescales its own (L2-hot) writes in place.  Every
// thread of the workgroup calls it (it holds a barrier).
__device__ __forceinline__ void softmax_finish(float (*s_max)[64], float (*s_sum)[64], int q, int lane, float run_max,
                                               float run_sum, bool live, int n_chunks, int D, float* out_px, int HW) {
  s_max[q][lane] = run_max;
  s_sum[q][lane] = run_sum;
  __syncthreads();
  float M = s_max[0][lane];
  for (int k = 1; k < kWaves; ++k) M = fmaxf(M, s_max[k][lane]);
  float S = 0.0f;
  for (int k = 0; k < kWaves; ++k) S += s_sum[k][lane] * expf(s_max[k][lane] - M);
  const float inv = 1.0f / S;
  if (!live) return;
  for (int ch = q; ch < n_chunks; ch += kWaves) {
    const int d0 = ch * kJ;
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
      if (d0 + j < D) {
        float* p = out_px + (size_t)(d0 + j) * HW;
        *p = expf(*p - M) * inv;
      }
    }
  }
}

}  // namespace stereo
}  // namespace ocrf
