// Stereo cost volume of the depth network (view_transformer.py DepthNet.gen_grid :538-566 and
// calculate_cost_volumn :568-596) as one forward-only kernel: no (BN, 4, D*H, W) warped tensor per channel group, no
// per-group launches, no host synchronisation, no atomics.  The reference computes it under torch.no_grad(), so there
// is no backward.
//
// Semantics, including the reference's quirks:
//  * Projection order, per camera and frustum cell (u, v, d):
//      1. p = inv(post_rot) . ((u, v, d) - post_trans)
//      2. p = (p.x * p.z, p.y * p.z, p.z)
//      3. p = (R_k2s . inv(K)) . p + t_k2s
//      4. p.z < 1e-3 here, BEFORE the intrinsics, marks the cell invalid: its normalised coordinates become -2
//      5. p = K . p, then (x, y) = (p.x / p.z, p.y / p.z)
//      6. (x, y) = post_rot[:2, :2] . (x, y) + post_trans[:2]
//    The 3x3 inverses are closed-form here (the reference's torch.inverse differs in the last bits; tests treat cells
//    whose outcome hinges on those bits as ambiguous).
//  * Normalisation and sampling use different sizes: px = x / (wi - 1) * 2 - 1 with the IMAGE size wi = 4 W, hi = 4 H,
//    then grid_sample (align_corners=True) un-normalises with the FEATURE size: ix = (px + 1) / 2 * (W - 1).  The sample
//    position is therefore x (W - 1) / (wi - 1), not x / 4.
//  * Bilinear sampling with zero padding: a corner outside the feature map contributes 0; the four corner terms are
//    added in grid_sample's order (nw, ne, sw, se).
//  * cost = sum over c < 4 floor(C / 4) of |curr_c - warp(prev)_c|, summed per group of 4 channels and then over the
//    groups; channels past the last whole group are ignored.
//  * The bias test reads one channel only: with bias != 0 a cell gets + bias iff the warped value of channel
//    4 (floor(C / 4) - 1) — the first channel of the LAST group, whose warp leaks out of the reference's loop — is
//    exactly 0.0.  The stereo features follow a ReLU, so this also fires for valid samples whose corners are all zero.
//  * raw = -(cost + bias [warp == 0]); the product output is softmax over d of raw.  mode 1 writes raw (tests).
//
// Layout: one lane per output pixel.  A workgroup is 4 waves over the same 64 consecutive w of one (camera, h) row;
// wave q owns the depth chunks q, q + 4, q + 8, ... of kJ bins.  Per chunk a lane keeps the clamped corner offsets and
// the masked bilinear weights of its kJ samples in registers and walks the channels: one coalesced load of curr per
// channel, 4 gathers of prev per sample.  Neighbouring lanes sample neighbouring points of prev along an epipolar curve,
// so a wave's gathers fall on a few cache lines of one channel plane and the reuse is served by L1 / L2.  Pass 1 writes
// raw and keeps the lane's online max / sum over its bins; the 4 waves combine them through LDS; pass 2 rescales the
// lane's own (L2-hot) writes in place.  Stores are coalesced across lanes: the output is NCHW (BN, D, H, W).
#include <hip/hip_runtime.h>

#include <cmath>

#include "launch.h"
#include "ocrf_hip.h"

namespace {

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
// bytes within one channel plane: the voffset of a buffer load whose soffset selects the plane.
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
  o[0] = 4u * (unsigned)(cy0 * W + cx0);
  o[1] = 4u * (unsigned)(cy0 * W + cx1);
  o[2] = 4u * (unsigned)(cy1 * W + cx0);
  o[3] = 4u * (unsigned)(cy1 * W + cx1);
  w[0] = (bx0 && by0) ? nw : 0.0f;
  w[1] = (bx1 && by0) ? ne : 0.0f;
  w[2] = (bx0 && by1) ? sw : 0.0f;
  w[3] = (bx1 && by1) ? se : 0.0f;
}

__device__ __forceinline__ float ld(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)voff, (int)soff, 0));
}

__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3))) stereo_cost_volume_kernel(
    int C, int H, int W, int D, const float* __restrict__ prev, const float* __restrict__ curr,
    const float* __restrict__ fu, long long su, const float* __restrict__ fv, long long sv,
    const float* __restrict__ fd, long long sd, const float* __restrict__ k2s, const float* __restrict__ intrins,
    const float* __restrict__ post_rots, const float* __restrict__ post_trans, float bias, int raw_only,
    int blocks_per_row, float* __restrict__ out) {
  __shared__ float s_max[kWaves][64];
  __shared__ float s_sum[kWaves][64];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int row = blockIdx.x / blocks_per_row;             // cam * H + h
  const int cam = row / H, h = row - cam * H;
  const int w = (blockIdx.x - row * blocks_per_row) * 64 + lane;
  const bool live = w < W;
  const int wc = live ? w : W - 1;
  const int HW = H * W;
  const int G = C >> 2, cb = 4 * (G - 1);
  // one camera's prev is at most 2^32 - 1 bytes (host guard): its size and plane offsets in unsigned 32-bit bytes
  const unsigned plane_bytes = (unsigned)HW * (unsigned)sizeof(float);

  Cam cm;
  load_cam(cam, k2s, intrins, post_rots, post_trans, &cm);
  const float wi1 = (float)(4 * W) - 1.0f, hi1 = (float)(4 * H) - 1.0f;
  const float u = fu[(long long)wc * su], v = fv[(long long)h * sv];
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(prev + (size_t)cam * C * HW), 0, (int)((unsigned)C * plane_bytes), 0x00020000);
  const float* curr_px = curr + (size_t)cam * C * HW + (size_t)h * W + wc;
  float* out_px = out + (size_t)cam * D * HW + (size_t)h * W + wc;

  float run_max = -INFINITY, run_sum = 0.0f;
  const int n_chunks = (D + kJ - 1) / kJ;
  for (int ch = q; ch < n_chunks; ch += kWaves) {
    const int d0 = ch * kJ;
    unsigned o[kJ][4];
    float wt[kJ][4];
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
      const int d = min(d0 + j, D - 1);
      float px, py;
      grid_point(cm, u, v, fd[(long long)d * sd], wi1, hi1, &px, &py);
      taps(px, py, H, W, o[j], wt[j]);
    }
    float cost[kJ], grp[kJ];
    unsigned zero = 0u;
#pragma unroll
    for (int j = 0; j < kJ; ++j) cost[j] = 0.0f;
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
#pragma unroll 1
      for (int cc = 0; cc < 4; ++cc) {
        const int c = 4 * g + cc;
        const float cur = curr_px[(size_t)c * HW];
        const unsigned plane = (unsigned)c * plane_bytes;
        float warp[kJ];
#pragma unroll
        for (int j = 0; j < kJ; ++j) {
          if (cc == 0) grp[j] = 0.0f;
          float s = ld(rs, o[j][0], plane) * wt[j][0];
          s = s + ld(rs, o[j][1], plane) * wt[j][1];
          s = s + ld(rs, o[j][2], plane) * wt[j][2];
          s = s + ld(rs, o[j][3], plane) * wt[j][3];
          warp[j] = s;
          const float a = fabsf(cur - s);
          grp[j] = grp[j] + a;
        }
        if (c == cb) {
#pragma unroll
          for (int j = 0; j < kJ; ++j) zero |= (warp[j] == 0.0f ? 1u : 0u) << j;
        }
      }
#pragma unroll
      for (int j = 0; j < kJ; ++j) cost[j] += grp[j];
    }
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
      if (d0 + j < D) {
        const float r = -(((zero >> j) & 1u) ? cost[j] + bias : cost[j]);
        if (live) out_px[(size_t)(d0 + j) * HW] = r;
        const float m = fmaxf(run_max, r);
        run_sum = run_sum * expf(run_max - m) + expf(r - m);
        run_max = m;
      }
    }
  }
  if (raw_only) return;                 // uniform over the workgroup: no barrier is skipped by some waves only
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

}  // namespace

extern "C" {

int ocrf_stereo_cost_volume(int BN, int C, int H, int W, int D, const float* prev, const float* curr,
                            const float* frustum_u, long long stride_u, const float* frustum_v, long long stride_v,
                            const float* frustum_d, long long stride_d, const float* k2s_sensor, const float* intrins,
                            const float* post_rots, const float* post_trans, float bias, int mode, float* out,
                            ocrf_stream_t stream) {
  if (BN <= 0 || C < 4 || H < 2 || W < 2 || D <= 0 || (mode != 0 && mode != 1)) return (int)hipErrorInvalidValue;
  if (!prev || !curr || !frustum_u || !frustum_v || !frustum_d || !k2s_sensor || !intrins || !post_rots ||
      !post_trans || !out)
    return (int)hipErrorInvalidValue;
  // one camera's prev is addressed in unsigned 32-bit bytes (buffer size and plane offsets); out's planes and the
  // per-row block counts must fit int
  const long long HW = (long long)H * W;
  if ((long long)C * HW * (long long)sizeof(float) > 0xFFFFFFFFLL || (long long)D * HW >= (1LL << 31))
    return (int)hipErrorInvalidValue;
  const int per_row = (W + 63) / 64;
  const long long blocks = (long long)BN * H * per_row;
  if (blocks >= (1LL << 31)) return (int)hipErrorInvalidValue;
  ocrf::launch(OCRF_K_STEREO_COST_VOLUME, stereo_cost_volume_kernel, dim3((unsigned)blocks), dim3(kThreads), 0,
               (hipStream_t)stream, C, H, W, D, prev, curr, frustum_u, stride_u, frustum_v, stride_v, frustum_d,
               stride_d, k2s_sensor, intrins, post_rots, post_trans, bias, mode, per_row, out);
  return (int)hipGetLastError();
}

}  // extern "C"
