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
#include "stereo_common.h"

namespace {

using namespace ocrf::stereo;

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
    chunk_taps<sizeof(float), kJ>(cm, u, v, fd, sd, d0, D, wi1, hi1, H, W, o, wt);
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
          const float s = warp_value(ld(rs, o[j][0], plane), ld(rs, o[j][1], plane), ld(rs, o[j][2], plane),
                                     ld(rs, o[j][3], plane), wt[j]);
          warp[j] = s;
          grp[j] = group_add(grp[j], cur, s);
        }
        if (c == cb) {
#pragma unroll
          for (int j = 0; j < kJ; ++j) zero |= (warp[j] == 0.0f ? 1u : 0u) << j;
        }
      }
#pragma unroll
      for (int j = 0; j < kJ; ++j) cost[j] += grp[j];
    }
    chunk_emit<kJ>(cost, zero, bias, d0, D, live, out_px, HW, &run_max, &run_sum);
  }
  if (raw_only) return;                 // uniform over the workgroup: no barrier is skipped by some waves only
  softmax_finish(s_max, s_sum, q, lane, run_max, run_sum, live, n_chunks, D, out_px, HW);
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
