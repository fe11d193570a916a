// The stereo cost volume of stereo.hip for bfloat16 features (an image encoder under bf16 autocast), opt-in.  Semantics
// are exactly those listed at the top of stereo.hip; the arithmetic is that kernel's (stereo_common.h), float32 on the
// widened values in the same order, so the result is, bit for bit, what ocrf_stereo_cost_volume gives on the features
// cast to float32.  What differs is where the features are read from.
//
// Layout: both features are first packed (ocrf_stereo_pack_bf16, one launch per tensor) from planar NCHW into blocks of
// 8 channels per pixel, (BN, NB, H, W, 8) with G = C / 4 whole groups and NB = (G + 1) / 2: the 8 channels of two of the
// reference's groups at one pixel are 16 contiguous bytes.  Channels past the last whole group are dropped, the upper
// half of the last block is zero when G is odd (and never added).  The cost volume keeps the float32 kernel's
// decomposition (one lane per output pixel, 4 waves over the same 64 w, wave q owns depth chunks q, q + 4, ... of kJ
// bins, the waves' online softmax combined through 2 KB of LDS, pass 2 over the lane's own writes), which fixes the order
// of the softmax.  A chunk's bins are walked in sub-chunks of kSub, ascending, each with its own pass over the channels:
// per block of 8 channels a lane loads its 16 bytes of curr (coalesced) and, per sample, gathers the four corners of
// prev as four 16-byte buffer loads (voffset 16 (cy W + cx) from the clamped corners, the block's plane in soffset): one
// gather wave-instruction where the float32 kernel issues 8, and half the bytes.  No atomics, no scratch,
// deterministic, no host synchronisation.
#include <hip/hip_runtime.h>

#include <cmath>

#include "launch.h"
#include "ocrf_hip.h"
#include "stereo_common.h"

namespace {

using namespace ocrf::stereo;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 8;                              // channels per packed block
constexpr unsigned kPixelBytes = kBlock * 2;           // ... in bytes: one pixel of one block
constexpr int kPackThreads = 256;
#ifndef OCRF_STEREO_BF16_SUB
#define OCRF_STEREO_BF16_SUB 2                         // A/B builds only
#endif
// Samples of a chunk whose taps are held in registers at a time.  The float32 kernel holds all kJ = 8 and re-reads one
// float of curr per channel; here a block's 16 bytes of curr cost one load however few samples share it, and 16
// registers of corners per sample make a small sub-chunk the better trade: 2 samples take 88 VGPRs (5 waves per SIMD)
// and measured fastest, 8 take 157 (3 waves).  The chunk's bins are still visited in ascending order.
constexpr int kSub = OCRF_STEREO_BF16_SUB;
static_assert(kJ % kSub == 0, "a chunk is a whole number of sub-chunks");

// channel k of a block as float32: bf16 is the upper half of a float32, so widening is exact
__device__ __forceinline__ float widen(const u32x4& v, int k) {
  const unsigned d = v[k >> 1];
  return __uint_as_float((k & 1) ? (d & 0xFFFF0000u) : (d << 16));
}

__device__ __forceinline__ u32x4 ld16(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, (int)soff, 0));
}

// One group of 4 channels (the block's lower or upper half) of one sample: the group's sum as the float32 kernel forms
// it, channels ascending; *first is the warped value of the group's first channel (what the bias test reads)
template <int kHalf>
__device__ __forceinline__ float group_cost(const u32x4& cur, const u32x4& t0, const u32x4& t1, const u32x4& t2,
                                            const u32x4& t3, const float* w, float* first) {
  float grp = 0.0f;
#pragma unroll
  for (int k = 4 * kHalf; k < 4 * kHalf + 4; ++k) {
    const float s = warp_value(widen(t0, k), widen(t1, k), widen(t2, k), widen(t3, k), w);
    if (k == 4 * kHalf) *first = s;
    grp = group_add(grp, widen(cur, k), s);
  }
  return grp;
}

// One block of 8 channels for kSub samples.  kBoth: the block holds two whole groups (else only its lower
// half is added: the last block of an odd G).  last: the block holds channel 4 (G - 1), the bias test's.
template <bool kBoth>
__device__ __forceinline__ void block_cost(__amdgpu_buffer_rsrc_t rs, unsigned soff, const u32x4& cur,
                                           const unsigned (*o)[3], const float (*wt)[4], bool last, float* cost,
                                           unsigned* zero) {
#pragma unroll
  for (int j = 0; j < kSub; ++j) {
    // the clamped corners form a (possibly degenerate) rectangle: sw = nw + se - ne is not kept in a register
    const u32x4 t0 = ld16(rs, o[j][0], soff), t1 = ld16(rs, o[j][1], soff);
    const u32x4 t2 = ld16(rs, o[j][0] + o[j][2] - o[j][1], soff), t3 = ld16(rs, o[j][2], soff);
    float first;
    cost[j] += group_cost<0>(cur, t0, t1, t2, t3, wt[j], &first);
    if (kBoth) cost[j] += group_cost<1>(cur, t0, t1, t2, t3, wt[j], &first);
    if (last) *zero |= (first == 0.0f ? 1u : 0u) << j;
  }
}

__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3))) stereo_cost_volume_bf16_kernel(
    int G, int H, int W, int D, const unsigned short* __restrict__ prev, const unsigned short* __restrict__ curr,
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
  const int NB = (G + 1) >> 1, n_both = G >> 1;            // blocks; those with two whole groups come first
  // one camera's packed prev is at most 2^32 - 1 bytes (host guard): its size and block offsets in unsigned 32-bit bytes
  const unsigned block_bytes = (unsigned)HW * kPixelBytes;

  Cam cm;
  load_cam(cam, k2s, intrins, post_rots, post_trans, &cm);
  const float wi1 = (float)(4 * W) - 1.0f, hi1 = (float)(4 * H) - 1.0f;
  const float u = fu[(long long)wc * su], v = fv[(long long)h * sv];
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned short*>(prev + (size_t)cam * NB * HW * kBlock), 0, (int)((unsigned)NB * block_bytes),
      0x00020000);
  const u32x4* curr_px = reinterpret_cast<const u32x4*>(curr) + (size_t)cam * NB * HW + (size_t)h * W + wc;
  float* out_px = out + (size_t)cam * D * HW + (size_t)h * W + wc;

  float run_max = -INFINITY, run_sum = 0.0f;
  const int n_chunks = (D + kJ - 1) / kJ;
  for (int ch = q; ch < n_chunks; ch += kWaves) {
    // the chunk's bins in sub-chunks of kSub, ascending: the same bins in the same order as the float32 kernel's chunk
#pragma unroll 1
    for (int d0 = ch * kJ; d0 < min(ch * kJ + kJ, D); d0 += kSub) {
      unsigned o[kSub][3];              // nw, ne, se
      float wt[kSub][4];
      {
        unsigned o4[kSub][4];
        chunk_taps<kPixelBytes, kSub>(cm, u, v, fd, sd, d0, D, wi1, hi1, H, W, o4, wt);
#pragma unroll
        for (int j = 0; j < kSub; ++j) o[j][0] = o4[j][0], o[j][1] = o4[j][1], o[j][2] = o4[j][3];
      }
      float cost[kSub];
      unsigned zero = 0u;
#pragma unroll
      for (int j = 0; j < kSub; ++j) cost[j] = 0.0f;
#pragma unroll 1
      for (int b = 0; b < n_both; ++b)
        block_cost<true>(rs, (unsigned)b * block_bytes, curr_px[(size_t)b * HW], o, wt, b == NB - 1, cost, &zero);
      if (n_both < NB)
        block_cost<false>(rs, (unsigned)n_both * block_bytes, curr_px[(size_t)n_both * HW], o, wt, true, cost, &zero);
      chunk_emit<kSub>(cost, zero, bias, d0, D, live, out_px, HW, &run_max, &run_sum);
    }
  }
  if (raw_only) return;                 // uniform over the workgroup: no barrier is skipped by some waves only
  softmax_finish(s_max, s_sum, q, lane, run_max, run_sum, live, n_chunks, D, out_px, HW);
}

// Planar NCHW -> blocks of 8 channels per pixel: one lane per pixel of one block, eight coalesced 2-byte plane reads
// and one 16-byte store.  A block's valid channel count (8, or 4 in the last block of an odd G) is uniform.
__global__ void __launch_bounds__(kPackThreads) stereo_pack_bf16_kernel(int C, int HW, int NB, int chunks,
                                                                        const unsigned short* __restrict__ src,
                                                                        unsigned short* __restrict__ dst) {
  const int plane = blockIdx.x / chunks;                   // cam * NB + b
  const int cam = plane / NB, b = plane - cam * NB;
  const int p = (blockIdx.x - plane * chunks) * kPackThreads + threadIdx.x;
  if (p >= HW) return;
  const int n = min(kBlock, 4 * (C >> 2) - kBlock * b);    // 8 or 4
  const unsigned short* s = src + ((size_t)cam * C + (size_t)kBlock * b) * HW + p;
  unsigned v[kBlock];
#pragma unroll
  for (int k = 0; k < kBlock; ++k) v[k] = k < n ? (unsigned)s[(size_t)k * HW] : 0u;
  u32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = v[2 * i] | (v[2 * i + 1] << 16);
  reinterpret_cast<u32x4*>(dst)[(size_t)plane * HW + p] = r;
}

// The packed shape's limits: one camera's packed tensor is addressed in unsigned 32-bit bytes
bool packed_shape_ok(int BN, int C, int H, int W, int* NB) {
  if (BN <= 0 || C < 4 || H < 2 || W < 2) return false;
  *NB = ((C >> 2) + 1) >> 1;
  return (long long)*NB * H * W * (long long)kPixelBytes <= 0xFFFFFFFFLL;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" {

int ocrf_stereo_pack_bf16(int BN, int C, int H, int W, const unsigned short* src, unsigned short* dst,
                          ocrf_stream_t stream) {
  int NB = 0;
  if (!packed_shape_ok(BN, C, H, W, &NB) || !src || !dst || !aligned16(dst)) return (int)hipErrorInvalidValue;
  const long long HW = (long long)H * W;
  const long long chunks = (HW + kPackThreads - 1) / kPackThreads;
  const long long blocks = (long long)BN * NB * chunks;
  if (blocks >= (1LL << 31)) return (int)hipErrorInvalidValue;
  ocrf::launch(OCRF_K_STEREO_PACK_BF16, stereo_pack_bf16_kernel, dim3((unsigned)blocks), dim3(kPackThreads), 0,
               (hipStream_t)stream, C, (int)HW, NB, (int)chunks, src, dst);
  return (int)hipGetLastError();
}

int ocrf_stereo_cost_volume_bf16(int BN, int C, int H, int W, int D, const unsigned short* prev,
                                 const unsigned short* curr, const float* frustum_u, long long stride_u,
                                 const float* frustum_v, long long stride_v, const float* frustum_d, long long stride_d,
                                 const float* k2s_sensor, const float* intrins, const float* post_rots,
                                 const float* post_trans, float bias, int mode, float* out, ocrf_stream_t stream) {
  int NB = 0;
  if (!packed_shape_ok(BN, C, H, W, &NB) || D <= 0 || (mode != 0 && mode != 1)) return (int)hipErrorInvalidValue;
  if (!prev || !curr || !frustum_u || !frustum_v || !frustum_d || !k2s_sensor || !intrins || !post_rots ||
      !post_trans || !out)
    return (int)hipErrorInvalidValue;
  if (!aligned16(prev) || !aligned16(curr)) return (int)hipErrorInvalidValue;
  // out's planes and the per-row block counts must fit int
  if ((long long)D * H * W >= (1LL << 31)) return (int)hipErrorInvalidValue;
  const int per_row = (W + 63) / 64;
  const long long blocks = (long long)BN * H * per_row;
  if (blocks >= (1LL << 31)) return (int)hipErrorInvalidValue;
  ocrf::launch(OCRF_K_STEREO_COST_VOLUME_BF16, stereo_cost_volume_bf16_kernel, dim3((unsigned)blocks), dim3(kThreads),
               0, (hipStream_t)stream, C >> 2, H, W, D, prev, curr, frustum_u, stride_u, frustum_v, stride_v, frustum_d,
               stride_d, k2s_sensor, intrins, post_rots, post_trans, bias, mode, per_row, out);
  return (int)hipGetLastError();
}

}  // extern "C"
