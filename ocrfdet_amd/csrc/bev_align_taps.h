// The taps of the temporal BEV alignment, shared by the kernels that warp a plane (bev_align.hip, bev_stream_align.hip):
// the four tap addresses, their validity and the two fractions of one output pixel under bev_align_index.h's sampling
// rule, and the ONE float32 expression of the sampled value.  Both files evaluate these very functions, so a plane warped
// by either under the same transform has the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "bev_align_index.h"
#include "plane_walk.h"

namespace bev_align {

struct Taps {
  int r0, r1, c0, c1;                              // row offsets (row * w) and columns of the taps, clamped to the plane
  float lx, ly;
  bool v00, v01, v10, v11;                         // the tap lies inside the plane
};

__device__ __forceinline__ Taps taps_at(const float* t, int i, int j, int h, int w) {
  const Sample s = sample_at(t, i, j);
  const bool x0_in = s.x0 >= 0.0f && s.x0 <= (float)(w - 1), x1_in = s.x0 >= -1.0f && s.x0 <= (float)(w - 2);
  const bool y0_in = s.y0 >= 0.0f && s.y0 <= (float)(h - 1), y1_in = s.y0 >= -1.0f && s.y0 <= (float)(h - 2);
  const int x0 = clamped_floor(s.x0, w), y0 = clamped_floor(s.y0, h);
  Taps p;
  p.c0 = max(x0, 0);
  p.c1 = min(x0 + 1, w - 1);
  p.r0 = max(y0, 0) * w;
  p.r1 = min(y0 + 1, h - 1) * w;
  p.lx = s.lx;
  p.ly = s.ly;
  p.v00 = x0_in && y0_in;
  p.v01 = x1_in && y0_in;
  p.v10 = x0_in && y1_in;
  p.v11 = x1_in && y1_in;
  return p;
}

// T: float or bf16_t.  ONE float32 expression for both: the bf16 form widens its taps, the caller rounds the result once
template <typename T>
__device__ __forceinline__ float sample_value(const T* __restrict__ s, const Taps& p) {
  using plane::load_f32;
  const float v00 = p.v00 ? load_f32(s + (p.r0 + p.c0)) : 0.0f, v01 = p.v01 ? load_f32(s + (p.r0 + p.c1)) : 0.0f;
  const float v10 = p.v10 ? load_f32(s + (p.r1 + p.c0)) : 0.0f, v11 = p.v11 ? load_f32(s + (p.r1 + p.c1)) : 0.0f;
  const float mx = 1.0f - p.lx, my = 1.0f - p.ly;
  const float top = mx * v00 + p.lx * v01, bot = mx * v10 + p.lx * v11;
  return my * top + p.ly * bot;
}

}  // namespace bev_align
