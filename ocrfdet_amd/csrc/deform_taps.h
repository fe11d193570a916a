// The sampling rule of the deformable convolution (deform_conv.hip), shared by its im2col, its col2im and the host-only
// query ocrf_deform_taps: where a tap samples the map, whether it samples it at all, and the four corners it reads.
//
// base = ho * stride - pad + i * dil of the axis (an int, exact as a float), off the tap's offset.  The coordinate is
//   h = (float)base_h + off_h,   w = (float)base_w + off_w                      (one rounding each)
// and the sample is 0 unless h > -1 && w > -1 && h < H && w < W, tested in float so that a NaN fails.  Inside that range
// hl = floorf(h) lies in [-1, H - 1] and only then is it converted to int.  The corners (hl | hl + 1, wl | wl + 1) carry
// (1 - lh | lh) * (1 - lw | lw), lh = h - hl; a corner outside the map contributes 0.  For ANY float offset (NaN,
// infinities, 1e30) the weights are 0 where nothing is sampled and the four indices lie inside the map.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>

namespace deform {

struct Taps {
  int r0, r1, c0, c1;                              // rows and columns of the corners, clamped into the map
  float lh, lw;                                    // fractions; 0 when the range test fails
  float v00, v01, v10, v11;                        // 1 where the corner (row 0 | 1, column 0 | 1) is read, else 0
};

__host__ __device__ inline Taps taps_at(int base_h, int base_w, float off_h, float off_w, int H, int W) {
  const float h = (float)base_h + off_h, w = (float)base_w + off_w;
  const bool in = h > -1.0f && w > -1.0f && h < (float)H && w < (float)W;        // false for a NaN
  Taps t;
  t.r0 = t.r1 = t.c0 = t.c1 = 0;
  t.lh = t.lw = 0.0f;
  t.v00 = t.v01 = t.v10 = t.v11 = 0.0f;
  if (in) {
    const float fh = floorf(h), fw = floorf(w);    // in [-1, H - 1] and [-1, W - 1]
    const int hl = (int)fh, wl = (int)fw;
    t.lh = h - fh;
    t.lw = w - fw;
    const bool r0_in = hl >= 0, r1_in = hl + 1 <= H - 1, c0_in = wl >= 0, c1_in = wl + 1 <= W - 1;
    t.r0 = r0_in ? hl : 0;
    t.r1 = r1_in ? hl + 1 : H - 1;
    t.c0 = c0_in ? wl : 0;
    t.c1 = c1_in ? wl + 1 : W - 1;
    t.v00 = r0_in && c0_in ? 1.0f : 0.0f;
    t.v01 = r0_in && c1_in ? 1.0f : 0.0f;
    t.v10 = r1_in && c0_in ? 1.0f : 0.0f;
    t.v11 = r1_in && c1_in ? 1.0f : 0.0f;
  }
  return t;
}

// the corner weights (1 - lh | lh) * (1 - lw | lw), 0 for a corner that is not read
struct Weights {
  float w00, w01, w10, w11;
};

__host__ __device__ inline Weights weights_of(const Taps& t) {
  const float mh = 1.0f - t.lh, mw = 1.0f - t.lw;
  Weights q;
  q.w00 = t.v00 * (mh * mw);
  q.w01 = t.v01 * (mh * t.lw);
  q.w10 = t.v10 * (t.lh * mw);
  q.w11 = t.v11 * (t.lh * t.lw);
  return q;
}

}  // namespace deform
