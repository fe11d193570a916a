// The index rules of the temporal BEV alignment (bev_align.hip), shared by its forward, its backward and the host-only
// box query: where an output pixel samples its source plane, and which output pixels can read a given source pixel.
//
// Sampling rule.  t = rows 0 and 1 of the (3, 3) transform, row-major: t[0..2], t[3..5].  Output pixel (row i, column j)
// samples the source at
//   sx = fmaf(t00, j, fmaf(t01, i, t02)),   sy = fmaf(t10, j, fmaf(t11, i, t12))
// with x0 = floorf(sx), lx = sx - x0 (and y alike): the taps are (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)
// with weights (1 - lx)(1 - ly), lx (1 - ly), (1 - lx) ly, lx ly, and a tap outside [0, W) x [0, H) reads 0.  The
// library is built with -ffp-contract=off, so the two fmaf per axis are exactly these and the same in every caller.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>

namespace bev_align {

struct Sample {
  float x0, y0;                                    // floorf of the coordinates: kept as floats, they may be huge or NaN
  float lx, ly;
};

__host__ __device__ inline Sample sample_at(const float* t, int i, int j) {
  const float fi = (float)i, fj = (float)j;
  const float sx = fmaf(t[0], fj, fmaf(t[1], fi, t[2]));
  const float sy = fmaf(t[3], fj, fmaf(t[4], fi, t[5]));
  Sample s;
  s.x0 = floorf(sx);
  s.y0 = floorf(sy);
  s.lx = sx - s.x0;
  s.ly = sy - s.y0;
  return s;
}

// weight with which a sample whose floor is `f0` and fraction `l` reads index q of its axis (0: it does not)
__host__ __device__ inline float axis_weight(float f0, float l, float q) {
  const float a = f0 == q ? 1.0f - l : 0.0f;
  const float b = f0 + 1.0f == q ? l : 0.0f;
  return a + b;
}

// floor of a coordinate as an int in [-1, n - 1] (-1: both taps of the axis lie outside or the value is NaN; n - 1 also
// stands for everything beyond), formed from a clamped float so that no out-of-range conversion happens
__host__ __device__ inline int clamped_floor(float f0, int n) {
  const float lo = f0 >= -1.0f ? f0 : -1.0f;       // NaN -> -1
  const float top = (float)(n - 1);
  return (int)(lo <= top ? lo : top);
}

struct Box {
  int x0, x1, y0, y1;                              // inclusive; empty: (0, -1, 0, -1)
};

// integers j with lo <= j <= hi inside [0, n - 1]; a NaN bound stands for the plane's own end (a comparison with NaN is
// false), and the clamping is done on the doubles so that only values in [-1, n] are converted to int
__host__ __device__ inline void clamp_axis(double lo, double hi, int n, int* a, int* b) {
  double l = lo >= 0.0 ? lo : 0.0;
  l = l <= (double)n ? l : (double)n;
  double u = hi <= (double)(n - 1) ? hi : (double)(n - 1);
  u = u >= -1.0 ? u : -1.0;
  *a = (int)ceil(l);
  *b = (int)floor(u);
}

// The output pixels that may read source pixel (qx, qy) of an h x w plane: a box that holds every (i, j) whose
// sample_at() has x0 in {qx - 1, qx} and y0 in {qy - 1, qy}.
//
// The map is affine: (sx, sy) = A (j, i) + (t02, t12).  A reader has its exact sample inside the square q + [-r, r]^2,
// r = 1 + the float32 error of the two fmaf (at most 2 * 2^-24 of |t00| (w-1) + |t01| (h-1) + |t02| per axis; twice that
// is taken).  The image of a rectangle with centre a and half widths (rx, ry) under inv(A) has centre inv(A) a and half
// widths (rx |t11| + ry |t01|) / |det| in j and (ry |t00| + rx |t10|) / |det| in i.  All of it in double: the products
// of two floats are exact there and det has one rounding, so a nearly singular A is seen as what it is; the centre's
// own rounding (2^-45 of its terms) and one pixel are added to the half widths.  det = 0, a non-finite entry, or a box
// larger than the plane give the plane itself, or nothing where the box misses it.  Never anything outside the plane.
__host__ __device__ inline Box source_box(const float* t, int h, int w, int qx, int qy) {
  Box box;
  box.x0 = 0, box.x1 = w - 1, box.y0 = 0, box.y1 = h - 1;
  const double t00 = t[0], t01 = t[1], t02 = t[2], t10 = t[3], t11 = t[4], t12 = t[5];
  const double det = t00 * t11 - t01 * t10;
  if (fabs(det) > 0.0) {                           // false for NaN too
    const double inv = 1.0 / det, ainv = fabs(inv);
    const double e = 4.0 / 16777216.0, k = 1.0 / 35184372088832.0;     // 4 * 2^-24, 2^-45
    const double rx = 1.0 + e * (fabs(t00) * (w - 1) + fabs(t01) * (h - 1) + fabs(t02) + 1.0);
    const double ry = 1.0 + e * (fabs(t10) * (w - 1) + fabs(t11) * (h - 1) + fabs(t12) + 1.0);
    const double ax = (double)qx - t02, ay = (double)qy - t12;
    const double uc = (ax * t11 - ay * t01) * inv, vc = (ay * t00 - ax * t10) * inv;
    const double ru = ((rx * fabs(t11) + ry * fabs(t01)) + k * (fabs(ax * t11) + fabs(ay * t01))) * ainv + 1.0;
    const double rv = ((ry * fabs(t00) + rx * fabs(t10)) + k * (fabs(ay * t00) + fabs(ax * t10))) * ainv + 1.0;
    clamp_axis(uc - ru, uc + ru, w, &box.x0, &box.x1);
    clamp_axis(vc - rv, vc + rv, h, &box.y0, &box.y1);
  }
  if (box.x0 > box.x1 || box.y0 > box.y1) box.x0 = 0, box.x1 = -1, box.y0 = 0, box.y1 = -1;
  return box;
}

}  // namespace bev_align
