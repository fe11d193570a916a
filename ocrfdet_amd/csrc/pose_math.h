// Float64 algebra of affine 4 x 4 poses on the device, shared by frame_poses.hip and bev_stream_align.hip: loads widen
// float32 operands (exact), products are full 4 x 4 products, the inverse is the closed form of an AFFINE map (last row
// (0, 0, 0, 1), as poses have): the 3 x 3 block from its adjugate and determinant, the translation -inv(R) t.  Nothing
// assumes an orthonormal rotation; a singular block gives inf / nan as it does in torch.
#pragma once
#include <hip/hip_runtime.h>

namespace pose {

struct Mat4 {
  double m[4][4];
};

__device__ __forceinline__ Mat4 load4(const float* __restrict__ p) {
  Mat4 a;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) a.m[i][j] = (double)p[i * 4 + j];
  }
  return a;
}

__device__ __forceinline__ Mat4 mul4(const Mat4& a, const Mat4& b) {
  Mat4 c;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j] + a.m[i][3] * b.m[3][j];
    }
  }
  return c;
}

// inverse of an affine map [R t; 0 0 0 1]: cofactor (i, j) of R is R[i+1][j+1] R[i+2][j+2] - R[i+1][j+2] R[i+2][j+1]
// with the indices modulo 3 (temporal._inverse3), inv(R) = adjugate / det, translation -inv(R) t
__device__ __forceinline__ Mat4 affine_inverse(const Mat4& a) {
  double cof[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      cof[i][j] = a.m[i1][j1] * a.m[i2][j2] - a.m[i1][j2] * a.m[i2][j1];
    }
  }
  const double det = a.m[0][0] * cof[0][0] + a.m[0][1] * cof[0][1] + a.m[0][2] * cof[0][2];
  Mat4 r;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) r.m[i][j] = cof[j][i] / det;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    r.m[i][3] = -(r.m[i][0] * a.m[0][3] + r.m[i][1] * a.m[1][3] + r.m[i][2] * a.m[2][3]);
    r.m[3][i] = 0.0;
  }
  r.m[3][3] = 1.0;
  return r;
}

__device__ __forceinline__ void store4(float* __restrict__ p, const Mat4& a) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) p[i * 4 + j] = (float)a.m[i][j];
  }
}

}  // namespace pose
