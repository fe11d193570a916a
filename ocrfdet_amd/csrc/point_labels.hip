// Point labels of the input pipeline: PrepareImageInputs.point_label_transform (mmdet3d/datasets/pipelines/loading.py:
// 858-891) for all B * N cameras of a batch in TWO launches.  Per camera the reference scales, shifts, mirrors and
// rotates the projected lidar points (u, v, depth, label) in float64, truncates the coordinates with astype(int16) and
// scatters depth and (label >= 0) into two (H, W) maps with numpy's indexed assignment, where the LAST point written
// to a pixel wins.
//
//   mark     one thread per (camera, point): the reference's float64 operations in the reference's order, each product
//            and sum rounded on its own (the library is built with -ffp-contract=off; cos and sin come from the host), then
//            atomicMax(winner[camera][v][u], point index + 1) on an int32 plane
//   resolve  one thread per pixel: depth and semantic of the winning point, or 0; the pixel of the plane is put back
//            to 0, so the plane is all zero again when the launch ends
//
// An integer maximum does not depend on the order the threads arrive in: the output is deterministic, and no float atomic
// is needed.  The plane belongs to the caller: all zero before the call (and therefore after it), used by one stream at
// a time.  Precondition: |coordinate| < 32768, where astype(int16) is a plain truncation toward zero; a point beyond that
// (or a NaN) is dropped here, while numpy wraps it around.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "ocrf_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRow = OCRF_POINT_LABELS_ROW;        // doubles per camera row

// grid (point tiles, cameras)
__global__ void __launch_bounds__(kThreads) point_labels_mark_kernel(
    int P, int H, int W, const double* __restrict__ points, const int* __restrict__ counts,
    const double* __restrict__ cams, int* __restrict__ winner) {
  const int cam = blockIdx.y;
  const int p = blockIdx.x * kThreads + (int)threadIdx.x;
  int count = counts[cam];
  count = count < P ? count : P;
  if (p >= count) return;
  const double* c = cams + (size_t)cam * kRow;
  const double resize = c[0], crop_x = c[1], crop_y = c[2], flip = c[3], cosv = c[4], sinv = c[5];
  const double* pt = points + ((size_t)cam * P + p) * 4;
  double x = pt[0] * resize;
  double y = pt[1] * resize;
  x -= crop_x;
  y -= crop_y;
  if (flip != 0.0) x = (double)W - x;              // resize_dims[1] - x with resize_dims = input_size = (H, W)
  const double half_w = (double)W / 2.0, half_h = (double)H / 2.0;
  x -= half_w;
  y -= half_h;
  // [[cos, sin], [-sin, cos]] . (x, y): two products and one sum per row, each rounded
  const double xc = cosv * x, ys = sinv * y, xs = (-sinv) * x, yc = cosv * y;
  double u = xc + ys;
  double v = xs + yc;
  u += half_w;
  v += half_h;
  if (!(fabs(u) < 32768.0) || !(fabs(v) < 32768.0)) return;
  const int iu = (int)u, iv = (int)v;              // toward zero: a value in (-1, 0) lands on pixel 0
  if (iu < 0 || iu >= W || iv < 0 || iv >= H) return;
  atomicMax(winner + ((size_t)cam * H + iv) * W + iu, p + 1);
}

// grid (pixel tiles, cameras)
__global__ void __launch_bounds__(kThreads) point_labels_resolve_kernel(
    int P, int H, int W, const double* __restrict__ points, int* __restrict__ winner, float* __restrict__ depth,
    float* __restrict__ semantic) {
  const int cam = blockIdx.y;
  const int px = blockIdx.x * kThreads + (int)threadIdx.x;
  if (px >= H * W) return;
  const size_t o = (size_t)cam * H * W + px;
  const int w = winner[o];
  float d = 0.f, s = 0.f;
  if (w > 0 && w <= P) {
    const double* pt = points + ((size_t)cam * P + (w - 1)) * 4;
    d = (float)pt[2];
    s = pt[3] >= 0.0 ? 1.f : 0.f;
  }
  if (w != 0) winner[o] = 0;
  depth[o] = d;
  semantic[o] = s;
}

}  // namespace

extern "C" int ocrf_point_labels(int cameras, int P, int H, int W, const double* points, const int* counts,
                                 const double* cams, int* winner, float* gt_depth, float* gt_semantic,
                                 ocrf_stream_t stream) {
  if (cameras <= 0 || cameras > 65535 || P < 0 || H <= 0 || W <= 0) return (int)hipErrorInvalidValue;
  if (H > OCRF_IMAGE_PREP_MAX_OUTPUT || W > OCRF_IMAGE_PREP_MAX_OUTPUT) return (int)hipErrorInvalidValue;
  if (!counts || !cams || !winner || !gt_depth || !gt_semantic || (P > 0 && !points)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  if (P > 0) {
    ocrf::launch(OCRF_K_POINT_LABELS_MARK, point_labels_mark_kernel, dim3((unsigned)((P + kThreads - 1) / kThreads), cameras),
                 dim3(kThreads), 0, s, P, H, W, points, counts, cams, winner);
  }
  ocrf::launch(OCRF_K_POINT_LABELS_RESOLVE, point_labels_resolve_kernel,
               dim3((unsigned)((H * W + kThreads - 1) / kThreads), cameras), dim3(kThreads), 0, s, P, H, W, points, winner,
               gt_depth, gt_semantic);
  return (int)hipGetLastError();
}
