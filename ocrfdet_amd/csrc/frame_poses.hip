// Frame poses of the 4D detectors: the pose algebra of BEVDet4D.prepare_inputs (mmdet3d/models/detectors/bevdet.py:
// 435-456) and the per-frame get_mlp_input of extract_img_feat (ocrfdet.py:229-231) as ONE launch per forward.  The
// reference runs two torch.inverse calls on float64 4 x 4 stacks (each synchronises the host) and one get_mlp_input per
// frame: a few dozen small launches.  Here a thread owns one (sample b, frame f, camera n) and writes
//
//   sensor2keyegos[b][f][n] = inv(ego2globals[b][0][0]) . ego2globals[b][f][n] . sensor2egos[b][f][n]
//   curr2adjsensor[b][f][n] = inv(ego2globals[b][f+1][n] . sensor2egos[b][f+1][n]) . ego2globals[b][f][n] .
//                             sensor2egos[b][f][n]                                              for f < T
//   mlp_input[f][b][n][0..26]: the 27 scalars of get_mlp_input(rots[:, 0], trans[:, 0], intrins[:, f], post_rots[:, f],
//                              post_trans[:, f], bda)
//
// in float64, each result rounded once to float32.  The inverses are closed forms of AFFINE maps (last row (0, 0, 0, 1),
// as poses have): the 3 x 3 block from its adjugate and determinant, the translation -inv(R) t.  Nothing assumes an
// orthonormal rotation; a singular block gives inf / nan as it does in torch.  The products are full 4 x 4 products
// (pose_math.h).
// mlp_input is copied, so it is bit-equal to the torch formulation.  No workspace, no atomics, no host reads; reruns
// give the same bits.  It is a launch-count optimisation: a few hundred threads of a few hundred flops each.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "ocrf_hip.h"
#include "pose_math.h"

namespace {

using namespace pose;

constexpr int kThreads = 64;
constexpr long long kMaxMatrices = 1 << 24;        // 16 floats each: every operand far below 2 GiB, indices fit int

__global__ void __launch_bounds__(kThreads) frame_poses_kernel(
    int B, int F, int N, int T, const float* __restrict__ sensor2egos, const float* __restrict__ ego2globals,
    const float* __restrict__ rots, const float* __restrict__ trans, const float* __restrict__ intrins,
    const float* __restrict__ post_rots, const float* __restrict__ post_trans, const float* __restrict__ bda,
    float* __restrict__ sensor2keyegos, float* __restrict__ curr2adjsensor, float* __restrict__ mlp_input) {
  const int total = B * F * N;
  const int idx = blockIdx.x * kThreads + (int)threadIdx.x;
  if (idx >= total) return;
  const int b = idx / (F * N), rest = idx - b * (F * N);
  const int f = rest / N, n = rest - f * N;

  const Mat4 sensor2global = mul4(load4(ego2globals + (size_t)idx * 16), load4(sensor2egos + (size_t)idx * 16));
  const Mat4 global2keyego = affine_inverse(load4(ego2globals + (size_t)b * F * N * 16));
  store4(sensor2keyegos + (size_t)idx * 16, mul4(global2keyego, sensor2global));

  if (f < T) {                                       // T < F: frame f + 1 exists
    const int adj = idx + N;
    const Mat4 adj2global = mul4(load4(ego2globals + (size_t)adj * 16), load4(sensor2egos + (size_t)adj * 16));
    store4(curr2adjsensor + ((size_t)(b * T + f) * N + n) * 16, mul4(affine_inverse(adj2global), sensor2global));
  }

  // get_mlp_input: intrinsics and image augmentation of THIS frame, the key frame's sensor2ego, the BEV augmentation
  const float* K = intrins + (size_t)idx * 9;
  const float* pr = post_rots + (size_t)idx * 9;
  const float* pt = post_trans + (size_t)idx * 3;
  const float* a = bda + (size_t)b * 9;
  const int key = b * F * N + n;
  const float* r = rots + (size_t)key * 9;
  const float* t = trans + (size_t)key * 3;
  float* o = mlp_input + ((size_t)(f * B + b) * N + n) * 27;
  o[0] = K[0], o[1] = K[4], o[2] = K[2], o[3] = K[5];
  o[4] = pr[0], o[5] = pr[1], o[6] = pt[0], o[7] = pr[3], o[8] = pr[4], o[9] = pt[1];
  o[10] = a[0], o[11] = a[1], o[12] = a[3], o[13] = a[4], o[14] = a[8];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    o[15 + i * 4 + 0] = r[i * 3 + 0];
    o[15 + i * 4 + 1] = r[i * 3 + 1];
    o[15 + i * 4 + 2] = r[i * 3 + 2];
    o[15 + i * 4 + 3] = t[i];
  }
}

}  // namespace

extern "C" int ocrf_frame_poses(int B, int F, int N, int T, const float* sensor2egos, const float* ego2globals,
                                const float* rots, const float* trans, const float* intrins, const float* post_rots,
                                const float* post_trans, const float* bda, float* sensor2keyegos,
                                float* curr2adjsensor, float* mlp_input, ocrf_stream_t stream) {
  if (B <= 0 || F <= 0 || N <= 0 || T < 0 || T >= F) return (int)hipErrorInvalidValue;
  const long long total = (long long)B * F * N;
  if ((long long)B * F >= kMaxMatrices || total >= kMaxMatrices) return (int)hipErrorInvalidValue;
  if (!sensor2egos || !ego2globals || !rots || !trans || !intrins || !post_rots || !post_trans || !bda ||
      !sensor2keyegos || !mlp_input || (T > 0 && !curr2adjsensor)) {
    return (int)hipErrorInvalidValue;
  }
  const unsigned grid = (unsigned)((total + kThreads - 1) / kThreads);
  ocrf::launch(OCRF_K_FRAME_POSES, frame_poses_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, B, F, N, T,
               sensor2egos, ego2globals, rots, trans, intrins, post_rots, post_trans, bda, sensor2keyegos,
               curr2adjsensor, mlp_input);
  return (int)hipGetLastError();
}
