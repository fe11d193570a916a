// Temporal BEV alignment: BEVDet4D.shift_feature (mmdet3d/models/detectors/bevdet.py:305-376), the warp of an adjacent
// frame's BEV feature into the key ego frame, written straight into its channels of the concatenation that feeds the BEV
// encoder (bevdet.py:529-536, ocrfdet.py:267-274).  The transform is affine in pixel coordinates (gen_grid's tf), so
// the forward is grid_sample(bilinear, zeros, align_corners=True) without the grid tensor and without the normalise /
// unnormalise round trip, and the backward is a gather: no atomics, no workspace, no host synchronisation; repeated runs
// are bit-identical.  The sampling rule and the box of candidates are in bev_align_index.h, the taps of an output
// pixel and the value sampled at them in bev_align_taps.h (bev_stream_align.hip warps with the same).
//
// Forward.  A unit is (batch, block of kChannels channels, chunk of the plane); a thread walks its groups of V output
// pixels as plane_walk.h describes, computes the four tap addresses, the validity of the taps and the two fractions of
// each pixel once, and then loops over the channels of the block: 4 V loads and one V-wide store per channel.  V = 4
// when the plane is a multiple of 4 floats and the destination (pointer and batch stride) is 16-byte aligned.  The
// source is read with 4-byte loads: for the motions this is made for (a few pixels of shift, a few degrees) the lanes of
// a wave read neighbouring addresses of two source rows, served by L1 / L2; HBM sees every source element once.
//
// Backward.  A thread owns one source pixel and kBwdChannels channels (their sums stay in registers).  It walks the
// box of output pixels that may read its pixel, rows ascending, columns ascending, re-evaluates the forward's own
// expressions for each candidate and adds weight * grad_out where one of the candidate's taps is its pixel.  For a
// realistic motion that is at most 25 candidates and at most 4 hits.  The lanes of a wave are neighbouring source
// pixels, so their candidates are neighbouring output pixels.  A singular or strongly shrinking transform makes the box
// the whole plane: slow, but correct and bounded.
//
// bfloat16 (the *_bf16 entry points: bf16 maps kept bf16 under autocast).  The kernels are templates on the element type
// and the bf16 forms are the same bodies: coordinates, taps, validity and the box come from bev_align_index.h unchanged
// and in float32, the taps / gradients are 2-byte loads widened exactly, the value and the gradient sum are the float32
// expressions above, and the result is rounded once to nearest even.  So a bf16 kernel returns, bit for bit, what the
// float32 kernel returns on the widened operands, rounded once.  Strides are counted in elements; a 16-byte store is
// V = 8 pixels (h * w and the stride multiples of 8), the narrow form a 2-byte store.
#include <hip/hip_runtime.h>

#include "bev_align_index.h"
#include "bev_align_taps.h"
#include "launch.h"
#include "ocrf_hip.h"
#include "plane_walk.h"

namespace {

using namespace plane;
using namespace bev_align;

constexpr int kChannels = 2;                       // channels per forward unit: coordinates are computed once for them
constexpr int kBwdChannels = 4;                    // channels per backward thread

template <typename T, int V>
__global__ void __launch_bounds__(kThreads) bev_align_kernel(int c, int h, int w, int cblocks, int chunks, int units,
                                                             const T* __restrict__ x, const float* __restrict__ tf,
                                                             T* __restrict__ out, long long out_batch_stride) {
  const int P = h * w;
  const Walk<V> walk(w);
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int rest = u / chunks, chunk = u - rest * chunks;
    const int b = rest / cblocks, c0 = (rest - b * cblocks) * kChannels;
    const int nc = min(kChannels, c - c0);
    float t[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) t[k] = tf[b * 9 + k];
    const T* s = x + ((size_t)b * c + c0) * P;
    T* o = out + (size_t)b * out_batch_stride + (size_t)c0 * P;
    walk.groups(walk.first(chunk), P, [&](int idx, int y, int xx) {
      Taps p[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        p[k] = taps_at(t, y, xx, h, w);
        if (++xx == w) {
          xx = 0;
          ++y;                                     // past the last row only behind the group's last pixel
        }
      }
#pragma unroll
      for (int ch = 0; ch < kChannels; ++ch) {
        if (ch < nc) {
          const T* sc = s + ch * P;
          float v[V];
#pragma unroll
          for (int k = 0; k < V; ++k) v[k] = sample_value(sc, p[k]);
          store_group<V>(o + ch * P + idx, v);
        }
      }
    });
  }
}

// grad_x[b][ch][qy][qx] = sum over the output pixels (i, j) one of whose taps is (qx, qy) of weight * grad_out[b][ch][i][j]
template <typename T>
__global__ void __launch_bounds__(kThreads) bev_align_backward_kernel(int c, int h, int w, int cblocks, int total,
                                                                      const T* __restrict__ grad_out,
                                                                      long long grad_batch_stride,
                                                                      const float* __restrict__ tf,
                                                                      T* __restrict__ grad_x) {
  const int P = h * w;
  for (int n = blockIdx.x * kThreads + (int)threadIdx.x; n < total; n += gridDim.x * kThreads) {
    const int rest = n / P, pix = n - rest * P;
    const int b = rest / cblocks, c0 = (rest - b * cblocks) * kBwdChannels;
    const int nc = min(kBwdChannels, c - c0);
    const int qy = pix / w, qx = pix - qy * w;
    float t[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) t[k] = tf[b * 9 + k];
    const Box box = source_box(t, h, w, qx, qy);
    const float fqx = (float)qx, fqy = (float)qy;
    const T* g = grad_out + (size_t)b * grad_batch_stride + (size_t)c0 * P;
    float acc[kBwdChannels];
#pragma unroll
    for (int ch = 0; ch < kBwdChannels; ++ch) acc[ch] = 0.0f;
    for (int i = box.y0; i <= box.y1; ++i) {
      for (int j = box.x0; j <= box.x1; ++j) {
        const Sample s = sample_at(t, i, j);
        const bool hit = (s.x0 == fqx || s.x0 + 1.0f == fqx) && (s.y0 == fqy || s.y0 + 1.0f == fqy);
        if (hit) {
          const float wgt = axis_weight(s.y0, s.ly, fqy) * axis_weight(s.x0, s.lx, fqx);
          const T* gp = g + i * w + j;
#pragma unroll
          for (int ch = 0; ch < kBwdChannels; ++ch) {
            if (ch < nc) acc[ch] += wgt * load_f32(gp + ch * P);
          }
        }
      }
    }
    T* d = grad_x + ((size_t)b * c + c0) * P + pix;
#pragma unroll
    for (int ch = 0; ch < kBwdChannels; ++ch) {
      if (ch < nc) store_f32(d + ch * P, acc[ch]);             // bf16: the one rounding
    }
  }
}

// The shapes the entry points accept: positive sizes, the contiguous (n, c, h, w) operand and the strided one (n rows
// of c * h * w elements, `stride` elements apart) both below 2 GiB, counted in bytes of the element.  *P: elements per
// plane
bool shapes_ok(int n, int c, int h, int w, long long stride, long long elem_bytes, long long* P) {
  if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return false;
  const long long planes = (long long)n * c, plane = (long long)h * w;           // each below 2^62
  const long long limit = kTwoGiB / elem_bytes;
  if (planes >= limit || plane >= limit || planes * plane >= limit) return false;
  const long long row = (long long)c * plane;
  if (stride < row || stride >= limit || (n - 1) * stride + row >= limit) return false;
  *P = plane;
  return true;
}

template <typename T>
int forward(int kernel_id, int n, int c, int h, int w, const T* x, const float* tf, T* out, long long out_batch_stride,
            ocrf_stream_t stream) {
  long long P;
  if (!shapes_ok(n, c, h, w, out_batch_stride, sizeof(T), &P) || !x || !tf || !out) return (int)hipErrorInvalidValue;
  constexpr int W = kWide<T>;
  const int cblocks = (c + kChannels - 1) / kChannels;
  const bool vec = P % W == 0 && out_batch_stride % W == 0 && aligned16(out);
  const Units u = units_of((long long)n * cblocks, P, vec ? W : 1);
  if (u.units >= kTwoGiB) return (int)hipErrorInvalidValue;
  if (vec) {
    ocrf::launch(kernel_id, bev_align_kernel<T, W>, dim3(u.grid), dim3(kThreads), 0, (hipStream_t)stream, c, h, w,
                 cblocks, u.chunks, (int)u.units, x, tf, out, out_batch_stride);
  } else {
    ocrf::launch(kernel_id, bev_align_kernel<T, 1>, dim3(u.grid), dim3(kThreads), 0, (hipStream_t)stream, c, h, w,
                 cblocks, u.chunks, (int)u.units, x, tf, out, out_batch_stride);
  }
  return (int)hipGetLastError();
}

template <typename T>
int backward(int kernel_id, int n, int c, int h, int w, const T* grad_out, long long grad_batch_stride, const float* tf,
             T* grad_x, ocrf_stream_t stream) {
  long long P;
  if (!shapes_ok(n, c, h, w, grad_batch_stride, sizeof(T), &P) || !grad_out || !tf || !grad_x) {
    return (int)hipErrorInvalidValue;
  }
  const int cblocks = (c + kBwdChannels - 1) / kBwdChannels;
  const long long total = (long long)n * cblocks * P;                            // <= n c h w < 2^30
  const unsigned grid = capped_grid((total + kThreads - 1) / kThreads);
  ocrf::launch(kernel_id, bev_align_backward_kernel<T>, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, c, h, w,
               cblocks, (int)total, grad_out, grad_batch_stride, tf, grad_x);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int ocrf_bev_align_forward(int n, int c, int h, int w, const float* x, const float* tf, float* out,
                           long long out_batch_stride, ocrf_stream_t stream) {
  return forward(OCRF_K_BEV_ALIGN, n, c, h, w, x, tf, out, out_batch_stride, stream);
}

int ocrf_bev_align_backward(int n, int c, int h, int w, const float* grad_out, long long grad_batch_stride,
                            const float* tf, float* grad_x, ocrf_stream_t stream) {
  return backward(OCRF_K_BEV_ALIGN_BWD, n, c, h, w, grad_out, grad_batch_stride, tf, grad_x, stream);
}

int ocrf_bev_align_forward_bf16(int n, int c, int h, int w, const unsigned short* x, const float* tf,
                                unsigned short* out, long long out_batch_stride, ocrf_stream_t stream) {
  return forward(OCRF_K_BEV_ALIGN_BF16, n, c, h, w, x, tf, out, out_batch_stride, stream);
}

int ocrf_bev_align_backward_bf16(int n, int c, int h, int w, const unsigned short* grad_out,
                                 long long grad_batch_stride, const float* tf, unsigned short* grad_x,
                                 ocrf_stream_t stream) {
  return backward(OCRF_K_BEV_ALIGN_BWD_BF16, n, c, h, w, grad_out, grad_batch_stride, tf, grad_x, stream);
}

int ocrf_bev_align_source_box(const float* tf, int h, int w, int qx, int qy, int* box) {
  if (!tf || !box || h <= 0 || w <= 0) return (int)hipErrorInvalidValue;
  const Box b = source_box(tf, h, w, qx, qy);
  box[0] = b.x0, box[1] = b.x1, box[2] = b.y0, box[3] = b.y1;
  return 0;
}

}  // extern "C"
