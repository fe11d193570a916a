// Streaming temporal alignment: the whole concatenation in front of the BEV encoder in ONE launch, from a ring of the
// last S = K + 1 key-frame BEV maps (OcRFDet4D.stream_step).  The batch forward pays one feature_transform (about forty
// small torch launches) and one warp launch per adjacent frame plus a copy of the key frame (temporal.align_and_cat);
// here the transforms are evaluated inside the kernel from the raw poses kept with each ring slot.
//
// Selection.  Channel group g = 0 .. K - 1 of `out` holds age a = K - g (oldest first), group K the key frame (age 0).
// For sample b the effective age is e = min(a, valid[b]) (valid[b] clamped to >= 0) and the source slot
// (head - e) mod S: a sample with fewer than `a` real history frames repeats its oldest one, down to the key frame
// itself right after a reset.  e = 0 or align = 0: the group is a copy of the source plane.  Otherwise it is the
// bilinear warp under tf, with bev_align_taps.h's taps and value: bit for bit what bev_align_kernel<float, V> writes for
// the same plane and the same tf.
//
// tf is temporal.feature_transform's value for curr = inv(E_h) E_h S_h and adj = inv(E_h) E_s S_s (E = ego2global0,
// S = sensor2ego0, h the head slot, s the source slot), bda = bda[h], bda_adj = bda[s]: evaluated as that function does,
// in float64 with closed-form affine inverses (pose_math.h), rounded once to float32.  It is needed once per (b, age),
// not per pixel: thread 0 of the workgroup evaluates it at the head of a unit and leaves its six floats in LDS, the
// other threads wait at the barrier.  (The operands are uniform over the workgroup, but there is no scalar float64 ALU to
// evaluate them on: "per unit in registers" would mean every lane of every wave issuing the same few hundred float64
// operations.  One lane and 24 bytes of LDS cost the unit the same latency and a 256th of the issue slots.)  The unit
// whose channel block and chunk are 0 also writes the nine floats to tf_out[g][b]; a copied group gets the identity.
//
// Units are the forward kernel's: (sample, group, block of kChannels channels, chunk of the plane), plane_walk.h groups,
// 16-byte stores when the plane, the stride and the pointer allow it.  Every destination element is written once; no
// atomics, no workspace, no host read; reruns are bit-identical.
//
// bfloat16 (ocrf_bev_stream_align_bf16: the ring of a streaming step under bf16 autocast).  The kernel is a template on
// the element type and the bf16 form is the same body: units, selection, slot_transform and the tf_out report do not
// depend on the element, the taps are 2-byte loads widened exactly (sample_value<T>), the value is the float32
// expression and store_group rounds it once to nearest even: bit for bit what bev_align_kernel<unsigned short, V> writes
// for the same plane and tf.  A copied group moves the bits (no widening, no rounding).  Strides are counted in
// elements; a 16-byte store is V = 8 pixels, the narrow form a 2-byte store.
#include <hip/hip_runtime.h>

#include "bev_align_taps.h"
#include "launch.h"
#include "ocrf_hip.h"
#include "plane_walk.h"
#include "pose_math.h"

namespace {

using namespace plane;
using namespace bev_align;
using namespace pose;

constexpr int kChannels = 2;                       // channels per unit, as in bev_align.hip
constexpr long long kMaxSlots = 1 << 24;           // S * B: the pose operands (16 floats each) far below 2 GiB

template <typename T>
struct Args {
  int S, B, C, h, w, head, align;
  int cblocks, chunks, units;
  int wide_source;                                 // the ring is 16-byte aligned: a copied group may be one 16-byte load
  const T* ring;
  const int* valid;
  const float* sensor2ego0;
  const float* ego2global0;
  const float* bda;
  double ix, iy, lx, ly;
  T* out;
  long long out_batch_stride;
  float* tf_out;
};

// a (3, 3) float32 augmentation applied to the affine map p: the 3 x 3 block and the translation of bda4 . p
__device__ __forceinline__ void augmented(const float* __restrict__ a, const Mat4& p, double (&r)[3][3],
                                          double (&t)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double a0 = (double)a[i * 3], a1 = (double)a[i * 3 + 1], a2 = (double)a[i * 3 + 2];
#pragma unroll
    for (int j = 0; j < 3; ++j) r[i][j] = a0 * p.m[0][j] + a1 * p.m[1][j] + a2 * p.m[2][j];
    t[i] = a0 * p.m[0][3] + a1 * p.m[1][3] + a2 * p.m[2][3];
  }
}

// temporal.feature_transform from the raw poses of head slot `hs` and source slot `ss` (indices of (slot, sample)
// matrices): rows 0 and 1 of tf, rounded once to float32
template <typename T>
__device__ __forceinline__ void slot_transform(const Args<T>& a, size_t hs, size_t ss, float (&tf)[6]) {
  const Mat4 head2global = load4(a.ego2global0 + hs * 16);
  const Mat4 global2head = affine_inverse(head2global);
  const Mat4 curr = mul4(global2head, mul4(head2global, load4(a.sensor2ego0 + hs * 16)));
  const Mat4 adj = mul4(global2head, mul4(load4(a.ego2global0 + ss * 16), load4(a.sensor2ego0 + ss * 16)));
  double rc[3][3], tc[3], ra[3][3], ta[3];
  augmented(a.bda + hs * 9, curr, rc, tc);
  augmented(a.bda + ss * 9, adj, ra, ta);
  // rm = rc . inv(ra) for rows 0 and 1, inv(ra) = adjugate / det (temporal._inverse3); tm = tc - rm . ta
  double cof[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      cof[i][j] = ra[i1][j1] * ra[i2][j2] - ra[i1][j2] * ra[i2][j1];
    }
  }
  const double det = ra[0][0] * cof[0][0] + ra[0][1] * cof[0][1] + ra[0][2] * cof[0][2];
  double rm[2][3], tm[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      rm[i][j] = rc[i][0] * (cof[j][0] / det) + rc[i][1] * (cof[j][1] / det) + rc[i][2] * (cof[j][2] / det);
    }
    tm[i] = tc[i] - (rm[i][0] * ta[0] + rm[i][1] * ta[1] + rm[i][2] * ta[2]);
  }
  // inv(feat2bev) . L . feat2bev, row by row
  tf[0] = (float)rm[0][0];
  tf[1] = (float)(rm[0][1] * a.iy / a.ix);
  tf[2] = (float)((rm[0][0] * a.lx + rm[0][1] * a.ly + tm[0] - a.lx) / a.ix);
  tf[3] = (float)(rm[1][0] * a.ix / a.iy);
  tf[4] = (float)rm[1][1];
  tf[5] = (float)((rm[1][0] * a.lx + rm[1][1] * a.ly + tm[1] - a.ly) / a.iy);
}

// One group of a copied plane, bits unchanged: one 16-byte load when the source allows it (`wide`), else element loads;
// the store is the group's (16 bytes for V > 1)
template <int V>
__device__ __forceinline__ void copy_group(float* __restrict__ d, const float* __restrict__ p, bool wide) {
  if constexpr (V == 4) {
    if (wide) {
      *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(p);
      return;
    }
  }
  float v[V];
#pragma unroll
  for (int k = 0; k < V; ++k) v[k] = p[k];
  store_group<V>(d, v);
}
template <int V>
__device__ __forceinline__ void copy_group(bf16_t* __restrict__ d, const bf16_t* __restrict__ p, bool wide) {
  if constexpr (V == 8) {
    uint4 q;
    if (wide) {
      q = *reinterpret_cast<const uint4*>(p);
    } else {
      q.x = (unsigned)p[0] | ((unsigned)p[1] << 16);
      q.y = (unsigned)p[2] | ((unsigned)p[3] << 16);
      q.z = (unsigned)p[4] | ((unsigned)p[5] << 16);
      q.w = (unsigned)p[6] | ((unsigned)p[7] << 16);
    }
    *reinterpret_cast<uint4*>(d) = q;
  } else {
    static_assert(V == 1, "a group of bf16 is 8 or 1");
    *d = *p;
  }
}

template <typename T, int V>
__global__ void __launch_bounds__(kThreads) bev_stream_align_kernel(Args<T> a) {
  __shared__ float tf_shared[6];
  const int P = a.h * a.w, K = a.S - 1;
  const Walk<V> walk(a.w);
  for (int u = blockIdx.x; u < a.units; u += gridDim.x) {        // u depends on the workgroup only: uniform barriers
    int rest = u / a.chunks;
    const int chunk = u - rest * a.chunks;
    const int cb = rest % a.cblocks;
    rest /= a.cblocks;
    const int b = rest / a.S, g = rest - b * a.S;
    const int c0 = cb * kChannels, nc = min(kChannels, a.C - c0);
    const int e = min(K - g, max(a.valid[b], 0));                // 0 <= e <= K
    const int slot = a.head - e + (a.head < e ? a.S : 0);        // in [0, S)
    const bool warp = e > 0 && a.align != 0;
    const bool reports = a.tf_out != nullptr && g < K && cb == 0 && chunk == 0;
    __syncthreads();                                             // the previous unit's readers are done with tf_shared
    if (threadIdx.x == 0 && (warp || reports)) {
      float tf[6] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
      if (warp) {
        slot_transform(a, (size_t)a.head * a.B + b, (size_t)slot * a.B + b, tf);
#pragma unroll
        for (int k = 0; k < 6; ++k) tf_shared[k] = tf[k];
      }
      if (reports) {
        float* o = a.tf_out + ((size_t)g * a.B + b) * 9;
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = tf[k];
        o[6] = 0.0f, o[7] = 0.0f, o[8] = 1.0f;
      }
    }
    __syncthreads();
    const T* s = a.ring + (((size_t)slot * a.B + b) * a.C + c0) * P;
    T* o = a.out + (size_t)b * a.out_batch_stride + ((size_t)g * a.C + c0) * P;
    if (!warp) {
      walk.groups(walk.first(chunk), P, [&](int idx, int, int) {
#pragma unroll
        for (int ch = 0; ch < kChannels; ++ch) {
          if (ch < nc) copy_group<V>(o + ch * P + idx, s + ch * P + idx, a.wide_source != 0);
        }
      });
      continue;
    }
    float t[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) t[k] = tf_shared[k];
    walk.groups(walk.first(chunk), P, [&](int idx, int y, int xx) {
      Taps p[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        p[k] = taps_at(t, y, xx, a.h, a.w);
        if (++xx == a.w) {
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

template <typename T>
int stream_align(int kernel_id, int S, int B, int C, int h, int w, const T* ring, int head, const int* valid,
                 const float* sensor2ego0, const float* ego2global0, const float* bda, double interval_x,
                 double interval_y, double lower_x, double lower_y, int align, T* out, long long out_batch_stride,
                 float* tf_out, ocrf_stream_t stream) {
  if (S <= 0 || B <= 0 || C <= 0 || h <= 0 || w <= 0 || head < 0 || head >= S) return (int)hipErrorInvalidValue;
  if (!ring || !valid || !sensor2ego0 || !ego2global0 || !bda || !out) return (int)hipErrorInvalidValue;
  if (!(interval_x > 0.0) || !(interval_y > 0.0)) return (int)hipErrorInvalidValue;          // NaN too
  const long long limit = kTwoGiB / (long long)sizeof(T);            // elements of the operand's type
  const long long slots = (long long)S * B, P = (long long)h * w;                            // each below 2^62
  if (slots >= kMaxSlots || P >= limit) return (int)hipErrorInvalidValue;
  const long long planes = slots * C;                                                        // below 2^55
  if (planes >= limit || planes * P >= limit) return (int)hipErrorInvalidValue;              // the ring
  const long long row = (long long)S * C * P;                                                // <= planes * P
  if (out_batch_stride < row || out_batch_stride >= limit || (B - 1) * out_batch_stride + row >= limit) {
    return (int)hipErrorInvalidValue;
  }
  const int cblocks = (C + kChannels - 1) / kChannels;
  constexpr int W = kWide<T>;                                    // elements of a 16-byte group: 4 floats, 8 bf16
  const bool vec = P % W == 0 && out_batch_stride % W == 0 && aligned16(out);
  const Units n = units_of(slots * cblocks, P, vec ? W : 1);
  if (n.units >= kTwoGiB) return (int)hipErrorInvalidValue;
  Args<T> a;
  a.S = S, a.B = B, a.C = C, a.h = h, a.w = w, a.head = head, a.align = align;
  a.cblocks = cblocks, a.chunks = n.chunks, a.units = (int)n.units;
  a.wide_source = aligned16(ring) ? 1 : 0;                       // with P % W == 0 every plane of the ring then is
  a.ring = ring, a.valid = valid, a.sensor2ego0 = sensor2ego0, a.ego2global0 = ego2global0, a.bda = bda;
  a.ix = interval_x, a.iy = interval_y, a.lx = lower_x, a.ly = lower_y;
  a.out = out, a.out_batch_stride = out_batch_stride, a.tf_out = tf_out;
  if (vec) {
    ocrf::launch(kernel_id, bev_stream_align_kernel<T, W>, dim3(n.grid), dim3(kThreads), 0, (hipStream_t)stream, a);
  } else {
    ocrf::launch(kernel_id, bev_stream_align_kernel<T, 1>, dim3(n.grid), dim3(kThreads), 0, (hipStream_t)stream, a);
  }
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int ocrf_bev_stream_align(int S, int B, int C, int h, int w, const float* ring, int head, const int* valid,
                          const float* sensor2ego0, const float* ego2global0, const float* bda, double interval_x,
                          double interval_y, double lower_x, double lower_y, int align, float* out,
                          long long out_batch_stride, float* tf_out, ocrf_stream_t stream) {
  return stream_align(OCRF_K_BEV_STREAM_ALIGN, S, B, C, h, w, ring, head, valid, sensor2ego0, ego2global0, bda,
                      interval_x, interval_y, lower_x, lower_y, align, out, out_batch_stride, tf_out, stream);
}

int ocrf_bev_stream_align_bf16(int S, int B, int C, int h, int w, const unsigned short* ring, int head,
                               const int* valid, const float* sensor2ego0, const float* ego2global0, const float* bda,
                               double interval_x, double interval_y, double lower_x, double lower_y, int align,
                               unsigned short* out, long long out_batch_stride, float* tf_out, ocrf_stream_t stream) {
  return stream_align(OCRF_K_BEV_STREAM_ALIGN_BF16, S, B, C, h, w, ring, head, valid, sensor2ego0, ego2global0, bda,
                      interval_x, interval_y, lower_x, lower_y, align, out, out_batch_stride, tf_out, stream);
}

}  // extern "C"
