// Bilinear upsampling (align_corners=True, integer factor) written straight into its place in a channel concatenation:
// FPN_LSS.forward's x = cat([x2, up(x1)], 1) (mmdet3d/models/necks/lss_fpn.py:93-94) as ONE launch that writes every
// element of the result once, and up2[0] (:64-67) as the same launch with nothing to concatenate (C2 = 0).  The
// backward is the transpose of the upsampling as a gather: one thread per input pixel sums the output pixels that read
// it, in a fixed order.  No atomics, no workspace, no host synchronisation; repeated runs are bit-identical.
//
// Sampling rule, per axis, for output index d of out = in * scale points:
//   n = d (in - 1);  i0 = n / (out - 1);  lambda = float(n % (out - 1)) / float(out - 1);  i1 = min(i0 + 1, in - 1)
// in integer arithmetic with one rounding (in = 1: i0 = 0, lambda = 0).  torch computes lambda from the float product
// (in - 1) / (out - 1) * d, which differs in its last bits.  The value is
//   (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11)
// in float32, each operation rounded once (the library is built with -ffp-contract=off).
//
// Layout.  Both kernels keep the (i0, lambda) pairs of the two axes in LDS (Hout + Wout entries of 8 bytes, built by
// every workgroup at its start: two integer divisions per entry, once).  The forward walks each (b, c) output plane as
// plane_walk.h describes; V = 4 holds for every even factor on torch's allocations, and V = 1 is also what handles a
// plane whose size is no multiple of 4.  Copied channels are a 16-byte load and store.
// The x1 plane of a channel is Hin * Win floats (1 KiB at the reference's 16 x 16, 16 KiB at 64 x 64): the lanes of a
// wave read neighbouring or equal addresses of two of its rows, served by L1 / L2; HBM sees every input once.
// The backward's lanes are neighbouring input pixels of a row: at each step they read grad_out addresses `scale`
// floats apart on the same output row, and the steps of a lane walk along that row, so every fetched line is used in
// full out of L1 / L2.
//
// bfloat16 (the *_bf16 entry points, for the BEV encoder under bf16 autocast).  The kernels are templates on the element
// type and the bf16 forms are the same bodies: the taps are 2-byte loads widened exactly, the value is the float32
// expression above and the backward's sum its float32 accumulator in the same order, and the result is rounded once to
// nearest even (plane_walk.h's round_pair / round_one).  So a bf16 kernel returns, bit for bit, what the float32 kernel
// returns on the widened operands, rounded once.  The access width is counted in bytes: a 16-byte group is V = 8
// elements (P % 8 == 0), the narrow form a 2-byte access, a copied channel one 16-byte load and store of 8 elements.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "ocrf_hip.h"
#include "plane_walk.h"

namespace {

using namespace plane;

struct Tap {
  int i0;
  float lam;
};

// (i0, lambda) of every output index of both axes: tab[0, Hout) the rows, tab[Hout, Hout + Wout) the columns
__device__ __forceinline__ void build_taps(Tap* tab, int Hin, int Win, int Hout, int Wout) {
  for (int i = threadIdx.x; i < Hout + Wout; i += kThreads) {
    const bool row = i < Hout;
    const int d = row ? i : i - Hout;
    const int in = row ? Hin : Win, out = row ? Hout : Wout;
    Tap t;
    t.i0 = 0;
    t.lam = 0.0f;
    if (in > 1) {                                  // out - 1 >= in - 1 >= 1
      const unsigned n = (unsigned)d * (unsigned)(in - 1), den = (unsigned)(out - 1);
      const unsigned q = n / den;
      t.i0 = (int)q;
      t.lam = (float)(n - q * den) / (float)den;
    }
    tab[i] = t;
  }
  __syncthreads();
}

// T: float or bf16_t.  The sampled value is ONE float32 expression for both: the bf16 form widens its four taps, and
// store_group rounds the result once.
template <typename T, int V>
__global__ void __launch_bounds__(kThreads) upsample_cat_kernel(int C2, int C1, int Hin, int Win, int scale,
                                                                 int chunks, int units, const T* __restrict__ x2,
                                                                 const T* __restrict__ x1, T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Tap* tab_y = reinterpret_cast<Tap*>(lds_raw);
  const int Hout = Hin * scale, Wout = Win * scale;
  Tap* tab_x = tab_y + Hout;
  build_taps(tab_y, Hin, Win, Hout, Wout);
  using VT = typename GroupOf<T, V>::type;
  const int P = Hout * Wout, Pin = Hin * Win, Ct = C2 + C1;
  const Walk<V> walk(Wout);
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int plane = u / chunks, chunk = u - plane * chunks;
    const int b = plane / Ct, c = plane - b * Ct;
    const int first = walk.first(chunk);
    T* o = out + (size_t)plane * P;
    if (c < C2) {                                  // uniform over the workgroup
      const T* s = x2 + ((size_t)b * C2 + c) * P;
#pragma unroll
      for (int g = 0; g < kGroups; ++g) {
        const int idx = first + g * walk.kStep;
        if (idx < P) *reinterpret_cast<VT*>(o + idx) = *reinterpret_cast<const VT*>(s + idx);
      }
      continue;
    }
    const T* s = x1 + ((size_t)b * C1 + (c - C2)) * Pin;
    walk.groups(first, P, [&](int idx, int y, int x) {
      float v[V];
      walk.values(v, y, x, [&](int yy, int xx) {
        const Tap ty = tab_y[yy], tx = tab_x[xx];
        const int r0 = ty.i0 * Win, r1 = min(ty.i0 + 1, Hin - 1) * Win;
        const int c0 = tx.i0, c1 = min(tx.i0 + 1, Win - 1);
        const float v00 = load_f32(s + (r0 + c0)), v01 = load_f32(s + (r0 + c1));
        const float v10 = load_f32(s + (r1 + c0)), v11 = load_f32(s + (r1 + c1));
        const float mx = 1.0f - tx.lam, my = 1.0f - ty.lam;
        const float top = mx * v00 + tx.lam * v01, bot = mx * v10 + tx.lam * v11;
        return my * top + ty.lam * bot;
      });
      store_group<V>(o + idx, v);
    });
  }
}

// grad_x1[b][c][iy][ix] = sum over the output pixels (oy, ox) that read input pixel (iy, ix) of
// wy(oy, iy) wx(ox, ix) grad_out[b][C2 + c][oy][ox]; rows ascending, columns ascending inside a row, the row sums
// weighted and added in that order.  An output index o reads i0(o) with weight 1 - lambda and min(i0 + 1, in - 1) with
// weight lambda; the candidates of input index i are the o with i0(o) in {i - 1, i}.
__device__ __forceinline__ float tap_weight(const Tap t, int i, int in) {
  const float a = t.i0 == i ? 1.0f - t.lam : 0.0f;
  const float b = min(t.i0 + 1, in - 1) == i ? t.lam : 0.0f;
  return a + b;
}

// first and last output index whose i0 lies in {i - 1, i}
__device__ __forceinline__ void tap_range(int i, int in, int out, int* lo, int* hi) {
  if (in == 1) {
    *lo = 0;
    *hi = out - 1;
    return;
  }
  const unsigned den = (unsigned)(in - 1), num = (unsigned)(out - 1);
  // i0(o) >= i - 1  <=>  o >= ceil((i - 1) num / den);   i0(o) <= i  <=>  o (in - 1) < (i + 1) num
  *lo = i == 0 ? 0 : (int)(((unsigned)(i - 1) * num + den - 1) / den);
  const int end = (int)(((unsigned)(i + 1) * num + den - 1) / den);   // first o with i0(o) > i
  *hi = min(end, out) - 1;
}

template <typename T>
__global__ void __launch_bounds__(kThreads) upsample_cat_backward_kernel(int C2, int C1, int Hin, int Win, int scale,
                                                                          int total, const T* __restrict__ grad_out,
                                                                          T* __restrict__ grad_x1) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Tap* tab_y = reinterpret_cast<Tap*>(lds_raw);
  const int Hout = Hin * scale, Wout = Win * scale;
  Tap* tab_x = tab_y + Hout;
  build_taps(tab_y, Hin, Win, Hout, Wout);
  const int P = Hout * Wout, Pin = Hin * Win, Ct = C2 + C1;
  for (int i = blockIdx.x * kThreads + (int)threadIdx.x; i < total; i += gridDim.x * kThreads) {
    const int plane = i / Pin, pix = i - plane * Pin;            // plane = b * C1 + c
    const int iy = pix / Win, ix = pix - iy * Win;
    const int b = plane / C1, c = plane - b * C1;
    const T* g = grad_out + ((size_t)b * Ct + C2 + c) * P;
    int ylo, yhi, xlo, xhi;
    tap_range(iy, Hin, Hout, &ylo, &yhi);
    tap_range(ix, Win, Wout, &xlo, &xhi);
    float acc = 0.0f;
    for (int oy = ylo; oy <= yhi; ++oy) {
      const float wy = tap_weight(tab_y[oy], iy, Hin);
      const T* row = g + oy * Wout;
      float r = 0.0f;
      for (int ox = xlo; ox <= xhi; ++ox) r += tap_weight(tab_x[ox], ix, Win) * load_f32(row + ox);
      acc += wy * r;
    }
    store_f32(grad_x1 + i, acc);                   // bf16: the one rounding
  }
}

// the shapes the entry points accept; *P / *Pin: elements (of elem_bytes) per output / input plane
bool shapes_ok(int B, int C2, int C1, int Hin, int Win, int scale, long long elem_bytes, long long* P, long long* Pin) {
  if (B <= 0 || C2 < 0 || C1 <= 0 || Hin <= 0 || Win <= 0 || scale <= 0) return false;
  const long long Hout = (long long)Hin * scale, Wout = (long long)Win * scale;
  // out / grad_out are the largest
  if (!planes_ok((long long)B * (C2 + (long long)C1), Hout, Wout, elem_bytes)) return false;
  *P = Hout * Wout;
  *Pin = (long long)Hin * Win;
  return true;
}

template <typename T>
int forward(int kernel_id, int B, int C2, int C1, int Hin, int Win, int scale, const T* x2, const T* x1, T* out,
            ocrf_stream_t stream) {
  long long P, Pin;
  if (!shapes_ok(B, C2, C1, Hin, Win, scale, sizeof(T), &P, &Pin)) return (int)hipErrorInvalidValue;
  if (!x1 || !out || (C2 > 0 && !x2)) return (int)hipErrorInvalidValue;
  constexpr int W = kWide<T>;
  const size_t lds = (size_t)(Hin + Win) * scale * sizeof(Tap);
  const bool vec = P % W == 0 && aligned16(out) && (C2 == 0 || aligned16(x2));
  const Units n = units_of((long long)B * (C2 + C1), P, vec ? W : 1);
  if (n.units >= kTwoGiB) return (int)hipErrorInvalidValue;
  if (vec) {
    ocrf::launch(kernel_id, upsample_cat_kernel<T, W>, dim3(n.grid), dim3(kThreads), lds, (hipStream_t)stream, C2, C1,
                 Hin, Win, scale, n.chunks, (int)n.units, x2, x1, out);
  } else {
    ocrf::launch(kernel_id, upsample_cat_kernel<T, 1>, dim3(n.grid), dim3(kThreads), lds, (hipStream_t)stream, C2, C1,
                 Hin, Win, scale, n.chunks, (int)n.units, x2, x1, out);
  }
  return (int)hipGetLastError();
}

template <typename T>
int backward(int kernel_id, int B, int C2, int C1, int Hin, int Win, int scale, const T* grad_out, T* grad_x1,
             ocrf_stream_t stream) {
  long long P, Pin;
  if (!shapes_ok(B, C2, C1, Hin, Win, scale, sizeof(T), &P, &Pin)) return (int)hipErrorInvalidValue;
  if (!grad_out || !grad_x1) return (int)hipErrorInvalidValue;
  const size_t lds = (size_t)(Hin + Win) * scale * sizeof(Tap);
  const long long total = (long long)B * C1 * Pin;                // < 2^30
  const unsigned grid = capped_grid((total + kThreads - 1) / kThreads);
  ocrf::launch(kernel_id, upsample_cat_backward_kernel<T>, dim3(grid), dim3(kThreads), lds, (hipStream_t)stream, C2, C1,
               Hin, Win, scale, (int)total, grad_out, grad_x1);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int ocrf_upsample_cat_forward(int B, int C2, int C1, int Hin, int Win, int scale, const float* x2, const float* x1,
                              float* out, ocrf_stream_t stream) {
  return forward(OCRF_K_UPSAMPLE_CAT, B, C2, C1, Hin, Win, scale, x2, x1, out, stream);
}

int ocrf_upsample_cat_backward(int B, int C2, int C1, int Hin, int Win, int scale, const float* grad_out,
                               float* grad_x1, ocrf_stream_t stream) {
  return backward(OCRF_K_UPSAMPLE_CAT_BWD, B, C2, C1, Hin, Win, scale, grad_out, grad_x1, stream);
}

int ocrf_upsample_cat_forward_bf16(int B, int C2, int C1, int Hin, int Win, int scale, const unsigned short* x2,
                                   const unsigned short* x1, unsigned short* out, ocrf_stream_t stream) {
  return forward(OCRF_K_UPSAMPLE_CAT_BF16, B, C2, C1, Hin, Win, scale, x2, x1, out, stream);
}

int ocrf_upsample_cat_backward_bf16(int B, int C2, int C1, int Hin, int Win, int scale, const unsigned short* grad_out,
                                    unsigned short* grad_x1, ocrf_stream_t stream) {
  return backward(OCRF_K_UPSAMPLE_CAT_BWD_BF16, B, C2, C1, Hin, Win, scale, grad_out, grad_x1, stream);
}

}  // extern "C"
