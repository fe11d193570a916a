// Image stage of the input pipeline: what PrepareImageInputs (mmdet3d/datasets/pipelines/loading.py:1071-1123) does to
// every camera frame with Pillow and mmcv, for all M = B * N * F frames of a batch in THREE launches:
//
//   horizontal  Pillow's 8-bit bicubic resample along x (ImagingResampleHorizontal_8bpc): only the source rows the crop's
//               vertical taps read and only the output columns inside the crop; a uint8 intermediate, as Pillow has
//   vertical    the resample along y, written as the cropped (M, fH, fW, 3) uint8 image, zero where the crop leaves the
//               resized image (Image.crop)
//   epilogue    reads the cropped image and writes imgs, imgs_wo_aug and imgs_wo_norm (M, 3, fH, fW) float32: the
//               left-right flip, the NEAREST rotation in 16.16 fixed point (Image.rotate -> affine_fixed) and mmcv's
//               imnormalize(to_rgb=True) are index arithmetic and one multiply per value
//
// Everything that depends on an image is read from one int32 table in device memory (include/ocrf_hip.h lays it out):
// a parameter row per camera and that camera's coefficient tables, already cut to the crop window.  The host builds the
// coefficients in float64 exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do, so no device arithmetic can
// differ from Pillow's: both passes are acc = 2^21 + sum(pixel * k), clamp(acc >> 22, 0, 255) in 32-bit integers.  A pass
// Pillow skips (the size along that axis does not change) arrives as the one-tap table k = 2^22, which copies the pixel.
// A column or row outside the resized image has no taps and yields 0.  No atomics, no host reads; reruns give the same
// bits.  Every table index and tap range is checked against the sizes before it is used: a malformed table yields
// zeros, never an access outside the buffers.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.h"
#include "ocrf_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRow = OCRF_IMAGE_PREP_ROW;          // int32 words per camera row

struct Camera {
  int r0, rows;                   // first source row held by the intermediate, and how many
  int hb, hk, hks;                // horizontal: offsets of bounds (fW x 2) and coefficients (hks x fW), taps per column
  int vb, vk, vks;                // vertical: bounds (fH x 2), coefficients (fH x vks), taps per row
  int flip, identity;             // left-right flip; rotate(0) is a copy
  int a[6];                       // the rotation's affine map, 16.16 fixed point
};

__device__ __forceinline__ Camera load_camera(const int* __restrict__ table, int g) {
  const int* p = table + (size_t)g * kRow;
  Camera c;
  c.r0 = p[0], c.rows = p[1], c.hb = p[2], c.hk = p[3], c.hks = p[4], c.vb = p[5], c.vk = p[6], c.vks = p[7];
  c.flip = p[8], c.identity = p[9];
#pragma unroll
  for (int i = 0; i < 6; ++i) c.a[i] = p[10 + i];
  return c;
}

// [off, off + count) lies inside the table (count >= 0)
__device__ __forceinline__ bool inside(long long off, long long count, long long n_table) {
  return off >= 0 && count >= 0 && off + count <= n_table;
}

__device__ __forceinline__ unsigned char clip8(int acc) {
  const int v = acc >> 22;                         // arithmetic shift, as Pillow's clip8 lookup indexes
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// grid (column tiles, rows of the intermediate, images)
__global__ void __launch_bounds__(kThreads) image_prep_horizontal_kernel(
    int F, int Hs, int Ws, int fW, int r_max, const unsigned char* __restrict__ frames, const int* __restrict__ table,
    long long n_table, unsigned char* __restrict__ tmp) {
  const int m = blockIdx.z, r = blockIdx.y;
  const int j = blockIdx.x * kThreads + (int)threadIdx.x;
  const Camera c = load_camera(table, m / F);
  if (r >= c.rows || r >= r_max || j >= fW) return;
  const int y = c.r0 + r;
  int acc[3] = {1 << 21, 1 << 21, 1 << 21};
  if (y >= 0 && y < Hs && c.hks > 0 && inside(c.hb, 2LL * fW, n_table) && inside(c.hk, (long long)fW * c.hks, n_table)) {
    const int xmin = table[c.hb + 2 * j];
    int n = table[c.hb + 2 * j + 1];
    if (xmin < 0 || n < 0 || n > c.hks || xmin > Ws - n) n = 0;
    const unsigned char* src = frames + (((size_t)m * Hs + y) * Ws + (n > 0 ? xmin : 0)) * 3;
    const int* k = table + c.hk + j;                // tap-major: the lanes of a wave read adjacent words
    for (int t = 0; t < n; ++t) {
      const int w = k[(size_t)t * fW];
      acc[0] += (int)src[3 * t + 0] * w;
      acc[1] += (int)src[3 * t + 1] * w;
      acc[2] += (int)src[3 * t + 2] * w;
    }
  }
  unsigned char* out = tmp + (((size_t)m * r_max + r) * fW + j) * 3;
  out[0] = clip8(acc[0]), out[1] = clip8(acc[1]), out[2] = clip8(acc[2]);
}

// grid (tiles of the row's fW * 3 bytes, fH, images).  The vertical taps are the same for every byte of a row, so a thread
// owns V adjacent bytes of it, whatever pixel and channel they belong to: V = 4 (one 32-bit load per tap) when the row
// pitch is a multiple of 4, which keeps every row 4-byte aligned, else V = 1.
template <int V>
__global__ void __launch_bounds__(kThreads) image_prep_vertical_kernel(
    int F, int fH, int fW, int r_max, const unsigned char* __restrict__ tmp, const int* __restrict__ table,
    long long n_table, unsigned char* __restrict__ crop) {
  const int m = blockIdx.z, i = blockIdx.y;
  const int pitch = fW * 3;
  const int b = (blockIdx.x * kThreads + (int)threadIdx.x) * V;
  if (b >= pitch) return;                          // pitch % V == 0: a thread's bytes are all inside or all outside
  const Camera c = load_camera(table, m / F);
  int acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = 1 << 21;
  if (c.vks > 0 && c.rows <= r_max && inside(c.vb, 2LL * fH, n_table) && inside(c.vk, (long long)fH * c.vks, n_table)) {
    const int rel = table[c.vb + 2 * i] - c.r0;    // first tap as a row of the intermediate
    int n = table[c.vb + 2 * i + 1];
    if (rel < 0 || n < 0 || n > c.vks || rel > c.rows - n) n = 0;
    const unsigned char* src = tmp + ((size_t)m * r_max + (n > 0 ? rel : 0)) * pitch + b;
    const int* k = table + c.vk + (size_t)i * c.vks;
    for (int t = 0; t < n; ++t) {
      const int w = k[t];
      if constexpr (V == 4) {
        const unsigned px = *reinterpret_cast<const unsigned*>(src + (size_t)t * pitch);
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[v] += (int)((px >> (8 * v)) & 0xffu) * w;
      } else {
        acc[0] += (int)src[(size_t)t * pitch] * w;
      }
    }
  }
  unsigned char* out = crop + ((size_t)m * fH + i) * pitch + b;
  if constexpr (V == 4) {
    *reinterpret_cast<unsigned*>(out) = (unsigned)clip8(acc[0]) | ((unsigned)clip8(acc[1]) << 8) |
                                        ((unsigned)clip8(acc[2]) << 16) | ((unsigned)clip8(acc[3]) << 24);
  } else {
    out[0] = clip8(acc[0]);
  }
}

struct Norm {
  float mean[3], stdinv[3];
};

// grid (column tiles, fH, images).  Output channel c of the normalised images reads RGB channel 2 - c: imnormalize with
// to_rgb=True swaps the channels of what is already an RGB array (loading.py:785-792), and the mean / std stay in place.
__global__ void __launch_bounds__(kThreads) image_prep_epilogue_kernel(
    int F, int fH, int fW, const unsigned char* __restrict__ crop, const int* __restrict__ table, Norm norm,
    float* __restrict__ imgs, float* __restrict__ wo_aug, float* __restrict__ wo_norm) {
  const int m = blockIdx.z, y = blockIdx.y;
  const int x = blockIdx.x * kThreads + (int)threadIdx.x;
  if (x >= fW) return;
  const Camera c = load_camera(table, m / F);
  const unsigned char* img = crop + (size_t)m * fH * fW * 3;
  const size_t plane = (size_t)fH * fW;
  const size_t o = (size_t)m * 3 * plane + (size_t)y * fW + x;

  const unsigned char* p = img + ((size_t)y * fW + x) * 3;
  const unsigned char* q = img + ((size_t)y * fW + (c.flip ? fW - 1 - x : x)) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    wo_aug[o + ch * plane] = ((float)p[2 - ch] - norm.mean[ch]) * norm.stdinv[ch];
    wo_norm[o + ch * plane] = (float)q[ch];
  }

  // Image.rotate: the source pixel of (x, y) in the flipped image; outside it the fill is 0, normalised like a pixel
  int xin = x, yin = y;
  if (!c.identity) {
    xin = (int)(((long long)c.a[2] + (long long)c.a[1] * y + (long long)c.a[0] * x) >> 16);
    yin = (int)(((long long)c.a[5] + (long long)c.a[4] * y + (long long)c.a[3] * x) >> 16);
  }
  float v[3] = {0.f, 0.f, 0.f};
  if (xin >= 0 && xin < fW && yin >= 0 && yin < fH) {
    const unsigned char* s = img + ((size_t)yin * fW + (c.flip ? fW - 1 - xin : xin)) * 3;
    v[0] = (float)s[0], v[1] = (float)s[1], v[2] = (float)s[2];
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) imgs[o + ch * plane] = (v[2 - ch] - norm.mean[ch]) * norm.stdinv[ch];
}

}  // namespace

extern "C" int ocrf_image_prep(int M, int F, int Hs, int Ws, int fH, int fW, int r_max, const unsigned char* frames,
                               const int* table, long long n_table, unsigned char* tmp, unsigned char* crop,
                               float mean0, float mean1, float mean2, float stdinv0, float stdinv1, float stdinv2,
                               float* imgs, float* imgs_wo_aug, float* imgs_wo_norm, ocrf_stream_t stream) {
  if (M <= 0 || F <= 0 || M % F || M > 65535) return (int)hipErrorInvalidValue;
  if (Hs <= 0 || Ws <= 0 || Hs > OCRF_IMAGE_PREP_MAX_SOURCE || Ws > OCRF_IMAGE_PREP_MAX_SOURCE) return (int)hipErrorInvalidValue;
  if (fH <= 0 || fW <= 0 || fH > OCRF_IMAGE_PREP_MAX_OUTPUT || fW > OCRF_IMAGE_PREP_MAX_OUTPUT) return (int)hipErrorInvalidValue;
  if (r_max <= 0 || r_max > Hs || n_table < (long long)(M / F) * kRow) return (int)hipErrorInvalidValue;
  if (!frames || !table || !tmp || !crop || !imgs || !imgs_wo_aug || !imgs_wo_norm) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const unsigned tiles = (unsigned)((fW + kThreads - 1) / kThreads);
  ocrf::launch(OCRF_K_IMAGE_PREP_HORIZONTAL, image_prep_horizontal_kernel, dim3(tiles, r_max, M), dim3(kThreads), 0, s, F,
               Hs, Ws, fW, r_max, frames, table, n_table, tmp);
  // tmp and crop are 4-byte aligned and every image and row starts a multiple of the pitch behind them
  const int pitch = fW * 3;
  if (pitch % 4 == 0 && (uintptr_t)tmp % 4 == 0 && (uintptr_t)crop % 4 == 0) {
    ocrf::launch(OCRF_K_IMAGE_PREP_VERTICAL, image_prep_vertical_kernel<4>,
                 dim3((unsigned)((pitch / 4 + kThreads - 1) / kThreads), fH, M), dim3(kThreads), 0, s, F, fH, fW, r_max,
                 (const unsigned char*)tmp, table, n_table, crop);
  } else {
    ocrf::launch(OCRF_K_IMAGE_PREP_VERTICAL, image_prep_vertical_kernel<1>,
                 dim3((unsigned)((pitch + kThreads - 1) / kThreads), fH, M), dim3(kThreads), 0, s, F, fH, fW, r_max,
                 (const unsigned char*)tmp, table, n_table, crop);
  }
  const Norm norm = {{mean0, mean1, mean2}, {stdinv0, stdinv1, stdinv2}};
  ocrf::launch(OCRF_K_IMAGE_PREP_EPILOGUE, image_prep_epilogue_kernel, dim3(tiles, fH, M), dim3(kThreads), 0, s, F, fH, fW,
               (const unsigned char*)crop, table, norm, imgs, imgs_wo_aug, imgs_wo_norm);
  return (int)hipGetLastError();
}
