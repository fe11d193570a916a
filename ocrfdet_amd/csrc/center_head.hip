// Training targets and losses of the detection head (mmdet3d/models/dense_heads/centerpoint_head.py CenterHead:
// get_targets_single :437-585, loss :587-668; gaussian_radius / draw_heatmap_gaussian of core/utils/gaussian.py; mmdet
// 2.x gaussian_focal_loss and l1_loss with weight_reduce_loss).  Every task and sample in one call, nothing read back
// to the host.
//
// Targets, two launches after a memset of the counts:
//   assign   one block per sample: zeroes the sample's anno_box / ind / mask rows of every task, then one thread per
//            box finds its task, class and slot (rank within the task after the class-by-class regrouping), its radius
//            and centre cell, and writes its row.  Each box leaves a record {task, class, cx, cy, radius} for:
//   heatmap  gather form: one thread per heatmap pixel, max over the records of its (sample, task, class) in LDS.  No
//            memset of the heatmap and no atomics on it; max is order-independent, so the result is the reference's
//            sequence of torch.max draws.
// counts[0, T) (heatmap pixels == 1 per task) and counts[T, 2T) (mask sums per task) are float atomic adds of small
// integers: exact, so independent of order.
//
// Losses: per-block partials reduced in a fixed order by one final block; the backward of the regression loss sums
// duplicate indices in slot order from the first slot holding the index, so reruns are bit-identical.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "launch.h"
#include "ocrf_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kHmChunk = kThreads * 8;        // heatmap-loss elements per block
constexpr float kClipLo = 1e-4f;
constexpr float kClipHi = (float)(1.0 - 1e-4);
constexpr double kF32Eps = 1.1920928955078125e-07;   // torch.finfo(torch.float32).eps, added in double

struct TargetArgs {
  int B, T, box_dim, n_labels, H, W, M, C, with_vel, norm_bbox, min_radius;
  float vs0, vs1, pc0, pc1, osf;
  float k_omo, k_opo, k_om1, k_a3x4, k_b3;    // float32 roundings of the radius formula's Python scalars
  const float* boxes;
  const long long* labels;
  const long long* offsets;
  const int* table;                           // (n_labels, 2): task, class in task; task -1 = in no task
  float* heat;
  float* anno;
  long long* ind;
  unsigned char* mask;
  float* counts;
  int4* rec;
  int ncls[OCRF_CH_MAX_TASKS];
  int plane_task[OCRF_CH_MAX_PLANES], plane_cls[OCRF_CH_MAX_PLANES];
  long long heat_off[OCRF_CH_MAX_TASKS];      // element offset of task t's (B, ncls, H, W) block
};

__device__ __forceinline__ void lookup(const TargetArgs& a, long long lab, int* t, int* c) {
  if (lab < 0 || lab >= a.n_labels) {
    *t = -1;
    *c = 0;
    return;
  }
  *t = a.table[2 * lab];
  *c = a.table[2 * lab + 1];
}

// gaussian_radius((length, width), overlap) in float32, the reference's operation order
__device__ float gaussian_radius_f32(const TargetArgs& a, float height, float width) {
  const float b1 = height + width;
  const float c1 = __fdiv_rn((width * height) * a.k_omo, a.k_opo);
  const float r1 = __fdiv_rn(b1 + __fsqrt_rn(b1 * b1 - 4.0f * c1), 2.0f);
  const float b2 = 2.0f * (height + width);
  const float c2 = (a.k_omo * width) * height;
  const float r2 = __fdiv_rn(b2 + __fsqrt_rn(b2 * b2 - 16.0f * c2), 2.0f);
  const float b3 = a.k_b3 * (height + width);
  const float c3 = (a.k_om1 * width) * height;
  const float r3 = __fdiv_rn(b3 + __fsqrt_rn(b3 * b3 - a.k_a3x4 * c3), 2.0f);
  float r = r1;                                // Python min(): the first of the smallest
  if (r2 < r) r = r2;
  if (r3 < r) r = r3;
  return r;
}

__global__ void __launch_bounds__(kThreads) ch_assign_kernel(TargetArgs a) {
  const int b = blockIdx.x;
  const long long o0 = a.offsets[b], n = a.offsets[b + 1] - o0;
  __shared__ int drawn[OCRF_CH_MAX_TASKS];
  if (threadIdx.x < OCRF_CH_MAX_TASKS) drawn[threadIdx.x] = 0;
  for (long long i = threadIdx.x; i < (long long)a.T * a.M; i += kThreads) {
    const int t = (int)(i / a.M), k = (int)(i % a.M);
    const size_t row = ((size_t)t * a.B + b) * a.M + k;
    for (int c = 0; c < a.C; ++c) a.anno[row * a.C + c] = 0.0f;
    a.ind[row] = 0;
    a.mask[row] = 0;
  }
  __syncthreads();
  for (long long i = threadIdx.x; i < n; i += kThreads) {
    int t, c;
    lookup(a, a.labels[o0 + i], &t, &c);
    int4 r = make_int4(t, c, 0, -1);
    if (t >= 0) {
      long long k = 0;                         // slot: rank after the per-class torch.where + cat of the task
      for (long long j = 0; j < n; ++j) {
        int tj, cj;
        lookup(a, a.labels[o0 + j], &tj, &cj);
        k += (tj == t) && (cj < c || (cj == c && j < i));
      }
      const float* bx = a.boxes + (size_t)(o0 + i) * a.box_dim;
      const float width = __fdiv_rn(__fdiv_rn(bx[3], a.vs0), a.osf);
      const float length = __fdiv_rn(__fdiv_rn(bx[4], a.vs1), a.osf);
      if (k < a.M && width > 0.0f && length > 0.0f) {
        const float rf = gaussian_radius_f32(a, length, width);   // NaN (an infinite dimension) counts as 0
        const int radius = max(a.min_radius, rf == rf ? (int)fminf(rf, 65536.0f) : 0);
        const float cx = __fdiv_rn(__fdiv_rn(bx[0] - a.pc0, a.vs0), a.osf);
        const float cy = __fdiv_rn(__fdiv_rn(bx[1] - a.pc1, a.vs1), a.osf);
        const int ix = (int)cx, iy = (int)cy;  // .to(torch.int32): toward zero
        if (ix >= 0 && ix < a.W && iy >= 0 && iy < a.H) {
          r = make_int4(t, c, ix | (iy << 16), radius);
          const size_t row = ((size_t)t * a.B + b) * a.M + k;
          float* o = a.anno + row * a.C;
          o[0] = cx - (float)ix;
          o[1] = cy - (float)iy;
          o[2] = bx[2] + bx[5] * 0.5f;         // gravity centre
          for (int d = 0; d < 3; ++d) o[3 + d] = a.norm_bbox ? logf(bx[3 + d]) : bx[3 + d];
          o[6] = sinf(bx[6]);
          o[7] = cosf(bx[6]);
          if (a.with_vel) {
            o[8] = bx[7];
            o[9] = bx[8];
          }
          a.ind[row] = (long long)iy * a.W + ix;
          a.mask[row] = 1;
          atomicAdd(&drawn[t], 1);
        }
      }
    }
    a.rec[o0 + i] = r;
  }
  __syncthreads();
  if ((int)threadIdx.x < a.T && drawn[threadIdx.x]) atomicAdd(&a.counts[a.T + threadIdx.x], (float)drawn[threadIdx.x]);
}

// draw_heatmap_gaussian's value at offset (dx, dy) of radius r: numpy's float64 gaussian_2d, zeroed below eps * max
// (max = exp(0) = 1), then cast to float32
__device__ __forceinline__ float gauss_value(int r, int dx, int dy) {
  const double sigma = (double)(2 * r + 1) / 6.0;
  const double v = exp(-((double)dx * dx + (double)dy * dy) / (2.0 * sigma * sigma));
  return v < DBL_EPSILON ? 0.0f : (float)v;
}

__global__ void __launch_bounds__(kThreads) ch_heatmap_kernel(TargetArgs a) {
  const int plane = blockIdx.y, b = blockIdx.z;
  const int t = a.plane_task[plane], c = a.plane_cls[plane];
  const int HW = a.H * a.W;
  const int p = blockIdx.x * kThreads + threadIdx.x;
  const int py = p / a.W, px = p % a.W;
  const long long o0 = a.offsets[b], n = a.offsets[b + 1] - o0;
  __shared__ int4 objs[kThreads];
  __shared__ int n_objs;
  float v = 0.0f;
  for (long long base = 0; base < n; base += kThreads) {
    if (threadIdx.x == 0) n_objs = 0;
    __syncthreads();
    if (base + threadIdx.x < n) {
      const int4 r = a.rec[o0 + base + threadIdx.x];
      if (r.x == t && r.y == c && r.w >= 0) objs[atomicAdd(&n_objs, 1)] = r;
    }
    __syncthreads();
    const int m = n_objs;
    for (int j = 0; j < m; ++j) {
      const int4 r = objs[j];
      const int dx = px - (r.z & 0xffff), dy = py - (r.z >> 16);
      if (dx >= -r.w && dx <= r.w && dy >= -r.w && dy <= r.w) v = fmaxf(v, gauss_value(r.w, dx, dy));
    }
    __syncthreads();
  }
  const bool in = p < HW;
  if (in) a.heat[a.heat_off[t] + ((size_t)b * a.ncls[t] + c) * HW + p] = v;
  const int ones = __syncthreads_count(in && v == 1.0f);
  if (threadIdx.x == 0 && ones) atomicAdd(&a.counts[t], (float)ones);
}

// ------------------------------------------------------------------------------------------------ heatmap loss
struct HmArgs {
  int T, B, HW, n_blocks;
  int ncls[OCRF_CH_MAX_TASKS];
  int block0[OCRF_CH_MAX_TASKS + 1];          // first block of each task
  const float* logits[OCRF_CH_MAX_TASKS];
  const float* heat;                          // the targets' flat heatmap buffer
  long long heat_off[OCRF_CH_MAX_TASKS];
  float* clipped[OCRF_CH_MAX_TASKS];          // forward: clip_sigmoid outputs; backward: logit gradients
};

__device__ __forceinline__ int hm_task(const HmArgs& a, int blk) {
  int t = 0;
  while (t + 1 < a.T && blk >= a.block0[t + 1]) ++t;
  return t;
}

__device__ __forceinline__ float focal(float p, float g) {
  const float pos = g == 1.0f ? 1.0f : 0.0f;
  const float neg_w = powf(1.0f - g, 4.0f);
  const float q = 1.0f - p;
  const float pos_loss = -logf(p + 1e-12f) * (q * q) * pos;
  const float neg_loss = -logf(1.0f - p + 1e-12f) * (p * p) * neg_w;
  return pos_loss + neg_loss;
}

__device__ __forceinline__ float focal_grad(float p, float g) {
  const float pos = g == 1.0f ? 1.0f : 0.0f;
  const float neg_w = powf(1.0f - g, 4.0f);
  const float q = 1.0f - p, pe = p + 1e-12f, qe = 1.0f - p + 1e-12f;
  return pos * (-(q * q) / pe + 2.0f * q * logf(pe)) + neg_w * ((p * p) / qe - 2.0f * p * logf(qe));
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

template <typename T>
__device__ T block_sum(T v, T* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const T r = red[0];
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(kThreads) ch_hm_loss_partial_kernel(HmArgs a, float* partial) {
  __shared__ float red[kThreads];
  const int blk = blockIdx.x, t = hm_task(a, blk);
  const long long n = (long long)a.B * a.ncls[t] * a.HW;
  const long long e0 = (long long)(blk - a.block0[t]) * kHmChunk;
  const float* x = a.logits[t];
  const float* g = a.heat + a.heat_off[t];
  float acc = 0.0f;
  for (int i = threadIdx.x; i < kHmChunk; i += kThreads) {
    const long long e = e0 + i;
    if (e >= n) break;
    const float p = fminf(fmaxf(sigmoidf(x[e]), kClipLo), kClipHi);
    a.clipped[t][e] = p;
    acc += focal(p, g[e]);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) partial[blk] = acc;
}

// out[t] = w * sum_t / den_t, den_t = (float)(max(count_t, 1) + eps) as weight_reduce_loss's Python division
__global__ void __launch_bounds__(kThreads) ch_hm_loss_final_kernel(HmArgs a, const float* partial,
                                                                    const float* counts, float w, float* out,
                                                                    float* dens) {
  __shared__ float red[kThreads];
  for (int t = 0; t < a.T; ++t) {
    float acc = 0.0f;
    for (int i = a.block0[t] + threadIdx.x; i < a.block0[t + 1]; i += kThreads) acc += partial[i];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) {
      const float den = (float)((double)fmaxf(counts[t], 1.0f) + kF32Eps);
      out[t] = w * (acc / den);
      dens[t] = den;
    }
  }
}

__global__ void __launch_bounds__(kThreads) ch_hm_loss_backward_kernel(HmArgs a, const float* dens, const float* grad_out,
                                                                       float w) {
  const int blk = blockIdx.x, t = hm_task(a, blk);
  const long long n = (long long)a.B * a.ncls[t] * a.HW;
  const long long e0 = (long long)(blk - a.block0[t]) * kHmChunk;
  const float scale = (grad_out[t] * w) / dens[t];
  const float* x = a.logits[t];
  const float* g = a.heat + a.heat_off[t];
  float* gx = a.clipped[t];                   // the backward's table of logit gradients
  for (int i = threadIdx.x; i < kHmChunk; i += kThreads) {
    const long long e = e0 + i;
    if (e >= n) break;
    const float s = sigmoidf(x[e]);
    const float p = fminf(fmaxf(s, kClipLo), kClipHi);
    const float pass = (s >= kClipLo && s <= kClipHi) ? 1.0f : 0.0f;
    gx[e] = ((scale * focal_grad(p, g[e])) * pass) * ((1.0f - s) * s);
  }
}

// ------------------------------------------------------------------------------------------------ regression loss
struct RegArgs {
  int T, B, HW, M, C;
  const float* heads[OCRF_CH_MAX_TASKS][5];   // reg (B,2,HW), height (B,1,HW), dim (B,3,HW), rot (B,2,HW), vel (B,2,HW)
  const float* anno;                          // (T, B, M, C)
  const long long* ind;                       // (T, B, M)
  const unsigned char* mask;                  // (T, B, M)
  float code_w[10];
  float* grads[OCRF_CH_MAX_TASKS][5];         // backward: the same layout as heads
};

__constant__ int kCodeHead[10] = {0, 0, 1, 2, 2, 2, 3, 3, 4, 4};
__constant__ int kCodeChan[10] = {0, 1, 0, 0, 1, 2, 0, 1, 0, 1};
__constant__ int kCodeGroup[10] = {0, 0, 1, 2, 2, 2, 3, 3, 4, 4};
__constant__ int kHeadChans[5] = {2, 1, 3, 2, 2};

__device__ __forceinline__ float pred_at(const RegArgs& a, int t, int b, int c, long long idx) {
  return a.heads[t][kCodeHead[c]][((size_t)b * kHeadChans[kCodeHead[c]] + kCodeChan[c]) * a.HW + idx];
}

// weight of code c of a slot: mask * isnotnan(target) * code_weight, in the reference's order
__device__ __forceinline__ float reg_weight(const RegArgs& a, unsigned char m, float tgt, int c) {
  return ((float)m * (tgt == tgt ? 1.0f : 0.0f)) * a.code_w[c];
}

// block (t, b): partial[(t * B + b) * 6 + g] = sum of |pred - target| * weight over group g (g = 5: all codes)
__global__ void __launch_bounds__(kThreads) ch_reg_loss_partial_kernel(RegArgs a, float* partial) {
  __shared__ float red[kThreads];
  const int t = blockIdx.x, b = blockIdx.y;
  float acc[6] = {0, 0, 0, 0, 0, 0};
  const size_t row0 = ((size_t)t * a.B + b) * a.M;
  for (int k = threadIdx.x; k < a.M; k += kThreads) {
    const long long idx = a.ind[row0 + k];
    const unsigned char m = a.mask[row0 + k];
    for (int c = 0; c < a.C; ++c) {
      const float tgt = a.anno[(row0 + k) * a.C + c];
      const float l = fabsf(pred_at(a, t, b, c, idx) - tgt) * reg_weight(a, m, tgt, c);
      acc[kCodeGroup[c]] += l;
      acc[5] += l;
    }
  }
  for (int g = 0; g < 6; ++g) {
    const float s = block_sum(acc[g], red);
    if (threadIdx.x == 0) partial[((size_t)t * a.B + b) * 6 + g] = s;
  }
}

// out (T, 6): groups 0..4 divided by (num + 1e-4) + eps, 5 (all codes) by num + eps, num = max(mask count, 1e-4)
__global__ void ch_reg_loss_final_kernel(int T, int B, const float* partial, const float* counts, float w, float* out,
                                         float* dens) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const float num = fmaxf(counts[T + t], 1e-4f);
  const float den_ts = (float)(((double)num + 1e-4) + kF32Eps);
  const float den_all = (float)((double)num + kF32Eps);
  for (int g = 0; g < 6; ++g) {
    float s = 0.0f;
    for (int b = 0; b < B; ++b) s += partial[((size_t)t * B + b) * 6 + g];
    out[t * 6 + g] = w * (s / (g < 5 ? den_ts : den_all));
  }
  dens[2 * t] = den_ts;
  dens[2 * t + 1] = den_all;
}

// block (t, b): the slot holding the first occurrence of an index writes the sum, in slot order, of every slot's
// contribution at that index (the gradient buffers are zeroed by the caller)
__global__ void __launch_bounds__(kThreads) ch_reg_loss_backward_kernel(RegArgs a, const float* dens,
                                                                        const float* grad_out, float w) {
  extern __shared__ int s_ind[];
  const int t = blockIdx.x, b = blockIdx.y;
  const size_t row0 = ((size_t)t * a.B + b) * a.M;
  for (int k = threadIdx.x; k < a.M; k += kThreads) s_ind[k] = (int)a.ind[row0 + k];
  __syncthreads();
  float base_g[5];
  for (int g = 0; g < 5; ++g) base_g[g] = (grad_out[t * 6 + g] * w) / dens[2 * t];
  const float base_all = (grad_out[t * 6 + 5] * w) / dens[2 * t + 1];
  for (int k = threadIdx.x; k < a.M; k += kThreads) {
    const int idx = s_ind[k];
    bool first = true;
    for (int j = 0; j < k && first; ++j) first = s_ind[j] != idx;
    if (!first) continue;
    for (int c = 0; c < a.C; ++c) {
      const float p = pred_at(a, t, b, c, idx);
      float acc = 0.0f;
      for (int j = k; j < a.M; ++j) {
        if (s_ind[j] != idx) continue;
        const float tgt = a.anno[(row0 + j) * a.C + c];
        const float wt = reg_weight(a, a.mask[row0 + j], tgt, c);
        const float d = p - tgt;
        const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);   // sgn(NaN) = 0, as autograd's abs
        acc += (base_g[kCodeGroup[c]] * wt) * sg + (base_all * wt) * sg;
      }
      const int h = kCodeHead[c];
      a.grads[t][h][((size_t)b * kHeadChans[h] + kCodeChan[c]) * a.HW + idx] = acc;
    }
  }
}

bool fill_tasks(int T, const int* ncls, int B, int HW, int* out_ncls, long long* heat_off) {
  if (T < 1 || T > OCRF_CH_MAX_TASKS) return false;
  long long off = 0;
  for (int t = 0; t < T; ++t) {
    if (ncls[t] < 1) return false;
    out_ncls[t] = ncls[t];
    heat_off[t] = off;
    off += (long long)B * ncls[t] * HW;
  }
  return true;
}

}  // namespace

extern "C" {

size_t ocrf_center_head_targets_workspace_bytes(int n_boxes) { return (size_t)(n_boxes > 0 ? n_boxes : 1) * sizeof(int4); }

int ocrf_center_head_targets(int B, int T, const int* ncls, int n_labels, const int* class_table, int n_boxes,
                             int box_dim, const float* boxes, const long long* labels, const long long* offsets, int H,
                             int W, int max_objs, int with_velocity, int norm_bbox, const float* voxel_size,
                             const float* pc_range, int out_size_factor, double gaussian_overlap, int min_radius,
                             float* heatmap, float* anno_box, long long* ind, unsigned char* mask, float* counts,
                             void* workspace, size_t workspace_bytes, ocrf_stream_t stream) {
  if (B < 1 || H < 1 || W < 1 || H >= 32768 || W >= 32768 || max_objs < 1 || out_size_factor < 1 || n_boxes < 0 ||
      box_dim < (with_velocity ? 9 : 7) || n_labels < 1)
    return (int)hipErrorInvalidValue;
  if (workspace_bytes < ocrf_center_head_targets_workspace_bytes(n_boxes)) return (int)hipErrorInvalidValue;
  TargetArgs a{};
  if (!fill_tasks(T, ncls, B, H * W, a.ncls, a.heat_off)) return (int)hipErrorInvalidValue;
  int planes = 0;
  for (int t = 0; t < T; ++t)
    for (int c = 0; c < ncls[t]; ++c) {
      if (planes == OCRF_CH_MAX_PLANES) return (int)hipErrorInvalidValue;
      a.plane_task[planes] = t;
      a.plane_cls[planes++] = c;
    }
  const double o = gaussian_overlap;
  a.B = B; a.T = T; a.box_dim = box_dim; a.n_labels = n_labels; a.H = H; a.W = W; a.M = max_objs;
  a.C = with_velocity ? 10 : 8; a.with_vel = with_velocity; a.norm_bbox = norm_bbox; a.min_radius = min_radius;
  a.vs0 = voxel_size[0]; a.vs1 = voxel_size[1]; a.pc0 = pc_range[0]; a.pc1 = pc_range[1]; a.osf = (float)out_size_factor;
  a.k_omo = (float)(1.0 - o); a.k_opo = (float)(1.0 + o); a.k_om1 = (float)(o - 1.0);
  a.k_a3x4 = (float)(4.0 * (4.0 * o)); a.k_b3 = (float)(-2.0 * o);
  a.boxes = boxes; a.labels = labels; a.offsets = offsets; a.table = class_table;
  a.heat = heatmap; a.anno = anno_box; a.ind = ind; a.mask = mask; a.counts = counts; a.rec = (int4*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, sizeof(float) * 2 * T, s);
  if (e != hipSuccess) return (int)e;
  ocrf::launch(OCRF_K_CH_ASSIGN, ch_assign_kernel, dim3(B), dim3(kThreads), 0, s, a);
  ocrf::launch(OCRF_K_CH_HEATMAP, ch_heatmap_kernel, dim3((H * W + kThreads - 1) / kThreads, planes, B),
               dim3(kThreads), 0, s, a);
  return (int)hipGetLastError();
}

static bool fill_hm(HmArgs& a, int T, const int* ncls, int B, int HW, const float* const* logits, const float* heat,
                    float* const* clipped) {
  if (B < 1 || HW < 1 || !fill_tasks(T, ncls, B, HW, a.ncls, a.heat_off)) return false;
  a.T = T; a.B = B; a.HW = HW; a.heat = heat;
  int blocks = 0;
  for (int t = 0; t < T; ++t) {
    a.block0[t] = blocks;
    a.logits[t] = logits[t];
    a.clipped[t] = clipped ? clipped[t] : nullptr;
    blocks += (int)(((long long)B * ncls[t] * HW + kHmChunk - 1) / kHmChunk);
  }
  a.block0[T] = blocks;
  a.n_blocks = blocks;
  return true;
}

size_t ocrf_center_head_heatmap_loss_workspace_bytes(int B, int T, const int* ncls, int HW) {
  size_t blocks = 0;
  for (int t = 0; t < T; ++t) blocks += ((size_t)B * ncls[t] * HW + kHmChunk - 1) / kHmChunk;
  return (blocks > 0 ? blocks : 1) * sizeof(float);
}

int ocrf_center_head_heatmap_loss(int B, int T, const int* ncls, int HW, const float* const* logits,
                                  const float* heatmap, const float* counts, float loss_weight, float* const* clipped,
                                  float* out, float* dens, void* workspace, size_t workspace_bytes,
                                  ocrf_stream_t stream) {
  HmArgs a{};
  if (!fill_hm(a, T, ncls, B, HW, logits, heatmap, clipped)) return (int)hipErrorInvalidValue;
  if (workspace_bytes < ocrf_center_head_heatmap_loss_workspace_bytes(B, T, ncls, HW)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  float* partial = (float*)workspace;
  ocrf::launch(OCRF_K_CH_HM_LOSS, ch_hm_loss_partial_kernel, dim3(a.n_blocks), dim3(kThreads), 0, s, a, partial);
  ocrf::launch(OCRF_K_CH_FINAL, ch_hm_loss_final_kernel, dim3(1), dim3(kThreads), 0, s, a, (const float*)partial,
               counts, loss_weight, out, dens);
  return (int)hipGetLastError();
}

int ocrf_center_head_heatmap_loss_backward(int B, int T, const int* ncls, int HW, const float* const* logits,
                                           const float* heatmap, const float* dens, const float* grad_out,
                                           float loss_weight, float* const* grad_logits, ocrf_stream_t stream) {
  HmArgs a{};
  if (!grad_logits || !fill_hm(a, T, ncls, B, HW, logits, heatmap, grad_logits)) return (int)hipErrorInvalidValue;
  ocrf::launch(OCRF_K_CH_HM_LOSS_BWD, ch_hm_loss_backward_kernel, dim3(a.n_blocks), dim3(kThreads), 0,
               (hipStream_t)stream, a, dens, grad_out, loss_weight);
  return (int)hipGetLastError();
}

static bool fill_reg(RegArgs& a, int B, int T, int HW, int max_objs, int with_velocity, const float* const* heads,
                     const float* anno_box, const long long* ind, const unsigned char* mask, const float* code_weights) {
  if (B < 1 || T < 1 || T > OCRF_CH_MAX_TASKS || HW < 1 || max_objs < 1) return false;
  a.T = T; a.B = B; a.HW = HW; a.M = max_objs; a.C = with_velocity ? 10 : 8;
  for (int t = 0; t < T; ++t)
    for (int h = 0; h < 5; ++h) a.heads[t][h] = heads[t * 5 + h];
  for (int c = 0; c < a.C; ++c) a.code_w[c] = code_weights[c];
  a.anno = anno_box; a.ind = ind; a.mask = mask;
  return true;
}

size_t ocrf_center_head_reg_loss_workspace_bytes(int B, int T) { return (size_t)B * T * 6 * sizeof(float); }

int ocrf_center_head_reg_loss(int B, int T, int HW, int max_objs, int with_velocity, const float* const* heads,
                              const float* anno_box, const long long* ind, const unsigned char* mask,
                              const float* code_weights, const float* counts, float loss_weight, float* out,
                              float* dens, void* workspace, size_t workspace_bytes, ocrf_stream_t stream) {
  RegArgs a{};
  if (!fill_reg(a, B, T, HW, max_objs, with_velocity, heads, anno_box, ind, mask, code_weights))
    return (int)hipErrorInvalidValue;
  if (workspace_bytes < ocrf_center_head_reg_loss_workspace_bytes(B, T)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  float* partial = (float*)workspace;
  ocrf::launch(OCRF_K_CH_REG_LOSS, ch_reg_loss_partial_kernel, dim3(T, B), dim3(kThreads), 0, s, a, partial);
  ocrf::launch(OCRF_K_CH_FINAL, ch_reg_loss_final_kernel, dim3(1), dim3(64), 0, s, T, B, (const float*)partial, counts,
               loss_weight, out, dens);
  return (int)hipGetLastError();
}

int ocrf_center_head_reg_loss_backward(int B, int T, int HW, int max_objs, int with_velocity,
                                       const float* const* heads, const float* anno_box, const long long* ind,
                                       const unsigned char* mask, const float* code_weights, const float* dens,
                                       const float* grad_out, float loss_weight, float* const* grad_heads,
                                       ocrf_stream_t stream) {
  RegArgs a{};
  if (!grad_heads || !fill_reg(a, B, T, HW, max_objs, with_velocity, heads, anno_box, ind, mask, code_weights))
    return (int)hipErrorInvalidValue;
  if ((size_t)max_objs * sizeof(int) > 64 * 1024) return (int)hipErrorInvalidValue;
  for (int t = 0; t < T; ++t)
    for (int h = 0; h < 5; ++h) a.grads[t][h] = grad_heads[t * 5 + h];
  ocrf::launch(OCRF_K_CH_REG_LOSS_BWD, ch_reg_loss_backward_kernel, dim3(T, B), dim3(kThreads),
               (size_t)max_objs * sizeof(int), (hipStream_t)stream, a, dens, grad_out, loss_weight);
  return (int)hipGetLastError();
}

}  // extern "C"
