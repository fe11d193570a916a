// Test-time decode and NMS of the detection head (mmdet3d/models/dense_heads/centerpoint_head.py CenterHead.get_bboxes
// :670-763 and get_task_detections :765-898; core/bbox/coders/centerpoint_bbox_coders.py decode; core/post_processing/
// box3d_nms.py circle_nms and nms_bev with mmcv's nms_rotated).  Every sample and task in one call, four launches, no
// memset, no atomics on results and nothing read back to the host:
//
//   select  one 1024-thread block per (task, sample): a radix select (four 8-bit passes, LDS histogram) finds the K-th
//           largest sigmoid key over the task's ncls * H * W cells; the keys above it and the first of those equal to it
//           in (class, cell) order are compacted into LDS and bitonic-sorted by (score desc, index asc).  The same
//           block decodes its K boxes, applies the coder's and the test cfg's score and range filters, the
//           nms_rescale_factor and the xywhr -> xyxyr -> xywhr round trip, and writes the survivors in order, cut
//           to pre_max_size (rotate tasks), as the task's NMS candidates;
//   mask    one wave per (64-row block, 64-column block, task, sample), upper triangle only: bit j of row i is set when
//           candidate i suppresses j (rotated IoU > nms_thr, or squared centre distance <= min_radius for circle
//           tasks).  The IoU is float64 polygon clipping; disjoint enclosing circles skip it (exactly 0);
//   scan    one wave per (task, sample): the greedy scan over the mask rows (in LDS up to 64 KB), stopping at
//           post_max_size kept boxes;
//   write   one block per sample: the tasks' kept boxes in task order, the rotate tasks' post_center_limit_range
//           filter, z -= dz / 2, the class offsets; rows past the count are zeroed.
//
// bfloat16 heads (ocrf_center_decode_bf16: a head under bf16 autocast, read in place).  Only the select kernel reads the
// heads: the heatmap in the four radix passes and the compaction, and reg, height, dim, rot, vel at the K selected cells.
// It is a template on the element type; the bf16 form widens each load to float32 (a shift: exact) and everything after
// the load is the float32 code, so the four results are bit-equal to the float32 call on the widened heads.  bf16
// scores tie often.  Nothing is needed for that: the order (score descending, then (class, cell) index ascending, the
// first `remain` keys equal to the K-th in index order) already decides every tie, and it does not depend on how many
// keys are equal.  mask, scan and write read the workspace only and are shared.
#include <hip/hip_runtime.h>

#include <cmath>

#include "launch.h"
#include "ocrf_hip.h"
#include "plane_walk.h"

namespace {

using plane::bf16_t;
using plane::load_f32;

constexpr int kSelThreads = 1024;
constexpr int kMaxK = OCRF_CD_MAX_NUM;
constexpr int kWriteThreads = 256;
constexpr int kScanLdsBytes = 64 * 1024;

struct DecodeArgs {
  int B, T, H, W, K, pre_max, post_max, C, with_vel, norm_bbox, nw, M;
  float osf, vs0, vs1, pc0, pc1;
  int has_coder_thr, has_center_range, has_score_thr, has_limit_range;
  float coder_thr, score_thr;
  float center_range[6], limit_range[6];
  int ncls[OCRF_CD_MAX_TASKS], cls_off[OCRF_CD_MAX_TASKS], circle[OCRF_CD_MAX_TASKS];
  double thr[OCRF_CD_MAX_TASKS];
  float factor[OCRF_CD_MAX_TASKS][OCRF_CD_MAX_CLASSES];
  const void* heads[OCRF_CD_MAX_TASKS][6];    // heatmap logits, reg, height, dim, rot, vel: float or bf16_t (select)
  float* cand_row;                            // (B*T, K, 9): the decoded row with its final dims
  float* cand_bev;                            // (B*T, K, 5): the NMS box after the round trip
  float* cand_score;
  int* cand_label;                            // class in task
  int* ncand;                                 // (B*T)
  unsigned long long* mask;                   // (B*T, K, nw)
  int* keep;                                  // (B*T, post_max)
  int* nkeep;                                 // (B*T)
  float* boxes;
  float* scores;
  int* labels;
  int* counts;
};

__device__ __forceinline__ float sigmoid_key(float x) { return 1.0f / (1.0f + expf(-x)); }

// Exclusive prefix of `flag` over the block (blockDim.x a multiple of 64, at most 1024); *total = the block's sum.
__device__ int block_exclusive_scan(bool flag, int* total, int* s_wave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const unsigned long long bal = __ballot(flag);
  const int in_wave = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) s_wave[wave] = __popcll(bal);
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < waves; ++w) {
    const int c = s_wave[w];
    before += (w < wave) ? c : 0;
    all += c;
  }
  __syncthreads();
  *total = all;
  return before + in_wave;
}

// --------------------------------------------------------------------------------------------- rotated IoU
// The one place that fixes the rotation sense: corners c + R(a) (+-w/2, +-h/2), R counter-clockwise in x-right / y-up
// coordinates, listed counter-clockwise.  Mirrored by center_decode.py box_corners.
__device__ void box_corners(double cx, double cy, double w, double h, double a, double* px, double* py) {
  const double c = cos(a), s = sin(a);
  const double lx[4] = {-0.5 * w, 0.5 * w, 0.5 * w, -0.5 * w};
  const double ly[4] = {-0.5 * h, -0.5 * h, 0.5 * h, 0.5 * h};
  for (int k = 0; k < 4; ++k) {
    px[k] = cx + (c * lx[k] - s * ly[k]);
    py[k] = cy + (s * lx[k] + c * ly[k]);
  }
}

constexpr int kPolyCap = 12;

// mmcv's single_box_iou_rotated: intersection over area1 + area2 - inter, 0 when an area is below 1e-14, centres
// shifted to their mean.  Intersection by Sutherland-Hodgman clipping of box a by the four edges of box b.
__device__ double iou_rotated(const float* a, const float* b) {
  const double area_a = (double)a[2] * (double)a[3], area_b = (double)b[2] * (double)b[3];
  if (area_a < 1e-14 || area_b < 1e-14) return 0.0;
  const double sx = 0.5 * ((double)a[0] + (double)b[0]), sy = 0.5 * ((double)a[1] + (double)b[1]);
  double ax[4], ay[4], bx[4], by[4];
  box_corners((double)a[0] - sx, (double)a[1] - sy, a[2], a[3], a[4], ax, ay);
  box_corners((double)b[0] - sx, (double)b[1] - sy, b[2], b[3], b[4], bx, by);
  double px[kPolyCap], py[kPolyCap], qx[kPolyCap], qy[kPolyCap];
  int n = 4;
  for (int k = 0; k < 4; ++k) {
    px[k] = ax[k];
    py[k] = ay[k];
  }
  for (int e = 0; e < 4 && n > 0; ++e) {
    const double ex = bx[(e + 1) & 3] - bx[e], ey = by[(e + 1) & 3] - by[e];
    int m = 0;
    double prx = px[n - 1], pry = py[n - 1];
    double dp = ex * (pry - by[e]) - ey * (prx - bx[e]);
    for (int k = 0; k < n; ++k) {
      const double cx = px[k], cy = py[k];
      const double dc = ex * (cy - by[e]) - ey * (cx - bx[e]);
      if ((dc >= 0.0) != (dp >= 0.0) && m < kPolyCap) {
        const double t = dp / (dp - dc);
        qx[m] = prx + t * (cx - prx);
        qy[m] = pry + t * (cy - pry);
        ++m;
      }
      if (dc >= 0.0 && m < kPolyCap) {
        qx[m] = cx;
        qy[m] = cy;
        ++m;
      }
      prx = cx;
      pry = cy;
      dp = dc;
    }
    n = m;
    for (int k = 0; k < n; ++k) {
      px[k] = qx[k];
      py[k] = qy[k];
    }
  }
  double s2 = 0.0;
  for (int k = 0; k < n; ++k) {
    const int k1 = (k + 1 == n) ? 0 : k + 1;
    s2 += px[k] * py[k1] - px[k1] * py[k];
  }
  const double inter = n >= 3 ? fabs(0.5 * s2) : 0.0;
  return inter / (area_a + area_b - inter);
}

// --------------------------------------------------------------------------------------------- select + decode
// T: float or bf16_t, the element of the heads; every head value enters through load_f32
template <typename T>
__global__ void __launch_bounds__(kSelThreads) cd_select_kernel(DecodeArgs a) {
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int bt = b * a.T + t;
  const int HW = a.H * a.W, ncls = a.ncls[t], N = ncls * HW, K = a.K;
  const T* hm = static_cast<const T*>(a.heads[t][0]) + (size_t)b * N;
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_remain;
  __shared__ int s_wave[16];
  __shared__ unsigned long long comp[kMaxK];

  // K-th largest key, most significant byte first
  unsigned prefix = 0, pmask = 0, remain = (unsigned)K;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += kSelThreads) {
      const unsigned key = __float_as_uint(sigmoid_key(load_f32(hm + i)));
      if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned acc = 0;
      for (int d = 255; d >= 0; --d) {
        if (acc + hist[d] >= remain) {
          prefix |= (unsigned)d << shift;
          remain -= acc;
          break;
        }
        acc += hist[d];
      }
      s_prefix = prefix;
      s_remain = remain;
    }
    __syncthreads();
    prefix = s_prefix;
    remain = s_remain;
    pmask |= 255u << shift;
  }
  // keys above the threshold (exactly K - remain of them) go to [0, K - remain) in any order, the first `remain` equal
  // to it in index order to [K - remain, K)
  const unsigned v = prefix, need_eq = remain, n_gt = (unsigned)K - remain;
  __shared__ unsigned s_gt;
  if (tid == 0) s_gt = 0;
  const int P2 = K <= 1 ? 1 : 1 << (32 - __clz(K - 1));
  for (int i = tid; i < P2; i += kSelThreads) comp[i] = 0ull;
  __syncthreads();
  int eq_base = 0;
  for (int base = 0; base < N; base += kSelThreads) {
    const int i = base + tid;
    const unsigned key = i < N ? __float_as_uint(sigmoid_key(load_f32(hm + i))) : 0u;
    const unsigned long long c = ((unsigned long long)key << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
    if (i < N && key > v) comp[atomicAdd(&s_gt, 1u)] = c;
    int total;
    const int r = block_exclusive_scan(i < N && key == v, &total, s_wave);
    if (i < N && key == v && eq_base + r < (int)need_eq) comp[n_gt + eq_base + r] = c;
    eq_base += total;
  }
  __syncthreads();
  // bitonic sort, descending by (key, -index)
  for (int k = 2; k <= P2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P2; i += kSelThreads) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long x = comp[i], y = comp[ixj];
          if (((i & k) == 0) ? (x < y) : (x > y)) {
            comp[i] = y;
            comp[ixj] = x;
          }
        }
      }
      __syncthreads();
    }
  }
  // decode, filter, compact in order
  bool pass = false;
  float row[9], bev[5], score = 0.0f;
  int cls = 0;
  if (tid < K) {
    const unsigned long long c = comp[tid];
    const unsigned idx = 0xFFFFFFFFu - (unsigned)(c & 0xFFFFFFFFull);
    score = __uint_as_float((unsigned)(c >> 32));
    cls = (int)(idx / (unsigned)HW);
    const int cell = (int)(idx % (unsigned)HW);
    const T* reg = static_cast<const T*>(a.heads[t][1]) + (size_t)b * 2 * HW;
    const T* hei = static_cast<const T*>(a.heads[t][2]) + (size_t)b * HW;
    const T* dim = static_cast<const T*>(a.heads[t][3]) + (size_t)b * 3 * HW;
    const T* rot = static_cast<const T*>(a.heads[t][4]) + (size_t)b * 2 * HW;
    float xs = (float)(cell % a.W) + load_f32(reg + cell);
    float ys = (float)(cell / a.W) + load_f32(reg + HW + cell);
    xs = xs * a.osf;
    xs = xs * a.vs0;
    xs = xs + a.pc0;
    ys = ys * a.osf;
    ys = ys * a.vs1;
    ys = ys + a.pc1;
    row[0] = xs;
    row[1] = ys;
    row[2] = load_f32(hei + cell);
    for (int k = 0; k < 3; ++k) {
      const float d = load_f32(dim + k * HW + cell);
      row[3 + k] = a.norm_bbox ? expf(d) : d;
    }
    row[6] = atan2f(load_f32(rot + cell), load_f32(rot + HW + cell));
    if (a.with_vel) {
      const T* vel = static_cast<const T*>(a.heads[t][5]) + (size_t)b * 2 * HW;
      row[7] = load_f32(vel + cell);
      row[8] = load_f32(vel + HW + cell);
    } else {
      row[7] = row[8] = 0.0f;
    }
    pass = true;
    if (a.has_coder_thr) pass = pass && score > a.coder_thr;
    if (a.has_center_range)
      for (int k = 0; k < 3; ++k) pass = pass && row[k] >= a.center_range[k] && row[k] <= a.center_range[3 + k];
    if (a.circle[t]) {
      bev[0] = row[0];
      bev[1] = row[1];
      bev[2] = bev[3] = bev[4] = 0.0f;
    } else {
      if (a.has_score_thr) pass = pass && score >= a.score_thr;
      const float f = a.factor[t][cls < OCRF_CD_MAX_CLASSES ? cls : 0];
      float ds[3];
      for (int k = 0; k < 3; ++k) ds[k] = row[3 + k] * f;
      // xywhr2xyxyr and back, as nms_bev
      const float hw = ds[0] / 2.0f, hh = ds[1] / 2.0f;
      const float x1 = row[0] - hw, y1 = row[1] - hh, x2 = row[0] + hw, y2 = row[1] + hh;
      bev[0] = (x1 + x2) / 2.0f;
      bev[1] = (y1 + y2) / 2.0f;
      bev[2] = x2 - x1;
      bev[3] = y2 - y1;
      bev[4] = row[6];
      for (int k = 0; k < 3; ++k) row[3 + k] = ds[k] / f;
    }
  }
  int total;
  const int pos = block_exclusive_scan(pass, &total, s_wave);
  const int cut = a.circle[t] ? K : min(K, a.pre_max);
  if (pass && pos < cut) {
    const size_t o = (size_t)bt * K + pos;
    for (int k = 0; k < 9; ++k) a.cand_row[o * 9 + k] = row[k];
    for (int k = 0; k < 5; ++k) a.cand_bev[o * 5 + k] = bev[k];
    a.cand_score[o] = score;
    a.cand_label[o] = cls;
  }
  if (tid == 0) a.ncand[bt] = min(total, cut);
}

// --------------------------------------------------------------------------------------------- suppression mask
__global__ void __launch_bounds__(64) cd_mask_kernel(DecodeArgs a) {
  const int cb = blockIdx.x, rb = blockIdx.y, bt = blockIdx.z, t = bt % a.T, lane = threadIdx.x;
  const int n = a.ncand[bt];
  if (cb < rb || rb * 64 >= n) return;
  __shared__ float col[64][5];
  const int jl = cb * 64 + lane;
  if (jl < n)
    for (int k = 0; k < 5; ++k) col[lane][k] = a.cand_bev[((size_t)bt * a.K + jl) * 5 + k];
  __syncthreads();
  const int i = rb * 64 + lane;
  if (i >= n) return;
  float me[5];
  for (int k = 0; k < 5; ++k) me[k] = a.cand_bev[((size_t)bt * a.K + i) * 5 + k];
  const double thr = a.thr[t];
  const bool circle = a.circle[t] != 0;
  // enclosing-circle radius of this box, and a relative margin so that the skip is conservative
  const double ri = 0.5 * sqrt((double)me[2] * me[2] + (double)me[3] * me[3]);
  unsigned long long bits = 0;
  for (int jj = 0; jj < 64; ++jj) {
    const int j = cb * 64 + jj;
    if (j >= n) break;
    if (j <= i) continue;
    bool sup;
    if (circle) {
      const float dx = me[0] - col[jj][0], dy = me[1] - col[jj][1];
      const float d2 = dx * dx + dy * dy;
      sup = (double)d2 <= thr;
    } else {
      const double dx = (double)me[0] - col[jj][0], dy = (double)me[1] - col[jj][1];
      const double rj = 0.5 * sqrt((double)col[jj][2] * col[jj][2] + (double)col[jj][3] * col[jj][3]);
      const double rr = (ri + rj) * (1.0 + 1e-9) + 1e-9;
      sup = (dx * dx + dy * dy <= rr * rr) && iou_rotated(me, col[jj]) > thr;
    }
    if (sup) bits |= 1ull << jj;
  }
  a.mask[((size_t)bt * a.K + i) * a.nw + cb] = bits;
}

// --------------------------------------------------------------------------------------------- greedy scan
__global__ void __launch_bounds__(64) cd_scan_kernel(DecodeArgs a) {
  extern __shared__ unsigned long long rows[];
  const int bt = blockIdx.x, lane = threadIdx.x;
  const int n = a.ncand[bt], nwn = (n + 63) / 64, nw = a.nw;
  const unsigned long long* g = a.mask + (size_t)bt * a.K * nw;
  const int lds_rows = min(n, kScanLdsBytes / (8 * nw));
  for (int e = lane; e < lds_rows * nw; e += 64) {
    const int w = e % nw;
    if (w >= (e / nw) / 64) rows[e] = g[e];     // words left of the diagonal were never written
  }
  __syncthreads();
  unsigned long long removed = 0;
  int kept = 0;
  for (int i = 0; i < n && kept < a.post_max; ++i) {
    const unsigned long long word = __shfl(removed, i >> 6);
    if ((word >> (i & 63)) & 1ull) continue;
    if (lane == 0) a.keep[(size_t)bt * a.post_max + kept] = i;
    ++kept;
    if (lane < nwn && lane >= (i >> 6)) removed |= (i < lds_rows ? rows[(size_t)i * nw + lane] : g[(size_t)i * nw + lane]);
  }
  if (lane == 0) a.nkeep[bt] = kept;
}

// --------------------------------------------------------------------------------------------- merge
__global__ void __launch_bounds__(kWriteThreads) cd_write_kernel(DecodeArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, C = a.C;
  __shared__ int s_wave[16];
  int base = 0;
  for (int t = 0; t < a.T; ++t) {
    const int bt = b * a.T + t, nk = a.nkeep[bt];
    for (int c0 = 0; c0 < nk; c0 += kWriteThreads) {
      const int r = c0 + tid;
      const float* row = nullptr;
      size_t o = 0;
      bool pass = false;
      if (r < nk) {
        o = (size_t)bt * a.K + a.keep[(size_t)bt * a.post_max + r];
        row = a.cand_row + o * 9;
        pass = true;
        if (!a.circle[t] && a.has_limit_range)
          for (int k = 0; k < 3; ++k) pass = pass && row[k] >= a.limit_range[k] && row[k] <= a.limit_range[3 + k];
      }
      int total;
      const int pos = base + block_exclusive_scan(pass, &total, s_wave);
      if (pass) {
        float* dst = a.boxes + ((size_t)b * a.M + pos) * C;
        for (int k = 0; k < C; ++k) dst[k] = row[k];
        dst[2] = row[2] - row[5] * 0.5f;
        a.scores[(size_t)b * a.M + pos] = a.cand_score[o];
        a.labels[(size_t)b * a.M + pos] = a.cand_label[o] + a.cls_off[t];
      }
      base += total;
    }
  }
  for (int r = base + tid; r < a.M; r += kWriteThreads) {
    for (int k = 0; k < C; ++k) a.boxes[((size_t)b * a.M + r) * C + k] = 0.0f;
    a.scores[(size_t)b * a.M + r] = 0.0f;
    a.labels[(size_t)b * a.M + r] = 0;
  }
  if (tid == 0) a.counts[b] = base;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Layout {
  size_t row, bev, score, label, ncand, mask, keep, nkeep, total;
};

Layout layout(int B, int T, int K, int post_max) {
  const size_t bt = (size_t)B * T, nw = (size_t)(K + 63) / 64;
  Layout l;
  size_t o = 0;
  l.row = o;
  o += align256(bt * K * 9 * sizeof(float));
  l.bev = o;
  o += align256(bt * K * 5 * sizeof(float));
  l.score = o;
  o += align256(bt * K * sizeof(float));
  l.label = o;
  o += align256(bt * K * sizeof(int));
  l.ncand = o;
  o += align256(bt * sizeof(int));
  l.mask = o;
  o += align256(bt * K * nw * sizeof(unsigned long long));
  l.keep = o;
  o += align256(bt * (size_t)(post_max > 0 ? post_max : 1) * sizeof(int));
  l.nkeep = o;
  o += align256(bt * sizeof(int));
  l.total = o;
  return l;
}

// E: the element of the heads; select_id: the kernel id its select launch reports under
template <typename E>
int center_decode(int select_id, int B, int T, const int* ncls, int H, int W, const E* const* heads, int with_velocity,
                  int norm_bbox, int max_num, int pre_max_size, int post_max_size, float out_size_factor,
                  const float* voxel_size, const float* pc_range, int has_coder_score_threshold,
                  float coder_score_threshold, const float* post_center_range, int has_score_threshold,
                  float score_threshold, const float* post_center_limit_range, const int* nms_circle,
                  const double* nms_threshold, const float* rescale_factor, float* boxes, float* scores, int* labels,
                  int* counts, void* workspace, size_t workspace_bytes, ocrf_stream_t stream) {
  if (B <= 0 || T <= 0 || T > OCRF_CD_MAX_TASKS || H <= 0 || W <= 0 || max_num <= 0 || max_num > kMaxK ||
      max_num > H * W || pre_max_size <= 0 || post_max_size <= 0 || !heads || !ncls || !boxes || !scores ||
      !labels || !counts)
    return (int)hipErrorInvalidValue;
  if (workspace_bytes < layout(B, T, max_num, post_max_size).total || !workspace)
    return (int)hipErrorInvalidValue;
  DecodeArgs a{};
  a.B = B;
  a.T = T;
  a.H = H;
  a.W = W;
  a.K = max_num;
  a.pre_max = pre_max_size;
  a.post_max = post_max_size;
  a.C = with_velocity ? 9 : 7;
  a.with_vel = with_velocity;
  a.norm_bbox = norm_bbox;
  a.nw = (max_num + 63) / 64;
  a.M = T * post_max_size;
  a.osf = out_size_factor;
  a.vs0 = voxel_size[0];
  a.vs1 = voxel_size[1];
  a.pc0 = pc_range[0];
  a.pc1 = pc_range[1];
  a.has_coder_thr = has_coder_score_threshold;
  a.coder_thr = coder_score_threshold;
  a.has_center_range = post_center_range != nullptr;
  a.has_score_thr = has_score_threshold;
  a.score_thr = score_threshold;
  a.has_limit_range = post_center_limit_range != nullptr;
  for (int k = 0; k < 6; ++k) {
    a.center_range[k] = post_center_range ? post_center_range[k] : 0.0f;
    a.limit_range[k] = post_center_limit_range ? post_center_limit_range[k] : 0.0f;
  }
  int off = 0;
  for (int t = 0; t < T; ++t) {
    if (ncls[t] <= 0 || ncls[t] > OCRF_CD_MAX_CLASSES || (long long)ncls[t] * H * W >= 0x7FFFFFFFLL)
      return (int)hipErrorInvalidValue;
    a.ncls[t] = ncls[t];
    a.cls_off[t] = off;
    off += ncls[t];
    a.circle[t] = nms_circle[t];
    a.thr[t] = nms_threshold[t];
    for (int c = 0; c < OCRF_CD_MAX_CLASSES; ++c) a.factor[t][c] = rescale_factor[t * OCRF_CD_MAX_CLASSES + c];
    for (int h = 0; h < 6; ++h) {
      a.heads[t][h] = heads[t * 6 + h];
      if (!a.heads[t][h] && (h < 5 || with_velocity)) return (int)hipErrorInvalidValue;
    }
  }
  const Layout l = layout(B, T, max_num, post_max_size);
  char* ws = (char*)workspace;
  a.cand_row = (float*)(ws + l.row);
  a.cand_bev = (float*)(ws + l.bev);
  a.cand_score = (float*)(ws + l.score);
  a.cand_label = (int*)(ws + l.label);
  a.ncand = (int*)(ws + l.ncand);
  a.mask = (unsigned long long*)(ws + l.mask);
  a.keep = (int*)(ws + l.keep);
  a.nkeep = (int*)(ws + l.nkeep);
  a.boxes = boxes;
  a.scores = scores;
  a.labels = labels;
  a.counts = counts;
  hipStream_t s = (hipStream_t)stream;
  ocrf::launch(select_id, cd_select_kernel<E>, dim3(T, B), dim3(kSelThreads), 0, s, a);
  ocrf::launch(OCRF_K_CD_MASK, cd_mask_kernel, dim3(a.nw, a.nw, B * T), dim3(64), 0, s, a);
  const size_t lds = (size_t)std::min(max_num, kScanLdsBytes / (8 * a.nw)) * a.nw * 8;
  ocrf::launch(OCRF_K_CD_SCAN, cd_scan_kernel, dim3(B * T), dim3(64), lds, s, a);
  ocrf::launch(OCRF_K_CD_WRITE, cd_write_kernel, dim3(B), dim3(kWriteThreads), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t ocrf_center_decode_workspace_bytes(int B, int T, int max_num, int post_max_size) {
  if (B <= 0 || T <= 0 || max_num <= 0) return 0;
  return layout(B, T, max_num, post_max_size).total;
}

int ocrf_center_decode(int B, int T, const int* ncls, int H, int W, const float* const* heads, int with_velocity,
                       int norm_bbox, int max_num, int pre_max_size, int post_max_size, float out_size_factor,
                       const float* voxel_size, const float* pc_range, int has_coder_score_threshold,
                       float coder_score_threshold, const float* post_center_range, int has_score_threshold,
                       float score_threshold, const float* post_center_limit_range, const int* nms_circle,
                       const double* nms_threshold, const float* rescale_factor, float* boxes, float* scores,
                       int* labels, int* counts, void* workspace, size_t workspace_bytes, ocrf_stream_t stream) {
  return center_decode(OCRF_K_CD_SELECT, B, T, ncls, H, W, heads, with_velocity, norm_bbox, max_num, pre_max_size,
                       post_max_size, out_size_factor, voxel_size, pc_range, has_coder_score_threshold,
                       coder_score_threshold, post_center_range, has_score_threshold, score_threshold,
                       post_center_limit_range, nms_circle, nms_threshold, rescale_factor, boxes, scores, labels, counts,
                       workspace, workspace_bytes, stream);
}

int ocrf_center_decode_bf16(int B, int T, const int* ncls, int H, int W, const unsigned short* const* heads,
                            int with_velocity, int norm_bbox, int max_num, int pre_max_size, int post_max_size,
                            float out_size_factor, const float* voxel_size, const float* pc_range,
                            int has_coder_score_threshold, float coder_score_threshold, const float* post_center_range,
                            int has_score_threshold, float score_threshold, const float* post_center_limit_range,
                            const int* nms_circle, const double* nms_threshold, const float* rescale_factor,
                            float* boxes, float* scores, int* labels, int* counts, void* workspace,
                            size_t workspace_bytes, ocrf_stream_t stream) {
  return center_decode(OCRF_K_CD_SELECT_BF16, B, T, ncls, H, W, heads, with_velocity, norm_bbox, max_num, pre_max_size,
                       post_max_size, out_size_factor, voxel_size, pc_range, has_coder_score_threshold,
                       coder_score_threshold, post_center_range, has_score_threshold, score_threshold,
                       post_center_limit_range, nms_circle, nms_threshold, rescale_factor, boxes, scores, labels, counts,
                       workspace, workspace_bytes, stream);
}

}  // extern "C"
