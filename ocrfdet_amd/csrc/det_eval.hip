// nuScenes detection metrics on the device (ocrf_det_eval_match, ocrf_det_eval_summary; the rules are stated in
// include/ocrf_hip.h, ocrfdet_amd/detection_eval.py is the caller).
//
// A prediction can only match a ground-truth box of its own sample and class, so the benchmark's greedy matching "in
// descending confidence over the whole split" is a set of independent greedy matchings per (sample, class, threshold):
// the shape of track_assoc.hip.  ocrf_det_eval_match, ONE launch per batch, one workgroup per sample, one wavefront per
// class (classes go round-robin over the waves when there are fewer waves):
//
//   1. all threads: per row and per ground-truth box the evaluated test and the class into LDS, a row's centre and
//      score key too.
//   2. wave c, alone: counts its class's rows and boxes (ballot passes), barrier, and with the counts of the classes
//      before it as its offsets gathers the rows in row order and the boxes in index order into LDS.  Every lane then
//      ranks its rows among the class's ((key, list position) pairs below its own: descending score, ties to the lowest
//      row) and stores them at their rank.  Four greedy loops, one per threshold: the rows in rank order, every lane
//      walks the class's unclaimed boxes lane, lane + 64, ..., keeps its smallest d2 (first wins: lowest index), six
//      xor-shuffles reduce (d2, list position) to the wave's argmin with ties to the lower position, and lane 0 claims
//      the box when d2 < t t.  No workgroup barrier inside.
//   3. barrier; all threads write the sample's M records (key, info, four matched indices, five errors) and the
//      per-class ground-truth counts.
//
// ocrf_det_eval_summary: the radix driver sorts the keys and then the classes (stable: descending score, ties by slot,
// within each class), a gather leaves order / sorted_cls / the TP flags, the look-back scan turns each threshold's flags
// into an exclusive prefix, one launch of (classes, 9) workgroups interpolates the curves (lane j does numpy's interp
// search for recall j / 100), and one workgroup reduces to mAP, mTP and NDS and checks the scans' give-up bits.
//
// Arithmetic: float64, every product and sum its own operation (the Makefile's -ffp-contract=off), in the order the
// header states.
//
// Bounds: rows are read below n = clamp(counts[b], 0, M), boxes below clamp(gt_counts[b], 0, G); a class list position
// is below the sum of the class counts <= M (G); a label indexes the tables only after its range test; a record slot is
// below (sample_index + B) M <= capacity M, which the host checks.  In the summary every position is inside the class's
// segment [lo, hi) of the n sorted slots.  `order` holds the sort's ids, a permutation of [0, n) unless a look-back scan
// gave up (the scatters then leave entries of the sort's buffers unwritten): the class-key and gather kernels clamp every
// id into [0, n) before they index with it, a segment of negative length counts as empty, and every search of the curve
// kernel stays inside its segment whatever the prefixes hold, so such a run reads in bounds until the final kernel turns
// its result into NaN.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "launch.h"
#include "ocrf_hip.h"
#include "radix_sort.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxWaves = OCRF_DET_EVAL_MAX_CLASSES;  // 1024 threads
constexpr int kNone = 31;                             // the class of what is not evaluated
constexpr int kRestClass = 16;                        // its digit in the second sort: behind every class
constexpr double kPi = 3.141592653589793;
constexpr double kTwoPi = 6.283185307179586;

struct MatchArgs {
  int M, D, G, n_classes, tp_index;
  long long sample_index;
  double t2[4];
  const float* boxes;
  const float* scores;
  const int* labels;
  const int* counts;
  const float* gt_boxes;
  const int* gt_labels;
  const int* gt_counts;
  const int* gt_attrs;
  const unsigned char* gt_valid;
  const float* class_range;
  const int* class_tab;
  unsigned* rec_key;
  int* rec_info;
  int* rec_match;
  double* rec_err;
  int* gt_count;
};

__device__ __forceinline__ bool finite32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// ascending keys are descending scores; -0 counts as +0
__device__ __forceinline__ unsigned score_key(float s) {
  unsigned u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;
  u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
  return ~u;
}

__device__ __forceinline__ float key_score(unsigned key) {
  const unsigned o = ~key;
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

// the evaluated test of one box: its class, or kNone
__device__ __forceinline__ int evaluated_class(const float* __restrict__ box, int label, int nc,
                                               const float* __restrict__ class_range) {
  if (label < 0 || label >= nc) return kNone;
  if (!(finite32(box[0]) && finite32(box[1]) && finite32(box[2]))) return kNone;
  const double x = (double)box[0], y = (double)box[1], r = (double)class_range[label];
  return x * x + y * y < r * r ? label : kNone;
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// what one wave writes to LDS is read by other lanes of the same wave afterwards
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void __launch_bounds__(kMaxWaves* kWave) det_eval_match_kernel(MatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int M = a.M, G = a.G, D = a.D, nc = a.n_classes;
  double* row_x = lds;                                // (M) a row's centre
  double* row_y = row_x + M;
  double* gl_x = row_y + M;                           // (G) the boxes' centres, class by class in index order
  double* gl_y = gl_x + G;
  int* row_cls = reinterpret_cast<int*>(gl_y + G);    // (M) the class of an evaluated row, else kNone
  unsigned* row_key = reinterpret_cast<unsigned*>(row_cls + M);  // (M)
  int* plist = reinterpret_cast<int*>(row_key + M);   // (M) the rows, class by class in row order
  int* sorted = plist + M;                            // (M) the rows, class by class in matching order
  int* row_tp = sorted + M;                           // (M) a row's true-positive bits
  int* row_match = row_tp + M;                        // (M, 4) the box a row claimed per threshold, else -1
  int* gt_cls = row_match + 4 * M;                    // (G) the class of an evaluated box, else kNone
  int* gl_idx = gt_cls + G;                           // (G) list position -> box index
  int* claim = gl_idx + G;                            // (G) per list position: claimed in the running loop
  int* class_np = claim + G;                          // (16) rows per class
  int* class_ng = class_np + OCRF_DET_EVAL_MAX_CLASSES;  // (16) boxes per class
  const int b = blockIdx.x, tid = threadIdx.x, threads = blockDim.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave, waves = threads / kWave;
  const int n = min(max(a.counts[b], 0), M);
  const int ng_all = min(max(a.gt_counts[b], 0), G);
  const float* boxes = a.boxes + (size_t)b * M * D;
  const float* scores = a.scores + (size_t)b * M;
  const int* labels = a.labels + (size_t)b * M;
  const float* gt_boxes = a.gt_boxes + (size_t)b * G * D;
  const int* gt_labels = a.gt_labels + (size_t)b * G;

  // 1. rows and boxes
  for (int r = tid; r < M; r += threads) {
    int cls = kNone;
    if (r < n && finite32(scores[r])) cls = evaluated_class(boxes + (size_t)r * D, labels[r], nc, a.class_range);
    row_cls[r] = cls;
    if (cls != kNone) {
      row_x[r] = (double)boxes[(size_t)r * D];
      row_y[r] = (double)boxes[(size_t)r * D + 1];
      row_key[r] = score_key(scores[r]);
    }
    row_tp[r] = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) row_match[4 * r + t] = -1;
  }
  for (int g = tid; g < G; g += threads) {
    int cls = kNone;
    if (g < ng_all && (a.gt_valid == nullptr || a.gt_valid[(size_t)b * G + g] != 0))
      cls = evaluated_class(gt_boxes + (size_t)g * D, gt_labels[g], nc, a.class_range);
    gt_cls[g] = cls;
  }
  __syncthreads();

  // 2. per class: count, gather, rank, match
  for (int c = wave; c < nc; c += waves) {
    int np = 0, ng = 0;
    for (int base = 0; base < n; base += kWave) {
      const int r = base + lane;
      np += __popcll(__ballot(r < n && row_cls[r] == c));
    }
    for (int base = 0; base < ng_all; base += kWave) {
      const int g = base + lane;
      ng += __popcll(__ballot(g < ng_all && gt_cls[g] == c));
    }
    if (lane == 0) class_np[c] = np, class_ng[c] = ng;
  }
  __syncthreads();
  for (int c = wave; c < nc; c += waves) {
    int first_p = 0, first_g = 0;
    for (int k = 0; k < c; ++k) first_p += class_np[k], first_g += class_ng[k];
    const int np = class_np[c], ng = class_ng[c];
    if (np == 0 || ng == 0) continue;                 // wave-uniform: every row of the class is a false positive
    int filled = 0;
    for (int base = 0; base < n; base += kWave) {
      const int r = base + lane;
      const bool mine = r < n && row_cls[r] == c;
      const unsigned long long mask = __ballot(mine);
      if (mine) plist[first_p + filled + __popcll(mask & lanes_below(lane))] = r;
      filled += __popcll(mask);
    }
    filled = 0;
    for (int base = 0; base < ng_all; base += kWave) {
      const int g = base + lane;
      const bool mine = g < ng_all && gt_cls[g] == c;
      const unsigned long long mask = __ballot(mine);
      if (mine) {
        const int at = first_g + filled + __popcll(mask & lanes_below(lane));
        gl_idx[at] = g;
        gl_x[at] = (double)gt_boxes[(size_t)g * D];
        gl_y[at] = (double)gt_boxes[(size_t)g * D + 1];
      }
      filled += __popcll(mask);
    }
    wave_sync();
    for (int i = lane; i < np; i += kWave) {
      const int r = plist[first_p + i];
      const unsigned key = row_key[r];
      int rank = 0;
      for (int j = 0; j < np; ++j) {
        const unsigned other = row_key[plist[first_p + j]];
        rank += (other < key || (other == key && j < i)) ? 1 : 0;
      }
      sorted[first_p + rank] = r;
    }
    wave_sync();
    for (int t = 0; t < 4; ++t) {
      const double t2 = a.t2[t];
      for (int k = lane; k < ng; k += kWave) claim[first_g + k] = 0;
      wave_sync();
      for (int i = 0; i < np; ++i) {                  // wave-uniform
        const int r = sorted[first_p + i];
        const double px = row_x[r], py = row_y[r];
        double best = __builtin_huge_val();
        int at = INT_MAX;
        for (int k = lane; k < ng; k += kWave) {
          if (claim[first_g + k] != 0) continue;
          const double dx = px - gl_x[first_g + k], dy = py - gl_y[first_g + k];
          const double d2 = dx * dx + dy * dy;
          if (d2 < best) best = d2, at = k;
        }
#pragma unroll
        for (int step = kWave / 2; step > 0; step >>= 1) {
          const double other = __shfl_xor(best, step, kWave);
          const int other_at = __shfl_xor(at, step, kWave);
          if (other < best || (other == best && other_at < at)) best = other, at = other_at;
        }
        if (at != INT_MAX && best < t2 && lane == 0) {
          claim[first_g + at] = 1;
          row_tp[r] |= 1 << t;
          row_match[4 * r + t] = gl_idx[first_g + at];
        }
        wave_sync();
      }
    }
  }
  __syncthreads();

  // 3. the records and the counts
  const size_t sample = (size_t)a.sample_index + (size_t)b;
  const double nan = __builtin_nan("");
  for (int r = tid; r < M; r += threads) {
    const size_t slot = sample * M + r;
    const int cls = row_cls[r];
    const bool evaluated = cls != kNone;
    a.rec_key[slot] = evaluated ? row_key[r] : 0xFFFFFFFFu;
    a.rec_info[slot] = evaluated ? (cls | OCRF_DET_EVAL_EVALUATED | (row_tp[r] << 8)) : kNone;
#pragma unroll
    for (int t = 0; t < 4; ++t) a.rec_match[slot * 4 + t] = row_match[4 * r + t];
    double e_trans = nan, e_scale = nan, e_orient = nan, e_vel = nan, e_attr = nan;
    const int g = row_match[4 * r + a.tp_index];
    if (evaluated && g >= 0) {
      const float* p = boxes + (size_t)r * D;
      const float* q = gt_boxes + (size_t)g * D;
      const double dx = row_x[r] - (double)q[0], dy = row_y[r] - (double)q[1];
      e_trans = sqrt(dx * dx + dy * dy);
      const double wp = p[3], lp = p[4], hp = p[5], wg = q[3], lg = q[4], hg = q[5];
      const double inter = (fmin(wp, wg) * fmin(lp, lg)) * fmin(hp, hg);
      const double vp = (wp * lp) * hp, vg = (wg * lg) * hg;
      e_scale = 1.0 - inter / ((vp + vg) - inter);
      const int flags = a.class_tab[cls * 3 + 2];
      const double period = (flags & OCRF_DET_EVAL_HALF_TURN) ? kPi : kTwoPi;
      const double half = period / 2.0;
      double m = fmod(((double)q[6] - (double)p[6]) + half, period);
      if (m < 0.0) m += period;
      double diff = m - half;
      if (diff > kPi) diff -= kTwoPi;
      e_orient = fabs(diff);
      bool moving = false;
      if (D == 9) {
        const double vx = p[7], vy = p[8];
        const double dvx = vx - (double)q[7], dvy = vy - (double)q[8];
        e_vel = sqrt(dvx * dvx + dvy * dvy);
        moving = vx * vx + vy * vy > 0.2 * 0.2;
      }
      const int ga = a.gt_attrs ? a.gt_attrs[(size_t)b * G + g] : -1;
      if (ga != -1) e_attr = a.class_tab[cls * 3 + (moving ? 0 : 1)] == ga ? 0.0 : 1.0;
    }
    double* err = a.rec_err + slot * 5;
    err[0] = e_trans, err[1] = e_scale, err[2] = e_orient, err[3] = e_vel, err[4] = e_attr;
  }
  // a class that was skipped above (no rows or no boxes) still has its counts from the first pass
  for (int c = tid; c < nc; c += threads) a.gt_count[sample * nc + c] = class_ng[c];
}

// ---------------------------------------------------------------------------------------------------------------
// the summary
// ---------------------------------------------------------------------------------------------------------------
constexpr int kFlat = 256;

__global__ void __launch_bounds__(kFlat) det_eval_copy_keys_kernel(const unsigned* __restrict__ rec_key, int n,
                                                                   unsigned* __restrict__ keys) {
  for (long i = (long)blockIdx.x * kFlat + threadIdx.x; i < n; i += (long)gridDim.x * kFlat) keys[i] = rec_key[i];
}

// the second sort's keys: the class of the slot at each position of the score order
__global__ void __launch_bounds__(kFlat) det_eval_class_keys_kernel(const int* __restrict__ ids, const int* __restrict__ rec_info,
                                                                    int n, unsigned* __restrict__ keys) {
  for (long i = (long)blockIdx.x * kFlat + threadIdx.x; i < n; i += (long)gridDim.x * kFlat) {
    const int info = rec_info[min(max(ids[i], 0), n - 1)];
    keys[i] = (info & OCRF_DET_EVAL_EVALUATED) ? (unsigned)(info & 31) : (unsigned)kRestClass;
  }
}

__global__ void __launch_bounds__(kFlat) det_eval_gather_kernel(const int* __restrict__ ids1, const int* __restrict__ ids2,
                                                                const unsigned* __restrict__ cls_sorted,
                                                                const int* __restrict__ rec_info, int n,
                                                                int* __restrict__ order, int* __restrict__ sorted_cls,
                                                                int* __restrict__ tp_flags) {
  for (long i = (long)blockIdx.x * kFlat + threadIdx.x; i < n; i += (long)gridDim.x * kFlat) {
    const int slot = min(max(ids1[min(max(ids2[i], 0), n - 1)], 0), n - 1);
    const int info = rec_info[slot];
    order[i] = slot;
    sorted_cls[i] = (int)cls_sorted[i];
#pragma unroll
    for (int t = 0; t < 4; ++t) tp_flags[(size_t)t * n + i] = (info >> (8 + t)) & 1;
  }
}

struct CurveArgs {
  int n, n_classes, tp_index, first;
  long long n_samples;
  double min_precision;
  const unsigned* rec_key;
  const int* rec_info;
  const double* rec_err;
  const int* gt_count;
  const int* class_tab;
  const int* order;
  const int* sorted_cls;
  const int* tp_excl;
  double* result;
};

constexpr int kCurveThreads = 128;
constexpr int kPoints = 101;

// a class's segment of the sorted slots, seen through one threshold's prefix
struct Segment {
  const unsigned* rec_key;
  const int* rec_info;
  const int* order;   // + lo
  const int* excl;    // + lo
  int shift, base, len;
  __device__ __forceinline__ int flag(int i) const { return (rec_info[order[i]] >> shift) & 1; }
  __device__ __forceinline__ int tp(int i) const { return excl[i] - base + flag(i); }     // inclusive
  __device__ __forceinline__ double conf(int i) const { return (double)key_score(rec_key[order[i]]); }
  // the position of match k < tp(len - 1): the first i with tp(i) >= k + 1
  __device__ __forceinline__ int match_pos(int k) const {
    int lo = -1, hi = len - 1;
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      if (tp(mid) >= k + 1) hi = mid; else lo = mid;
    }
    return hi;
  }
};

__device__ __forceinline__ int lower_bound_class(const int* __restrict__ sorted_cls, int n, int c) {
  int lo = 0, hi = n;                                 // the first position whose class is >= c
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (sorted_cls[mid] < c) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// numpy's interp for one x over the points (xp[j], fp[j]) = (lx, ly), (hx, hy) around it, lx <= x < hx
__device__ __forceinline__ double interp_between(double x, double lx, double ly, double hx, double hy) {
  const double slope = (hy - ly) / (hx - lx);
  double v = slope * (x - lx) + ly;
  if (v != v) {
    v = slope * (x - hx) + hy;
    if (v != v && ly == hy) v = ly;
  }
  return v;
}

// interp(x, rec, WHAT, right = 0) over the segment; WHAT: 0 prec, 1 conf
template <int WHAT>
__device__ __forceinline__ double interp_recall(const Segment& s, double x, double npos) {
  auto rec = [&](int i) { return (double)s.tp(i) / npos; };
  auto val = [&](int i) { return WHAT == 0 ? (double)s.tp(i) / (double)(i + 1) : s.conf(i); };
  if (x > rec(s.len - 1)) return 0.0;
  if (x < rec(0)) return val(0);
  int lo = 0, hi = s.len;                             // the last i with rec(i) <= x
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (rec(mid) <= x) lo = mid; else hi = mid;
  }
  if (lo == s.len - 1 || rec(lo) == x) return val(lo);
  return interp_between(x, rec(lo), val(lo), rec(lo + 1), val(lo + 1));
}

__global__ void __launch_bounds__(kCurveThreads) det_eval_curves_kernel(CurveArgs a) {
  __shared__ double s_curve[kPoints];
  __shared__ double s_conf[kPoints];
  __shared__ double s_sum[kCurveThreads];
  __shared__ int s_cnt[kCurveThreads];
  __shared__ int s_red[kCurveThreads];
  const int c = blockIdx.x, what = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int n = a.n, nc = a.n_classes;
  const bool is_ap = what < 4;
  const int t = is_ap ? what : a.tp_index, e = what - 4;
  double* out = is_ap ? a.result + c * 4 + what : a.result + nc * 4 + c * 5 + e;
  if (!is_ap) {
    const int flags = a.class_tab[c * 3 + 2];
    const bool none = (e == 2 && (flags & OCRF_DET_EVAL_NO_ORIENT)) || (e == 3 && (flags & OCRF_DET_EVAL_NO_VEL)) ||
                      (e == 4 && (flags & OCRF_DET_EVAL_NO_ATTR));
    if (none) {                                       // workgroup-uniform
      if (tid == 0) *out = __builtin_nan("");
      return;
    }
  }
  int part = 0;
  for (long long s = tid; s < a.n_samples; s += kCurveThreads) part += a.gt_count[s * nc + c];
  s_red[tid] = part;
  __syncthreads();
  int npos_i = 0;
  for (int k = 0; k < kCurveThreads; ++k) npos_i += s_red[k];
  const int lo = lower_bound_class(a.sorted_cls, n, c), hi = lower_bound_class(a.sorted_cls, n, c + 1);
  const int len = hi - lo;
  if (npos_i == 0 || len <= 0) {                      // workgroup-uniform
    if (tid == 0) *out = is_ap ? 0.0 : 1.0;
    return;
  }
  Segment seg;
  seg.rec_key = a.rec_key, seg.rec_info = a.rec_info, seg.order = a.order + lo;
  seg.excl = a.tp_excl + (size_t)t * n + lo;
  seg.shift = 8 + t, seg.base = seg.excl[0], seg.len = len;
  const double npos = (double)npos_i;
  const double x = tid == kPoints - 1 ? 1.0 : (double)tid * 0.01;
  const int first = a.first;
  if (is_ap) {
    if (tid < kPoints) s_curve[tid] = interp_recall<0>(seg, x, npos);
    __syncthreads();
    if (tid == 0) {
      double sum = 0.0;
      for (int j = first; j < kPoints; ++j) sum += fmax(s_curve[j] - a.min_precision, 0.0);
      *out = sum / (double)(kPoints - first) / (1.0 - a.min_precision);
    }
    return;
  }
  const int K = seg.tp(len - 1);
  if (K <= 0) {                                       // workgroup-uniform
    if (tid == 0) *out = 1.0;
    return;
  }
  if (tid < kPoints) s_conf[tid] = interp_recall<1>(seg, x, npos);
  __syncthreads();
  int last = 0;
  for (int j = 0; j < kPoints; ++j) last = s_conf[j] != 0.0 ? j : last;
  if (last < first) {                                 // workgroup-uniform
    if (tid == 0) *out = 1.0;
    return;
  }
  // interp(conf_i, conf_m, cm) over the reversed arrays: the matches around this lane's confidence
  int pos_a = -1, pos_b = -1;                         // pos_b >= 0: between match kb = ka - 1 (above) and ka (below)
  double conf_a = 0.0, conf_b = 0.0;
  const double xc = tid < kPoints ? s_conf[tid] : 0.0;
  if (tid < kPoints) {
    const int p0 = seg.match_pos(0), p_last = seg.match_pos(K - 1);
    if (xc > seg.conf(p0)) {
      pos_a = p0;                                     // right of every point: the first match's mean
    } else if (xc < seg.conf(p_last)) {
      pos_a = p_last;                                 // left of every point: the last match's mean
    } else {
      int klo = -1, khi = K - 1;                      // the first match whose confidence is <= xc
      while (khi - klo > 1) {
        const int mid = klo + (khi - klo) / 2;
        if (seg.conf(seg.match_pos(mid)) <= xc) khi = mid; else klo = mid;
      }
      pos_a = seg.match_pos(khi);
      conf_a = seg.conf(pos_a);
      if (khi != 0 && conf_a != xc) {
        pos_b = seg.match_pos(khi - 1);
        conf_b = seg.conf(pos_b);
      }
    }
  }
  // the NaN-aware prefix (sum, number) of error e over the segment: 128-wide chunks in sequence
  double carry_sum = 0.0, sum_a = 0.0, sum_b = 0.0;
  int carry_cnt = 0, cnt_a = 0, cnt_b = 0;
  for (int chunk = 0; chunk < len; chunk += kCurveThreads) {
    const int i = chunk + tid;
    double v = 0.0;
    int k = 0;
    if (i < len && seg.flag(i)) {
      const double err = a.rec_err[(size_t)seg.order[i] * 5 + e];
      if (err == err) v = err, k = 1;
    }
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const double ov = __shfl_up(v, off, kWave);
      const int ok = __shfl_up(k, off, kWave);
      if (lane >= off) v += ov, k += ok;
    }
    s_sum[tid] = v, s_cnt[tid] = k;
    __syncthreads();
    if (wave == 1) v += s_sum[kWave - 1], k += s_cnt[kWave - 1];
    v += carry_sum, k += carry_cnt;                   // carry + (wave 0's total +) the lane's inclusive prefix
    __syncthreads();
    s_sum[tid] = v, s_cnt[tid] = k;
    __syncthreads();
    if (pos_a >= chunk && pos_a < chunk + kCurveThreads) sum_a = s_sum[pos_a - chunk], cnt_a = s_cnt[pos_a - chunk];
    if (pos_b >= chunk && pos_b < chunk + kCurveThreads) sum_b = s_sum[pos_b - chunk], cnt_b = s_cnt[pos_b - chunk];
    carry_sum = s_sum[kCurveThreads - 1], carry_cnt = s_cnt[kCurveThreads - 1];
    __syncthreads();
  }
  if (tid < kPoints) {
    const bool all_nan = carry_cnt == 0;
    const double cm_a = all_nan ? 1.0 : (cnt_a > 0 ? sum_a / (double)cnt_a : 0.0);
    double v = cm_a;
    if (pos_b >= 0) {
      const double cm_b = all_nan ? 1.0 : (cnt_b > 0 ? sum_b / (double)cnt_b : 0.0);
      v = interp_between(xc, conf_a, cm_a, conf_b, cm_b);
    }
    s_curve[tid] = v;
  }
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int j = first; j <= last; ++j) sum += s_curve[j];
    *out = sum / (double)(last - first + 1);
  }
}

struct FinalArgs {
  int n_classes, n_sort1, n_sort2;
  long stride1, stride2;
  const unsigned long long* sort1;
  const unsigned long long* sort2;
  const unsigned long long* scan[4];
  double* result;
};

__global__ void __launch_bounds__(kWave) det_eval_final_kernel(FinalArgs a) {
  if (threadIdx.x != 0) return;
  const int nc = a.n_classes;
  double* ap = a.result;
  double* tp = ap + nc * 4;
  double* tail = tp + nc * 5;                         // mAP, mTP (5), NDS
  bool ok = true;
  for (int i = 0; i < a.n_sort1; ++i) ok = ok && (a.sort1[i * a.stride1] >> 63) == 0;
  for (int i = 0; i < a.n_sort2; ++i) ok = ok && (a.sort2[i * a.stride2] >> 63) == 0;
  for (int t = 0; t < 4; ++t) ok = ok && (a.scan[t][0] >> 63) == 0;
  if (!ok) {                                          // a scan gave up: no number rather than a wrong one
    for (int i = 0; i < nc * 9 + 7; ++i) a.result[i] = __builtin_nan("");
    return;
  }
  double map = 0.0;
  for (int c = 0; c < nc; ++c) map += (((ap[c * 4] + ap[c * 4 + 1]) + ap[c * 4 + 2]) + ap[c * 4 + 3]) / 4.0;
  map /= (double)nc;
  tail[0] = map;
  double nds = 5.0 * map;
  for (int e = 0; e < 5; ++e) {
    double sum = 0.0;
    int cnt = 0;
    for (int c = 0; c < nc; ++c) {
      const double v = tp[c * 5 + e];
      if (v == v) sum += v, ++cnt;
    }
    const double mean = cnt > 0 ? sum / (double)cnt : __builtin_nan("");
    tail[1 + e] = mean;
    nds += 1.0 - (mean == mean ? fmin(1.0, mean) : 1.0);
  }
  tail[6] = nds / 10.0;
}

struct SummaryLayout {
  size_t keys, keys2, sort1, sort2, scan[4], bytes, sort_bytes, scan_bytes;
};

SummaryLayout summary_layout(long long n) {
  SummaryLayout w{};
  auto take = [&](size_t b) { size_t o = w.bytes; w.bytes += ocrf::align_up(b, 256); return o; };
  w.sort_bytes = ocrf::radix_sort_ids_bytes((int)n);
  w.scan_bytes = ocrf::exclusive_scan_bytes((long)n);
  w.keys = take((size_t)n * 4);
  w.keys2 = take((size_t)n * 4);
  w.sort1 = take(w.sort_bytes);
  w.sort2 = take(w.sort_bytes);
  for (int t = 0; t < 4; ++t) w.scan[t] = take(w.scan_bytes);
  return w;
}

}  // namespace

extern "C" {

size_t ocrf_det_eval_match_lds_bytes(int M, int G) {
  if (M <= 0 || G <= 0) return 0;
  return (size_t)M * 52 + (size_t)G * 28 + (size_t)OCRF_DET_EVAL_MAX_CLASSES * 8;
}

int ocrf_det_eval_match(int B, int M, int D, int G, int n_classes, long long sample_index, long long capacity,
                        double th0, double th1, double th2, double th3, int tp_index, const float* boxes,
                        const float* scores, const int* labels, const int* counts, const float* gt_boxes,
                        const int* gt_labels, const int* gt_counts, const int* gt_attrs, const unsigned char* gt_valid,
                        const float* class_range, const int* class_tab, unsigned* rec_key, int* rec_info,
                        int* rec_match, double* rec_err, int* gt_count, ocrf_stream_t stream) {
  if (B <= 0 || B > 65535 || M <= 0 || G <= 0 || (D != 9 && D != 7)) return (int)hipErrorInvalidValue;
  if (n_classes <= 0 || n_classes > OCRF_DET_EVAL_MAX_CLASSES || tp_index < 0 || tp_index > 3) return (int)hipErrorInvalidValue;
  if (sample_index < 0 || capacity <= 0 || sample_index + B > capacity || capacity * (long long)M >= (1ll << 31)) {
    return (int)hipErrorInvalidValue;
  }
  const double th[4] = {th0, th1, th2, th3};
  for (double t : th)
    if (!(t - t == 0.0)) return (int)hipErrorInvalidValue;                                    // NaN or infinite
  const size_t lds = ocrf_det_eval_match_lds_bytes(M, G);
  if (lds == 0 || lds > OCRF_DET_EVAL_MAX_LDS) return (int)hipErrorInvalidValue;
  if (!boxes || !scores || !labels || !counts || !gt_boxes || !gt_labels || !gt_counts || !class_range || !class_tab ||
      !rec_key || !rec_info || !rec_match || !rec_err || !gt_count) {
    return (int)hipErrorInvalidValue;
  }
  MatchArgs a;
  a.M = M, a.D = D, a.G = G, a.n_classes = n_classes, a.tp_index = tp_index, a.sample_index = sample_index;
  for (int t = 0; t < 4; ++t) a.t2[t] = th[t] * th[t];
  a.boxes = boxes, a.scores = scores, a.labels = labels, a.counts = counts;
  a.gt_boxes = gt_boxes, a.gt_labels = gt_labels, a.gt_counts = gt_counts, a.gt_attrs = gt_attrs, a.gt_valid = gt_valid;
  a.class_range = class_range, a.class_tab = class_tab;
  a.rec_key = rec_key, a.rec_info = rec_info, a.rec_match = rec_match, a.rec_err = rec_err, a.gt_count = gt_count;
  const int waves = n_classes < 2 ? 2 : n_classes;
  ocrf::launch(OCRF_K_DET_EVAL_MATCH, det_eval_match_kernel, dim3(B), dim3(waves * kWave), lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

size_t ocrf_det_eval_summary_workspace_bytes(long long n_slots) {
  if (n_slots <= 0 || n_slots >= (1ll << 31)) return 0;
  return summary_layout(n_slots).bytes;
}

int ocrf_det_eval_summary(long long n_samples, int M, int n_classes, int tp_index, int first, double min_precision,
                          const unsigned* rec_key, const int* rec_info, const double* rec_err, const int* gt_count,
                          const int* class_tab, int* order, int* sorted_cls, int* tp_excl, double* result,
                          void* workspace, size_t workspace_bytes, ocrf_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (n_samples <= 0 || M <= 0 || n_samples * (long long)M >= (1ll << 31)) return (int)hipErrorInvalidValue;
  if (n_classes <= 0 || n_classes > OCRF_DET_EVAL_MAX_CLASSES || tp_index < 0 || tp_index > 3) return (int)hipErrorInvalidValue;
  if (first < 1 || first > 100 || !(min_precision >= 0.0 && min_precision < 1.0)) return (int)hipErrorInvalidValue;
  if (!rec_key || !rec_info || !rec_err || !gt_count || !class_tab || !order || !sorted_cls || !tp_excl || !result ||
      !workspace || (reinterpret_cast<size_t>(workspace) & 255) != 0) {
    return (int)hipErrorInvalidValue;
  }
  const int n = (int)(n_samples * M);
  const SummaryLayout w = summary_layout(n);
  if (workspace_bytes < w.bytes) return (int)hipErrorInvalidValue;
  char* base = static_cast<char*>(workspace);
  unsigned* keys = reinterpret_cast<unsigned*>(base + w.keys);
  unsigned* keys2 = reinterpret_cast<unsigned*>(base + w.keys2);
  const unsigned grid = (unsigned)std::min<long>(((long)n + kFlat - 1) / kFlat, 4096);
  ocrf::launch(OCRF_K_DET_EVAL_COPY_KEYS, det_eval_copy_keys_kernel, dim3(grid), dim3(kFlat), 0, stream, rec_key, n, keys);
  const unsigned* score_sorted = nullptr;               // where the sort leaves the keys; only the ids are used
  const int* ids1 = nullptr;
  hipError_t err = ocrf::radix_sort_ids(keys, n, 32, base + w.sort1, w.sort_bytes, &score_sorted, &ids1, stream);
  (void)score_sorted;
  if (err != hipSuccess) return (int)err;
  ocrf::launch(OCRF_K_DET_EVAL_CLASS_KEYS, det_eval_class_keys_kernel, dim3(grid), dim3(kFlat), 0, stream, ids1, rec_info, n,
               keys2);
  const unsigned* cls_sorted = nullptr;
  const int* ids2 = nullptr;
  err = ocrf::radix_sort_ids(keys2, n, 5, base + w.sort2, w.sort_bytes, &cls_sorted, &ids2, stream);
  if (err != hipSuccess) return (int)err;
  ocrf::launch(OCRF_K_DET_EVAL_GATHER, det_eval_gather_kernel, dim3(grid), dim3(kFlat), 0, stream, ids1, ids2, cls_sorted,
               rec_info, n, order, sorted_cls, tp_excl);
  for (int t = 0; t < 4; ++t) {
    err = ocrf::exclusive_scan_ints(tp_excl + (size_t)t * n, n, nullptr, base + w.scan[t], w.scan_bytes, stream);
    if (err != hipSuccess) return (int)err;
  }
  CurveArgs c;
  c.n = n, c.n_classes = n_classes, c.tp_index = tp_index, c.first = first, c.n_samples = n_samples;
  c.min_precision = min_precision;
  c.rec_key = rec_key, c.rec_info = rec_info, c.rec_err = rec_err, c.gt_count = gt_count, c.class_tab = class_tab;
  c.order = order, c.sorted_cls = sorted_cls, c.tp_excl = tp_excl, c.result = result;
  ocrf::launch(OCRF_K_DET_EVAL_CURVES, det_eval_curves_kernel, dim3(n_classes, 9), dim3(kCurveThreads), 0, stream, c);
  FinalArgs f;
  f.n_classes = n_classes, f.result = result;
  ocrf::radix_sort_states(base + w.sort1, n, 32, &f.sort1, &f.n_sort1, &f.stride1);
  ocrf::radix_sort_states(base + w.sort2, n, 5, &f.sort2, &f.n_sort2, &f.stride2);
  for (int t = 0; t < 4; ++t) f.scan[t] = reinterpret_cast<const unsigned long long*>(base + w.scan[t]);
  ocrf::launch(OCRF_K_DET_EVAL_FINAL, det_eval_final_kernel, dim3(1), dim3(kWave), 0, stream, f);
  return (int)hipGetLastError();
}

}  // extern "C"
