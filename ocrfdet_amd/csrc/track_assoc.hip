// Streaming object tracking: one step of greedy closest-centre association for all B samples in ONE launch
// (ocrf_track_step; the rules are stated in include/ocrf_hip.h, OcRFDet4D.track_stream is the caller).  The detections
// are the padded output of the fused decode; the tracks live in the global frame in float64, because a nuScenes global
// pose is thousands of metres from the origin and a matching radius is one metre.
//
// One workgroup per sample, one wavefront per class (classes go round-robin over the waves when there are fewer waves).
// Only equal labels match, so the sequential greedy rule is a per-class rule: the waves never meet inside the loop.
//
//   1. all threads: per row the tracked test and (px, py), the centre moved back by one time lag, into LDS; per old slot
//      the claim word, -1.
//   2. wave c, alone: counts the tracks of class c (a ballot pass over the old labels), barrier, and with the counts of
//      the classes before it as its offset gathers their slots and positions into LDS in slot order (a second ballot
//      pass).  Then for each row of class c in row order (a ballot pass over the row labels, the set bits taken lowest
//      first): every lane walks the class's tracks lane, lane + 64, ..., keeps its smallest d2 within the radius (first
//      wins: lowest slot), six xor-shuffles reduce (d2, list position) to the wave's argmin with ties to the lower
//      position, and lane 0 claims the slot.  No workgroup barrier inside.
//   3. barrier; wave 0 ranks the rows (tracked rows: their new slot; unmatched tracked rows: their id offset) and wave 1
//      the unclaimed old slots that stay (misses + 1 < max_age), both by ballot scans with a running count; barrier.
//   4. all threads write ids / hits, the new state (every one of the cap slots: zeros past the new count) and the counts.
//
// Arithmetic: float64, every product and sum its own operation (the Makefile's -ffp-contract=off), in the order the
// header states, and step 4 recomputes a row's global centre and velocity with step 1's function: the same bits.  A NaN
// distance (a non-finite time lag or a track that drifted to infinity) fails `d2 <= r2` and matches nothing.
//
// Bounds: rows are read below n = clamp(counts[b], 0, M), old slots below C = clamp(count_in[b], 0, cap), a class list
// position is below the sum of the class counts <= C, a new slot is written only when it is below cap, a label indexes
// max_dist only after the range test.
#include <hip/hip_runtime.h>

#include <climits>

#include "launch.h"
#include "ocrf_hip.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxWaves = OCRF_TRACK_MAX_CLASSES;  // 1024 threads

struct Args {
  int M, D, n_classes, max_age, cap;
  float min_score;
  const float* boxes;
  const float* scores;
  const int* labels;
  const int* counts;
  const float* ego2global;
  const float* time_lag;
  const unsigned char* new_sequence;
  const float* max_dist;
  const double* pos_in;
  const double* vel_in;
  const int* label_in;
  const int* id_in;
  const int* misses_in;
  const int* hits_in;
  const int* count_in;
  const int* next_id_in;
  double* pos_out;
  double* vel_out;
  int* label_out;
  int* id_out;
  int* misses_out;
  int* hits_out;
  int* count_out;
  int* next_id_out;
  int* ids;
  int* hits;
};

__device__ __forceinline__ bool finite32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

struct Global {
  double gx, gy, vgx, vgy;
};

// a row's centre and velocity in the global frame; E: rows 0 and 1 of ego2global, widened
__device__ __forceinline__ Global to_global(const float* __restrict__ box, int D, const double (&E)[8]) {
  const double x = (double)box[0], y = (double)box[1], z = (double)box[2];
  const double vx = D == 9 ? (double)box[7] : 0.0, vy = D == 9 ? (double)box[8] : 0.0;
  Global g;
  g.gx = ((E[0] * x + E[1] * y) + E[2] * z) + E[3];
  g.gy = ((E[4] * x + E[5] * y) + E[6] * z) + E[7];
  g.vgx = E[0] * vx + E[1] * vy;
  g.vgy = E[4] * vx + E[5] * vy;
  return g;
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// what one wave writes to LDS is read by other lanes of the same wave afterwards
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void __launch_bounds__(kMaxWaves* kWave) track_step_kernel(Args a) {
  extern __shared__ double lds[];
  __shared__ int class_count[OCRF_TRACK_MAX_CLASSES];
  __shared__ int totals[3];  // tracked rows, new ids, kept old tracks
  const int M = a.M, cap = a.cap, D = a.D, nc = a.n_classes;
  double* row_px = lds;                               // (M) a tracked row's centre one time lag back
  double* row_py = row_px + M;
  double* list_x = row_py + M;                        // (cap) the old tracks' positions, class by class in slot order
  double* list_y = list_x + cap;
  int* row_label = reinterpret_cast<int*>(list_y + cap);  // (M) the label of a tracked row, else -1
  int* row_slot = row_label + M;                      // (M) the old slot a row claimed, else -1
  int* row_rank = row_slot + M;                       // (M) a tracked row's new slot
  int* row_new = row_rank + M;                        // (M) an unmatched tracked row's id offset
  int* list_slot = row_new + M;                       // (cap) list position -> old slot
  int* claim = list_slot + cap;                       // (cap) per old slot: -1 free, >= 0 the claiming row; after step 3
                                                      // -1 dropped, <= -2 kept with rank -2 - claim
  const int b = blockIdx.x, tid = threadIdx.x, threads = blockDim.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave, waves = threads / kWave;
  const int n = min(max(a.counts[b], 0), M);
  const bool restart = a.new_sequence != nullptr && a.new_sequence[b] != 0;
  const int C = restart ? 0 : min(max(a.count_in[b], 0), cap);
  double E[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) E[k] = (double)a.ego2global[(size_t)b * 16 + k];
  const double dt = (double)a.time_lag[b];
  const float* boxes = a.boxes + (size_t)b * M * D;
  const float* scores = a.scores + (size_t)b * M;
  const int* labels = a.labels + (size_t)b * M;
  const size_t s0 = (size_t)b * cap;                  // the sample's first state slot
  const double* pos_in = a.pos_in + s0 * 2;
  const double* vel_in = a.vel_in + s0 * 2;
  const int* label_in = a.label_in + s0;

  // 1. rows and claim words
  for (int r = tid; r < M; r += threads) {
    int label = -1;
    if (r < n) {
      const int l = labels[r];
      const float* box = boxes + (size_t)r * D;
      bool ok = l >= 0 && l < nc && !(scores[r] < a.min_score);
      ok = ok && a.max_dist[l] > 0.0f;
      ok = ok && finite32(box[0]) && finite32(box[1]) && finite32(box[2]);
      if (ok && D == 9) ok = finite32(box[7]) && finite32(box[8]);
      if (ok) {
        const Global g = to_global(box, D, E);
        row_px[r] = g.gx - g.vgx * dt;
        row_py[r] = g.gy - g.vgy * dt;
        label = l;
      }
    }
    row_label[r] = label;
    row_slot[r] = -1;
  }
  for (int s = tid; s < C; s += threads) claim[s] = -1;

  // 2. per class: count, gather, match
  for (int c = wave; c < nc; c += waves) {
    int count = 0;
    for (int base = 0; base < C; base += kWave) {
      const int s = base + lane;
      count += __popcll(__ballot(s < C && label_in[s] == c));
    }
    if (lane == 0) class_count[c] = count;
  }
  __syncthreads();
  for (int c = wave; c < nc; c += waves) {
    int first = 0;
    for (int k = 0; k < c; ++k) first += class_count[k];
    const int count = class_count[c];
    if (count == 0) continue;                         // wave-uniform: nothing to match, every row of the class is new
    int filled = 0;
    for (int base = 0; base < C; base += kWave) {
      const int s = base + lane;
      const bool mine = s < C && label_in[s] == c;
      const unsigned long long mask = __ballot(mine);
      if (mine) {
        const int at = first + filled + __popcll(mask & lanes_below(lane));
        list_slot[at] = s;
        list_x[at] = pos_in[2 * s];
        list_y[at] = pos_in[2 * s + 1];
      }
      filled += __popcll(mask);
    }
    wave_sync();
    const double radius = (double)a.max_dist[c];
    const double r2 = radius * radius;
    for (int base = 0; base < n; base += kWave) {
      const int rr = base + lane;
      unsigned long long rows = __ballot(rr < n && row_label[rr] == c);
      while (rows != 0) {                             // wave-uniform
        const int r = base + __ffsll((long long)rows) - 1;
        rows &= rows - 1;
        const double px = row_px[r], py = row_py[r];
        double best = __builtin_huge_val();
        int at = INT_MAX;
        for (int k = lane; k < count; k += kWave) {
          if (claim[list_slot[first + k]] >= 0) continue;
          const double dx = list_x[first + k] - px, dy = list_y[first + k] - py;
          const double d2 = dx * dx + dy * dy;
          if (d2 <= r2 && d2 < best) best = d2, at = k;
        }
#pragma unroll
        for (int step = kWave / 2; step > 0; step >>= 1) {
          const double other = __shfl_xor(best, step, kWave);
          const int other_at = __shfl_xor(at, step, kWave);
          if (other < best || (other == best && other_at < at)) best = other, at = other_at;
        }
        if (at != INT_MAX && lane == 0) {
          const int slot = list_slot[first + at];
          claim[slot] = r;
          row_slot[r] = slot;
        }
        wave_sync();
      }
    }
  }
  __syncthreads();

  // 3. ranks: wave 0 the rows, the last of the first two waves the old slots
  if (wave == 0) {
    int tracked = 0, fresh = 0;
    for (int base = 0; base < n; base += kWave) {
      const int r = base + lane;
      const bool is_tracked = r < n && row_label[r] >= 0;
      const bool is_new = is_tracked && row_slot[r] < 0;
      const unsigned long long mt = __ballot(is_tracked), mn = __ballot(is_new);
      if (r < n) {
        row_rank[r] = tracked + __popcll(mt & lanes_below(lane));
        row_new[r] = fresh + __popcll(mn & lanes_below(lane));
      }
      tracked += __popcll(mt);
      fresh += __popcll(mn);
    }
    if (lane == 0) totals[0] = tracked, totals[1] = fresh;
  }
  if (wave == min(1, waves - 1)) {
    int kept = 0;
    const int* misses_in = a.misses_in + s0;
    for (int base = 0; base < C; base += kWave) {
      const int s = base + lane;
      const bool is_free = s < C && claim[s] < 0;
      const bool stays = is_free && misses_in[s] < a.max_age - 1;        // misses + 1 < max_age, without the overflow
      const unsigned long long mk = __ballot(stays);
      if (is_free) claim[s] = stays ? -2 - (kept + __popcll(mk & lanes_below(lane))) : -1;
      kept += __popcll(mk);
    }
    if (lane == 0) totals[2] = kept;
  }
  __syncthreads();

  // 4. outputs and the new state
  const int tracked = totals[0], fresh = totals[1], kept = totals[2];
  const unsigned next_id = (unsigned)a.next_id_in[b];
  double* pos_out = a.pos_out + s0 * 2;
  double* vel_out = a.vel_out + s0 * 2;
  int* label_out = a.label_out + s0;
  int* id_out = a.id_out + s0;
  int* misses_out = a.misses_out + s0;
  int* hits_out = a.hits_out + s0;
  for (int r = tid; r < M; r += threads) {
    int id = -1, hit = 0;
    if (r < n && row_label[r] >= 0) {
      const int slot = row_slot[r];
      if (slot >= 0) {
        id = a.id_in[s0 + slot];
        hit = (int)((unsigned)a.hits_in[s0 + slot] + 1u);
      } else {
        id = (int)(next_id + (unsigned)row_new[r]);
        hit = 1;
      }
      const int j = row_rank[r];
      if (j < cap) {
        const Global g = to_global(boxes + (size_t)r * D, D, E);
        pos_out[2 * j] = g.gx, pos_out[2 * j + 1] = g.gy;
        vel_out[2 * j] = g.vgx, vel_out[2 * j + 1] = g.vgy;
        label_out[j] = row_label[r], id_out[j] = id, misses_out[j] = 0, hits_out[j] = hit;
      }
    }
    a.ids[(size_t)b * M + r] = id;
    a.hits[(size_t)b * M + r] = hit;
  }
  for (int s = tid; s < C; s += threads) {
    const int word = claim[s];
    const int j = tracked + (-2 - word);
    if (word <= -2 && j < cap) {
      const double vx = vel_in[2 * s], vy = vel_in[2 * s + 1];
      pos_out[2 * j] = pos_in[2 * s] + vx * dt, pos_out[2 * j + 1] = pos_in[2 * s + 1] + vy * dt;
      vel_out[2 * j] = vx, vel_out[2 * j + 1] = vy;
      label_out[j] = label_in[s], id_out[j] = a.id_in[s0 + s], misses_out[j] = a.misses_in[s0 + s] + 1, hits_out[j] = 0;
    }
  }
  const int total = min(tracked + kept, cap);
  for (int j = total + tid; j < cap; j += threads) {
    pos_out[2 * j] = 0.0, pos_out[2 * j + 1] = 0.0, vel_out[2 * j] = 0.0, vel_out[2 * j + 1] = 0.0;
    label_out[j] = 0, id_out[j] = 0, misses_out[j] = 0, hits_out[j] = 0;
  }
  if (tid == 0) {
    a.count_out[b] = total;
    a.next_id_out[b] = (int)(next_id + (unsigned)fresh);
  }
}

}  // namespace

extern "C" {

size_t ocrf_track_step_lds_bytes(int M, int cap) {
  if (M <= 0 || cap <= 0) return 0;
  return (size_t)M * 32 + (size_t)cap * 24;
}

int ocrf_track_step(int B, int M, int D, int n_classes, int max_age, float min_score, int cap, const float* boxes,
                    const float* scores, const int* labels, const int* counts, const float* ego2global,
                    const float* time_lag, const unsigned char* new_sequence, const float* max_dist,
                    const double* pos_in, const double* vel_in, const int* label_in, const int* id_in,
                    const int* misses_in, const int* hits_in, const int* count_in, const int* next_id_in,
                    double* pos_out, double* vel_out, int* label_out, int* id_out, int* misses_out, int* hits_out,
                    int* count_out, int* next_id_out, int* ids, int* hits, ocrf_stream_t stream) {
  if (B <= 0 || B > 65535 || M <= 0 || (D != 9 && D != 7)) return (int)hipErrorInvalidValue;
  if (n_classes <= 0 || n_classes > OCRF_TRACK_MAX_CLASSES || max_age <= 0) return (int)hipErrorInvalidValue;
  if (!(min_score == min_score)) return (int)hipErrorInvalidValue;                           // NaN
  if ((long long)max_age * M != (long long)cap) return (int)hipErrorInvalidValue;
  const size_t lds = ocrf_track_step_lds_bytes(M, cap);
  if (lds == 0 || lds > OCRF_TRACK_MAX_LDS) return (int)hipErrorInvalidValue;
  if (!boxes || !scores || !labels || !counts || !ego2global || !time_lag || !max_dist || !ids || !hits) {
    return (int)hipErrorInvalidValue;
  }
  if (!pos_in || !vel_in || !label_in || !id_in || !misses_in || !hits_in || !count_in || !next_id_in || !pos_out ||
      !vel_out || !label_out || !id_out || !misses_out || !hits_out || !count_out || !next_id_out) {
    return (int)hipErrorInvalidValue;
  }
  if (pos_in == pos_out || vel_in == vel_out || label_in == label_out || id_in == id_out || misses_in == misses_out ||
      hits_in == hits_out || count_in == count_out || next_id_in == next_id_out) {
    return (int)hipErrorInvalidValue;
  }
  Args a;
  a.M = M, a.D = D, a.n_classes = n_classes, a.max_age = max_age, a.cap = cap, a.min_score = min_score;
  a.boxes = boxes, a.scores = scores, a.labels = labels, a.counts = counts, a.ego2global = ego2global;
  a.time_lag = time_lag, a.new_sequence = new_sequence, a.max_dist = max_dist;
  a.pos_in = pos_in, a.vel_in = vel_in, a.label_in = label_in, a.id_in = id_in, a.misses_in = misses_in;
  a.hits_in = hits_in, a.count_in = count_in, a.next_id_in = next_id_in;
  a.pos_out = pos_out, a.vel_out = vel_out, a.label_out = label_out, a.id_out = id_out, a.misses_out = misses_out;
  a.hits_out = hits_out, a.count_out = count_out, a.next_id_out = next_id_out;
  a.ids = ids, a.hits = hits;
  const int waves = n_classes < 2 ? 2 : n_classes;
  ocrf::launch(OCRF_K_TRACK_STEP, track_step_kernel, dim3(B), dim3(waves * kWave), lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"
