// The stable LSD radix sort and the in-place exclusive scan that the LSS index preparation (index_prep.hip) and the
// render-plan build (raster_plan.hip) share (csrc/radix_sort.hip).  Host side only.
#pragma once
#include <hip/hip_runtime.h>

#include "radix_emit.h"

namespace ocrf {

// One pass sorts by one 9-bit digit: a workgroup histograms kSortChunk consecutive keys into table[d * n_wg + workgroup]
// (d < kBins, n_wg = ceil(n / kSortChunk)), one look-back scan of the table gives every (digit, workgroup) its first
// output position, the scatter keeps the input order among equal digits.  A caller whose own kernel produces the keys may
// leave pass 0's table in the same launch (lss_keys_hist_kernel): this and SortLayout::table / n_wg are all it must know.
constexpr int kRadixBits = 9, kBins = 1 << kRadixBits, kSortChunk = 2048;
inline int radix_passes_of_bits(int key_bits) { return (key_bits + kRadixBits - 1) / kRadixBits; }

// The sort's workspace as byte offsets: keys A (only if the caller keeps its keys there), keys B, values A / B, the
// table, then the look-back state blocks: one of st_words words per pass (4, the most a 32-bit key needs), then
// tail_state_bytes of the caller's own.  state_bytes covers them all: one zero-fill per call.
struct SortLayout {
  size_t keys_a, keys_b, vals_a, vals_b, table, state, state_bytes, bytes;
  long st_words;
  int n_wg;
};
SortLayout radix_sort_layout(long n, bool keys_a_inside, size_t tail_state_bytes);

// Passes 0 .. passes - 1 (<= 4) over the n keys at `keys` (clobbered) in a workspace laid out as `w`.
//   hist0_ready   the caller has zero-filled the state blocks and written pass 0's table; else the driver launches both
//   ranks / plan  at most one: what the LAST pass writes besides the keys (radix_emit.h); `plan` needs a pass > 0
//   keys_out / vals_out   in: where the last pass writes keys / values, null = the workspace's buffers; out: where the
//                 sorted keys / values (original positions, ascending among equal keys) are; values null with `plan`
hipError_t radix_sort_passes(unsigned* keys, int n, int passes, bool hist0_ready, void* workspace, const SortLayout& w,
                             const RadixRankEmit* ranks, const RadixPlanEmit* plan, unsigned** keys_out, int** vals_out,
                             hipStream_t stream);

// Stable sort of n keys of key_bits (1 .. 32) significant bits carrying their original index.  `keys` is clobbered; the
// sorted keys / ids are returned through the two pointers (into `scratch`, >= radix_sort_ids_bytes(n) bytes, or at `keys`).
// With `plan_emit` the last pass writes the render plan's lists itself, *sorted_ids is null and key_bits <= 9 is refused.
size_t radix_sort_ids_bytes(int n);
hipError_t radix_sort_ids(unsigned* keys, int n, int key_bits, void* scratch, size_t scratch_bytes,
                          const unsigned** sorted_keys, const int** sorted_ids, hipStream_t stream,
                          const RadixPlanEmit* plan_emit = nullptr);
// where that call leaves the state blocks of its look-back scans (one per pass): bit 63 of a block's first word says that
// scan gave up (the caller's last kernel checks them on the device)
void radix_sort_states(void* scratch, int n, int key_bits, const unsigned long long** states, int* n_states,
                       long* stride_words);

// in-place exclusive prefix sum of n non-negative ints (*total = their sum, may be null): a zero-fill + ONE launch
size_t exclusive_scan_bytes(long n);
hipError_t exclusive_scan_ints(int* data, long n, int* total, void* scratch, size_t scratch_bytes, hipStream_t stream);

}  // namespace ocrf
