// What the LAST pass of a radix sort (csrc/radix_sort.hip) may write besides — or instead of — the sorted (key, value)
// pairs: the consumer's own arrays, so that no further launch has to turn the pairs into them.
#pragma once
#include <hip/hip_runtime.h>

namespace ocrf {

// LSS index preparation (csrc/index_prep.hip), EMIT 1: the (voxel, point) pairs leave as ranks_bev / ranks_depth (the
// pass's key / value outputs) and ranks_feat[pos] = (b*N + n)*H*W + h*W + w of the point (view_transformer.py:232-236).
struct RadixRankEmit {
  int* ranks_feat;
  int DHW, HW;
};

// render-plan build (csrc/raster_plan.hip), EMIT 2: value = the record's Gaussian-major index e.  The per-view lists in
// blend order leave the sort as s_e = e, s_id = rec_id[e], s_key = depth bits of the key, s_pix = pixel centre of e.
struct RadixPlanEmit {
  const int* rec_id;
  const float4* e_q1;
  unsigned* s_e;
  unsigned* s_id;
  unsigned* s_key;
  float2* s_pix;
  unsigned depth_mask, key_base;
};

}  // namespace ocrf
