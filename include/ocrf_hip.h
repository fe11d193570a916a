/*
 * ocrf_hip.h — C ABI of libocrf_hip.so: the MI355X (gfx950) implementation of OcRFDet's
 * render + BEV-pool + HOA hot path.  Plain pointers and sizes only; every pointer is a DEVICE
 * pointer unless its comment says "host".  Every function returns 0 on success or a hipError_t
 * value (as int); nothing is allocated, freed or synchronised inside a call (all of them are
 * hipGraph-capturable), the caller owns every buffer, and `stream` is a hipStream_t (NULL =
 * the legacy default stream, which is what the reference launches on).
 *
 * File:line citations are into the reference tree (Mingqj/OcRFDet), i.e. the interface each
 * entry point replaces.
 */
#ifndef OCRF_HIP_H
#define OCRF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *ocrf_stream_t; /* hipStream_t */

/* Library / build identification: returns e.g. "ocrf_hip 0.1 gfx950". Host pointer, static. */
const char *ocrf_version(void);

/* ------------------------------------------------------------------------------------------
 * BEVPoolv2 voxel pooling
 * ------------------------------------------------------------------------------------------ */

/*
 * Exact signature of the reference's C-level launcher
 *   void bev_pool_v2(int c, int n_intervals, const float* depth, const float* feat,
 *                    const int* ranks_depth, const int* ranks_feat, const int* ranks_bev,
 *                    const int* interval_starts, const int* interval_lengths, float* out)
 * (mmdet3d/ops/bev_pool_v2/src/bev_pool.cpp:7-9, defined src/bev_pool_cuda.cu:123-131).
 * Same contract: `out` is (B,Z,Y,X,C) and must be pre-zeroed by the caller; for interval k,
 *   out[ranks_bev[starts[k]]*c + ch] = sum_i depth[ranks_depth[starts[k]+i]] * feat[ranks_feat[starts[k]+i]*c + ch]
 * (assignment, accumulated in list order); launches on the legacy default stream; any interval
 * layout is accepted (one lane group per interval).  No error is reported (the reference
 * reports none) — use ocrf_bev_pool_v2 for an error code, a stream and the tiled kernel.
 */
void bev_pool_v2(int c, int n_intervals, const float *depth, const float *feat,
                 const int *ranks_depth, const int *ranks_feat, const int *ranks_bev,
                 const int *interval_starts, const int *interval_lengths, float *out);

/*
 * Exact signature of the reference's backward launcher (src/bev_pool.cpp:11-14,
 * src/bev_pool_cuda.cu:133-140).  Intervals are runs of equal ranks_feat (the Python wrapper
 * re-sorts, bev_pool.py:47-57).  depth_grad/feat_grad must be pre-zeroed.
 *   feat_grad[ranks_feat[s]*c + ch] = sum_i out_grad[ranks_bev[s+i]*c + ch] * depth[ranks_depth[s+i]]
 *   depth_grad[ranks_depth[p]]      = sum_ch out_grad[ranks_bev[p]*c + ch] * feat[ranks_feat[p]*c + ch]
 */
void bev_pool_v2_grad(int c, int n_intervals, const float *out_grad, const float *depth,
                      const float *feat, const int *ranks_depth, const int *ranks_feat,
                      const int *ranks_bev, const int *interval_starts,
                      const int *interval_lengths, float *depth_grad, float *feat_grad);

/*
 * Tiled forward (one output-stationary pass: csrc/bev_pool.hip).  Same arithmetic contract as bev_pool_v2 —
 * `out` is (B,Z,Y,X,C) = (n_voxels, C) rows — with these additions / differences:
 *   n_points        length of the three rank vectors (the reference passes it implicitly as
 *                   tensor sizes, bev_pool.cpp:30-57);
 *   n_voxels        rows of `out` (B*Z*Y*X, < 2^30); EVERY row is written (empty voxels as 0), so `out`
 *                   needs no pre-zeroing (pre-zeroed, as the reference's caller does, is fine too);
 *   workspace       scratch of at least ocrf_bev_pool_v2_workspace_bytes(c, n_points, n_voxels) bytes,
 *                   16-byte aligned; contents are don't-care on entry and exit;
 *   stream          hipStream_t.
 * ANY interval layout is accepted, like the reference's kernel: unsorted, overlapping, empty intervals, gaps
 * (points outside every interval are ignored).  Two intervals that name the same voxel race in the reference
 * (two threads assign the same row); here one of them wins as well.  Channel counts outside C % 4 == 0,
 * 32 <= C <= 256 take the reference's own thread mapping (then `out` must be pre-zeroed).
 * Results are bitwise reproducible run to run (no float atomics); a voxel whose points lie inside one 32-point
 * sub-chunk of its tile's point list is summed in exactly the reference's order.
 */
int ocrf_bev_pool_v2(int c, int n_intervals, int n_points, long n_voxels, const float *depth, const float *feat,
                     const int *ranks_depth, const int *ranks_feat, const int *ranks_bev,
                     const int *interval_starts, const int *interval_lengths, float *out,
                     void *workspace, size_t workspace_bytes, ocrf_stream_t stream);

size_t ocrf_bev_pool_v2_workspace_bytes(int c, int n_points, long n_voxels);

/*
 * Fused forward: the same pass writing the layout the reference reaches with its passes AFTER the op, directly:
 *   layout 0: out[b][c][z][y][x]      == bev_pool_v2(...) of the reference, i.e. the op's
 *                                        permute(0,4,1,2,3).contiguous() (bev_pool.py:91);
 *   layout 1: out[b][z*C + c][y][x]   == torch.cat(bev_feat.unbind(dim=2), 1), what
 *                                        voxel_pooling_v2 / fast_sampling return
 *                                        (view_transformer.py:194, view_transformer_ocrf.py:781).
 * Every element of `out` is written exactly once (64 voxels x C channels per workgroup, 256-byte runs per
 * channel).  (B,Z,Y,X) is the reference's bev_feat_shape without C (B*Z*Y*X < 2^30).  Needs C % 4 == 0,
 * 32 <= C <= 256; ranks_bev values outside [0, B*Z*Y*X) are ignored.
 * workspace >= ocrf_bev_pool_v2_nchw_workspace_bytes(c, n_intervals, n_points, B, Z, Y, X).
 */
int ocrf_bev_pool_v2_nchw(int c, int n_intervals, int n_points, const float *depth,
                          const float *feat, const int *ranks_depth, const int *ranks_feat,
                          const int *ranks_bev, const int *interval_starts,
                          const int *interval_lengths, float *out, int B, int Z, int Y, int X,
                          int layout, void *workspace, size_t workspace_bytes,
                          ocrf_stream_t stream);

/*
 * Plans for rank vectors that stay the same across calls (static calibration: the reference's
 * `accelerate=True`, pre_compute at view_transformer.py:257-262 / view_transformer_ocrf.py:854-866).
 * ocrf_bev_pool_plan_build runs the rank-only part of the pooling once — the dense voxel table, the list of
 * work units (tiles and slices of heavy tiles), their split over the XCDs — and keeps it in `plan` (device
 * memory, caller-owned, >= ocrf_bev_pool_plan_bytes(c, n_points, B, Z, Y, X) bytes, 16-byte aligned);
 * ocrf_bev_pool_v2_nchw_planned is ocrf_bev_pool_v2_nchw for exactly those rank vectors (same c, n_points,
 * grid) as ONE launch: same results bit for bit.  ranks_bev / interval_* are not needed again after the build.
 * The plan holds the arrival counters of the cut tiles (left at zero by every call), so a plan serves one
 * stream at a time.  workspace >= ocrf_bev_pool_planned_workspace_bytes(c, n_points).
 */
size_t ocrf_bev_pool_plan_bytes(int c, int n_points, int B, int Z, int Y, int X);
int ocrf_bev_pool_plan_build(int c, int n_intervals, int n_points, const int *ranks_bev,
                             const int *interval_starts, const int *interval_lengths, int B, int Z, int Y, int X,
                             void *plan, size_t plan_bytes, ocrf_stream_t stream);
size_t ocrf_bev_pool_planned_workspace_bytes(int c, int n_points);
int ocrf_bev_pool_v2_nchw_planned(int c, int n_points, const float *depth, const float *feat,
                                  const int *ranks_depth, const int *ranks_feat, void *plan, float *out,
                                  int B, int Z, int Y, int X, int layout, void *workspace,
                                  size_t workspace_bytes, size_t depth_bytes, size_t feat_bytes, ocrf_stream_t stream);
/* depth_bytes / feat_bytes: the sizes of the two operand tensors in bytes (0: not stated).  The kernels address them with
 * 32-bit byte offsets (the reference indexes with int, bev_pool_cuda.cu:39-47): an operand or an output of 2 GiB or more is
 * refused (hipErrorInvalidValue), and a stated feat_bytes bounds the kernel's feature loads (a rank beyond it reads 0). */

/* Same, for rank vectors whose lengths were produced on the device (ocrf_lss_prepare /
 * ocrf_ht_prepare): the vectors are passed at their capacities and `counts` (device, int32) holds
 * [n_points, n_intervals]; the launches are sized for the capacities and workgroups past the real
 * end retire at once, so nothing between index preparation and pooling reads the device.
 * Workspace: ocrf_bev_pool_v2_nchw_workspace_bytes(c, cap_intervals, cap_points, B, Z, Y, X). */
int ocrf_bev_pool_v2_nchw_dyn(int c, int cap_intervals, int cap_points, const int *counts,
                              const float *depth, const float *feat, const int *ranks_depth,
                              const int *ranks_feat, const int *ranks_bev, const int *interval_starts,
                              const int *interval_lengths, float *out, int B, int Z, int Y, int X,
                              int layout, void *workspace, size_t workspace_bytes, ocrf_stream_t stream);
size_t ocrf_bev_pool_v2_nchw_workspace_bytes(int c, int n_intervals, int n_points, int B, int Z, int Y, int X);

/*
 * Writes *flag (device int) = 0 if interval_starts/lengths are the ascending, non-overlapping cover the
 * reference's producers build (view_transformer.py:240-255) for n_points points, else a non-zero bit mask
 * (1: not ascending / overlapping, 2: interval exceeds n_points, 4: negative start or length).
 */
int ocrf_bev_pool_v2_check_intervals(int n_intervals, int n_points, const int *interval_starts,
                                     const int *interval_lengths, int *flag, ocrf_stream_t stream);

/* Stream-taking, error-returning form of bev_pool_v2_grad (same arithmetic; deterministic). */
int ocrf_bev_pool_v2_grad(int c, int n_intervals, const float *out_grad, const float *depth,
                          const float *feat, const int *ranks_depth, const int *ranks_feat,
                          const int *ranks_bev, const int *interval_starts,
                          const int *interval_lengths, float *depth_grad, float *feat_grad,
                          ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Gaussian rasteriser forward (RGB + depth + transmittance), batched over views
 * ------------------------------------------------------------------------------------------
 * Replaces `rasterize_gaussians` of the w-depth `diff_gaussian_rasterization` extension,
 *   std::tuple<int, Tensor color, Tensor radii, Tensor geomBuffer, Tensor binningBuffer,
 *              Tensor imgBuffer[, Tensor depth]>
 *   RasterizeGaussiansCUDA(background, means3D, colors, opacity, scales, rotations,
 *                          scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
 *                          tan_fovy, image_height, image_width, sh, degree, campos, prefiltered)
 * (mmdet3d/models/necks/MVSGaussian/lib/submodules/diff-gaussian-rasterization/
 *  rasterize_points.cu:35-115), for the argument combination OcRFDet uses
 * (gaussian_renderer/__init__.py:62-70): colours precomputed (no SH evaluation), covariance from
 * (scales, rotations) or cov3D_precomp.  One call renders n_views cameras over the same P
 * Gaussians (n_views = 1 is the reference's call).
 *
 *   means3D (P,3)  colors (P,3)  opacities (P)  scales (P,3)  rotations (P,4) [r,x,y,z; not
 *   normalised, forward.cu:127]  cov3D_precomp (P,6) or NULL (then scales/rotations are used)
 *   cameras (n_views, 36) floats: viewmatrix[16] | projmatrix[16] | tanfovx | tanfovy |
 *           focal_x = W/(2 tanfovx) | focal_y = H/(2 tanfovy); both matrices are the TRANSPOSED
 *           (row-vector) 4x4 the reference passes (auxiliary.h:58-77)
 *   bg (3)         depth_mode 0 = median depth (w-depth default, 15.0 where T never crosses 0.5),
 *                             1 = mean depth (the fork's commented-out alternative)
 * outputs (caller-allocated, fully written):
 *   out_color (n_views,3,H,W)  out_depth (n_views,H,W)  out_final_T (n_views,H,W) [= 1 - accumulated
 *   opacity]  out_n_contrib (n_views,H,W) or NULL (inference: only the backward reads it; NULL drops its
 *   tracking from the blend)  radii (n_views,P)  tiles_touched (n_views,P) or NULL
 *   status (device int, may be NULL; written by the call): informational.  Bit 1 (value 2) is set when
 *   some tile met more than ~1 000 Gaussians inside ONE 0.2 %-wide depth bucket, more than the in-LDS
 *   sort holds; such a tile is then blended by an exact but slower streaming selection over that
 *   bucket.  Results are exact either way; bit 0 is never set (reserved).
 * P == 0 zero-fills the outputs like the reference (rasterize_points.cu:68-69).
 * No host synchronisation happens (the reference reads num_rendered back, rasterizer_impl.cu:281).
 */
int ocrf_rasterize_forward(int P, int n_views, int H, int W, const float *means3D,
                           const float *colors, const float *opacities, const float *scales,
                           float scale_modifier, const float *rotations, const float *cov3D_precomp,
                           const float *cameras, const float *bg, int depth_mode, float *out_color,
                           float *out_depth, float *out_final_T, uint32_t *out_n_contrib, int *radii,
                           uint32_t *tiles_touched, int *status, void *workspace,
                           size_t workspace_bytes, ocrf_stream_t stream);

/*
 * The same forward over n_sets Gaussian sets of P Gaussians each in ONE set of launches: the arrays
 * are (n_sets, P, .), `cameras` holds n_sets * views_per_set rows and view v renders set
 * v / views_per_set (the per-sample loop of view_transformer_ocrf.py:1090-1153 — every sample has its
 * own Gaussian parameters and one camera — or the frames of a multi-frame batch).  Outputs are indexed
 * by view as above; workspace as for n_sets * views_per_set views.
 */
int ocrf_rasterize_forward_sets(int P, int n_sets, int views_per_set, int H, int W, const float *means3D,
                                const float *colors, const float *opacities, const float *scales,
                                float scale_modifier, const float *rotations, const float *cov3D_precomp,
                                const float *cameras, const float *bg, int depth_mode, float *out_color,
                                float *out_depth, float *out_final_T, uint32_t *out_n_contrib, int *radii,
                                uint32_t *tiles_touched, int *status, void *workspace,
                                size_t workspace_bytes, ocrf_stream_t stream);

size_t ocrf_rasterize_workspace_bytes(int P, int n_views);

/*
 * Static render plans (csrc/raster_plan.hip).  In OcRFDet the Gaussian means are the fixed voxel grid
 * (view_transformer_ocrf.py:651-673,690-692) and the cameras are fixed per calibration; what depends on
 * (mean, camera) alone — the near-plane cull and view-space depth (auxiliary.h:139-164), the projected centre and
 * the Jacobian of computeCov2D (forward.cu:83-98,196-199), hence the whole (depth bits, id) blend order the
 * reference obtains by sorting every step (rasterizer_impl.cu:226-267) — is computed ONCE:
 *
 *   1. ocrf_raster_plan_count     (sizing, optional) how many (Gaussian, view) records a plan for these cameras keeps:
 *      g_mask (device, P words; bit v = view v keeps the Gaussian) and their number in *total (device).  The caller
 *      reads the total once and chooses a record CAPACITY (with headroom if the plan will be rebuilt for other poses).
 *   2. ocrf_raster_plan_build     writes the plan (device, >= ocrf_raster_plan_bytes(P, n_views, capacity) bytes,
 *      256-byte aligned): header, cameras; per view the kept records in blend order (id, depth bits, pixel centre);
 *      per Gaussian the views that keep it (never visible = behind the near plane, or outside the frame for every
 *      world-space extent <= extent_bound) and, per (Gaussian, view), the record's place in that order with the rows
 *      of J W (forward.cu:83-98).  NO host read and kernels only (hipGraph-capturable): classify all views ->
 *      exclusive scan -> records + one 32-bit sort key per record (view << 27 | depth bits - 0x3E000000: view-space
 *      depths in [0.125, 8191) m) -> ONE stable radix sort -> gather.  It may be called again on the same buffers
 *      with other cameras — the reference recomputes the render cameras from the dataloader's c2w for every sample
 *      (view_transformer_ocrf.py:1140-1152) — a rebuild per sample is ~ 20 launches.  A plan whose records exceed
 *      `capacity`, a depth outside the key range or a scan that gave up leave the plan marked unusable ON THE DEVICE
 *      (every render of it raises status bit 8).  workspace >= ocrf_raster_plan_build_workspace_bytes(P, n_views,
 *      capacity).
 *
 * extent_bound bounds scale_modifier * max_k |s_k| * |R(q)|_2 (|R(q)|_2 = |1 - |q|^2| + |q|^2: 1 for a normalised
 * quaternion) of every Gaussian the plan will be rendered with; a plan stays valid for ANY parameters within it.
 *
 *   3. ocrf_rasterize_planned     one render = the front end + the blend of the sorted lists.  Front end, when radii
 *      are an output (radii != NULL with guard 0, or guard bit 1): one thread per Gaussian builds its 3D covariance once
 *      and writes conic / tile rect of EVERY rendered view's record (record order: coalesced; the blend walks a view's
 *      depth-ordered list through the plan's static list -> record map).  Else (round 5): only the HEAD of every rendered
 *      view's list is prepared, in list order (a tile pair stops scanning once its pixels are saturated — at cfg2 after
 *      ~500 of 120 000 entries); a tile pair that scans further extends the arrays itself, and the head's length
 *      follows what the previous call needed (kept in `workspace`, no host read).  The extent check of all Gaussians
 *      then runs behind the blend (a status bit) — or in front of it with the device guard.
 *      n_items views are rendered; item z renders plan view item_view[z] (device ints; NULL = z, then n_items /
 *      n_sets must equal the plan's view count) with Gaussian set z / (n_items / n_sets) of the (n_sets, P, .)
 *      parameter arrays; the items of one set name distinct views.  Outputs as
 *      ocrf_rasterize_forward, indexed by item; colour / depth / final_T are bit-identical to it.  radii
 *      (n_items, P) or NULL.  `capacity`: the plan's record capacity (as given to the build).
 *      workspace >= ocrf_rasterize_planned_workspace_bytes(capacity, n_sets).
 *      views_disjoint = 1: the caller states that every plan view is rendered by at most ONE set of this call (frames
 *      of a sample sharing a plan, each with its own parameter set): all sets then share one copy of the per-call
 *      record arrays (workspace >= ocrf_rasterize_planned_workspace_bytes(capacity, 1)), every line of which is
 *      written once; a view named by two sets raises status bit 3 (value 8).  0: a copy per set.
 *      call_cameras (device, n_plan_views x 36 floats, or NULL): the cameras THIS call means to render with.  The
 *      head kernel compares them with the plan's, bit for bit, on the device; a difference raises status bit 4
 *      (value 16) and — with guard = 1 — hands the call to the armed per-call pipeline, which then renders with
 *      call_cameras: a stale plan can not silently render another pose.
 *      status (device int, NOT written unless something is wrong: zero it once): bit 2 (value 4) = some Gaussian
 *      exceeded extent_bound this call, bit 3 (value 8) = bad item_view / unusable plan.
 *      guard = 0: with bit 2 set the outputs of that call are not valid (the caller re-renders with
 *      ocrf_rasterize_forward or rebuilds the plan with a larger bound).
 *      guard = 1 (+ 2: the radii are an output too; without it the radii buffer is the armed chain's scratch only):
 *      the per-call pipeline of ocrf_rasterize_forward is enqueued behind the planned one, armed by the
 *      extent check: all of its kernels retire at once when the bound holds, and render the call instead when it
 *      does not — exact results either way, no host involvement (hipGraph-capturable), at the price of four
 *      near-empty launches (no memsets: the flag is raised by the extent check / head kernel and lowered by the armed blend, the
 *      chain's histograms are cleared by the planned blend when the flag is up, radii zeros come from the update
 *      kernel).  Needs means3D, radii and chain_workspace >= ocrf_rasterize_workspace_bytes(P, n_items); `workspace`
 *      must be zero-filled when it is allocated and belong to this plan alone (it carries the flag between calls; a
 *      stale non-zero flag costs one slow, still exact, call).
 *      blend_workgroups: size of the blend's persistent grid (its workgroups draw tile pairs from a ticket queue);
 *      0 = as many as the device holds at once (fastest alone).  The blend is VALU-bound: two workgroups per CU keep
 *      most of its speed and leave the other wave slots to kernels of other streams (the hot path renders beside its
 *      latency-bound poolings with 2 x CUs: -13 % step time at cfg2).
 *      yield_if (device int or NULL): a scheduling hint.  With it the blend is launched on every slot the device has
 *      and the workgroups beyond `blend_workgroups` leave at once while *yield_if != 0 — the caller raises the word
 *      (ocrf_stream_write_value32) while another stream's chain should keep those wave slots and lowers it when that
 *      chain is done, so that later renders of the same step take the whole chip.  Any value renders the same image.
 *      phase: 0 = both launches; 1 = only the update, 2 = only the blend of a call whose update already ran (guard 0
 *      only) — the two may then sit on different streams (the update is memory-bound, the blend VALU-bound: frame
 *      n + 1's update runs under frame n's blend), ordered by the caller's events.
 * Forward only (no n_contrib): training renders through ocrf_rasterize_forward / _backward.
 */
size_t ocrf_raster_plan_count_workspace_bytes(int P);
int ocrf_raster_plan_count(int P, int n_views, int H, int W, const float *means3D, const float *cameras,
                           float extent_bound, unsigned *g_mask, int *total, void *workspace,
                           size_t workspace_bytes, ocrf_stream_t stream);
size_t ocrf_raster_plan_build_workspace_bytes(int P, int n_views, long capacity);
size_t ocrf_raster_plan_bytes(int P, int n_views, long capacity);
int ocrf_raster_plan_build(int P, int n_views, int H, int W, const float *means3D, const float *cameras,
                           float extent_bound, long capacity, void *workspace, size_t workspace_bytes, void *plan,
                           size_t plan_bytes, ocrf_stream_t stream);
size_t ocrf_rasterize_planned_workspace_bytes(long capacity, int n_sets);
int ocrf_rasterize_planned(const void *plan, size_t plan_bytes, int P, int n_plan_views, long capacity,
                           int H, int W, int n_sets, int n_items, const int *item_view,
                           const float *colors, const float *opacities, const float *scales, float scale_modifier,
                           const float *rotations, const float *bg, int depth_mode, float *out_color,
                           float *out_depth, float *out_final_T, int *radii, int *status, void *workspace,
                           size_t workspace_bytes, int guard, const float *means3D, void *chain_workspace,
                           size_t chain_workspace_bytes, int blend_workgroups, const int *yield_if, int phase,
                           const float *call_cameras, int views_disjoint, const void *bins, size_t bins_bytes,
                           int bin_w, int bin_h, long cand_capacity, int *hint, ocrf_stream_t stream);
/* hint (or NULL): one int in memory BOTH the host and the device can address (pinned host memory: hipHostMalloc), zero at
 * first.  The last workgroup of a render writes "some rendered view is deep" into it; the next call reads it ON THE HOST,
 * without a copy or a wait, to choose between the two builds of the blend — the plain one, and the one that compacts the
 * candidates of deep views per call (see ocrf_rasterize_planned_bins_workspace_bytes).  A stale value costs time, never
 * correctness; a replayed step (ocrf_step_*) re-reads it at every replay. */
/*
 * Candidate lists of a built plan — the static part of what the reference builds per call as its per-tile lists
 * (cuda_rasterizer/rasterizer_impl.cu:70-138 duplicateWithKeys + identifyTileRanges, consumed forward.cu:261-374): per
 * (plan view, bin of bin_w x bin_h tile PAIRS, i.e. bin_w x 2 bin_h tiles of 16 x 16 px) the positions, ascending (= blend
 * order), of the view's records whose tile rect for ANY parameters within the plan's extent bound reaches the bin.  With
 * them (bins != NULL in ocrf_rasterize_planned; bin_w / bin_h / cand_capacity as given to the build) a tile pair tests the
 * rects of its bin's candidates instead of the view's whole list: its cost is O(own records).  Same images bit for bit.
 *   ocrf_raster_plan_bins_build: `plan` built on this stream before; no host read, kernels only.  cand_capacity = 0 is a
 *   sizing pass (only *total_out, a device int, is written); lists that do not fit the capacity leave `bins` unusable — it
 *   is then ignored by renders (whole lists are walked), never wrong.  workspace >=
 *   ocrf_raster_plan_bins_workspace_bytes(...), bins >= ocrf_raster_plan_bins_bytes(...).
 * A planned render runs in two passes of the blend: the first renders every tile pair as far as the PREPARED head of its
 * view's list reaches (the head follows what the last call needed, up to the whole list) and hands the tile pairs that
 * need more to the second; between them the records behind the heads are prepared ONCE (inside the extent-check launch),
 * only if a tile pair asked.  A tile pair never prepares records itself.
 */
size_t ocrf_raster_plan_bins_bytes(int n_views, int H, int W, int bin_w, int bin_h, long cand_capacity);
/* per-call scratch of ocrf_rasterize_planned when it is given candidate lists: as ocrf_rasterize_planned_workspace_bytes
 * plus room for the per-call compaction of "deep" views — views whose last render walked 8 192 list entries or more
 * (pixels that do not saturate early: an object-centric opacity field).  For those the head of the list is the whole
 * list and, per segment of 1 024 candidates of a bin, the candidates whose rect of THIS call reaches the bin are moved to
 * the front with the mask of the bin's tiles they cover (the per-call half of duplicateWithKeys,
 * rasterizer_impl.cu:70-109), so that a tile pair reads only records that can concern it.  A workspace of the smaller
 * size is accepted when bins == NULL. */
size_t ocrf_rasterize_planned_bins_workspace_bytes(long capacity, int n_sets, int n_views, int H, int W, int bin_w,
                                                   int bin_h, long cand_capacity);
size_t ocrf_raster_plan_bins_workspace_bytes(int P, int n_views, int H, int W, int bin_w, int bin_h, long capacity);
int ocrf_raster_plan_bins_build(const void *plan, size_t plan_bytes, int P, int n_views, long capacity, int H, int W,
                                float extent_bound, int bin_w, int bin_h, long cand_capacity, void *bins,
                                size_t bins_bytes, int *total_out, void *workspace, size_t workspace_bytes,
                                ocrf_stream_t stream);

/*
 * bev_pool_v2 forward as per-tile MFMA panels (csrc/bev_pool_mfma.hip): out[64 voxels x C] = W[64 x R] . F[R x C]
 * with R the tile's UNIQUE feature rows, W[v][r] = the summed depth weights of the tile's points with voxel slot v
 * and row slot r, on v_mfma_f32_16x16x4_f32 (f32 in / f32 accumulate: an exact fmaf chain, bitwise reproducible).
 * Same result as ocrf_bev_pool_v2_nchw up to the summation order (reference semantics: bev_pool_cuda.cu:39-47).
 * The rank-only part is a plan the caller builds once (ocrfdet_amd/bevpool.MfmaPoolPlan shows how), all device ints:
 *   units (n_units x 4)      {tile, first panel, end panel, slice | n_slices << 16}: a tile's panels in groups; tiles
 *                            without points have one unit with no panel (they are written as zeros); every tile of the
 *                            (B*Z) planes x ceil(Y / 8) x ceil(X / 8) grid appears (tile = plane * tpp + ty * tx_count + tx)
 *   unit_slab (n_units)      first slab of the unit's tile (tiles of several units), else anything
 *   panel_rows (n_panels x R_p), panel_nrows (n_panels)   feature rows of a panel (R_p = ocrf_bev_pool_mfma_panel_rows())
 *   panel_cell_off (n_panels + 1), cells (n_cells x 4): {v | r << 8 | points << 16, depth ranks of the (up to three)
 *                            points in summation order}; a cell of more points: {v | r << 8 | 0xFFFF << 16, first
 *                            index into rd_sorted, points, -}; rd_sorted: depth ranks of all points in cell order
 *                            a unit holds at most ocrf_bev_pool_mfma_max_unit_panels() panels
 *   arrive (n_tiles ints, zero before the first call; left zero), slabs (>= ocrf_bev_pool_mfma_slab_bytes(c, slices))
 * C in {64, 80, 96, 128}; layouts as ocrf_bev_pool_v2_nchw (+ 2: rows (n_vox, C)).
 */
int ocrf_diag_pool_mfma_stamps(unsigned long long *buf); /* diagnostic: per-unit phase cycles of the next C = 80 calls */
int ocrf_bev_pool_mfma_panel_rows(void);
int ocrf_bev_pool_mfma_tile_side(void); /* tiles are side x side voxel blocks of a (b, z) plane, row-major; slot v = side * dy + dx */
size_t ocrf_bev_pool_mfma_slab_bytes(int c, int n_slab_slices);
int ocrf_bev_pool_mfma_max_unit_panels(void);
int ocrf_bev_pool_v2_nchw_mfma(int c, int n_units, const int *units, const int *unit_slab, const int *panel_rows,
                               const int *panel_nrows, const int *panel_cell_off, const int *cells,
                               const int *rd_sorted, const float *depth, const float *feat,
                               float *out, int B, int Z, int Y, int X, int layout, int *arrive, void *slabs,
                               ocrf_stream_t stream);

/*
 * The same plan as a latency kernel (csrc/bev_pool_panel.hip): the cells' depth weights are summed by a pre-pass
 * (ocrf_bev_pool_cell_weights: one thread per cell, up to two cell lists per launch — the LSS and the height-sampling
 * plan of a step read the same depth tensor; either list may be empty); in the pooling kernel a lane is a voxel slot
 * (a wave a quarter of the channels) and walks its cells out of LDS: acc = fma(F[r], w(v, r), acc) with rows ascending,
 * panel after panel — the k order of the MFMA form, bit-identical to it on finite inputs; bitwise reproducible.
 * Extra plan arrays (device): the cells of a panel are stored VOXEL-major (v ascending, then r —
 * ocrf_bev_pool_v2_nchw_mfma does not depend on the order inside a panel),
 *   panel_voff (n_panels x 64)   first cell of voxel slot v, relative to the panel's first cell
 *   cell_code (n_cells u16)      row slot | voxel slot << 8;     cw (n_cells floats)  the pre-pass's output
 */
int ocrf_diag_pool_panel_stamps(unsigned long long *buf); /* diagnostic: per-unit phase cycles of the next C = 80 calls */
int ocrf_bev_pool_cell_weights(int n_cells0, const int *cells0, const int *rd_sorted0, float *cw0, int n_cells1,
                               const int *cells1, const int *rd_sorted1, float *cw1, const float *depth,
                               ocrf_stream_t stream);
int ocrf_bev_pool_v2_nchw_panel(int c, int n_units, const int *units, const int *unit_slab, const int *panel_rows,
                                const int *panel_nrows, const int *panel_cell_off, const int *panel_voff,
                                const unsigned short *cell_code, const float *cw, const float *feat, float *out, int B,
                                int Z, int Y, int X, int layout, int *arrive, void *slabs, size_t feat_bytes,
                                ocrf_stream_t stream); /* feat_bytes: as for ocrf_bev_pool_v2_nchw_planned */
/*
 * ocrf_bev_pool_v2_nchw_panel + the channel statistics of its output in the same launch: the workgroup that writes a
 * finished tile also writes stats[b][0][y][x] = mean_c out, stats[b][1][y][x] = max_c out for the tile's pixels — what
 * ocrf_hoa_channel_stats computes from the pooled BEV, bit for bit, without reading it again (the height-sampling BEV is
 * what HOA-3 gates: hand stats to ocrf_hoa_opacity_mask_gate).  Every pixel of stats (B, 2, Y, X) is written, empty
 * tiles as zeros.  Z == 1 and layout 0 or 1 only; everything else as ocrf_bev_pool_v2_nchw_panel.
 */
int ocrf_bev_pool_v2_nchw_panel_stats(int c, int n_units, const int *units, const int *unit_slab, const int *panel_rows,
                                      const int *panel_nrows, const int *panel_cell_off, const int *panel_voff,
                                      const unsigned short *cell_code, const float *cw, const float *feat, float *out,
                                      int B, int Z, int Y, int X, int layout, int *arrive, void *slabs, size_t feat_bytes,
                                      float *stats, ocrf_stream_t stream);

/*
 * Backward of the colour output of ocrf_rasterize_forward (the w-depth fork has no depth backward,
 * diff-gaussian-rasterization-w-depth/README.md:13).  Replaces RasterizeGaussiansBackwardCUDA
 * (rasterize_points.cu:117-196 -> rasterizer_impl.cu:338-434 -> cuda_rasterizer/backward.cu) for
 * colours precomputed and covariance from (scales, rotations); gradients are summed over the views.
 *   fwd_color / fwd_final_T / fwd_n_contrib: the forward's outputs for the same inputs
 *   dL_dcolor (n_views,3,H,W)
 * outputs (fully written): dL_dmeans3D (P,3)  dL_dcolors (P,3)  dL_dopacity (P)  dL_dscales (P,3)
 *   dL_drotations (P,4) [w.r.t. the un-normalised quaternion, like the reference]
 *   dL_dmeans2D (n_views,P,3) or NULL [NDC-space screen gradient, z = 0; the reference returns it
 *   for densification statistics]
 * Float atomics are used per (tile, Gaussian): results vary in the last bits run to run, like the
 * reference's (backward.cu:509-541).  Reference quirk kept: a clamped t.x / t.y is treated as a
 * constant (x_grad_mul / y_grad_mul, backward.cu:174-175).
 */
int ocrf_rasterize_backward(int P, int n_views, int H, int W, const float *means3D, const float *colors,
                            const float *opacities, const float *scales, float scale_modifier,
                            const float *rotations, const float *cameras, const float *bg,
                            const float *fwd_color, const float *fwd_final_T, const uint32_t *fwd_n_contrib,
                            const float *dL_dcolor, float *dL_dmeans3D, float *dL_dcolors,
                            float *dL_dopacity, float *dL_dscales, float *dL_drotations,
                            float *dL_dmeans2D, void *workspace, size_t workspace_bytes,
                            ocrf_stream_t stream);
/* The same with the 3-D covariance handed over (cov3D_precomp (P,6): xx xy xz yy yz zz, as the forward takes it):
 * the reference stops at dL/dcov3D then (backward.cu:346-396 without computeCov3D's backward, :598-613):
 * dL_dcov3D (P,6), fully written, off-diagonal entries carry both symmetric halves (backward.cu:251-260). */
int ocrf_rasterize_backward_cov3d(int P, int n_views, int H, int W, const float *means3D, const float *colors,
                                  const float *opacities, const float *cov3D_precomp, const float *cameras,
                                  const float *bg, const float *fwd_color, const float *fwd_final_T,
                                  const uint32_t *fwd_n_contrib, const float *dL_dcolor, float *dL_dmeans3D,
                                  float *dL_dcolors, float *dL_dopacity, float *dL_dcov3D, float *dL_dmeans2D,
                                  void *workspace, size_t workspace_bytes, ocrf_stream_t stream);
size_t ocrf_rasterize_backward_workspace_bytes(int P, int n_views);
/* The backward with the gradients of the two outputs the w-depth fork leaves without one: the MEAN depth
 * D = sum_i alpha_i T_i z_i of depth_mode 1 (unnormalised, 0 where nothing is hit; the median depth is piecewise
 * constant and has no gradient) and final_T.  D and 1 - final_T are two more colour channels with the constant colours
 * z_i and 1 over a zero background; z_i = view[:,2] . (mean_i, 1) adds (view[0][2], view[1][2], view[2][2]) * dL/dz_i to
 * dL_dmeans3D.
 *   fwd_depth (n_views,H,W): the forward's out_depth at depth_mode 1 for the same inputs
 *   dL_ddepth / dL_dfinal_T (n_views,H,W): either may be NULL (zeros), not both: that is the case of the two entries
 *   above.  dL_ddepth without fwd_depth is refused.  dL_dcolor is required (zeros if the colour got no gradient).
 * Covariance as in the two entries above: cov3D_precomp (then dL_dcov3D is written, scales / rotations and their
 * gradients are ignored) or (scales, rotations) with scale_modifier.  Every other argument, output and refusal as
 * there; the workspace is larger (ten sums per (view, Gaussian) instead of nine).  Float atomics per (tile, Gaussian):
 * reproducible to rounding only, exactly as the colour backward. */
int ocrf_rasterize_backward_depth(int P, int n_views, int H, int W, const float *means3D, const float *colors,
                                  const float *opacities, const float *scales, float scale_modifier,
                                  const float *rotations, const float *cov3D_precomp, const float *cameras,
                                  const float *bg, const float *fwd_color, const float *fwd_depth,
                                  const float *fwd_final_T, const uint32_t *fwd_n_contrib, const float *dL_dcolor,
                                  const float *dL_ddepth, const float *dL_dfinal_T, float *dL_dmeans3D,
                                  float *dL_dcolors, float *dL_dopacity, float *dL_dscales, float *dL_drotations,
                                  float *dL_dcov3D, float *dL_dmeans2D, void *workspace, size_t workspace_bytes,
                                  ocrf_stream_t stream);
size_t ocrf_rasterize_backward_depth_workspace_bytes(int P, int n_views);

/*
 * Spherical-harmonics colours (the `shs` argument of the reference's rasteriser; computeColorFromSH,
 * cuda_rasterizer/forward.cu:20-71, used by preprocessCUDA when colors_precomp is NULL, :240-247): for one camera centre
 * `campos` (3 floats on the device), colors[g] = max(0.5 + sum_{i < (deg+1)^2} basis_i(dir_g) * shs[g][i], 0) with dir_g the
 * unit vector from campos to means3D[g]; clamped (P,3) bytes record which channels were clamped (the backward zeroes their
 * gradient, backward.cu:33-36).  shs (P, max_coeffs, 3), deg in 0..3, max_coeffs >= (deg+1)^2.  The (P,3) colours feed
 * ocrf_rasterize_forward as its `colors` for that view.
 * Backward (backward.cu:20-140): dL_dshs (P, max_coeffs, 3) is fully written (zero above the active degree); the
 * direction's dependence on the mean is ADDED to dL_dmeans3D (P,3) (which already holds the rasteriser's part).
 */
int ocrf_sh_to_rgb(int P, int deg, int max_coeffs, const float *means3D, const float *campos, const float *shs,
                   float *colors, unsigned char *clamped, ocrf_stream_t stream);
int ocrf_sh_to_rgb_backward(int P, int deg, int max_coeffs, const float *means3D, const float *campos,
                            const float *shs, const unsigned char *clamped, const float *dL_dcolors,
                            float *dL_dmeans3D, float *dL_dshs, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training losses of the neck (csrc/losses.hip): view_transformer_ocrf.py get_loss (:1354-1417) and its helpers.
 * Deterministic: per-block partials, then one fixed-order final sum; no float atomics.  No entry writes its inputs.
 *
 * ocrf_depth_labels (get_downsampled_gt_depth_and_semantic, :1203-1282): gt_depth / gt_semantic (BN,H,W) f32, H and W
 *   multiples of ds -> depth_labels (BN*h*w, D) and semantic_labels (BN*h*w, 2), h = H/ds, w = W/ds.  Depths outside
 *   [d_min, d_max] (strict comparisons) and their semantics count as 0; the bin is (m - (float)(d_min - d_step)) /
 *   (float)d_step; rows whose semantic max is 1 get the normalised histogram of the patch's depth x semantic bins
 *   (NaN when it is empty, as the reference).  Bit for bit the reference's labels.
 * ocrf_depth_semantic_loss (get_depth_and_semantic_loss, :1284-1314): depth (BN,D,h,w) and semantic (BN,2,h,w) softmax
 *   outputs in NCHW, HW = h*w.  out[0] = w_depth * sum BCE * w / max(0.1, sum w), out[1] = w_semantic * focal BCE /
 *   max(1, rows) over the rows whose depth label max is > 0; denoms[2] (device) keeps the two divisors for the backward.
 *   Two launches; workspace from ocrf_depth_semantic_loss_workspace_bytes(BN*HW).
 * ocrf_depth_semantic_loss_backward: grad_out (2 floats, device) -> grad_depth (BN,D,h,w), grad_semantic (BN,2,h,w),
 *   every element written.
 * ocrf_render_losses (the per-sample loop of get_loss, :1370-1410): K (1..3) renders r0..r2 (B,C,H,W) against gt
 *   (>= B,C,H,W), all multiplied by the Box2dtoMask mask of boxes (B,n_max,4) (n_max <= 256) when use_mask; meta (int,
 *   device): [0,B) box counts, [B,2B) camera of each sample.  With gt_depth (B,n_cams,H,W) also the depth L1 of rd0..rd2
 *   (B,1,H,W) against the range-zeroed, min-max normalised gt depth of the sample's camera (gt_depth NULL: no depth
 *   term).  out[3] (device) = {w_color * mean MSE, w_ssim * mean (1 - SSIM), w_depth * mean L1}, means over samples and
 *   renders; SSIM window 11, sigma 1.5, zero padding.  saved (B*C*K*3*H*W floats) and depth_stats (2B floats) are the
 *   state of the backward.  Three launches (two without the depth term); workspace from
 *   ocrf_render_losses_workspace_bytes(B, C, H, W).
 * ocrf_render_losses_backward: the same arguments + saved state and grad_out (3 floats, device) -> grad_r0..2 (B,C,H,W)
 *   and grad_rd0..2 (B,1,H,W); NULL outputs are skipped.  One launch.
 */
int ocrf_depth_labels(int BN, int H, int W, int ds, int D, double d_min, double d_max, double d_step,
                      const float *gt_depth, const float *gt_semantic, float *depth_labels, float *semantic_labels,
                      ocrf_stream_t stream);
size_t ocrf_depth_semantic_loss_workspace_bytes(int rows);
int ocrf_depth_semantic_loss(int BN, int HW, int D, const float *depth_labels, const float *semantic_labels,
                             const float *depth, const float *semantic, float w_depth, float w_semantic, float *out,
                             float *denoms, void *workspace, size_t workspace_bytes, ocrf_stream_t stream);
int ocrf_depth_semantic_loss_backward(int BN, int HW, int D, const float *depth_labels, const float *semantic_labels,
                                      const float *depth, const float *semantic, float w_depth, float w_semantic,
                                      const float *denoms, const float *grad_out, float *grad_depth,
                                      float *grad_semantic, ocrf_stream_t stream);
size_t ocrf_render_losses_workspace_bytes(int B, int C, int H, int W);
int ocrf_render_losses(int B, int K, int C, int H, int W, const float *gt, const float *r0, const float *r1,
                       const float *r2, const float *boxes, const int *meta, int n_max, int use_mask,
                       const float *gt_depth, int n_cams, const float *rd0, const float *rd1, const float *rd2,
                       float d_min, float d_max, float w_color, float w_ssim, float w_depth, float *out, float *saved,
                       float *depth_stats, void *workspace, size_t workspace_bytes, ocrf_stream_t stream);
int ocrf_render_losses_backward(int B, int K, int C, int H, int W, const float *gt, const float *r0, const float *r1,
                                const float *r2, const float *boxes, const int *meta, int n_max, int use_mask,
                                const float *gt_depth, int n_cams, const float *rd0, const float *rd1, const float *rd2,
                                float d_min, float d_max, float w_color, float w_ssim, float w_depth, const float *saved,
                                const float *depth_stats, const float *grad_out, float *grad_r0, float *grad_r1,
                                float *grad_r2, float *grad_rd0, float *grad_rd1, float *grad_rd2,
                                ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Stereo cost volume of the depth network (csrc/stereo.hip): view_transformer.py DepthNet.gen_grid +
 * calculate_cost_volumn (:538-596), forward only (the reference runs it under no_grad).
 *
 * ocrf_stereo_cost_volume: prev, curr (BN,C,H,W) f32 contiguous, C >= 4 (channels past the last whole group of 4 are
 *   ignored); the frustum's axes u[W], v[H], d[D] as strided views (element strides stride_*, e.g. the (D,H,W,3)
 *   cv_frustum's [0,0,:,0], [0,:,0,1], [:,0,0,2]); per camera the raw k2s_sensor (BN,4,4), intrins (BN,3,3),
 *   post_rots (BN,3,3) and post_trans (BN,3), contiguous.  The image size is (4 H, 4 W).  out (BN,D,H,W) NCHW:
 *   mode 0 the softmax over D of raw, mode 1 raw = -(cost + bias [warped channel 4 (C/4 - 1) == 0]).  The 3x3 inverses
 *   are taken in the kernel.  One launch, deterministic, no atomics.  Limits: one camera's prev is addressed in unsigned
 *   32-bit bytes, so C*H*W*sizeof(float) <= 2^32 - 1 (C = 256 allows H*W < 2^22), and D*H*W < 2^31; larger shapes
 *   return hipErrorInvalidValue and launch nothing.
 */
int ocrf_stereo_cost_volume(int BN, int C, int H, int W, int D, const float *prev, const float *curr,
                            const float *frustum_u, long long stride_u, const float *frustum_v, long long stride_v,
                            const float *frustum_d, long long stride_d, const float *k2s_sensor, const float *intrins,
                            const float *post_rots, const float *post_trans, float bias, int mode, float *out,
                            ocrf_stream_t stream);
/*
 * The same volume from bfloat16 features (csrc/stereo_bf16.hip), opt-in: two packs and one launch, float32 arithmetic
 * on the widened values in ocrf_stereo_cost_volume's order, so out holds, bit for bit, what that entry gives on the
 * features cast to float32.
 *
 * ocrf_stereo_pack_bf16: src (BN,C,H,W) bf16 contiguous -> dst (BN,NB,H,W,8) bf16, blocks of 8 channels per pixel, with
 *   G = C / 4 whole groups and NB = (G + 1) / 2: dst[cam][b][y][x][k] = src[cam][8 b + k][y][x] where 8 b + k < 4 G, else
 *   +0 (channels past the last whole group are dropped; the upper half of the last block is zero when G is odd).  Every
 *   element of dst is written; one launch per tensor.  dst 16-byte aligned.
 * ocrf_stereo_cost_volume_bf16: the arguments of ocrf_stereo_cost_volume with prev, curr PACKED as above (16-byte
 *   aligned) and C the channel count of the unpacked features; out (BN,D,H,W) f32, mode as above.  One launch,
 *   deterministic, no atomics.
 * Limits of both: C >= 4, H >= 2, W >= 2; one camera's packed tensor is addressed in unsigned 32-bit bytes, so
 *   NB*H*W*16 <= 2^32 - 1; D*H*W < 2^31; fewer than 2^31 workgroups.  Anything else, a NULL or a misaligned packed
 *   pointer returns hipErrorInvalidValue and launches nothing.
 */
int ocrf_stereo_pack_bf16(int BN, int C, int H, int W, const unsigned short *src, unsigned short *dst,
                          ocrf_stream_t stream);
int ocrf_stereo_cost_volume_bf16(int BN, int C, int H, int W, int D, const unsigned short *prev,
                                 const unsigned short *curr, const float *frustum_u, long long stride_u,
                                 const float *frustum_v, long long stride_v, const float *frustum_d, long long stride_d,
                                 const float *k2s_sensor, const float *intrins, const float *post_rots,
                                 const float *post_trans, float bias, int mode, float *out, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training targets and losses of the detection head (csrc/center_head.hip): centerpoint_head.py CenterHead
 * get_targets_single (:437-585) and loss (:587-668) for every sample and task in one call each.  Deterministic, no host
 * reads, no entry writes its inputs.  T <= OCRF_CH_MAX_TASKS tasks of ncls[t] classes, at most OCRF_CH_MAX_PLANES
 * classes in all; HW = H * W of the feature map.
 *
 * ocrf_center_head_targets: boxes (n_boxes, box_dim) f32 as LiDARInstance3DBoxes.tensor (bottom-centre z; box_dim >= 9
 *   with velocity, else >= 7), labels (n_boxes) int64, offsets (B + 1) int64 (sample b owns rows [offsets[b],
 *   offsets[b+1])), class_table (n_labels, 2) int32 = (task, class in task), task -1 for a label in no task.  The
 *   train_cfg scalars: voxel_size[2], pc_range[2] (host), out_size_factor, gaussian_overlap, min_radius.  Outputs
 *   (device): heatmap = the tasks' (B, ncls[t], H, W) blocks back to back, anno_box (T, B, max_objs, 10 | 8), ind
 *   (T, B, max_objs) int64, mask (T, B, max_objs) uint8, counts[2T] f32 = per task the heatmap pixels equal to 1 and
 *   the mask sum.  A memset of counts and two launches; workspace from ocrf_center_head_targets_workspace_bytes.
 *   A label outside [0, n_labels) is in no task.  radius = max(min_radius, (int)r) of the float32 gaussian_radius r,
 *   with two rules of this library's: a NaN r (an infinite box dimension; the reference raises there) counts as 0, so
 *   the radius falls to min_radius, and r is capped at 65536.
 * ocrf_center_head_heatmap_loss: logits[T] (host table of device (B, ncls[t], HW) f32) against the targets' heatmap ->
 *   clipped[T] (clip_sigmoid, same shapes), out[T] = loss_weight * gaussian focal sum / (float)(max(counts[t], 1) +
 *   FLT_EPSILON) and dens[T] for the backward.  Two launches; workspace from ..._heatmap_loss_workspace_bytes.
 * ocrf_center_head_heatmap_loss_backward: grad_out[T] (device) -> grad_logits[T] (host table), every element written.
 *   One launch.
 * ocrf_center_head_reg_loss: heads[5T] (host table: per task reg (B,2,HW), height (B,1,HW), dim (B,3,HW), rot (B,2,HW),
 *   vel (B,2,HW); vel unused without velocity), the targets' anno_box / ind / mask, code_weights[10 | 8] (host) ->
 *   out (T, 6) f32: loss_weight * the L1 sums of code groups [0,2,3,6,8,10) over (num + 1e-4) + FLT_EPSILON, and in
 *   column 5 of all codes over num + FLT_EPSILON, num = max(counts[T + t], 1e-4); dens (T, 2) for the backward.  Two
 *   launches; workspace from ocrf_center_head_reg_loss_workspace_bytes.
 * ocrf_center_head_reg_loss_backward: grad_out (T, 6) (device) -> grad_heads[5T] (host table, zero-filled by the
 *   caller): only the pixels at ind are written, duplicate indices summed in slot order.  One launch, max_objs <= 16384.
 *   The sign of pred - target is 0 where it is NaN, as autograd's abs has it: a NaN target code (weight 0) makes its
 *   loss NaN and its gradient 0, and leaves every other gradient finite.
 */
#define OCRF_CH_MAX_TASKS 8
#define OCRF_CH_MAX_PLANES 64
size_t ocrf_center_head_targets_workspace_bytes(int n_boxes);
int ocrf_center_head_targets(int B, int T, const int *ncls, int n_labels, const int *class_table, int n_boxes,
                             int box_dim, const float *boxes, const long long *labels, const long long *offsets, int H,
                             int W, int max_objs, int with_velocity, int norm_bbox, const float *voxel_size,
                             const float *pc_range, int out_size_factor, double gaussian_overlap, int min_radius,
                             float *heatmap, float *anno_box, long long *ind, unsigned char *mask, float *counts,
                             void *workspace, size_t workspace_bytes, ocrf_stream_t stream);
size_t ocrf_center_head_heatmap_loss_workspace_bytes(int B, int T, const int *ncls, int HW);
int ocrf_center_head_heatmap_loss(int B, int T, const int *ncls, int HW, const float *const *logits,
                                  const float *heatmap, const float *counts, float loss_weight, float *const *clipped,
                                  float *out, float *dens, void *workspace, size_t workspace_bytes,
                                  ocrf_stream_t stream);
int ocrf_center_head_heatmap_loss_backward(int B, int T, const int *ncls, int HW, const float *const *logits,
                                           const float *heatmap, const float *dens, const float *grad_out,
                                           float loss_weight, float *const *grad_logits, ocrf_stream_t stream);
size_t ocrf_center_head_reg_loss_workspace_bytes(int B, int T);
int ocrf_center_head_reg_loss(int B, int T, int HW, int max_objs, int with_velocity, const float *const *heads,
                              const float *anno_box, const long long *ind, const unsigned char *mask,
                              const float *code_weights, const float *counts, float loss_weight, float *out,
                              float *dens, void *workspace, size_t workspace_bytes, ocrf_stream_t stream);
int ocrf_center_head_reg_loss_backward(int B, int T, int HW, int max_objs, int with_velocity,
                                       const float *const *heads, const float *anno_box, const long long *ind,
                                       const unsigned char *mask, const float *code_weights, const float *dens,
                                       const float *grad_out, float loss_weight, float *const *grad_heads,
                                       ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Test-time decode and NMS of the detection head (csrc/center_decode.hip): centerpoint_head.py CenterHead.get_bboxes
 * (:670-763), get_task_detections (:765-898), CenterPointBBoxCoder.decode, circle_nms and nms_bev (mmcv nms_rotated)
 * for every sample and task in one call.  Deterministic, no atomics on results, no host reads.
 *
 * ocrf_center_decode: heads[6T] (host table of device f32 pointers, per task heatmap logits (B, ncls[t], H, W), reg
 *   (B, 2, H, W), height (B, 1, H, W), dim (B, 3, H, W), rot (B, 2, H, W) and vel (B, 2, H, W), vel NULL without
 *   velocity).  Host scalars: max_num = K (<= OCRF_CD_MAX_NUM, <= H * W), pre_max_size, post_max_size (> 0), out_size_factor,
 *   voxel_size[2], pc_range[2], the coder's score threshold (applied when has_coder_score_threshold) and
 *   post_center_range[6] (NULL = none), the test cfg's score threshold (>=, when has_score_threshold) and
 *   post_center_limit_range[6] (NULL = none), per task nms_circle[T] (1 = circle NMS), nms_threshold[T] (the IoU
 *   threshold, or min_radius for circle tasks) and rescale_factor[T * OCRF_CD_MAX_CLASSES] (per class in task).
 *   Outputs (device), M = T * post_max_size: boxes (B, M, 9 | 7) with bottom-centre z, scores (B, M), labels (B, M)
 *   int32 (with the task's class offset), counts (B) int32; rows past counts[b] are zero.  Four launches, no memset;
 *   workspace from ocrf_center_decode_workspace_bytes.
 */
#define OCRF_CD_MAX_TASKS 8
#define OCRF_CD_MAX_CLASSES 8
#define OCRF_CD_MAX_NUM 1024
size_t ocrf_center_decode_workspace_bytes(int B, int T, int max_num, int post_max_size);
int ocrf_center_decode(int B, int T, const int *ncls, int H, int W, const float *const *heads, int with_velocity,
                       int norm_bbox, int max_num, int pre_max_size, int post_max_size, float out_size_factor,
                       const float *voxel_size, const float *pc_range, int has_coder_score_threshold,
                       float coder_score_threshold, const float *post_center_range, int has_score_threshold,
                       float score_threshold, const float *post_center_limit_range, const int *nms_circle,
                       const double *nms_threshold, const float *rescale_factor, float *boxes, float *scores,
                       int *labels, int *counts, void *workspace, size_t workspace_bytes, ocrf_stream_t stream);
/*
 * ocrf_center_decode_bf16: the same call with the 6T head tensors read as bfloat16 in place (a head under bf16 autocast):
 *   heads[6T] is a host table of device bf16 pointers (passed as unsigned short), same shapes.  Only the select kernel
 *   reads the heads; it widens every load to f32 (exact) and is the f32 code from there on, so boxes, scores, labels
 *   and counts are bit-equal to ocrf_center_decode on the widened heads.  bf16 scores tie often: the order (score
 *   descending, then (class, cell) index ascending, the first `remain` equals in index order) decides ties as it does
 *   in f32.  Same workspace, same workspace query, four launches.
 */
int ocrf_center_decode_bf16(int B, int T, const int *ncls, int H, int W, const unsigned short *const *heads,
                            int with_velocity, int norm_bbox, int max_num, int pre_max_size, int post_max_size,
                            float out_size_factor, const float *voxel_size, const float *pc_range,
                            int has_coder_score_threshold, float coder_score_threshold, const float *post_center_range,
                            int has_score_threshold, float score_threshold, const float *post_center_limit_range,
                            const int *nms_circle, const double *nms_threshold, const float *rescale_factor,
                            float *boxes, float *scores, int *labels, int *counts, void *workspace,
                            size_t workspace_bytes, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Upsample + concatenate of the BEV encoder's neck (csrc/upsample_cat.hip): FPN_LSS.forward's
 * x = cat([x2, up(x1)], 1) (mmdet3d/models/necks/lss_fpn.py:93-94) and up2[0] (:64-67): bilinear upsampling with
 * align_corners=True and an integer factor, written into its channels of the concatenation.  Deterministic, no
 * atomics, no workspace, no host reads.
 *
 * Sampling rule per axis, output index d of out = in * scale points: n = d (in - 1), i0 = n / (out - 1),
 *   lambda = float(n % (out - 1)) / float(out - 1) (integer arithmetic, one rounding; in = 1: lambda = 0),
 *   i1 = min(i0 + 1, in - 1); value (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11) in f32.  torch's
 *   lambda comes from a float product and differs in its last bits.
 *
 * ocrf_upsample_cat_forward: x2 (B, C2, Hin*scale, Win*scale), x1 (B, C1, Hin, Win) f32 NCHW contiguous -> out
 *   (B, C2 + C1, Hin*scale, Win*scale): channels [0, C2) a copy of x2, channels [C2, C2 + C1) the upsampled x1; every
 *   element written once.  C2 = 0 with x2 = NULL: upsampling alone.  One launch; 16-byte accesses along the output
 *   rows when the output plane is a multiple of 4 floats and out / x2 are 16-byte aligned, 4-byte accesses otherwise.
 * ocrf_upsample_cat_backward: grad_out (B, C2 + C1, Hin*scale, Win*scale) -> grad_x1 (B, C1, Hin, Win), the transpose
 *   of the upsampling as a gather per input pixel over the output pixels that read it (fixed order; every element
 *   written).  One launch.  There is no grad_x2: it is grad_out[:, :C2].
 * Limits: scale >= 1, (Hin + Win) * scale <= 8192, every operand below 2 GiB (the kernels index with int); anything
 *   else returns hipErrorInvalidValue and launches nothing.
 */
int ocrf_upsample_cat_forward(int B, int C2, int C1, int Hin, int Win, int scale, const float *x2, const float *x1,
                              float *out, ocrf_stream_t stream);
int ocrf_upsample_cat_backward(int B, int C2, int C1, int Hin, int Win, int scale, const float *grad_out,
                               float *grad_x1, ocrf_stream_t stream);
/*
 * The same pair on bfloat16 data, for the BEV encoder under bf16 autocast: every operand and result is bf16, passed as
 * unsigned short (the upper half of the f32 with the same value), same layouts and arguments.  The kernels are the f32
 * kernels' bodies instantiated for the 2-byte element: taps and gradients are widened to f32 (exact), the value and the
 * backward's sum are the f32 expressions above in the same order, and the result is rounded ONCE to bf16, to nearest
 * even.  Each entry point therefore returns, bit for bit, what its f32 counterpart returns on the widened operands,
 * rounded once; a copied channel keeps its bits.  A NaN stays a NaN; which NaN is not specified.
 * 16-byte accesses (8 elements) along the output rows when the output plane is a multiple of 8 elements and out / x2
 * are 16-byte aligned, 2-byte accesses otherwise.  Limits: those above, with every operand below 2 GiB of bf16.
 */
int ocrf_upsample_cat_forward_bf16(int B, int C2, int C1, int Hin, int Win, int scale, const unsigned short *x2,
                                   const unsigned short *x1, unsigned short *out, ocrf_stream_t stream);
int ocrf_upsample_cat_backward_bf16(int B, int C2, int C1, int Hin, int Win, int scale, const unsigned short *grad_out,
                                    unsigned short *grad_x1, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Temporal BEV alignment (csrc/bev_align.hip, csrc/bev_align_index.h, csrc/bev_align_taps.h):
 * BEVDet4D.shift_feature (mmdet3d/models/detectors/bevdet.py:305-376), the warp of an adjacent frame's BEV feature into the key ego frame,
 * written into its channels of the concatenation in front of the BEV encoder (bevdet.py:529-536, ocrfdet.py:267-274).
 * Deterministic, no atomics, no workspace, no host reads.  f32.
 *
 * Sampling rule.  tf (n, 3, 3) f32 row-major, gen_grid's tf rounded to f32; rows 0 and 1 are read.  Output pixel
 *   (row i, column j) of sample b samples the source plane at
 *     sx = fmaf(t00, j, fmaf(t01, i, t02)),  sy = fmaf(t10, j, fmaf(t11, i, t12)),
 *   x0 = floorf(sx), lx = sx - x0 (y alike), value (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11), each
 *   operation rounded once, a tap outside [0, w) x [0, h) read as 0: grid_sample(bilinear, zeros, align_corners=True) on
 *   the reference's normalised grid without the normalise / unnormalise round trip.
 *
 * ocrf_bev_align_forward: x (n, c, h, w) contiguous -> element [b][ch][i][j] at out + b * out_batch_stride +
 *   (ch * h + i) * w + j (floats), so that out may be a channel slice of a wider concatenation; out_batch_stride >=
 *   c * h * w.  One launch, every destination element written once; 16-byte stores when h * w and out_batch_stride are
 *   multiples of 4 and out is 16-byte aligned, 4-byte stores otherwise.
 * ocrf_bev_align_backward: grad_out addressed like out (grad_batch_stride) -> grad_x (n, c, h, w) contiguous, the
 *   transpose of the forward as a gather: per source pixel the output pixels inside its box (below) are walked rows
 *   ascending, columns ascending, the forward's expressions re-evaluated, and weight * grad_out added where a tap is
 *   that pixel.  One launch, every element written.  There is no gradient of tf.
 * ocrf_bev_align_source_box: host only, touches no GPU.  box[0..3] = first and last column, first and last row
 *   (inclusive) of a box that holds every output pixel of an h x w plane one of whose taps is source pixel (qx, qy)
 *   under the 6 floats tf[0..5] (rows 0 and 1 of one transform).  For ANY float input (NaN, infinities, det = 0) the
 *   box lies inside the plane or is the empty box (0, -1, 0, -1); a singular or strongly shrinking transform gives the
 *   whole plane.  The backward kernel uses this very function.
 * Limits: n, c, h, w > 0; the contiguous operand and the strided one ((n - 1) * stride + c * h * w floats) below 2 GiB
 *   (the kernels index with int); anything else returns hipErrorInvalidValue and launches nothing.  With non-finite tf
 *   the results are unspecified, but no address outside the operands is formed.
 */
int ocrf_bev_align_forward(int n, int c, int h, int w, const float *x, const float *tf, float *out,
                           long long out_batch_stride, ocrf_stream_t stream);
int ocrf_bev_align_backward(int n, int c, int h, int w, const float *grad_out, long long grad_batch_stride,
                            const float *tf, float *grad_x, ocrf_stream_t stream);
int ocrf_bev_align_source_box(const float *tf, int h, int w, int qx, int qy, int *box);
/*
 * The same pair on bfloat16 maps (kept bf16 under autocast): x / out / grad_out / grad_x are bf16, passed as unsigned
 * short; tf stays f32; out_batch_stride / grad_batch_stride are counted in elements.  Coordinates, taps, validity and the
 * box are the f32 ones; taps and gradients are widened to f32 (exact), the value and the gradient sum are the f32
 * expressions in the same order, and the result is rounded ONCE to bf16, to nearest even: bit for bit what the f32 entry
 * point returns on the widened operands, rounded once.  A NaN stays a NaN; which NaN is not specified.
 * 16-byte stores (8 elements) when h * w and out_batch_stride are multiples of 8 and out is 16-byte aligned, 2-byte
 * stores otherwise.  Limits: those above, the 2 GiB counted in bytes of the 2-byte element.
 */
int ocrf_bev_align_forward_bf16(int n, int c, int h, int w, const unsigned short *x, const float *tf,
                                unsigned short *out, long long out_batch_stride, ocrf_stream_t stream);
int ocrf_bev_align_backward_bf16(int n, int c, int h, int w, const unsigned short *grad_out,
                                 long long grad_batch_stride, const float *tf, unsigned short *grad_x,
                                 ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Streaming temporal alignment (csrc/bev_stream_align.hip): the whole concatenation in front of the BEV encoder in ONE
 * launch, from a ring of the last S = K + 1 key-frame BEV maps (OcRFDet4D.stream_step; K = num_adj).  Forward only,
 * f32.  Deterministic, no atomics, no workspace, no host reads; every destination element is written once.
 *
 * Operands:
 *   ring (S, B, C, h, w) f32 contiguous: slot `head` (0 <= head < S) holds the current key frame's map (the caller
 *     writes it there; the kernel does not copy it in), slot (head - e) mod S the map of e steps ago.
 *   valid (B) int32 on the device: the number of real history frames of each sample (0 right after a reset); a negative
 *     value counts as 0, one above K as K.
 *   sensor2ego0, ego2global0 (S, B, 4, 4) f32, bda (S, B, 3, 3) f32: per slot the raw poses of camera 0 and the BEV
 *     augmentation at that slot's time.  Affine (last row (0, 0, 0, 1), not checked).
 *   interval_x / _y, lower_x / _y: the view transformer's grid_interval and grid_lower_bound, x and y; intervals > 0.
 *   align: 0 copies every group (align_after_view_transfromation = False).
 *   out: element [b][g * C + ch][i][j] at out + b * out_batch_stride + ((g * C + ch) * h + i) * w + j (floats), so that
 *     out may be a channel slice of a wider buffer; out_batch_stride >= S * C * h * w.
 *   tf_out (K, B, 3, 3) f32 or NULL: tf_out[g][b] receives the nine floats that group g of sample b was warped with, the
 *     identity for a copied group.
 *
 * Channel group g = 0 .. K - 1 holds age a = K - g (oldest first, as extract_img_feat orders its list), group K the key
 * frame.  For sample b the effective age is e = min(a, valid[b]) and the source slot s = (head - e) mod S.  e = 0 or
 * align = 0: the group is a copy of the source plane.  Otherwise it is the warp of the source plane under tf by the
 * sampling rule of the temporal BEV alignment above, the same code: bit for bit what ocrf_bev_align_forward writes for
 * that plane and that tf.  tf is temporal.feature_transform's value for curr = inv(E_h) E_h S_h, adj = inv(E_h) E_s S_s
 * (E = ego2global0, S = sensor2ego0, h = head), bda = bda[h], bda_adj = bda[s], evaluated in f64 with closed-form affine
 * inverses (adjugate / determinant) and rounded once to f32; once per (b, g) and workgroup, not per pixel.
 * 16-byte stores when h * w and out_batch_stride are multiples of 4 and out is 16-byte aligned, 4-byte stores otherwise.
 * With S = 1 (K = 0) the launch only copies.
 * Limits: S, B, C, h, w > 0, S * B < 2^24, the ring and out ((B - 1) * out_batch_stride + S * C * h * w floats) below
 * 2 GiB; anything else (a head out of range, a stride below a row, a NULL operand other than tf_out, an interval that is
 * not > 0) returns hipErrorInvalidValue and launches nothing.  With non-finite poses the result is unspecified, but no
 * address outside the operands is formed.
 */
int ocrf_bev_stream_align(int S, int B, int C, int h, int w, const float *ring, int head, const int *valid,
                          const float *sensor2ego0, const float *ego2global0, const float *bda, double interval_x,
                          double interval_y, double lower_x, double lower_y, int align, float *out,
                          long long out_batch_stride, float *tf_out, ocrf_stream_t stream);
/*
 * The same launch on a bfloat16 ring (a streaming step under bf16 autocast): ring and out are bf16, passed as unsigned
 * short; the poses, valid and tf_out stay as above, out_batch_stride is counted in elements.  The kernel is the f32
 * kernel's body instantiated for the 2-byte element: units, selection rule, the f64 transform by one lane and the tf_out
 * report are the same code.  Contracts:
 *   a warped group is bit for bit what ocrf_bev_align_forward_bf16 writes for the same plane and the returned tf: the
 *     f32 value on the widened taps, rounded ONCE to bf16, to nearest even;
 *   a copied group is a bit copy of its source plane (no widening, no rounding: a NaN keeps its payload);
 *   tf_out is bit-equal to what ocrf_bev_stream_align reports for the same poses.
 * 16-byte stores (8 elements) when h * w and out_batch_stride are multiples of 8 and out is 16-byte aligned, 2-byte
 * stores otherwise; a copied group of the wide form loads 16 bytes when the ring is 16-byte aligned too, 2 bytes at a
 * time otherwise.  Limits: those above, the 2 GiB counted in bytes of the 2-byte element.
 */
int ocrf_bev_stream_align_bf16(int S, int B, int C, int h, int w, const unsigned short *ring, int head,
                               const int *valid, const float *sensor2ego0, const float *ego2global0, const float *bda,
                               double interval_x, double interval_y, double lower_x, double lower_y, int align,
                               unsigned short *out, long long out_batch_stride, float *tf_out, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Frame poses of the 4D detectors (csrc/frame_poses.hip): the pose algebra of BEVDet4D.prepare_inputs
 * (mmdet3d/models/detectors/bevdet.py:435-456) and the per-frame get_mlp_input of extract_img_feat (ocrfdet.py:229-231)
 * in ONE launch, one thread per (sample, frame, camera).  Deterministic, no atomics, no workspace, no host reads.
 *
 * Inputs, f32 contiguous: sensor2egos, ego2globals (B, F, N, 4, 4) affine (last row (0, 0, 0, 1), not checked); rots,
 * intrins, post_rots (B, F, N, 3, 3); trans, post_trans (B, F, N, 3); bda (B, 3, 3).  0 <= T < F (temporal_frame).
 * Outputs, f32 contiguous, every element written:
 *   sensor2keyegos (B, F, N, 4, 4) = inv(ego2globals[b][0][0]) . ego2globals[b][f][n] . sensor2egos[b][f][n]
 *   curr2adjsensor (B, T, N, 4, 4) = inv(ego2globals[b][f+1][n] . sensor2egos[b][f+1][n]) . ego2globals[b][f][n] .
 *                                    sensor2egos[b][f][n]; may be NULL when T = 0
 *   mlp_input (F, B, N, 27): per frame f what get_mlp_input(rots[:, 0], trans[:, 0], intrins[:, f], post_rots[:, f],
 *                            post_trans[:, f], bda) returns (view_transformer.py:696-722); copies, bit-equal
 * The products and inverses are evaluated in f64 and each result is rounded once to f32.  An inverse is the closed form
 * of an affine map: the 3 x 3 block as adjugate / determinant, the translation -inv(R) t; no orthonormality is assumed,
 * a singular block gives inf / nan.  Limits: B, F, N > 0 and B * F * N < 2^24; anything else returns
 * hipErrorInvalidValue and launches nothing.
 */
int ocrf_frame_poses(int B, int F, int N, int T, const float *sensor2egos, const float *ego2globals, const float *rots,
                     const float *trans, const float *intrins, const float *post_rots, const float *post_trans,
                     const float *bda, float *sensor2keyegos, float *curr2adjsensor, float *mlp_input,
                     ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Image stage of the input pipeline (csrc/image_prep.hip): Pillow's resize (BICUBIC, 8-bit), crop, left-right flip and
 * NEAREST rotate, and mmcv's imnormalize, as PrepareImageInputs applies them to every camera frame
 * (mmdet3d/datasets/pipelines/loading.py:1071-1123), for all M frames in three launches: a horizontal and a vertical
 * resampling pass in Pillow's integer arithmetic, and an epilogue that writes the three float outputs.  Bit-equal to
 * Pillow by construction: the coefficient tables are built on the host (ocrfdet_amd/inputs.py).  Deterministic, no
 * atomics, no host reads.
 *
 * frames (M, Hs, Ws, 3) u8 RGB, M = cameras * F with a camera's F frames adjacent; they share the camera's augmentation.
 * table: n_table int32 words.  Camera g owns words [g * OCRF_IMAGE_PREP_ROW, (g + 1) * OCRF_IMAGE_PREP_ROW):
 *   0 r0, 1 rows      the source rows [r0, r0 + rows) the vertical taps of the crop read; rows <= r_max
 *   2 hb, 3 hk, 4 hks horizontal pass: word offsets of bounds (fW x 2: first source column, tap count) and of the
 *                     coefficients (hks x fW, tap-major, 22 fractional bits), one entry per column of the CROP; a column
 *                     outside the resized image has tap count 0
 *   5 vb, 6 vk, 7 vks vertical pass: bounds (fH x 2) and coefficients (fH x vks, row-major) per row of the crop, the
 *                     first tap an absolute source row
 *   8 flip, 9 identity (rotate(0): a copy), 10..15 a0..a5: Image.rotate's affine map in 16.16 fixed point
 * A pass over an axis whose size does not change is the one-tap table with coefficient 2^22.
 * tmp (M, r_max, fW, 3) u8 and crop (M, fH, fW, 3) u8 are scratch; crop holds resize + crop afterwards.
 * Outputs (M, 3, fH, fW) f32, every element written:
 *   imgs         normalise(rotate(flip(crop)))      imgs_wo_aug  normalise(crop)      imgs_wo_norm  float(flip(crop)), RGB
 *   normalise: output channel c = (float(rgb[2 - c]) - mean[c]) * stdinv[c] (imnormalize with to_rgb=True on an RGB array)
 * Limits: M <= 65535, M a multiple of F, source sides <= OCRF_IMAGE_PREP_MAX_SOURCE, output sides <=
 * OCRF_IMAGE_PREP_MAX_OUTPUT, 0 < r_max <= Hs; anything else returns hipErrorInvalidValue and launches nothing.  A table
 * entry that points outside the table or the source yields zeros.
 */
#define OCRF_IMAGE_PREP_ROW 16
#define OCRF_IMAGE_PREP_MAX_SOURCE 32767
#define OCRF_IMAGE_PREP_MAX_OUTPUT 8192
int ocrf_image_prep(int M, int F, int Hs, int Ws, int fH, int fW, int r_max, const unsigned char *frames,
                    const int *table, long long n_table, unsigned char *tmp, unsigned char *crop, float mean0,
                    float mean1, float mean2, float stdinv0, float stdinv1, float stdinv2, float *imgs,
                    float *imgs_wo_aug, float *imgs_wo_norm, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Point labels of the input pipeline (csrc/point_labels.hip): point_label_transform (loading.py:858-891) for all
 * cameras in two launches.  points (cameras, P, 4) f64: (u, v, depth, label) padded to P; counts (cameras) i32: the real
 * length of each row.  cams (cameras, OCRF_POINT_LABELS_ROW) f64: resize, crop[0], crop[1], flip (0 / 1), cos and sin
 * of rotate / 180 * pi (computed on the host), two unused.  winner (cameras, H, W) i32 scratch: ALL ZERO on entry, all
 * zero again when the launches end; one stream at a time.  Outputs (cameras, H, W) f32, every element written: gt_depth
 * (depth of the last point that lands on the pixel, else 0) and gt_semantic (that point's label >= 0).  float64
 * arithmetic in the reference's order, no fused multiply-add; coordinates truncate toward zero; a point with a
 * coordinate of magnitude >= 32768 (where numpy's int16 cast wraps) or NaN is dropped.  Deterministic: an integer
 * atomicMax over point indices.  P = 0 launches the second kernel only.
 */
#define OCRF_POINT_LABELS_ROW 8
int ocrf_point_labels(int cameras, int P, int H, int W, const double *points, const int *counts, const double *cams,
                      int *winner, float *gt_depth, float *gt_semantic, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The tail of a training iteration (csrc/optim.hip): clip_grad_norm_(max_norm, norm_type=2), torch.optim.AdamW and the
 * weight EMA of mmdet3d/core/hook/ema.py:48-60 (v *= d; v += (1 - d) * msd[k]) over ALL tensors of a model in three
 * launches, whatever their count (configs/ocrfdet/ocrfdet.py:259-274, 329-330).  f32, contiguous tensors.
 * Deterministic: no float atomics, the norm is summed in a fixed order, reruns give the same bits.  No host reads.
 *
 * The kernels read two device tables, passed as const void * and laid out as the structs below (ocrf_optim_layout
 * reports their sizes and field offsets, so that a host packing them without this header can check itself).
 *
 * Static table, built once per set of tensors:
 *   tensors   n_tensors x ocrf_optim_tensor: the device addresses of p, exp_avg, exp_avg_sq and ema, the element count n
 *             and the mode: OCRF_OPTIM_ADAM_EMA (AdamW, then the EMA of the new p), OCRF_OPTIM_ADAM (no EMA; ema is
 *             not read) or OCRF_OPTIM_EMA_ONLY (p is the SOURCE buffer and is only read; exp_avg / exp_avg_sq and
 *             the tensor's gradient are not read).
 *   chunks    n_chunks x ocrf_optim_chunk: tensor index and first element.  A chunk is the at most OCRF_OPTIM_CHUNK
 *             elements of ONE tensor from `offset` on; offset is a multiple of OCRF_OPTIM_CHUNK.  Every element of
 *             every tensor belongs to exactly one chunk; a tensor of 0 elements has none.  A chunk whose tensor index
 *             or offset lies outside the tables is skipped (nothing outside the named tensors is addressed).
 * Per-step record, step_recs: n_tensors x ocrf_optim_step_rec, entry i for tensor i: the gradient's address (0: no
 *   gradient this step) and the scalars of that tensor's param group and step count, computed by the host in double and
 *   rounded once to f32: decay = 1 - lr * weight_decay, one_minus_beta1, beta2, one_minus_beta2, bc2_sqrt =
 *   sqrt(1 - beta2^step) (the DIVISOR, as torch's bias_correction2_sqrt), eps, step_size = lr / (1 - beta1^step).
 *
 * ocrf_optim_layout: host only.  out[0..OCRF_OPTIM_LAYOUT_INTS): sizeof and the field offsets, in declaration order,
 *   of ocrf_optim_tensor, then ocrf_optim_chunk, then ocrf_optim_step_rec.
 * ocrf_optim_grad_sqnorm: two launches.  partials[c] (n_chunks doubles, scratch) = sum of g * g over chunk c, each
 *   square and sum in double, 0 for a chunk whose tensor has no gradient or is EMA_ONLY; then *total_norm (f32, device)
 *   = sqrt(sum of the partials), the partials added in a fixed order in double.
 * ocrf_optim_step: one launch.  Per element, in f32, every operation rounded once:
 *     coef = min(1, max_norm / (*total_norm + 1e-6))     total_norm == NULL: no clipping, coef = 1
 *     g    = g * coef                                     (g itself is NOT written back; clip_grad_norm_ does write it)
 *     p    = p * decay
 *     m    = m + one_minus_beta1 * (g - m)
 *     v    = v * beta2 + one_minus_beta2 * g * g
 *     p    = p - step_size * (m / (sqrt(v) / bc2_sqrt + eps))
 *     ema  = ema * ema_decay + ema_one_minus_decay * p    EMA_ONLY: just this line
 *   A tensor without a gradient skips the AdamW lines and still takes the EMA line.  A NaN or infinite norm propagates
 *   as in torch: there is no check.  16-byte accesses for a chunk all of whose addresses are 16-byte aligned, 4-byte
 *   accesses otherwise, the same arithmetic either way.
 * Limits: NULL tables (or partials / total_norm of ocrf_optim_grad_sqnorm), n_tensors, n_chunks or max_elements <= 0,
 *   or max_elements (the largest element count in `tensors`, stated by the caller: the kernels index a tensor with
 *   int) of 2 GiB / 4 or more return hipErrorInvalidValue and launch nothing.
 * The per-step record changes every step, so these entry points are not held by a step object (csrc/step.hip).
 */
#define OCRF_OPTIM_CHUNK 8192
#define OCRF_OPTIM_ADAM_EMA 0
#define OCRF_OPTIM_ADAM 1
#define OCRF_OPTIM_EMA_ONLY 2
#define OCRF_OPTIM_LAYOUT_INTS 19
typedef struct ocrf_optim_tensor {
  unsigned long long p, exp_avg, exp_avg_sq, ema; /* device addresses; 0 where the mode does not use one */
  long long n;                                    /* elements */
  int mode, reserved;
} ocrf_optim_tensor;
typedef struct ocrf_optim_chunk {
  int tensor, offset;
} ocrf_optim_chunk;
typedef struct ocrf_optim_step_rec {
  unsigned long long grad;
  float decay, one_minus_beta1, beta2, one_minus_beta2, bc2_sqrt, eps, step_size;
  int reserved;
} ocrf_optim_step_rec;
int ocrf_optim_layout(int *out);
int ocrf_optim_grad_sqnorm(const void *tensors, int n_tensors, const void *chunks, int n_chunks, const void *step_recs,
                           long long max_elements, double *partials, float *total_norm, ocrf_stream_t stream);
int ocrf_optim_step(const void *tensors, int n_tensors, const void *chunks, int n_chunks, const void *step_recs,
                    long long max_elements, const float *total_norm, float max_norm, float ema_decay,
                    float ema_one_minus_decay, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The memory-bound passes between the image encoder's convolutions (csrc/resnet_fuse.hip): the residual tail of a
 * ResNet block and CustomFPN's top-down step (mmdet3d/models/necks/fpn.py:190-196), one launch each.  Deterministic, no
 * atomics, no workspace, no host reads.  f32, contiguous; 16-byte accesses when every pointer is 16-byte aligned (and,
 * for ocrf_upsample_add_forward, the destination plane a multiple of 4 floats), 4-byte accesses otherwise.
 *
 * ocrf_add_relu_forward: out[i] = relu(a[i] + b[i]), i in [0, n): one f32 addition rounded once, then
 *   s < 0 ? 0 : s (torch's clamp_min: a NaN sum stays NaN).
 * ocrf_add_relu_backward: grad[i] = out[i] <= 0 ? 0 : grad_out[i] (torch's threshold_backward: a NaN out passes the
 *   gradient); the gradient of both addends.
 * ocrf_upsample_add_forward: dst (B, C, Hout, Wout), src (B, C, Hin, Win) NCHW -> out = dst + nearest(src), every
 *   element written once.  Index rule per axis, torch's mode='nearest' for destination index d:
 *   i = min((int)floorf(d * ((float)in / (float)out)), in - 1).
 * ocrf_upsample_add_backward: grad_out (B, C, Hout, Wout) -> grad_src (B, C, Hin, Win): per source pixel the sum of the
 *   destination pixels that read it (one contiguous run per axis), rows ascending, columns ascending inside a row, into
 *   one f32 accumulator; every element written.  There is no grad_dst: it is grad_out.
 * Limits: n > 0; Hout >= Hin, Wout >= Win, Hout + Wout <= 8192; every operand below 2 GiB (the kernels index with int);
 *   anything else returns hipErrorInvalidValue and launches nothing.
 */
int ocrf_add_relu_forward(long long n, const float *a, const float *b, float *out, ocrf_stream_t stream);
int ocrf_add_relu_backward(long long n, const float *grad_out, const float *out, float *grad, ocrf_stream_t stream);
int ocrf_upsample_add_forward(int B, int C, int Hin, int Win, int Hout, int Wout, const float *dst, const float *src,
                              float *out, ocrf_stream_t stream);
int ocrf_upsample_add_backward(int B, int C, int Hin, int Win, int Hout, int Wout, const float *grad_out,
                               float *grad_src, ocrf_stream_t stream);
/*
 * The same four passes on bfloat16 data, for the encoder under bf16 autocast: every operand and result is bf16, passed
 * as unsigned short (the upper half of the f32 with the same value), contiguous.  16-byte accesses (8 elements) when
 * every pointer accessed by groups is 16-byte aligned (and, for ocrf_upsample_add_forward_bf16, the destination plane a
 * multiple of 8 elements); 2-byte accesses otherwise.  Deterministic, no atomics, no workspace, no host reads.
 *
 * Arithmetic, that of torch's bf16 element-wise ops: both operands widened to f32 (exact), ONE f32 addition, ONE
 * rounding to bf16, to nearest even.  A NaN stays a NaN; which NaN is not specified.
 * ocrf_add_relu_forward_bf16: out[i] = relu(bf16(a[i] + b[i])), the ReLU on the rounded sum s as `s < 0 ? 0 : s` (a NaN
 *   sum stays NaN).
 * ocrf_add_relu_backward_bf16: grad[i] = out[i] <= 0 ? 0 : grad_out[i], a select: grad_out's bits pass unchanged, a
 *   NaN out passes the gradient.
 * ocrf_upsample_add_forward_bf16: out = bf16(dst + nearest(src)) with the index rule of ocrf_upsample_add_forward.
 * ocrf_upsample_add_backward_bf16: per source pixel the sum of its run in the order of ocrf_upsample_add_backward (rows
 *   ascending, columns ascending inside a row) into one f32 accumulator, rounded once to bf16.
 * Limits: those of the f32 entry points, every operand below 2 GiB included (n < 2^30 elements); anything else returns
 *   hipErrorInvalidValue and launches nothing.
 */
int ocrf_add_relu_forward_bf16(long long n, const unsigned short *a, const unsigned short *b, unsigned short *out,
                               ocrf_stream_t stream);
int ocrf_add_relu_backward_bf16(long long n, const unsigned short *grad_out, const unsigned short *out,
                                unsigned short *grad, ocrf_stream_t stream);
int ocrf_upsample_add_forward_bf16(int B, int C, int Hin, int Win, int Hout, int Wout, const unsigned short *dst,
                                   const unsigned short *src, unsigned short *out, ocrf_stream_t stream);
int ocrf_upsample_add_backward_bf16(int B, int C, int Hin, int Win, int Hout, int Wout, const unsigned short *grad_out,
                                    unsigned short *grad_src, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Batch norm fused with the ReLU and the residual addition behind it (csrc/bn_act.hip; ocrfdet_amd/norm_ops.py):
 * out = [relu](bn(x) [+ residual]) over (N, C, H, W) contiguous tensors, forward and backward.  Deterministic: no
 * atomics, no workgroup waits for another, no host reads; a reduction that spans workgroups is two launches with
 * `partials` between them.  x, residual, out, grad_out, dx and dresidual are f32, or bf16 (unsigned short) in the _bf16
 * forms; every per-channel vector, `partials` and all arithmetic are f32, and each result element is rounded once.
 * 16-byte accesses where a plane's piece allows it (every base pointer 16-byte aligned), single elements at its ragged
 * head and tail.
 *
 * The N * H * W values of a channel are cut into ocrf_bn_chunks(N, C, H, W) chunks of 4096 (a function of the shape
 * alone; host only, 0 for a shape the kernels refuse).
 * ocrf_bn_stats: partials (C, chunks, 4) <- (count, mean as anchor and offset, M2) of every chunk, M2 the sum of squared
 *   deviations from the chunk's mean, combined with the pairwise update (Chan et al.): nothing cancels.
 * ocrf_bn_finalize: one wave per channel merges the chunks in a fixed order.  from_running == 0: mean, invstd =
 *   1 / sqrt(M2 / n + eps), scale = weight invstd, shift = bias - mean scale; with running_mean and running_var not
 *   NULL they are updated, running <- (1 - m) running + m (mean | M2 / (n - 1)), m = momentum, or
 *   1 / *num_batches_tracked (a device int64, read by the kernel) when momentum < 0.  from_running == 1: mean =
 *   running_mean, invstd = 1 / sqrt(running_var + eps), scale and shift from those; nothing is updated.
 * ocrf_bn_act_forward: v = fmaf(x, scale[c], shift[c]); residual not NULL: v = v + residual (one f32 addition);
 *   relu != 0: v < 0 ? 0 : v (a NaN stays a NaN).
 * ocrf_bn_act_backward_reduce: partials (C, chunks, 2) <- (sum g, sum g x^) of every chunk, x^ = (x - mean) invstd,
 *   g = out <= 0 ? 0 : grad_out (torch's threshold_backward), or grad_out with out == NULL (the forward had no ReLU).
 * ocrf_bn_act_backward: merges the partial sums in a fixed order; dx = weight invstd (g - sum g / n - x^ sum(g x^) / n)
 *   with batch_stats != 0, weight invstd g with 0; dresidual = g; dweight = sum g x^, dbias = sum g, once per channel.
 *   dx, dresidual, dweight, dbias may each be NULL and are then not written; partials may be NULL when neither dx with
 *   batch_stats nor a parameter gradient needs the sums.
 * Limits: N, C, H, W > 0 and fewer than 2^31 elements; anything else returns hipErrorInvalidValue and launches nothing.
 */
int ocrf_bn_chunks(int N, int C, int H, int W);
int ocrf_bn_stats(int N, int C, int H, int W, const float *x, float *partials, ocrf_stream_t stream);
int ocrf_bn_finalize(int N, int C, int H, int W, int from_running, const float *partials, const float *weight,
                     const float *bias, float *running_mean, float *running_var, const long long *num_batches_tracked,
                     float momentum, float eps, float *mean, float *invstd, float *scale, float *shift,
                     ocrf_stream_t stream);
int ocrf_bn_act_forward(int N, int C, int H, int W, const float *x, const float *residual, const float *scale,
                        const float *shift, int relu, float *out, ocrf_stream_t stream);
int ocrf_bn_act_backward_reduce(int N, int C, int H, int W, const float *grad_out, const float *x, const float *out,
                                const float *mean, const float *invstd, float *partials, ocrf_stream_t stream);
int ocrf_bn_act_backward(int N, int C, int H, int W, const float *grad_out, const float *x, const float *out,
                         const float *mean, const float *invstd, const float *weight, const float *partials,
                         int batch_stats, float *dx, float *dresidual, float *dweight, float *dbias,
                         ocrf_stream_t stream);
int ocrf_bn_stats_bf16(int N, int C, int H, int W, const unsigned short *x, float *partials, ocrf_stream_t stream);
int ocrf_bn_act_forward_bf16(int N, int C, int H, int W, const unsigned short *x, const unsigned short *residual,
                             const float *scale, const float *shift, int relu, unsigned short *out,
                             ocrf_stream_t stream);
int ocrf_bn_act_backward_reduce_bf16(int N, int C, int H, int W, const unsigned short *grad_out,
                                     const unsigned short *x, const unsigned short *out, const float *mean,
                                     const float *invstd, float *partials, ocrf_stream_t stream);
int ocrf_bn_act_backward_bf16(int N, int C, int H, int W, const unsigned short *grad_out, const unsigned short *x,
                              const unsigned short *out, const float *mean, const float *invstd, const float *weight,
                              const float *partials, int batch_stats, unsigned short *dx, unsigned short *dresidual,
                              float *dweight, float *dbias, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Index preparation of the two poolings on the device (csrc/index_prep.hip).
 *
 * ocrf_lss_prepare replaces get_lidar_coor + voxel_pooling_prepare_v2
 * (mmdet3d/models/necks/view_transformer.py:108-147,197-255) for one batch of B samples x N cameras:
 *   frustum   (D,H,W,3) device   the create_frustum template (:77-106), (u, v, depth) per cell
 *   cams      (B*N,33)  device   per camera-frame, row-major 3x3s:
 *                                inv(post_rots) 9 | rots . inv(cam2imgs) 9 | post_trans 3 | trans 3 | bda 9
 *                                (the tiny per-camera algebra stays with the caller: the same torch
 *                                calls the reference makes at :128-146)
 *   grid_lower_host / grid_interval_host   3 floats each in HOST memory (create_grid_infos, :59-75)
 *   gx, gy, gz                    grid size (X, Y, Z)
 * outputs (device, int32; capacities: B*N*D*H*W for the three rank vectors, min(that, B*Z*Y*X) for
 * the interval vectors): ranks_bev / ranks_depth / ranks_feat sorted by voxel, ascending point
 * index inside a voxel (stable, where the reference's argsort is not); interval_starts /
 * interval_lengths; counts[0] = Np (kept points), counts[1] = Nv (intervals) — device ints, so that
 * the call itself never synchronises.  Bit-exact against the reference's vectors.
 *
 * ocrf_ht_prepare replaces get_sampling_point + fast_sample_prepare
 * (mmdet3d/models/necks/view_transformer_ocrf.py:687-740,785-852):
 *   ref_points (Z,n_pillars,3) device   get_reference_points_3d template (:651-673), normalised
 *   cams       (B*N,24) device          lidar2img 3x4 | img_aug 3x4 per camera-frame (get_projection, :675-685)
 *   pc_range_host  6 floats in HOST memory; w_in / h_in: network input size; depth0 / depth1:
 *   grid_config['depth'][0:2]; Wf, Hf, D: feature-map size and depth bins
 * outputs as above with ranks_bev = b*n_pillars + pillar; inside a pillar the order is (camera,
 * height) ascending = the reference's flattening order under a stable sort.
 * The workspace holds the look-back states of the single-launch prefix sums: one call at a time per workspace
 * (two calls that share it on different streams overwrite each other's states; a tile that waits ~a second for a
 * predecessor gives up instead of spinning for ever, and the call leaves counts = -1).
 */
int ocrf_lss_prepare(int B, int N, int D, int H, int W, const float *frustum, const float *cams,
                     const float *grid_lower_host, const float *grid_interval_host, int gx, int gy, int gz,
                     int *ranks_bev, int *ranks_depth, int *ranks_feat, int *interval_starts,
                     int *interval_lengths, int *counts, void *workspace, size_t workspace_bytes,
                     ocrf_stream_t stream);
size_t ocrf_lss_prepare_workspace_bytes(int B, int N, int D, int H, int W, int gx, int gy, int gz);
int ocrf_ht_prepare(int B, int N, int Z, int n_pillars, int Wf, int Hf, int D, const float *ref_points,
                    const float *cams, const float *pc_range_host, float w_in, float h_in, float depth0,
                    float depth1, int *ranks_bev, int *ranks_depth, int *ranks_feat, int *interval_starts,
                    int *interval_lengths, int *counts, void *workspace, size_t workspace_bytes,
                    ocrf_stream_t stream);
size_t ocrf_ht_prepare_workspace_bytes(int B, int n_pillars);

/*
 * Per-forward calibration algebra on the device (the host glue of view_transformer.py:128-146,
 * view_transformer_ocrf.py:675-685 and :1135-1152 with data_utils.py:703-733): from the seven calibration
 * tensors of the reference's input tuple, where they already live, to the camera blocks the kernels above take —
 *   lss_block   (B*N,33)  inv(post_rots) | rots inv(intrins) | post_trans | trans | bda      (ocrf_lss_prepare)
 *   ht_block    (B*N,24)  lidar2img 3x4 | img_aug 3x4                        (ocrf_ht_prepare / ocrf_ht_project)
 *   camera_rows (B*N,36)  the `cameras` rows of ocrf_rasterize_forward for every camera-frame, built as the
 *                         reference builds its render camera (quirks included); needs c2w (B*N,4,4)
 * (any of the three may be NULL).  3x3 inverses and products are evaluated in double precision and rounded to
 * float once, so the values agree with the reference's float32 LAPACK / matmul chain to ~1 ulp, not bit for bit:
 * a pillar sample or frustum point that sits within that distance of a cell border can land in the neighbouring
 * cell (as it can between the reference's own CPU and CUDA runs).  No host read, no synchronisation.
 */
int ocrf_geometry_blocks(int B, int N, const float *rots, const float *trans, const float *intrins,
                         const float *post_rots, const float *post_trans, const float *bda, const float *c2w,
                         int H_in, int W_in, float znear, float zfar, float *lss_block, float *ht_block,
                         float *camera_rows, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Height-aware Opacity-based Attention (HOA) reductions
 * ------------------------------------------------------------------------------------------
 * All tensors float32, NCHW contiguous.
 *
 * ocrf_hoa_channel_stats + ocrf_hoa_opacity_mask_gate replace ObatinOpacityMask.forward
 * (mmdet3d/models/necks/view_transformer_ocrf.py:236-242) and `geom_feat * opacity_mask`
 * (:1197-1199):
 *   stats[b][0] = mean_c x[b][c], stats[b][1] = max_c x[b][c]                       (B,2,Y,X)
 *   mask  = sigmoid(conv2d(stats, conv_w (1,2,k,k), padding k/2, no bias) + opacity_bev)  (B,1,Y,X)
 *   gated = x * mask (skipped when gated == NULL)                                    (B,C,Y,X)
 */
int ocrf_hoa_channel_stats(const float *x, int B, int C, int Y, int X, float *stats,
                           ocrf_stream_t stream);
int ocrf_hoa_opacity_mask_gate(const float *x, const float *stats, const float *opacity_bev,
                               const float *conv_w, int k, int B, int C, int Y, int X, float *mask,
                               float *gated, ocrf_stream_t stream);

/*
 * Depthwise 3x3 convolution, padding 1, stride 1 (the first layer of OpacityVoxelToBEVConverter.conv_block,
 * view_transformer_ocrf.py:483-489) for the TRAINING path, where MIOpen's depthwise backward-weight costs
 * milliseconds on these 4..16-channel maps:
 *   ocrf_hoa_dw3x3:        y[b][c] = conv3x3(x[b][c], w[c] (9 floats)) + bias[c]   (bias may be NULL); also the
 *                          input gradient when called with dy and the flipped weights
 *   ocrf_hoa_dw3x3_wgrad:  partial[(b*C + c) * n_bands + band][10]: per 16-row band the nine sums
 *                          dy[y][x] * x[y+i-1][x+j-1] and the sum of dy; n_bands = ocrf_hoa_dw3x3_wgrad_bands(Y);
 *                          the caller adds the bands and samples (fixed order: deterministic).
 */
int ocrf_hoa_dw3x3(const float *x, const float *w, const float *bias, int B, int C, int Y, int X, float *y,
                   ocrf_stream_t stream);
int ocrf_hoa_dw3x3_wgrad_bands(int Y);
int ocrf_hoa_dw3x3_wgrad(const float *x, const float *dy, int B, int C, int Y, int X, float *partial,
                         ocrf_stream_t stream);

/*
 * HeightAttention.forward (view_transformer_ocrf.py:447-461) and its use `ca(x) * x`
 * (:499-514): the C channels are four height quarters of q = C/4 channels; per quarter g
 *   gate[b][g*q + o] = sigmoid( sum_h w2[g][o][h] * relu( sum_i w1[g][h][i] * max_{y,x} x[b][g*q+i] ) )
 * w1 is [4][hid][q] (convN.0.weight), w2 is [4][q][hid] (convN.2.weight), no biases.
 *   gate (B,C) is always written; gated = gate * x (B,C,Y,X) when gated != NULL.
 * C % 4 == 0, C <= 64, 4*hid <= 64.  workspace >= ocrf_hoa_height_attention_workspace_bytes(B, C).
 */
int ocrf_hoa_height_attention(const float *x, int B, int C, int hid, int Y, int X, const float *w1,
                              const float *w2, float *gate, float *gated, void *workspace,
                              size_t workspace_bytes, ocrf_stream_t stream);
size_t ocrf_hoa_height_attention_workspace_bytes(int B, int C);

/*
 * OpacityVoxelToBEVConverter (view_transformer_ocrf.py:463-518) as fused blocks, eval mode.
 * ocrf_hoa_unet_block = one `conv_block` (depthwise 3x3 + bias -> 1x1 + bias -> BatchNorm folded into
 * pw_w/pw_b by the caller -> ReLU, :485-491) over the virtual input
 *   mode 0: src0 (B,C0,H,W)                                   [encoder1, :498]
 *   mode 1: maxpool2x2(src0 (B,C0,2H,2W))                     [encoder2 / bottleneck, :501,:504]
 *   mode 2: cat(ConvTranspose2d_k2s2(src0 (B,C0,H/2,W/2); up_w (C0,Cup,2,2), up_b), src1 (B,C1,H,W))
 *                                                             [decoder2 / decoder1, :507-514]
 * with gate0 (B,C0) / gate1 (B,C1) (the producers' HeightAttention gates, NULL = none) multiplied in
 * while reading, `addend` (B,Cout,H,W) added after the ReLU (positional encoding, NULL = none), and
 * partial_max (B*Cout, ocrf_hoa_unet_tiles(H,W)) receiving per-tile channel maxima (NULL = skip).
 * Channel counts <= 16.  ocrf_hoa_height_gate_from_tiles turns those maxima into the HeightAttention
 * gate (B,C) (same w1/w2 layout as ocrf_hoa_height_attention); ocrf_hoa_gated_conv1x1 is the final
 * `output_conv` (:516) over gate * x: out (B,1,H,W) = bias[0] + sum_c w[c] * gate[b][c] * x[b][c].
 */
int ocrf_hoa_unet_block(const float *src0, const float *gate0, int C0, int H0, int W0, int mode,
                        const float *up_w, const float *up_b, int Cup, const float *src1,
                        const float *gate1, int C1, const float *dw_w, const float *dw_b,
                        const float *pw_w, const float *pw_b, int Cout, const float *addend, float *out,
                        float *partial_max, int B, int H, int W, ocrf_stream_t stream);
int ocrf_hoa_unet_tiles(int H, int W);
/* The whole converter of the architecture OcRFDet instantiates (input_channel = 13: 13 -> 4 -> 8 -> 16 -> 8 -> 4 -> 1,
 * ratio-1 HeightAttention gates, view_transformer_ocrf.py:463-518) as ONE call of six launches (csrc/hoa_v2b.hip:
 * latency-shaped forms of the five blocks above on 16 x 4 pixel tiles, each computing the gates of its producers in
 * its own prologue from the per-tile maxima they left, and the gated output conv; bit-identical to the block-wise
 * calls).  x (B,13,H,W), position (B,4,H,W), out (B,1,H,W); H and W multiples of 4.  `weights` (16-byte aligned):
 * ocrf_hoa_v2b_weights_len() floats — per block (encoder1, encoder2, bottleneck, decoder2, decoder1): dw_w (Cin,9),
 * dw_b (Cin), pw_w (Cout,Cin) and pw_b (Cout) with BatchNorm folded, the block's gate w1 (4,hid,q), w2 (4,q,hid);
 * then upconv2 w (16,8,2,2), b (8), upconv1 w (8,4,2,2), b (4), output conv w (4), b (1); zero-padded to a whole
 * number of 16-byte words (the kernels copy it to LDS with 16-byte loads).
 * workspace (16-byte aligned) >= ocrf_hoa_v2b_workspace_bytes(B, H, W) bytes (the five intermediates and their tile
 * maxima). */
int ocrf_hoa_v2b_weights_len(void);
size_t ocrf_hoa_v2b_workspace_bytes(int B, int H, int W);
int ocrf_hoa_v2b_forward(const float *x, const float *position, const float *weights, int B, int H, int W,
                         void *workspace, size_t workspace_bytes, float *out, ocrf_stream_t stream);
int ocrf_hoa_height_gate_from_tiles(int B, int C, int hid, int n_tiles, const float *partial_max,
                                    const float *w1, const float *w2, float *gate, ocrf_stream_t stream);
int ocrf_hoa_gated_conv1x1(const float *x, const float *gate, int B, int C, int H, int W, const float *w,
                           const float *bias, float *out, ocrf_stream_t stream);

/*
 * HOA-1 (view_transformer_ocrf.py:1159-1161): deformable cross attention between the Gaussian
 * opacity volume and the NeRF-branch alpha volume, eval mode, for the DeformableAttention2D that
 * OcRFDet instantiates (:639-648: dim 13, heads 1, dim_head 8, offset_groups 1, downsample_factor 4,
 * offset_kernel_size 6; mmdet3d/ops/cross_attention_2d.py:93-220):
 *   out (B,13,Y,X) = upsample(att(down(opacity), down(alpha)), (Y,X)) + opacity,
 * down/up = bilinear align_corners=True to/from (Y/6, X/6).  opacity, alpha: (B,13,Y,X).
 * weights: ocrf_hoa1_weights_len() floats packed as documented in csrc/hoa.hip (the Python module
 * packs its state_dict).  att_workspace: B*((13+8)*(Y/6)*(X/6) + 18*128) floats.  (Y/6)*(X/6) <= 1600.
 * Two kernel launches: the key / value tokens (one workgroup per group of kv tokens rebuilds the rows of q its
 * offset convolution reads), then attention + output projection + upsample + residual per 16x16 output tile.
 */
int ocrf_hoa1_forward(const float *opacity, const float *alpha, const float *weights, int B, int Y, int X,
                      float offset_scale, float *att_workspace, float *out, ocrf_stream_t stream);
int ocrf_hoa1_weights_len(void);

/*
 * HOA-1 under autograd (csrc/hoa1_train.hip), same configuration and limits as ocrf_hoa1_forward (Y/6 >= 6, X/6 >= 6,
 * <= 1600 query tokens, <= 128 kv tokens; anything else: hipErrorInvalidValue).
 * ocrf_hoa1_train_workspace_floats (host only): floats of the workspace both calls take, 0 for an unsupported shape.  The
 *   forward keeps the kv tokens (k | v | grid) and every query token's softmax maximum and sum in it; the rest is the
 *   backward's scratch.  The caller keeps it untouched between the forward and its backward.
 * ocrf_hoa1_forward_train: out as ocrf_hoa1_forward, bit for bit when dropout_mask is NULL.  dropout_mask
 *   (B, ntok, nkv) bytes, 1 = keep: the attention weights are multiplied by mask * dropout_scale (1 / (1 - p)) after the
 *   softmax normalisation, as nn.Dropout does on attn.  Two launches.
 * ocrf_hoa1_backward: grad_out (B,13,Y,X) -> grad_opacity, grad_alpha (B,13,Y,X) and grad_weights
 *   (ocrf_hoa1_weights_len() floats, the layout of `weights`), with the inputs, mask and workspace of the forward.  Six
 *   launches, no atomics (reruns are bit-identical), no host read, no memset.
 */
size_t ocrf_hoa1_train_workspace_floats(int B, int Y, int X);
int ocrf_hoa1_forward_train(const float *opacity, const float *alpha, const float *weights, int B, int Y, int X,
                            float offset_scale, const unsigned char *dropout_mask, float dropout_scale, float *workspace,
                            float *out, ocrf_stream_t stream);
int ocrf_hoa1_backward(const float *grad_out, const float *opacity, const float *alpha, const float *weights, int B, int Y,
                       int X, float offset_scale, const unsigned char *dropout_mask, float dropout_scale, float *workspace,
                       float *grad_opacity, float *grad_alpha, float *grad_weights, ocrf_stream_t stream);

/*
 * Pillar projections consumed by the colour / alpha sampling and retain_valid_pixels
 * (view_transformer_ocrf.py:1057-1066 from get_sampling_point :687-740), same inputs as
 * ocrf_ht_prepare (pc_range: 6 floats in HOST memory):
 *   pix   (B,N,Z,n_pillars,2)  (u_norm*w_in, v_norm*h_in) of every sample, masked ones included
 *   mask  (B,N,Z,n_pillars)    bytes, the get_sampling_point mask
 *   voxel (B,Z,n_pillars,3)    metric voxel centres (the in-place scaled reference points, :690-692); may be NULL
 */
int ocrf_ht_project(int B, int N, int Z, int n_pillars, const float *ref_points, const float *cams,
                    const float *pc_range, float w_in, float h_in, float depth0, float depth1,
                    float *pix, unsigned char *mask, float *voxel, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Neck glue between the poolings, the render and HOA (eval mode; csrc/neck.hip)
 * ------------------------------------------------------------------------------------------ */

/*
 * OcRFViewTransformerFull.forward's pre-filter (view_transformer_ocrf.py:1323-1331) fused with the
 * channels-last permute the poolings need (:875, :901).  x (BN, D+2+C, HW) = DepthNet output:
 *   depth         (BN,D,HW)  softmax over the D depth logits (returned to the caller, :1334)
 *   filter_depth  (BN,D,HW)  depth, zeroed where depth < depth_threshold (= depth_threshold/D of the ctor)
 *   semantic      (BN,2,HW)  softmax over the 2 semantic logits
 *   feat_channels_last (BN,HW,C)  tran_feat * (semantic[:,1] >= semantic_threshold), i.e. the
 *                 (B,N,H,W,C) operand of bev_pool_v2
 * D <= 512.
 */
int ocrf_prefilter(const float *x, int BN, int D, int C, int HW, float depth_threshold,
                   float semantic_threshold, float *depth, float *filter_depth, float *semantic,
                   float *feat_channels_last, ocrf_stream_t stream);

/*
 * lidar_points_to_image_values + color_voxels' avg_color (view_transformer_ocrf.py:924-959):
 *   avg[b][q][c] = sum_{n: mask[b][n][q]} bilinear(imgs[b][n][c], pix[b][n][q]) / max(1, #valid n)
 * imgs (B,N,C,Hi,Wi) with C in {1,3}; pix (B,N,ZQ,2) PIXEL coordinates (x,y) — normalised as
 * (p/(size-1))*2-1 and sampled like F.grid_sample(bilinear, zeros, align_corners=True), :929-936;
 * mask (B,N,ZQ) bytes (torch.bool); avg (B,ZQ,C).  Hi/Wi are the extents the reference's view of the
 * image claims: for the alpha volume it passes the (H,W) stack viewed as (W,H) (:1123).
 */
int ocrf_pillar_sample_mean(const float *imgs, const float *pix, const unsigned char *mask, float *avg,
                            int B, int N, int C, int Hi, int Wi, int ZQ, ocrf_stream_t stream);

/*
 * retain_valid_pixels (view_transformer_ocrf.py:1004-1024): out = 255 except pixels
 * (clamp(trunc(pix.x)), clamp(trunc(pix.y))) of valid projections, which keep imgs' value.
 * imgs (B,N,C,H,W); cam_sel == NULL: every camera, out (B,N,C,H,W); cam_sel (B) int32 device
 * pointer: only camera cam_sel[b] of sample b (the one the caller consumes, :1104), out (B,C,H,W).
 */
int ocrf_retain_valid_pixels(const float *imgs, const float *pix, const unsigned char *mask,
                             const int *cam_sel, float *out, int B, int N, int C, int H, int W, int ZQ,
                             ocrf_stream_t stream);

/*
 * VoxelFeatureExtractor (view_transformer_ocrf.py:520-531, call :1051; Conv3d(1->Zh,k=1) +
 * BatchNorm3d folded by the caller into lift_a/lift_b + ReLU) fused with the four Gaussian heads
 * (:272-320, calls :1130-1133).  bev (B,C,YX) is the HT BEV feature, rgb_avg (B,Zh,YX,3) the
 * sampled voxel colour in 0..255 (divided by 255 inside, :1071).  Gaussian g = (b, h, q):
 *   f[c] = relu(lift_a[h]*bev[b][c][q] + lift_b[h]);  opacity (B,Zh*YX,1) = sigmoid(A_MLP(f)),
 *   scales (.,3) = softplus(S_MLP(f)), rotations (.,4) = normalize(R_MLP(f)), color (.,3) =
 *   sigmoid(C_MLP([f, rgb/255])).
 * params: ocrf_gauss_heads_params_len(C, Zh) floats packed as documented in csrc/neck.hip.
 * rotations must be 16-byte aligned, params 8-byte aligned; Zh in {1,2,4,6,8,13} (register tile).
 */
int ocrf_gauss_heads(const float *bev, const float *rgb_avg, const float *params, int B, int C, int Zh,
                     int YX, float *opacity, float *scales, float *rotations, float *color,
                     ocrf_stream_t stream);
int ocrf_gauss_heads_params_len(int C, int Zh);

/*
 * Backward of ocrf_gauss_heads: what autograd does for the reference through VoxelFeatureExtractor (:520-531) and the four
 * heads (:272-320, calls :1130-1133) on the (B,Zh,Y,X,C) voxel feature, here without that tensor (the lift and the hidden
 * units are recomputed from bev).  g_* are the gradients of the four outputs (same shapes; NULL = zero); d_bev (B,C,YX) is
 * fully written here; d_params receives the gradient w.r.t. every entry of `params`, in the layout of `params`
 * (lift_a / lift_b first: the caller owns the folding of Conv3d + BatchNorm3d — batch statistics in training — and
 * differentiates through it).  No gradient for rgb_avg (sampled from the camera images, :1071).  Deterministic.
 * workspace: ocrf_gauss_heads_backward_workspace_bytes(B, C, Zh, YX) bytes (0: unsupported shape).
 */
size_t ocrf_gauss_heads_backward_workspace_bytes(int B, int C, int Zh, int YX);
int ocrf_gauss_heads_backward(const float *bev, const float *rgb_avg, const float *params, int B, int C, int Zh, int YX,
                              const float *g_opacity, const float *g_scales, const float *g_rotations,
                              const float *g_color, float *d_bev, float *d_params, void *workspace,
                              size_t workspace_bytes, ocrf_stream_t stream);

/*
 * NeRF branch (view_transformer_ocrf.py:1094-1121) from z (M,32,h2,w2) = ResizeNetwork.conv2's
 * output (:546); the caller composes upsample2 (k2 s2) -> upsample3 (k4 s4) -> first Linear of each
 * consumer into per-sub-position maps (64 positions of the 8x8 up-sampling cell):
 *   ocrf_nerf_alpha:  alpha (M,8*h2,8*w2) = 1 - exp(-softplus(w_sigma[:,pos] . z + c_sigma[pos]))
 *                     (sigma = Softplus(Linear(Linear(.))), :605, :1099-1102)
 *   ocrf_nerf_render: for sample b and camera cam_sel[b] (int32 device vector), with sparse_rgb
 *                     (B,3,H,W) from ocrf_retain_valid_pixels: render_image_n (B,3,H,W) =
 *                     alpha * relu(img_feat_resize1) * softmax(C_MLP_nerf), render_depth_n (B,1,H,W) =
 *                     alpha * relu(img_feat_resize2)   (T == 1 and the depth weight == 1, :1108-1117).
 * params of ocrf_nerf_render: ocrf_nerf_render_params_len() floats, layout in csrc/neck.hip.
 */
int ocrf_nerf_alpha(const float *z, const float *w_sigma, const float *c_sigma, float *alpha, int M,
                    int h2, int w2, ocrf_stream_t stream);
int ocrf_nerf_render(const float *z, const int *cam_sel, const float *alpha, const float *sparse_rgb,
                     const float *params, int B, int N, int h2, int w2, float *render_image_n,
                     float *render_depth_n, ocrf_stream_t stream);
int ocrf_nerf_render_params_len(void);

/*
 * DualFeatFusion.forward (view_transformer_ocrf.py:203-213; MS_CAM :36-66), eval mode, one pass:
 *   out = cf * x1 + (1 - cf) * x2,  cf = sigmoid(local_att([x1; x2]) + global_vec[b]),
 *   local_att = Conv1x1(2C->M) + BN + ReLU + Conv1x1(M->C) + BN with both BatchNorms folded by the
 *   caller into params = W1t[2C][M] | b1[M] | W2[C][M] | b2[C]; global_vec (B,C) is MS_CAM's
 *   global_att branch of the pooled map (a (B,2C) vector through two tiny layers: the caller's).
 * x1, x2, out: (B,C,YX).  (C, M) in {(80, 40), (64, 32)}; params 8-byte aligned.
 */
int ocrf_dual_feat_fusion(const float *x1, const float *x2, const float *params, const float *global_vec,
                          float *out, int B, int C, int M, int YX, ocrf_stream_t stream);
/* ... and, in the same pass, out_plus = addend + out (addend, out_plus (B,C,YX)): the fused map with the positional
 * encoding ProbNet's first convolution reads it with (view_transformer_ocrf.py:1188) — one more store per element
 * instead of an elementwise launch over the map. */
int ocrf_dual_feat_fusion_plus(const float *x1, const float *x2, const float *params, const float *global_vec,
                               float *out, const float *addend, float *out_plus, int B, int C, int M, int YX,
                               ocrf_stream_t stream);

/*
 * CBAM / ProbNet tail (view_transformer_ocrf.py:68-137 ChannelAttention, SpatialAttention, ResCBAMBlock;
 * :139-201 ProbNet; MS_CAM.global_att :50-58), eval mode.  The 3x3 convolutions stay with MIOpen; these four
 * entry points replace the ~30 elementwise / reduction launches between them.
 *
 * ocrf_plane_bias_act_stats: one pass over y (B,C,YX), in place when write != 0: y += bias[c] (bias may be
 *   NULL; BatchNorm folded by the caller), ReLU when relu != 0; when psum != NULL also S partial sums and
 *   maxima of the result per plane -> psum / pmax [(b*out_C + c_off + c)*S + s] (two inputs can fill one
 *   (B, out_C, S) block: MS_CAM pools cat(x1, x2)).  y 16-byte aligned.
 * ocrf_channel_mlp: v_mean = sum_s psum * inv_n, v_max = max_s pmax;
 *   out[b][n] = act(W2.relu(W1.v_mean + b1) + b2 [+ W2.relu(W1.v_max + b1) + b2]), act = sigmoid or identity;
 *   W1 (M,K), W2 (N,M) row-major, b1 / b2 may be NULL; K <= 256, M <= 64.
 * ocrf_scaled_channel_stats: stats (B,2,YX) = mean_c, max_c of scale[b][c] * x[b][c] (SpatialAttention's input
 *   of the channel-gated map, which is never materialised).
 * ocrf_cbam_tail: m = sigmoid(conv_kxk(stats)); o_c = relu(m * (scale_c * y_c) + res_c);
 *   logit (B,YX) = sum_c wm_c * o_c + bm (ProbNet.mask_net); block_out (B,C,YX) receives o when not NULL.
 */
int ocrf_plane_bias_act_stats(float *y, const float *bias, int B, int C, int YX, int relu, int write, int S,
                              int out_C, int c_off, float *psum, float *pmax, ocrf_stream_t stream);
/* the statistics of TWO tensors y1 (B,C1,YX), y2 (B,C2,YX) as if concatenated along the channels, in ONE launch:
 * psum / pmax (B, C1 + C2, S) (MS_CAM's global branch pools cat(x1, x2) :50-58; 16-byte aligned inputs) */
int ocrf_plane_stats_pair(const float *y1, const float *y2, int B, int C1, int C2, int YX, int S, float *psum,
                          float *pmax, ocrf_stream_t stream);
int ocrf_channel_mlp(const float *psum, const float *pmax, int B, int K, int S, float inv_n, const float *W1,
                     const float *b1, const float *W2, const float *b2, int M, int N, int use_max, int do_sigmoid,
                     float *out, ocrf_stream_t stream);
int ocrf_scaled_channel_stats(const float *x, const float *scale, int B, int C, int YX, float *stats,
                              ocrf_stream_t stream);
int ocrf_cbam_tail(const float *y, const float *scale, const float *stats, const float *conv_w, int k,
                   const float *res, const float *wm, float bm, int B, int C, int Y, int X, float *logit,
                   float *block_out, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Deformable convolution, DCN v1 (csrc/deform_conv.hip, csrc/deform_taps.h): the data-dependent bilinear gather of
 * mmcv 1.x deform_conv2d (the deformable im2col) and its transpose.  The dense products around them (weight x col,
 * weight^T x grad_out, grad_out x col^T) are GEMMs and stay with the caller (ocrfdet_amd/deform_conv.py).  f32, no
 * workspace, no host reads.
 *
 * Geometry.  x (n, C, H, W), offset (n, dg * 2 * kh * kw, Ho, Wo), both contiguous; K = kh * kw, P = Ho * Wo,
 *   Ho = (H + 2 pad_h - dil_h (kh - 1) - 1) / stride_h + 1 (Wo alike), which the entry points compute themselves.
 *   Input channel c belongs to deformable group g = c / (C / dg).
 * Sampling rule.  For tap k = i * kw + j of group g at output position (ho, wo), offset channel g * 2K + 2k is the ROW
 *   offset and 2k + 1 the COLUMN offset:
 *     h = (float)(ho * stride_h - pad_h + i * dil_h) + off_h,   w = (float)(wo * stride_w - pad_w + j * dil_w) + off_w.
 *   The sample is 0 unless h > -1 && w > -1 && h < H && w < W (in float, so that a NaN fails).  Inside, hl = floorf(h),
 *   lh = h - hl (w alike), and the corners (hl | hl + 1, wl | wl + 1) carry (1 - lh | lh) * (1 - lw | lw); a corner
 *   outside the map contributes 0.  The test comes before any conversion to int: for ANY float offset (NaN, infinities,
 *   1e30) the weights are 0 and the indices lie inside the map.
 *
 * ocrf_deform_im2col: col[b - n0][c * K + k][ho * Wo + wo] = the sample, for the images n0 <= b < n1; col holds
 *   (n1 - n0, C * K, P) floats.  One launch, every element written exactly once.  A thread takes one (image, group,
 *   chunk of 32 channels, tap, position), forms the coordinates and the four weights once and walks its channels; lanes
 *   are neighbouring positions, so the offset loads and the col stores are coalesced.
 * ocrf_deform_col2im: gcol laid out like col for the images n0 <= b < n1 -> grad_x and grad_offset of those images
 *   (both addressed as the whole (n, ...) tensors).  A thread takes one (image, group, tap, position), walks the group's
 *   channels in ascending order, adds the four corner terms gcol * weight to grad_x with float atomicAdd (the hardware
 *   add, no compare-and-swap loop) and sums
 *     d sample / d h = (1 - lw) (x[hl+1][wl] - x[hl][wl]) + lw (x[hl+1][wl+1] - x[hl][wl+1])   (w alike)
 *   times gcol in registers; each grad_offset element is written once.  grad_offset is deterministic; grad_x is a
 *   scatter to data-dependent targets and reproducible only to rounding (the order of the adds is not fixed).  The
 *   entry point zeroes grad_x of its images itself (hipMemsetAsync on the stream) and then launches once.  At an
 *   integer coordinate the derivative is the one floorf implies (from the right).
 * ocrf_deform_taps: host only, touches no GPU.  The kernels' own coordinate function (deform_taps.h) for one tap:
 *   base_h = ho * stride_h - pad_h + i * dil_h, base_w alike.  weights[0..3] and index[0..3] (row * W + column, clamped
 *   into the map) of the corners (hl, wl), (hl, wl + 1), (hl + 1, wl), (hl + 1, wl + 1); frac[0..1] = lh, lw (0 when the
 *   range test fails).
 * Limits: every size positive, stride and dilation >= 1, pad >= 0, C a multiple of dg, H, W, pad and the kernel's
 *   extent below 2^20, Ho and Wo >= 1, 0 <= n0 < n1 <= n, and x, offset, col (of the images given) each below 2 GiB
 *   (the kernels index with int); anything else returns hipErrorInvalidValue and launches nothing.
 */
int ocrf_deform_im2col(int n, int C, int H, int W, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w,
                       int dil_h, int dil_w, int dg, int n0, int n1, const float *x, const float *offset, float *col,
                       ocrf_stream_t stream);
int ocrf_deform_col2im(int n, int C, int H, int W, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w,
                       int dil_h, int dil_w, int dg, int n0, int n1, const float *gcol, const float *x,
                       const float *offset, float *grad_x, float *grad_offset, ocrf_stream_t stream);
int ocrf_deform_taps(int H, int W, int base_h, int base_w, float off_h, float off_w, float *weights, int *index,
                     float *frac);

/* ------------------------------------------------------------------------------------------
 * Geometry distillation of OcRFDet4DVGGT (csrc/group_corr.hip): the group-wise correlation volume over a camera pair
 * (mmdet3d/models/detectors/ocrfdet_vggt.py:205-216, build_cost_volume(method='group_corr')) and the two losses between
 * two volumes (:476-480).  f32, no atomics, no memset, no host reads; repeated runs are bit-identical.
 *
 * Volume.  left, right: the two views, each B blocks of (C, H, W) contiguous floats, `batch_stride` floats from one
 *   sample to the next: feats[:, 0] and feats[:, 1] of a contiguous (B, 2, C, H, W) tensor are left = feats,
 *   right = feats + C * H * W, batch_stride = 2 * C * H * W, without a copy.  Cg = C / G.
 *     out[b][g][d][h][w] = sum_{c < Cg} left[b][g Cg + c][h][w] * right[b][g Cg + c][h][max(w - d, 0)],  0 <= d < D;
 *   out (B, G, D, H, W) contiguous.  The clamp is the only border rule (the reference's torch.clamp(idx - d, min=0)).
 *   The sum runs over c ascending, one fmaf per term.
 * ocrf_group_corr_forward: ONE launch; every element of out is written once.
 * ocrf_group_corr_backward: two launches, both gathers:
 *     grad_left[b][c][h][w]   = sum_d grad_out[b][g][d][h][w] * right[b][c][h][max(w - d, 0)]             (d ascending)
 *     grad_right[b][c][h][w'] = sum over the (w, d) with max(w - d, 0) = w' of grad_out[b][g][d][h][w] * left[b][c][h][w]
 *       (w' > 0: w = w' + d < W, d ascending; w' = 0: every w <= min(d, W - 1), d ascending, w ascending inside a d),
 *   grad_left / grad_right laid out like left / right with `grad_batch_stride` (the two halves of a (B, 2, C, H, W)
 *   gradient); every element written once.
 * Limits: every size positive, C a multiple of G, 1 <= D <= 16, a stride no smaller than C * H * W, and both views, the
 *   volume and the farthest element a stride reaches below 2^31 elements (the kernels index a sample with int); anything
 *   else, a NULL pointer included, returns hipErrorInvalidValue and launches nothing.
 *
 * Losses, for s, t (B, n) contiguous:
 *     *loss_smooth = 0.1 * mean(smooth_l1(s - t, beta = 1))
 *     *loss_cos    = 1 - mean_b(s_b . t_b / (max(|s_b|, 1e-8) * max(|t_b|, 1e-8)))     (torch's cosine_similarity)
 * ocrf_kd_losses_forward: two launches.  The sums (smooth-L1 and, per sample, s.t, s.s, t.t) are accumulated in double in
 *   a fixed two-stage order: per-workgroup partials in `workspace` (ocrf_kd_losses_workspace_bytes, 8-byte aligned),
 *   then one workgroup adds them and rounds each result to float32 once.  sums (B, 3) doubles receives (s.t, s.s, t.t)
 *   per sample, for the backward.
 * ocrf_kd_losses_backward: one elementwise launch.  grad_smooth, grad_cos: device floats, the gradients of the two
 *   results.  With ns = |s_b|, hs = max(ns, 1e-8), ht alike:
 *     grad_s = 0.1 clamp(s - t, -1, 1) / (B n) * grad_smooth
 *              - grad_cos / B * (t / (hs ht) - [ns > 1e-8] (s_b . t_b) s / (hs^2 ht ns)),
 *   what torch's autograd gives through the clamp (a sample with s_b = 0 gets -t / (1e-8 ht) / B); evaluated in double,
 *   rounded once.  t gets no gradient.
 * Limits: B in [1, 65535], n >= 1, B * n < 2^31, no NULL pointer, a workspace of the queried size; anything else
 *   returns hipErrorInvalidValue (the size query: 0) and launches nothing.
 */
int ocrf_group_corr_forward(int B, int C, int H, int W, int G, int D, const float *left, const float *right,
                            long long batch_stride, float *out, ocrf_stream_t stream);
int ocrf_group_corr_backward(int B, int C, int H, int W, int G, int D, const float *grad_out, const float *left,
                             const float *right, long long batch_stride, float *grad_left, float *grad_right,
                             long long grad_batch_stride, ocrf_stream_t stream);
size_t ocrf_kd_losses_workspace_bytes(int B, long long n);
int ocrf_kd_losses_forward(int B, long long n, const float *s, const float *t, float *loss_smooth, float *loss_cos,
                           double *sums, void *workspace, size_t workspace_bytes, ocrf_stream_t stream);
int ocrf_kd_losses_backward(int B, long long n, const float *s, const float *t, const double *sums,
                            const float *grad_smooth, const float *grad_cos, float *grad_s, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Streaming object tracking (csrc/track_assoc.hip): one step of greedy closest-centre association (the scheme of
 * CenterPoint's nuScenes tracker) for all B samples in ONE launch, on the padded output of the fused decode
 * (CenterHead.get_bboxes_padded).  No host reads, no atomics, no workspace; reruns are bit-identical.
 *
 * Inputs (device): boxes (B, M, D) f32, D = 9 or 7 (bottom-centre z; D = 7: zero velocity); scores (B, M) f32; labels
 *   (B, M) int32; counts (B) int32, clamped to [0, M] by the kernel; ego2global (B, 4, 4) f32, key ego -> global;
 *   time_lag (B) f32, seconds since that sample's previous frame; new_sequence (B) bytes or NULL; max_dist (n_classes)
 *   f32.  Host scalars: n_classes in [1, OCRF_TRACK_MAX_CLASSES], max_age >= 1, min_score, cap = max_age * M.
 * State, double-buffered (`*_in` is read, `*_out` fully written: all cap slots, the ones past the new count with zeros;
 *   no `_in` array may be its `_out` array): per track pos (2) f64 and vel (2) f64 in the global frame, label, id,
 *   misses, hits int32, each (B, cap); per sample count (B) and next_id (B) int32.  count_in is clamped to [0, cap].
 * Outputs: ids (B, M) and hits (B, M) int32; rows past counts[b] and untracked rows get id -1 and hits 0.
 *
 * A detection is untracked when its label is outside [0, n_classes), when max_dist[label] is not > 0, when
 * score < min_score, or when its centre, z or (D = 9) velocity is not finite.
 * Per tracked detection, in f64, one operation at a time in the order written, without contraction (E the widened
 * ego2global, (x, y, z) = boxes[..., 0:3] as stored, dt the widened time_lag[b]):
 *     gx = ((E00 x + E01 y) + E02 z) + E03,  gy likewise with row 1;
 *     vgx = E00 vx + E01 vy,  vgy = E10 vx + E11 vy;      px = gx - vgx dt,  py = gy - vgy dt;
 *     d2 = (tx - px) (tx - px) + (ty - py) (ty - py) against a stored track (tx, ty).
 * A track is a candidate when it has the detection's label, is unclaimed and d2 <= r r, r the widened max_dist[label]
 * (equality matches; no square root).  Matching is greedy in row order: each tracked detection takes the candidate of
 * smallest d2, ties to the lowest slot, and claims it.  Only equal labels match, so the classes are independent.
 * A matched detection keeps the track's id, hits = old hits + 1.  An unmatched one gets id = next_id[b] + rank (its
 * position among the sample's unmatched tracked detections in row order) and hits = 1; next_id grows by their number
 * (int32, no wrap-around handling).  An unmatched old track gets misses + 1, hits = 0 and pos += vel dt (a product, then
 * a sum), and is kept iff its new misses < max_age.
 * New state: first the tracked detections in row order (pos = (gx, gy), vel = (vgx, vgy), misses 0), then the kept old
 * tracks in old slot order; a slot beyond cap is dropped (it cannot occur with a state this kernel wrote).
 * A sample with new_sequence[b] != 0 starts from count 0 and keeps its next_id.
 *
 * Shape: one workgroup per sample, one wavefront per class (at least two, classes round-robin over the waves).  Each
 * wave gathers its class's tracks in slot order into LDS, runs its greedy loop alone (the argmin is a cross-lane
 * reduction over (d2, slot)), then one wave ranks the rows and one the old slots by ballot scans, and all threads write.
 * ocrf_track_step_lds_bytes(M, cap): the dynamic LDS of the launch (32 M + 24 cap bytes), 0 for sizes that are not
 * positive.  Limits: B in [1, 65535], M >= 1, cap == max_age * M, dynamic LDS <= OCRF_TRACK_MAX_LDS (64 KiB less the static words; M <= 627 at max_age 3),
 * no NULL operand but new_sequence; anything else returns hipErrorInvalidValue and launches nothing.
 */
#define OCRF_TRACK_MAX_CLASSES 16
#define OCRF_TRACK_MAX_LDS 65280
size_t ocrf_track_step_lds_bytes(int M, int cap);
int ocrf_track_step(int B, int M, int D, int n_classes, int max_age, float min_score, int cap, const float *boxes,
                    const float *scores, const int *labels, const int *counts, const float *ego2global,
                    const float *time_lag, const unsigned char *new_sequence, const float *max_dist,
                    const double *pos_in, const double *vel_in, const int *label_in, const int *id_in,
                    const int *misses_in, const int *hits_in, const int *count_in, const int *next_id_in,
                    double *pos_out, double *vel_out, int *label_out, int *id_out, int *misses_out, int *hits_out,
                    int *count_out, int *next_id_out, int *ids, int *hits, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * nuScenes detection metrics (csrc/det_eval.hip; ocrfdet_amd/detection_eval.py is the caller): AP over centre-distance
 * thresholds, the five true-positive errors, mAP and NDS of `detection_cvpr_2019`, from the padded output of the fused
 * decode and padded ground truth, accumulated batch by batch without a host read.  The rules below are written from
 * the benchmark's published procedure; they are the specification here (tests/eval_oracle.py restates them
 * sequentially), they have not been compared with the nuScenes devkit's own output.
 *
 * Inputs per batch (device), all in the key frame's ego frame: boxes (B, M, D) f32, D = 9 or 7, columns (x, y, z, w, l,
 *   h, yaw[, vx, vy]); scores (B, M) f32; labels (B, M) int32; counts (B) int32, clamped to [0, M]; gt_boxes (B, G, D)
 *   f32 in the same columns; gt_labels (B, G) int32; gt_counts (B) int32, clamped to [0, G]; gt_attrs (B, G) int32 or
 *   NULL, -1 = none; gt_valid (B, G) bytes or NULL (0 = not evaluated).  Tables: class_range (n_classes) f32 metres;
 *   class_tab (n_classes, 3) int32 = (attribute of a moving prediction, of a still one, -1 = none; flags:
 *   OCRF_DET_EVAL_HALF_TURN the yaw period is pi, _NO_ORIENT / _NO_VEL / _NO_ATTR the class has no such error).
 *   Host scalars: th (4) f64 the distance thresholds, tp_index in [0, 4) the one whose matches carry the errors,
 *   sample_index the number of samples accumulated before this batch, capacity the samples the buffers hold.
 *
 * Evaluated: a box whose label is in [0, n_classes), whose x, y, z (and score, for a prediction) are finite, whose
 *   gt_valid byte (ground truth) is not 0 and for which x x + y y < r r in f64 (a product, a product, a sum), r the
 *   widened class_range[label].  Centre distances, yaw and velocity differences and speeds are invariant under the
 *   rigid ego -> global map, so no pose is needed.
 * Predicted attribute: class_tab[label][0] when vx vx + vy vy > 0.2 0.2 in f64 (0.2 the double), else [1]; D = 7: [1].
 * Matching, per sample, class and threshold t = th[k]: the evaluated predictions of the class in descending score
 *   (-0 counts as +0), ties to the lowest row, each take the unclaimed evaluated ground truth of the class with the
 *   smallest d2 = dx dx + dy dy, dx = px - gx, dy = py - gy in f64, ties to the lowest index; the prediction is a
 *   true positive iff d2 < t t (strict) and then claims the box, else a false positive.  Four separate claim sets.
 * Errors of a prediction matched at th[tp_index], in f64, one operation at a time in the order written:
 *   trans  sqrt(d2)
 *   scale  1 - i / ((vp + vg) - i), i = (min(w) min(l)) min(h), v = (w l) h
 *   orient |a|, a = m - P / 2 with m = fmod((yaw_g - yaw_p) + P / 2, P), plus P when negative; a less 2 pi when a > pi;
 *          P = pi with OCRF_DET_EVAL_HALF_TURN, else 2 pi (the doubles nearest pi and 2 pi)
 *   vel    sqrt(dvx dvx + dvy dvy), dv = v_p - v_g; NaN when D = 7 or a ground-truth velocity component is NaN
 *   attr   0 when the predicted attribute equals gt_attrs, else 1; NaN when gt_attrs is NULL or -1
 * Record of slot (sample_index + b) M + row: key (u32: ~o, o the score's bits with the sign bit flipped when it is
 *   clear and all bits flipped when it is set, so that ascending keys are descending scores; 0xFFFFFFFF when not evaluated), info
 *   (int32: class | OCRF_DET_EVAL_EVALUATED | tp bits << 8; class 31 and nothing else when not evaluated), match (4
 *   int32: the claimed ground-truth index per threshold, -1 none), err (5 f64 in the order above, NaN when unmatched).
 *   gt_count[(sample_index + b) n_classes + c]: the evaluated ground truth of class c.  Every slot of the batch and
 *   every count is written on each call.
 * ocrf_det_eval_match: ONE launch, one workgroup per sample, one wavefront per class (at least two, classes
 *   round-robin over the waves); no atomics, no workspace, reruns bit-identical.  ocrf_det_eval_match_lds_bytes(M, G):
 *   its dynamic LDS (52 M + 28 G + 128 bytes), 0 for sizes that are not positive.  Limits: B in [1, 65535], M, G >= 1, D in
 *   {7, 9}, n_classes in [1, OCRF_DET_EVAL_MAX_CLASSES], 0 <= sample_index, sample_index + B <= capacity, capacity M
 *   < 2^31, dynamic LDS <= OCRF_DET_EVAL_MAX_LDS, finite th, no NULL operand but gt_attrs and gt_valid; anything else
 *   returns hipErrorInvalidValue and launches nothing.
 *
 * Summary over the first n_samples samples (n = n_samples M slots).  Global order per class: descending score, ties
 *   by slot (sample in order of arrival, then row): a stable LSD sort by key, then by class.  Per class c with its n_c
 *   evaluated predictions in that order and npos = the sum of its gt_count, per threshold, in f64 as numpy defines
 *   cumsum, linspace and interp:
 *     tp, fp the cumulative counts; prec = tp / (tp + fp); rec = tp / npos; conf the widened scores;
 *     rec_interp[j] = j 0.01 (j = 100: 1); prec_i = interp(rec_interp, rec, prec, right = 0), conf_i likewise;
 *     AP = (sum_j=first..100 max(prec_i[j] - min_precision, 0)) / (101 - first) / (1 - min_precision), summed in order;
 *   per error e over the K matches of th[tp_index] (conf_m, e_m in that order): cm[k] = (sum of the non-NaN e_m[0..k])
 *     / their number, 0 where that number is 0, all ones when every e_m is NaN; err_i = interp(conf_i, conf_m, cm)
 *     taken over the reversed (ascending) arrays; TP metric = the mean of err_i[first .. last], summed in order, last
 *     the largest j with conf_i[j] != 0 (0 when none); 1 when last < first.
 *   npos = 0 or n_c = 0: AP 0, errors 1.  K = 0: errors 1.  A class with _NO_ORIENT / _NO_VEL / _NO_ATTR: NaN there.
 *   mAP = the mean over classes of the mean over thresholds; mTP_e = the mean over the classes where it is not NaN (NaN
 *   when none); NDS = (5 mAP + sum_e (1 - min(1, mTP_e))) / 10, a NaN mTP_e counting as 1.
 * ocrf_det_eval_summary: copies the keys, sorts them and the classes (radix driver), gathers order / sorted_cls / the
 *   TP flags, scans the flags (look-back scan, one per threshold), one curve launch of (n_classes, 9) workgroups (the
 *   NaN-aware sums run as a fixed-order f64 prefix inside it: 128-wide chunks in sequence, a shuffle scan in each)
 *   and one final workgroup.  Outputs: order (n) int32 slots, sorted_cls (n) int32 (class; 16 for what is not
 *   evaluated, sorted last), tp_excl (4, n) int32 exclusive prefix of the TP flags over the whole order, result
 *   (9 n_classes + 7) f64 = AP (n_classes, 4), errors (n_classes, 5), mAP, mTP (5), NDS.  A look-back scan that gave up
 *   turns every result into NaN (the gather clamps the sort's ids into [0, n), so nothing is read out of bounds then).  Reads nothing back.  Limits: n_samples >= 1, n < 2^31, first in [1, 100],
 *   min_precision in [0, 1), a workspace of ocrf_det_eval_summary_workspace_bytes(n) bytes (0 for such n), 256-byte
 *   aligned; anything else returns hipErrorInvalidValue and launches nothing.
 */
#define OCRF_DET_EVAL_MAX_CLASSES 16
#define OCRF_DET_EVAL_MAX_LDS 65024
#define OCRF_DET_EVAL_EVALUATED 32
#define OCRF_DET_EVAL_HALF_TURN 1
#define OCRF_DET_EVAL_NO_ORIENT 2
#define OCRF_DET_EVAL_NO_VEL 4
#define OCRF_DET_EVAL_NO_ATTR 8
size_t ocrf_det_eval_match_lds_bytes(int M, int G);
int ocrf_det_eval_match(int B, int M, int D, int G, int n_classes, long long sample_index, long long capacity,
                        double th0, double th1, double th2, double th3, int tp_index, const float *boxes,
                        const float *scores, const int *labels, const int *counts, const float *gt_boxes,
                        const int *gt_labels, const int *gt_counts, const int *gt_attrs, const unsigned char *gt_valid,
                        const float *class_range, const int *class_tab, unsigned *rec_key, int *rec_info,
                        int *rec_match, double *rec_err, int *gt_count, ocrf_stream_t stream);
size_t ocrf_det_eval_summary_workspace_bytes(long long n_slots);
int ocrf_det_eval_summary(long long n_samples, int M, int n_classes, int tp_index, int first, double min_precision,
                          const unsigned *rec_key, const int *rec_info, const double *rec_err, const int *gt_count,
                          const int *class_tab, int *order, int *sorted_cls, int *tp_excl, double *result,
                          void *workspace, size_t workspace_bytes, ocrf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-kernel device timer (measurement aid for bench.py; not part of the reference's surface)
 * ------------------------------------------------------------------------------------------
 * While a timer is armed for kernel id K, every launch of K inside the library is bracketed by
 * a hipEvent pair recorded on the launch stream (hipExtLaunchKernelGGL), up to `capacity`
 * launches.  ocrf_timer_read waits for the recorded pairs and returns their elapsed
 * milliseconds.  Several timers (for different kernel ids) may be armed at once; arming with
 * timer == NULL disarms all of them.  Host-side only.  The rasteriser's front end (preprocess, scan,
 * gather) is launched by the backward too, under the same ids; nothing in the package arms those. */
enum {
  OCRF_K_BEV_POOL_FWD = 1,      /* bev_pool_tile_kernel */
  OCRF_K_BEV_POOL_FIXUP = 2,    /* (retired) */
  OCRF_K_BEV_POOL_INTERVAL = 3, /* bev_pool_interval_kernel */
  OCRF_K_BEV_POOL_GRAD = 4,     /* bev_pool_grad_vec_kernel */
  OCRF_K_BEV_POOL_NCHW = 5,     /* (retired: the tile kernel writes the final layout itself) */
  OCRF_K_BEV_POOL_MFMA = 6,     /* bev_pool_mfma_kernel<C / 16> */
  OCRF_K_BEV_POOL_PANEL = 7,    /* bev_pool_panel_kernel<C / 4> */
  OCRF_K_BEV_POOL_CELL_WEIGHTS = 8, /* bev_pool_cell_weights_kernel */
  OCRF_K_RASTER_PREPROCESS = 10, /* raster_preprocess_kernel */
  OCRF_K_RASTER_BLEND = 11,      /* raster_blend_kernel */
  OCRF_K_RASTER_GATHER = 12,     /* raster_scatter_kernel */
  OCRF_K_RASTER_SCAN = 13,       /* raster_bucket_scan_kernel */
  OCRF_K_RASTER_BLEND_BWD = 15,  /* raster_blend_kernel<false, true> */
  OCRF_K_RASTER_PRE_BWD = 16,    /* raster_preprocess_backward_kernel<false> */
  OCRF_K_RASTER_PLAN_UPDATE = 17,  /* raster_plan_head_kernel (rounds 3-4: raster_plan_update_kernel) */
  OCRF_K_RASTER_BLEND_SORTED = 18, /* raster_blend_sorted_kernel<*>, first pass */
  OCRF_K_RASTER_BLEND_SECOND = 19, /* raster_blend_sorted_kernel<*>, second pass (tile pairs handed over by the first) */
  OCRF_K_HOA_STATS = 20,         /* hoa_channel_stats_kernel */
  OCRF_K_HOA_MASK_GATE = 21,     /* hoa_mask_gate_kernel */
  OCRF_K_HOA_HEIGHT_MAX = 22,    /* hoa_height_max_kernel */
  OCRF_K_HOA_HEIGHT_GATE = 23,   /* hoa_height_gate_kernel / hoa_height_gate_from_tiles_kernel */
  OCRF_K_HOA_UNET_BLOCK = 24,    /* hoa_unet_block_kernel */
  OCRF_K_HOA_OUT_CONV = 25,      /* hoa_gated_conv1x1_kernel */
  OCRF_K_HOA1_ATTN = 26,         /* hoa1_attention_upsample_kernel */
  OCRF_K_HOA1_UP = 27,           /* unused since round 2 (fused into OCRF_K_HOA1_ATTN) */
  OCRF_K_HOA1_Q = 28,            /* unused since round 2 (q is rebuilt by its consumers) */
  OCRF_K_HOA1_KV = 29,           /* hoa1_kv_kernel */
  OCRF_K_HOA_DW3X3 = 30,         /* hoa_dw3x3_kernel */
  OCRF_K_HOA_DW3X3_WGRAD = 31,   /* hoa_dw3x3_wgrad_kernel */
  OCRF_K_LSS_KEYS = 40,          /* lss_keys_hist_kernel (keys + the first radix histogram) */
  OCRF_K_RADIX_HIST = 41,        /* radix_hist_kernel */
  OCRF_K_SCAN = 42,              /* scan_apply_kernel<T> */
  OCRF_K_RADIX_SCATTER = 43,     /* radix_scatter_kernel<*> */
  OCRF_K_LSS_BOUNDS = 44,        /* lss_intervals_kernel */
  OCRF_K_LSS_EMIT = 45,          /* unused since round 5 (the last radix pass scatters into the rank vectors) */
  OCRF_K_HT_COUNT = 46,          /* ht_valid_kernel */
  OCRF_K_HT_EMIT = 47,           /* ht_emit_kernel */
  OCRF_K_HT_PROJECT = 48,        /* ht_project_kernel */
  OCRF_K_NECK_PREFILTER = 60,    /* neck_prefilter_kernel */
  OCRF_K_NECK_SAMPLE = 61,       /* neck_pillar_sample_mean_kernel<C> */
  OCRF_K_NECK_RETAIN = 62,       /* neck_fill_kernel + neck_retain_scatter_kernel */
  OCRF_K_NECK_HEADS = 63,        /* neck_gauss_heads_kernel */
  OCRF_K_NECK_NERF_ALPHA = 64,   /* neck_nerf_alpha_kernel */
  OCRF_K_NECK_NERF_RENDER = 65,  /* neck_nerf_render_kernel */
  OCRF_K_NECK_FUSION = 66,       /* neck_dual_fusion_kernel<C, M> */
  OCRF_K_NECK_PLANE_PASS = 67,   /* neck_plane_pass_kernel<WRITE, RELU, STATS> */
  OCRF_K_NECK_CHANNEL_MLP = 68,  /* neck_channel_mlp_kernel */
  OCRF_K_NECK_SCALED_STATS = 69, /* neck_scaled_channel_stats_kernel */
  OCRF_K_NECK_CBAM_TAIL = 70,    /* neck_cbam_tail_kernel */
  OCRF_K_RASTER_SH = 50,         /* sh_colors_kernel */
  OCRF_K_RASTER_SH_BWD = 51,     /* sh_colors_backward_kernel */
  OCRF_K_NECK_HEADS_BWD = 71,    /* neck_gauss_heads_backward_kernel */
  OCRF_K_NECK_HEADS_BWD_SUM = 72, /* neck_partial_rows_sum_kernel (both stages) */
  OCRF_K_LOSS_DEPTH_LABELS = 80, /* depth_labels_kernel */
  OCRF_K_LOSS_DS = 81,           /* ds_loss_partial_kernel */
  OCRF_K_LOSS_FINAL = 82,        /* ds_loss_final_kernel, render_final_kernel */
  OCRF_K_LOSS_DS_BWD = 83,       /* ds_loss_backward_kernel */
  OCRF_K_LOSS_RENDER = 84,       /* render_tile_kernel */
  OCRF_K_LOSS_RENDER_DEPTH = 85, /* render_depth_kernel */
  OCRF_K_LOSS_RENDER_BWD = 86,  /* render_backward_kernel */
  OCRF_K_STEREO_COST_VOLUME = 90, /* stereo_cost_volume_kernel */
  OCRF_K_CH_ASSIGN = 91,         /* ch_assign_kernel */
  OCRF_K_CH_HEATMAP = 92,        /* ch_heatmap_kernel */
  OCRF_K_CH_HM_LOSS = 93,        /* ch_hm_loss_partial_kernel */
  OCRF_K_CH_FINAL = 94,          /* ch_hm_loss_final_kernel, ch_reg_loss_final_kernel */
  OCRF_K_CH_HM_LOSS_BWD = 95,    /* ch_hm_loss_backward_kernel */
  OCRF_K_CH_REG_LOSS = 96,       /* ch_reg_loss_partial_kernel */
  OCRF_K_CH_REG_LOSS_BWD = 97,   /* ch_reg_loss_backward_kernel */
  OCRF_K_CD_SELECT = 98,         /* cd_select_kernel */
  OCRF_K_CD_MASK = 99,           /* cd_mask_kernel */
  OCRF_K_CD_SCAN = 100,          /* cd_scan_kernel */
  OCRF_K_CD_WRITE = 101,         /* cd_write_kernel */
  OCRF_K_UPSAMPLE_CAT = 102,     /* upsample_cat_kernel<float, V> */
  OCRF_K_UPSAMPLE_CAT_BWD = 103, /* upsample_cat_backward_kernel<float> */
  OCRF_K_ADD_RELU = 104,         /* binary_kernel<V, AddRelu> */
  OCRF_K_ADD_RELU_BWD = 105,     /* binary_kernel<V, Threshold> */
  OCRF_K_UPSAMPLE_ADD = 106,     /* upsample_add_kernel<V> */
  OCRF_K_UPSAMPLE_ADD_BWD = 107, /* upsample_add_backward_kernel */
  OCRF_K_BEV_ALIGN = 108,        /* bev_align_kernel<float, V> */
  OCRF_K_BEV_ALIGN_BWD = 109,    /* bev_align_backward_kernel<float> */
  OCRF_K_OPTIM_SQNORM = 110,     /* optim_grad_sqnorm_kernel */
  OCRF_K_OPTIM_NORM_FINAL = 111, /* optim_norm_final_kernel */
  OCRF_K_OPTIM_STEP = 112,       /* optim_step_kernel */
  OCRF_K_ADD_RELU_BF16 = 113,     /* binary_bf16_kernel<V, AddRelu> */
  OCRF_K_ADD_RELU_BWD_BF16 = 114, /* binary_bf16_kernel<V, Threshold> */
  OCRF_K_UPSAMPLE_ADD_BF16 = 115, /* upsample_add_bf16_kernel<V> */
  OCRF_K_UPSAMPLE_ADD_BWD_BF16 = 116, /* upsample_add_backward_bf16_kernel */
  OCRF_K_UPSAMPLE_CAT_BF16 = 117,     /* upsample_cat_kernel<unsigned short, V> */
  OCRF_K_UPSAMPLE_CAT_BWD_BF16 = 118, /* upsample_cat_backward_kernel<unsigned short> */
  OCRF_K_BEV_ALIGN_BF16 = 119,        /* bev_align_kernel<unsigned short, V> */
  OCRF_K_BEV_ALIGN_BWD_BF16 = 120,    /* bev_align_backward_kernel<unsigned short> */
  OCRF_K_STEREO_PACK_BF16 = 121,      /* stereo_pack_bf16_kernel */
  OCRF_K_STEREO_COST_VOLUME_BF16 = 122, /* stereo_cost_volume_bf16_kernel */
  OCRF_K_BN_STATS = 123,              /* bn_stats_kernel<float, V> */
  OCRF_K_BN_FINALIZE = 124,           /* bn_finalize_kernel */
  OCRF_K_BN_ACT_FWD = 125,            /* bn_act_forward_kernel<float, V> */
  OCRF_K_BN_ACT_BWD_REDUCE = 126,     /* bn_act_backward_reduce_kernel<float, V> */
  OCRF_K_BN_ACT_BWD = 127,            /* bn_act_backward_kernel<float, V> */
  OCRF_K_BN_STATS_BF16 = 128,         /* bn_stats_kernel<unsigned short, V> */
  OCRF_K_BN_ACT_FWD_BF16 = 129,       /* bn_act_forward_kernel<unsigned short, V> */
  OCRF_K_BN_ACT_BWD_REDUCE_BF16 = 130, /* bn_act_backward_reduce_kernel<unsigned short, V> */
  OCRF_K_BN_ACT_BWD_BF16 = 131,       /* bn_act_backward_kernel<unsigned short, V> */
  OCRF_K_FRAME_POSES = 132,           /* frame_poses_kernel */
  OCRF_K_IMAGE_PREP_HORIZONTAL = 133, /* image_prep_horizontal_kernel */
  OCRF_K_IMAGE_PREP_VERTICAL = 134,   /* image_prep_vertical_kernel */
  OCRF_K_IMAGE_PREP_EPILOGUE = 135,   /* image_prep_epilogue_kernel */
  OCRF_K_POINT_LABELS_MARK = 136,     /* point_labels_mark_kernel */
  OCRF_K_POINT_LABELS_RESOLVE = 137,  /* point_labels_resolve_kernel */
  OCRF_K_DEFORM_IM2COL = 138,         /* deform_im2col_kernel */
  OCRF_K_DEFORM_COL2IM = 139,         /* deform_col2im_kernel */
  OCRF_K_GROUP_CORR = 140,            /* group_corr_forward_kernel<DT> */
  OCRF_K_GROUP_CORR_GRAD_LEFT = 141,  /* group_corr_grad_left_kernel<DT> */
  OCRF_K_GROUP_CORR_GRAD_RIGHT = 142, /* group_corr_grad_right_kernel<DT> */
  OCRF_K_KD_PARTIAL = 143,            /* kd_partial_kernel */
  OCRF_K_KD_FINAL = 144,              /* kd_final_kernel */
  OCRF_K_KD_BWD = 145,                /* kd_backward_kernel */
  OCRF_K_RASTER_BLEND_BWD_DEPTH = 146, /* raster_blend_kernel<false, true, true, true, true> */
  OCRF_K_RASTER_PRE_BWD_DEPTH = 147,  /* raster_preprocess_backward_kernel<true> */
  OCRF_K_HOA1_ATTN_TRAIN = 148,       /* hoa1_attention_train_kernel */
  OCRF_K_HOA1_UP_GRAD = 149,          /* hoa1_up_grad_kernel */
  OCRF_K_HOA1_ATTN_GRAD = 150,        /* hoa1_attn_grad_kernel */
  OCRF_K_HOA1_KV_GRAD = 151,          /* hoa1_kv_grad_kernel */
  OCRF_K_HOA1_TOKEN_GRAD = 152,       /* hoa1_token_grad_kernel */
  OCRF_K_HOA1_PIXEL_GRAD = 153,       /* hoa1_pixel_grad_kernel */
  OCRF_K_HOA1_WEIGHT_SUM = 154,       /* hoa1_weight_sum_kernel */
  OCRF_K_BEV_STREAM_ALIGN = 155,      /* bev_stream_align_kernel<float, V> */
  OCRF_K_BEV_STREAM_ALIGN_BF16 = 156, /* bev_stream_align_kernel<unsigned short, V> */
  OCRF_K_CD_SELECT_BF16 = 157,        /* cd_select_kernel<unsigned short> */
  OCRF_K_TRACK_STEP = 158,            /* track_step_kernel */
  OCRF_K_DET_EVAL_MATCH = 159,        /* det_eval_match_kernel */
  OCRF_K_DET_EVAL_GATHER = 160,       /* det_eval_gather_kernel */
  OCRF_K_DET_EVAL_CURVES = 161,       /* det_eval_curves_kernel */
  OCRF_K_DET_EVAL_FINAL = 162,        /* det_eval_final_kernel */
  OCRF_K_DET_EVAL_COPY_KEYS = 163,    /* det_eval_copy_keys_kernel */
  OCRF_K_DET_EVAL_CLASS_KEYS = 164    /* det_eval_class_keys_kernel */
};
const char *ocrf_kernel_name(int kernel_id);           /* symbol as rocprofv3 prints it */
/* Diagnostic: a one-thread kernel that stores the device's constant-rate clock (wall_clock64, 100 MHz)
 * into *slot (device) when the stream reaches it — timelines inside a hipGraph replay, where host
 * events cannot be placed and the profiler's per-kernel signals perturb the overlap. */
int ocrf_diag_stamp(unsigned long long *slot, void *stream);
/* Diagnostic: n_blocks one-wave workgroups that each record where they ran: out[b] = XCC_ID << 16 | HW_ID[15:0]
 * (CU_ID bits 11:8, SH_ID 12, SE_ID 15:13) after idling for spin_ticks of the 100 MHz clock — the compute units a
 * CU-masked stream really owns. */
/* Diagnostic: with a device buffer of (tile pairs x items x 4 waves x 8) u64 set, the next ocrf_rasterize_planned
 * calls run an instrumented build of the sorted blend: per wave scan / stage / blend cycles (s_memtime) and the
 * number of scanned, staged, listed and evaluated records.  NULL switches it off. */
int ocrf_diag_plan_stats(unsigned long long *buf);
int ocrf_diag_plan_resident(void); /* workgroups the persistent sorted blend launches (occupancy API x CUs) */
int ocrf_diag_where(int n_blocks, unsigned *out, int spin_ticks, void *stream);
/* Diagnostic: the library's stable radix sort (csrc/radix_sort.hip) on its own.  n device keys below 2^key_bits
 * (key_bits 1 .. 32; `keys` is clobbered) leave as out_keys ascending and out_ids = their original positions, ascending
 * among equal keys.  ocrf_diag_radix_sort_states (host pointers for the three results): where in the workspace the call
 * leaves the look-back state blocks of its n_states passes, stride_words 64-bit words apart; bit 63 of a block's first
 * word says that pass's scan gave up. */
int ocrf_diag_radix_sort(unsigned *keys, int n, int key_bits, unsigned *out_keys, int *out_ids, void *workspace,
                         size_t workspace_bytes, ocrf_stream_t stream);
size_t ocrf_diag_radix_sort_workspace_bytes(int n);
int ocrf_diag_radix_sort_states(void *workspace, int n, int key_bits, size_t *offset_bytes, int *n_states,
                                long *stride_words);
/* HIP streams for the hot path's chains (host pointers): cu_mask (n_words x 32 bits, NULL = every CU) restricts the
 * stream's kernels to those compute units (hipExtStreamCreateWithCUMask); without a mask `priority` is the HIP stream
 * priority (lower = more urgent).  The stream is non-blocking w.r.t. the legacy default stream. */
/* Node census of a captured hipGraph (hipGraph_t; host pointers).  Graphs with memset nodes fault on replay after an
 * intervening hipMemcpyAsync on ROCm 7.2 / gfx950: this library zero-fills with a kernel, and owners of captured graphs
 * (GraphedNeck) refuse a graph whose census shows a memset node (e.g. a torch.zeros added inside the captured region). */
int ocrf_graph_node_census(void *graph, int *n_kernel, int *n_memset, int *n_memcpy, int *n_other);
int ocrf_stream_create(const uint32_t *cu_mask, int n_words, int priority, void **stream_out);
/*
 * One host call per step (csrc/step.hip).  The reference's boundary is one pybind call per op
 * (mmdet3d/ops/bev_pool_v2/src/bev_pool.cpp:30-57); a step of the hot path here is ~18 launches behind seven of the
 * entry points above on two HIP streams, and issuing them from Python costs the host as long as the device needs to
 * run them.  An ocrf_step holds the calls of ONE step — entry point + argument values, recorded once while the step ran
 * eagerly — and the fork / join points between its streams; ocrf_hotpath_step replays them from C on the caller's
 * streams: the same entry points with the same arguments, launched eagerly (no hipGraph).  Pointer arguments are used as
 * recorded: the caller keeps inputs, outputs and scratch alive and in place, as for a captured graph.
 *   ocrf_step_fn_id(name)    id of an entry point a step can hold (-1: not supported — issue the step call by call):
 *                            ocrf_bev_pool_v2_nchw_planned / _mfma / _panel / _panel_stats, ocrf_bev_pool_cell_weights,
 *                            ocrf_rasterize_planned, ocrf_raster_plan_build, ocrf_hoa1_forward, ocrf_hoa_v2b_forward,
 *                            ocrf_hoa_channel_stats, ocrf_hoa_opacity_mask_gate, ocrf_stream_write_value32
 *   ocrf_step_add_call       args: the entry point's arguments WITHOUT its trailing stream, one 64-bit word each —
 *                            pointers / sizes / ints (sign-extended) as such, a float as its bit pattern in the low word;
 *                            slot: which of the streams handed to the replay the call goes to (< 8)
 *   ocrf_step_add_fork/_join stream slot `to` continues only after what slot `from` holds so far (an event record +
 *                            wait; the events belong to the step object)
 *   ocrf_step_run            replay on `streams[0 .. n_streams)`; ocrf_hotpath_step: slot 0 = main, slot 1 = side.
 * All host pointers; not thread-safe per object; returns the first non-zero status of a replayed call.
 */
typedef struct ocrf_step ocrf_step;
int ocrf_step_fn_id(const char *name);
int ocrf_step_fn_args(int fn);
int ocrf_step_create(ocrf_step **out);
void ocrf_step_destroy(ocrf_step *step);
int ocrf_step_add_call(ocrf_step *step, int fn, int slot, int n_args, const uint64_t *args);
int ocrf_step_add_fork(ocrf_step *step, int from, int to);
int ocrf_step_add_join(ocrf_step *step, int from, int to);
int ocrf_step_size(const ocrf_step *step);
int ocrf_step_run(ocrf_step *step, const ocrf_stream_t *streams, int n_streams);
int ocrf_hotpath_step(ocrf_step *step, ocrf_stream_t main_stream, ocrf_stream_t side_stream);

/* value -> *ptr (device int) in stream order, no kernel launch (hipStreamWriteValue32). */
int ocrf_stream_write_value32(int *ptr, int value, ocrf_stream_t stream);
int ocrf_stream_destroy(void *stream);
int ocrf_timer_create(int capacity, void **timer_out); /* host pointers */
int ocrf_timer_arm(void *timer, int kernel_id);
int ocrf_timer_read(void *timer, float *ms_out /* host */, int capacity, int *count_out /* host */);
int ocrf_timer_destroy(void *timer);

/* Diagnostics of the pooling kernel (A/B timing of variants in one process; never on the product path).
 * ocrf_tune_set: key 0 = rounds of the point walk per slice of a heavy tile (1..64; default 4), key 1 = deal
 * workgroups to XCDs in contiguous unit ranges (default 1), key 2 = cap on the workgroups of the launch (0 = one per
 * unit), key 3 = voxels per tile (32 | 64; default 64).  Plans and workspaces are sized for the values in
 * force when they were built.  ocrf_diag_bev_pool_stamps: the planned pooling with s_memtime accumulated per
 * phase and unit into stamps[ocrf_bev_pool_max_units(...)][8] = {table + zero-fill, staging, gather, combine,
 * write-out, points of the unit, -, -}. */
int ocrf_tune_set(int key, int value);
int ocrf_bev_pool_max_units(int c, int n_points, int B, int Z, int Y, int X);
int ocrf_diag_bev_pool_stamps(int c, int n_points, const float *depth, const float *feat, const int *ranks_depth,
                              const int *ranks_feat, void *plan, float *out, int B, int Z, int Y, int X, int layout,
                              void *workspace, unsigned long long *stamps, ocrf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* OCRF_HIP_H */
