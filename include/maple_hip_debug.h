/* include/maple_hip_debug.h -- measurement aids and test hooks of libmaple_hip_debug.so.
 *
 * NOT part of the operator boundary (include/maple_hip.h): the product library libmaple_hip.so does not export these.
 * __graft_entry__.build() links a second library, libmaple_hip_debug.so, from the product library's objects plus the one unit
 * that defines these (maple_amd/csrc/debug_abi.hip): every entry point of maple_hip.h plus the ones below.  The tests of the two innermost device functions (getPartialVec M:4073-4141,
 * simplify M:3697-3717: SURVEY 8a rows a3 / a4, which no batched operator exposes on their own), of the wavefront-wide
 * appendProbNode, the PMC calibration (tools/calib_fetch.py) and the level profile (tools/level_profile.py) load that one
 * (maple_amd.runtime.Device(..., debug=True)). */
#ifndef MAPLE_HIP_DEBUG_H
#define MAPLE_HIP_DEBUG_H
#include "maple_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Profile of the last frontier-tier pass of maple_spr_search_batch (until the next maple_timing_reset): per level of the
 * expansion, the items that still updated genome lists, the items in the cached regime, and the HIP-event time (ms) of the
 * level's two kernels; waveItems*: how many of the list-updating items were walked a wavefront each, by size class.  *n levels
 * (the first min(*n, cap) are written).  A measurement aid; nothing is computed with it. */
int maple_debug_frontier_levels(maple_ctx *ctx, int32_t cap, int64_t *itemsUpdating, int64_t *itemsCached, float *msUpdating,
                                float *msCached, int32_t *n, int64_t *waveItemsSmall /* or NULL */, int64_t *waveItemsBig /* or NULL */);

/* The items that the wavefront-wide kernels of that pass (k_fr_updating_wave_s / k_fr_updating_wave) handed whole to lane 0.
 * counts[3]: because [0] a list does not fit the staging areas, [1] the item is scored without the parent's upper list or without
 * probVectTotUp (the on-the-spot merge of M:7198-7200), [2] it sits at the root and still updates lists (rootVector).  A library
 * built with -DMAPLE_SPR_PROFILE sets *profiled = 1 and fills slots[3 * 8] -- per kind of item (small / 512 class: 0 1 by the
 * wavefront, 2 3 lane 0: no fit, 4 5 lane 0: on-the-spot probVectTotUp, 6 7 lane 0: root) its count, total ms and slowest ms --
 * and, for the first cap levels, the slowest wavefront-wide item of the level (ms) and its kind; otherwise *profiled = 0 and those
 * are zero. */
int maple_debug_frontier_wave_paths(maple_ctx *ctx, int64_t *counts, int32_t cap, float *levelSlowestMs, int32_t *levelSlowestSlot,
                                    double *slots, int32_t *profiled);

/* The searches that pass handed to the one-lane-per-search kernel (k_spr_search), so that a test of the frontier tier can tell
 * that the tier itself answered.  *searchesHandedBack: all of them, whatever the cause (a pool or a scratch slab too small
 * included).  reasons[8]: those the exact walk (k_fr_replay) and the whole-tree replay (k_fr_replay_wide) give a reason for --
 * [1] a merge within tolerance of the stop rule, [2] a list re-expressed through a reference branch from one that shorten()
 * (M:7087) changed, [3] a fifth shortened list, [4] the search's own first list shortened, [5] a marked list without a layout,
 * [0] other; whole-tree searches: [6] a short list, scan slots or a marked item list, [7] a scanned branch whose list shorten()
 * would change.  When maple_spr_search_batch runs the tier more than once (whole-tree searches found by their budget), this is
 * the last pass. */
int maple_debug_frontier_handbacks(maple_ctx *ctx, int64_t *reasons, int64_t *searchesHandedBack);

/* appendProbNode for n (parent list, child list) pairs with ONE WAVEFRONT per pair (maple_amd/csrc/wave_dev.h: the walk cut
 * along its merge path, the factors of all steps at once, the running product in walk order): the same results as
 * maple_append_batch bit for bit; *ms (optional) = kernel time.  A test and timing aid. */
int maple_debug_wave_append_batch(maple_ctx *ctx, int32_t n, const int32_t *parentList, const int32_t *childList,
                                  const uint8_t *isTipC, const double *bLen, double *outLK, float *ms);
/* Debugging aid: record the visit sequence of query index `query` of the next maple_spr_search_batch
 * (per visited item: t1, direction, needsUpdating, failedPasses | lastLK, midProb); -1 switches it off. */
int maple_debug_trace_query(maple_ctx *ctx, int32_t query);
/* PMC calibration: `repeats` launches of a kernel that reads `bytes` bytes with this library's access pattern
 * (one lane = one contiguous 512-byte list, dependent 8-byte loads); returns the total time. */
int maple_debug_calib_walk(maple_ctx *ctx, uint64_t bytes, int32_t repeats, float *ms);
/* ... and of WRITE_SIZE: mode 1 = `bytes` written as a coalesced stream, mode 2 = one 8-byte store into every 64-byte line
 * of a `bytes`-long buffer (the way the score matrix is written: bytes / 8 useful bytes). */
int maple_debug_calib_write(maple_ctx *ctx, uint64_t bytes, int32_t mode, int32_t repeats, float *ms);
int maple_debug_trace_read(maple_ctx *ctx, int32_t *n, int32_t *items4 /*[4*4096]*/, double *vals2 /*[2*4096]*/);
/* What the library holds at this moment, process-wide (every context, no context needed): device and page-locked allocations
 * and their bytes, and stream and event handles.  Kept by the types that own those resources, so a context that was destroyed
 * has left nothing behind exactly if the three values are what they were before it was created.  Compare differences: two
 * copies of the library in one process may share the counters. */
int maple_debug_live_resources(int64_t *allocs, int64_t *bytes, int64_t *handles);
/* Parity hooks for the two innermost device functions (one lane per call):
 * getPartialVec(i12, totLen, mutMatrix, errorRate, vect, upNode, flag), M:4073-4141, with the call's own 4x4 matrix
 * (M16[16*i..], row-major) and vect4[4*i..] (read when i12 == 6); whether `flag` matters follows the model's usingErrorRate
 * (M:4109).  simplify(vec, refA), M:3697-3717 -> 0-3 nucleotide, 4 = R, 6 = keep the vector, -1 = the reference raises. */
int maple_debug_gpv_batch(maple_ctx *ctx, int32_t n, const int32_t *i12, const double *totLen, const double *M16,
                          const double *errorRate, const double *vect4, const uint8_t *upNode, const uint8_t *flag,
                          double *out4);
int maple_debug_simplify_batch(maple_ctx *ctx, int32_t n, const double *vec4, const int32_t *refA, int32_t *out);
/* passGenomeListThroughBranch of a REMOVED list as the frontier tier of the SPR search runs it (maple_amd/csrc/frontier_dev.h),
 * for n (list, mutation list or -1, direction) items: waveForm 0 = one lane per item (fpass_removed: fpass_store, then
 * shorten_would_merge), 1 = one wavefront per item (wave_pass with `removed` set).  outList[i] = a new list with the result, or
 * list[i] itself where the tier hands the input handle back (no mutations on the branch: sameHandle[i] = 1); grade[i] = what the
 * tier marks the new list with -- 0: shorten() (M:7087) would leave it as it is, 1: it would merge entries whose tails are the
 * same doubles and flag, 2: it would merge tails that are equal only within thresholdProb.  The hook compiles the tier's device
 * functions into kernels of its own: it checks the source the search is built from, not the search's object code. */
int maple_debug_frontier_pass_batch(maple_ctx *ctx, int32_t n, const int32_t *list, const int32_t *mutList, const uint8_t *dirIsUp,
                                    int32_t waveForm, int32_t *outList, uint8_t *grade, uint8_t *sameHandle);
/* Rows of the score table of whole-tree SPR searches from explicit lists, by the launches maple_spr_search_batch makes them with:
 * form 0 = the dense kernel with the bitmap of finite scores, form 1 = the witness filter (maple_amd/csrc/witness.hip: every
 * qBLen must be 0 -- the caller's duty, as in the product -- and with an error model it returns MAPLE_ERR_STATE), then the bitmap's
 * prefix counts.  nQ searches (removed lists qList, qTip, qBLen) against nC candidate lists (cand; -1 = a column without a list).
 * out[nQ * ldOut] (ldOut >= nC) is filled with `fill` first; the score of (q, k) goes to out[q * ldOut + (outCol ? outCol[k] : k)]
 * if it is finite and nowhere if it is -inf.  finMask[nQ * nWords], nWords = ceil(nC / 64): bit k % 64 of word k / 64 of row q set
 * exactly for the finite scores; prefix[nQ * (nWords + 1)]: the set bits of the row before each word, then the row's total.
 * *pairsWalked (optional): the (search, candidate) pairs form 1 walked, -1 for form 0. */
int maple_debug_score_rows(maple_ctx *ctx, int32_t form, int32_t nQ, const int32_t *qList, const uint8_t *qTip, const double *qBLen,
                           int32_t nC, const int32_t *cand, const int32_t *outCol /* or NULL */, int64_t ldOut, double fill, double *out,
                           uint64_t *finMask, int32_t *prefix, int64_t *pairsWalked /* or NULL */);
/* One level's items of maple_update_partials / maple_tree_rebuild_lists on explicit lists, by the library's own host function and
 * fused kernels (maple_amd/csrc/update.hip: one wavefront per item up to the tuning's wavePerItemMax, one lane per item above it).
 * Item i: mergeVectors(l1, b1, t1, l2, b2, t2, upDown), then by mode[i] -- 0: shorten(), then areVectorsDifferent(new, old);
 * 1: shorten(); 2: areVectorsDifferent(old, new) and shorten() only if they differ.  old[i] = -1: nothing to compare with.
 * outList[i]: the new list (-1: the merge is None, or mode 2 and not different); outNone[i] = 1 if the merge is None; outDiff[i]:
 * the verdict (1 where none was asked). */
int maple_debug_update_items(maple_ctx *ctx, int32_t n, const int32_t *l1, const double *b1, const uint8_t *t1, const int32_t *l2,
                             const double *b2, const uint8_t *t2, const uint8_t *upDown, const uint8_t *mode, const int32_t *old,
                             int32_t *outList, uint8_t *outNone, uint8_t *outDiff);
/* One chunk's estimates of maple_tree_optimize_blens on explicit items, by the library's own host function and fused kernels
 * (maple_amd/csrc/blen_sweep.hip: one wavefront per item up to the tuning's wavePerItemMax, default 1 024 items, one lane per item
 * above it).  Item i: estimateBranchLengthWithDerivative(upList[i] passed downwards through mutList[i] (-1: no mutation list),
 * lowList[i], fromTipC = tip[i]): t[i] the length, isFalse[i] = 1 where the reference returns False.  The pass goes to scratch:
 * no list is made.  An id that is no list / no mutation list is MAPLE_ERR_ARG before anything is launched. */
int maple_debug_sweep_estimate(maple_ctx *ctx, int32_t n, const int32_t *upList, const int32_t *mutList, const int32_t *lowList,
                               const uint8_t *tip, double *t, uint8_t *isFalse);
/* The arms the last maple_update_partials of this context took (maple_amd/csrc/update_plan.h, UPDATE_PLAN_STATS): *n counters, the
 * first min(*n, cap) written; maple_debug_update_partials_stat_names gives their names in the same order, each followed by a blank. */
int maple_debug_update_partials_stats(maple_ctx *ctx, int64_t *counts, int32_t cap, int32_t *n);
const char *maple_debug_update_partials_stat_names(void);
/* The nodes that call visited, with repeats, in the order of the visits: the changed nodes, every node that entered a level of the
 * repair, the nodes whose length was estimated again and their parents -- the ones the reference's updatePartials sets `dirty` for,
 * and what maple_tree_optimize_blens takes them from.  *n nodes; more than cap is an error. */
int maple_debug_update_partials_visited(maple_ctx *ctx, int32_t cap, int32_t *nodes, int32_t *n);

#ifdef __cplusplus
}
#endif
#endif
