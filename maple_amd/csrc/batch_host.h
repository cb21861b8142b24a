// maple_amd/csrc/batch_host.h -- the small host-side helpers every translation unit with batch entry points shares (each gets its
// own copy: they only touch the context): launch geometry, list-id checks, the staging arena for a call's arguments, event pairs;
// the launch attributes the scoring kernels share; and the declarations of the host functions that cross translation units
// (hidden visibility: not part of the C ABI).  The dispatch over the three model switches, DISPATCH3, is in ctx_host.h.
// Included by every unit with batch entry points: maple_hip.hip, append_queries.hip, placement.hip, update.hip, spr_batch.hip,
// debug_abi.hip, blen_sweep.hip, em.hip, tree_lk.hip, root_search.hip, error_probs.hip, mat_events.hip.
#pragma once
#include "ctx_host.h"

#include <algorithm>
#include <cstring>
#include <vector>

// the best (score, earliest visit rank, column) of one query over one tile of candidates: k_append_queries* / k_argmax_reduce
struct alignas(16) TileBest { double score; int32_t rank, idx; };

#ifndef MAPLE_BLOCK
#define MAPLE_BLOCK 256
#endif
// the appendProbNode kernels (k_append*, k_place_score, k_pe_level, k_ahead_cols): 120 VGPRs / no scratch at 4 waves per SIMD
// measured fastest (5 waves spills, 3 waves loses latency hiding)
#ifndef MAPLE_APPEND_WAVES
#define MAPLE_APPEND_WAVES 4
#endif
#define MAPLE_APPEND_ATTR __launch_bounds__(MAPLE_BLOCK) __attribute__((amdgpu_waves_per_eu(MAPLE_APPEND_WAVES, MAPLE_APPEND_WAVES)))
#ifndef MAPLE_ZERO_DIST_BUDGET
#define MAPLE_ZERO_DIST_BUDGET 16      // traversal placements a search from a zero-length branch gets before the dense tier
#endif

static int grid_for(int n)
{
    int g = (n + MAPLE_BLOCK - 1) / MAPLE_BLOCK;
    if (g < 1) g = 1;
    if (g > 256 * 8) g = 256 * 8;      // 256 CUs x 8 workgroups, grid-stride beyond
    return g;
}


static int check_ids(maple_ctx *c, int32_t n, const int32_t *ids, bool allowNeg, const char *what)
{
    const int32_t nl = (int32_t)c->h_n_ent.size();
    for (int i = 0; i < n; i++)
        if (ids[i] >= nl || (ids[i] < 0 && !allowNeg))
            return fail(c, MAPLE_ERR_ARG, "%s[%d] = %d is not a list id (have %d)", what, i, ids[i], nl);
    return MAPLE_OK;
}

static inline int ev_pair(maple_ctx *c, hipEvent_t *a, hipEvent_t *b, int kind = 0, double units = 0.0, double bytes = 0.0,
                          size_t *slot = nullptr)
{
    return maple_internal_ev_pair(c, a, b, kind, units, bytes, slot);
}

template <class T> static int h2d(maple_ctx *c, DevBuf<T> &b, const T *src, size_t n)
{
    HIPCK(c, b.reserve(n ? n : 1));
    if (n) HIPCK(c, hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return MAPLE_OK;
}

// Start staging the arguments of one batch call (at most `bytes` of them).  The two arenas alternate from call to call:
// every batch operator synchronises its stream at least once after its first stage_flush, so by the time an arena comes
// round again every copy out of it -- including a trailing asynchronous one -- has completed.
static int stage_begin(maple_ctx *c, size_t bytes)
{
    c->stg_cur ^= 1;
    const int k = c->stg_cur;
    bytes += 4096;
    if (bytes > c->stg_d[k].cap) {
        HIPCK(c, hipStreamSynchronize(c->stream));
        c->stg_h[k].release(); c->stg_d[k].release();
        const size_t want = std::max(bytes * 2, (size_t)1 << 20);
        HIPCK(c, c->stg_h[k].reserve_exact(want));
        HIPCK(c, c->stg_d[k].reserve_exact(want));
    }
    c->stg_used = c->stg_flushed = 0;
    return MAPLE_OK;
}
// n items of `src` into the staging arena; returns where they will be on the device after stage_flush (null if out of room:
// stage_begin was given too small a bound)
template <class T> static T *stage_put(maple_ctx *c, const T *src, size_t n)
{
    const int k = c->stg_cur;
    const size_t off = (c->stg_used + 15) & ~(size_t)15, bytes = n * sizeof(T);
    if (off + bytes > c->stg_d[k].cap) return nullptr;
    if (bytes) memcpy(c->stg_h[k] + off, src, bytes);
    c->stg_used = off + bytes;
    return (T *)(c->stg_d[k] + off);
}
static int stage_flush(maple_ctx *c)
{
    const int k = c->stg_cur;
    if (c->stg_used > c->stg_flushed)
        HIPCK(c, hipMemcpyAsync(c->stg_d[k] + c->stg_flushed, c->stg_h[k] + c->stg_flushed, c->stg_used - c->stg_flushed,
                                hipMemcpyHostToDevice, c->stream));
    c->stg_flushed = c->stg_used;
    return MAPLE_OK;
}
#define STAGE(var, c, src, n) auto *var = stage_put((c), (src), (size_t)(n)); if (!var) return fail((c), MAPLE_ERR_NOMEM, "argument staging overflow")

static int need_model(maple_ctx *c)
{
    if (!c->model_set) return fail(c, MAPLE_ERR_STATE, "maple_set_model has not been called");
    return MAPLE_OK;
}

// An arena mark (maple_arena_mark) whose lists go on every path out of its scope: release() where the call is done with them
// and their release may fail the call, the destructor on the paths that return before that.
struct MarkGuard {
    maple_ctx *c; int64_t mark = 0; bool on = false;
    int take() { const int rc = maple_arena_mark(c, &mark); on = rc == MAPLE_OK; return rc; }
    int release() { if (!on) return MAPLE_OK; on = false; return maple_arena_release(c, mark); }
    ~MarkGuard() { if (on) (void)maple_arena_release(c, mark); }
};


// ---- defined in maple_hip.hip ---------------------------------------------------------------------------------------------
// scratch lists into the arena, ids handed out (-1 for None): see the definition
__attribute__((visibility("hidden")))
int commit_lists(maple_ctx *c, int32_t n, const int64_t *d_woff, const int64_t *d_aoff, int32_t *d_n_ent, int32_t *d_n_aux,
                 int32_t *outList, const uint2 *srcW = nullptr, const double *srcA = nullptr);
// ... with the sizes already on the host
__attribute__((visibility("hidden")))
int commit_known(maple_ctx *c, int32_t n, const int64_t *d_woff, const int64_t *d_aoff, const int32_t *d_n_ent, const int32_t *d_n_aux,
                 const std::vector<int32_t> &ne, const std::vector<int32_t> &na, int32_t *outList, const uint2 *srcW, const double *srcA);
// lists committed on the library's stream are not yet visible to work on another stream: wait once
__attribute__((visibility("hidden")))
int settle(maple_ctx *c);
static int need_tree_and_model(maple_ctx *c)
{
    if (!c->tree_set) return fail(c, MAPLE_ERR_STATE, "maple_tree_upload has not been called");
    return need_model(c);
}
// what every call over the uploaded tree begins with (a call with refusals of its own that touch nothing checks
// need_tree_and_model, refuses, and then begins)
static int begin_tree_call(maple_ctx *c)
{
    TRY(need_tree_and_model(c));
    HIPCK(c, hipSetDevice(c->device));
    ahead_quiesce(c);                                                    // (the rows made ahead stay as they are)
    return settle(c);
}
// evaluatePlacement for n items (maple_evaluate_placement_batch; comp2 optional, 2 doubles per item: see k_evalplace)
__attribute__((visibility("hidden")))
int evaluate_placement_items(maple_ctx *c, int32_t n, const int32_t *midTot, const int32_t *down, const int32_t *up, const double *dist,
                             const int32_t *rem, const uint8_t *remTip, const uint8_t *fromTip1, double *out4, double *comp2);
// k_wave_append (one wavefront per pair) on the context's stream, `grid` workgroups
__attribute__((visibility("hidden")))
void launch_wave_append(maple_ctx *c, int grid, int n, const int32_t *pl, const int32_t *cl, const uint8_t *tip, const double *bl, double *out);
// ---- defined in append_queries.hip -----------------------------------------------------------------------------------------
// one launch of the queries x candidates scoring kernel on stream s (k_append_queries / k_append_queries_lds)
__attribute__((visibility("hidden")))
int launch_append_queries(maple_ctx *c, hipStream_t s, int nQ, const int32_t *qList, int nC, const int32_t *cand, int isTip, double bLen,
                          double *out, long long ldOut, const int32_t *outCol, const uint8_t *qTip, const double *qBLen, int kind,
                          double algBytes, TileBest *tileBest = nullptr, const int32_t *visitRank = nullptr, const int4 *chunkTab = nullptr,
                          int nChunkTab = 0, int nF = 1, unsigned long long *finMask = nullptr, bool lanesOnly = false);
// ---- defined in placement.hip ----------------------------------------------------------------------------------------------
// one launch of the placement phase's scoring kernel (k_place_score) on the context's stream
__attribute__((visibility("hidden")))
int launch_place_score(maple_ctx *c, int nQ, int nF, const int32_t *qFrameLists, int nC, const int32_t *cand, const int32_t *candFrame,
                       int isTip, double bLen, double *out, long long ldOut, const int32_t *outCol, const uint8_t *qTip, const double *qBLen,
                       int kind = MAPLE_K_PLACE_SCORE, double algBytes = 0.0);
// ---- defined in update.hip (both are lists of update_plan::Scratch: update_plan.h holds the level loops that fill them) -----
// the nodes the last maple_update_partials visited, with repeats (the reference's updatePartials sets `dirty` for them)
__attribute__((visibility("hidden")))
const std::vector<int32_t> &update_partials_visited(maple_ctx *c);
// the list behind maple_update_partials_touched (a caller that repairs in several calls stores the union here)
__attribute__((visibility("hidden")))
std::vector<int32_t> &update_partials_replaced(maple_ctx *c);
// from now on maple_update_partials leaves the root's probVectUpRight as it is where only the root's child 1 changed (update_plan.h,
// Scratch::keepRootRight): the sweep's repair of the root's second child; the caller switches it off again
__attribute__((visibility("hidden")))
void update_partials_keep_root_right(maple_ctx *c, bool keep);
// the counters of the last maple_update_partials (update_plan::Stats, in the order of UPDATE_PLAN_STATS): writes the first
// min(cap, their number) and returns their number
__attribute__((visibility("hidden")))
int update_partials_stats(maple_ctx *c, int32_t cap, int64_t *counts);
// one level's items of the repair (the fused kernels k_update_items / k_update_items_wave): see update.hip
__attribute__((visibility("hidden")))
int update_items(maple_ctx *c, int32_t n, const int32_t *l1, const double *b1, const uint8_t *t1, const int32_t *l2, const double *b2,
                 const uint8_t *t2, const uint8_t *ud, const uint8_t *mode, const int32_t *old, int32_t *outList, uint8_t *outNone,
                 uint8_t *outDiff);
// ---- defined in blen_sweep.hip ---------------------------------------------------------------------------------------------
// the estimates of one chunk of the branch-length sweep (the fused kernels k_sweep_estimate / k_sweep_estimate_wave); t and isFalse
// must hold chunk.size() elements.  sweep_plan::SweepItem: sweep_plan.h
namespace sweep_plan { struct SweepItem; }
__attribute__((visibility("hidden")))
int sweep_estimate(maple_ctx *c, const std::vector<sweep_plan::SweepItem> &chunk, std::vector<double> &t, std::vector<uint8_t> &isFalse);
// ---- defined in spr_batch.hip ----------------------------------------------------------------------------------------------
// the device tree once more from the host copy of its columns (after maple_tree_patch left tables stale)
__attribute__((visibility("hidden")))
int tree_rebuild_from_host(maple_ctx *c);
// k_finite_prefix on stream st: prefix[row * (nWords + 1) + w] = the finite scores of the row before word w of its bitmap
// mask[row * nWords ..], prefix[.. + nWords] = the row's total (FiniteRows, search_dev.h)
__attribute__((visibility("hidden")))
int launch_finite_prefix(maple_ctx *c, hipStream_t st, size_t rows, int nWords, const unsigned long long *mask, int32_t *prefix);
