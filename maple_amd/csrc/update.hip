// maple_amd/csrc/update.hip -- updatePartials (MAPLEv0.7.5.4.py:5479-5815) for a set of local changes, level by level.
//
// The lists invalidated by ANY number of simultaneous changes are repaired level by level, every level a handful of batched
// launches, on the host side of the library and on the caller's own tree arrays (plain int32 / double columns, updated in
// place): no Python in the loop.  The level loops themselves -- which node enters which level, the stop rule, the zero-length
// branches, the rounds -- are pure host code in update_plan.h (tested on the CPU: tests/test_update_plan.py); this unit holds
// the fused kernel of a level's items and plugs it and the batch entry points of maple_hip.hip into that plan, for the repair
// (maple_update_partials) and for the list rebuild (maple_tree_rebuild_lists).  A translation unit of libmaple_hip.so (gfx950 only).
#include "../../include/maple_hip.h"
#include "genome_dev.h"
#include "wave_dev.h"
#include "wave_update.h"
#include "ctx_host.h"
#include "batch_host.h"
#include "update_plan.h"

#include <algorithm>
#include <cstring>
#include <vector>

// One item of a level of updatePartials (below): mergeVectors, then what the reference does with the result, in
// one go -- no trip to the host between the three.  mode 0 (a lower list, M:5760-5800): shorten(), then
// areVectorsDifferent(new, old); mode 1 (probVectTotUp, M:5525-5557): shorten(); mode 2 (probVectUpRight / UpLeft,
// M:5559-5660): areVectorsDifferent(old, new), and shorten() only if they differ.  The merged list goes to scratch slot A,
// the shortened one to slot B (what is committed).  n_ent: entries of B, -1 = None, < -1 = fatal; flag: "different".
#define MAPLE_UPDATE_ITEM_ARGS                                                                                                  \
    const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *l1, const double *b1, const uint8_t *t1,               \
        const int32_t *l2, const double *b2, const uint8_t *t2, const uint8_t *ud, const uint8_t *mode, const int32_t *old,     \
        uint2 *words, double *aux, const int64_t *woff, const int64_t *cap, int32_t *res3

template <bool RV, bool U, bool SS>
__device__ inline void update_item_lane(const Ctx<RV, U, SS> &c, const ArenaView &av, int n, int i, const int32_t *l1, const double *b1,
                                        const uint8_t *t1, const int32_t *l2, const double *b2, const uint8_t *t2, const uint8_t *ud,
                                        const uint8_t *mode, const int32_t *old, uint2 *words, double *aux, const int64_t *woff,
                                        const int64_t *cap, int32_t *res3)
{
    Writer wa, wb;
    wa.init(words + woff[i], aux + 5 * woff[i]);
    wb.init(words + woff[i] + cap[i], aux + 5 * (woff[i] + cap[i]));
    double lk = 0.0;
    const int r = merge_walk(c, list_ref(av, l1[i]), b1[i], t1[i] != 0, list_ref(av, l2[i]), b2[i], t2[i] != 0, ud[i] != 0, false, 0,
                             0, wa, &lk);
    int ne = r, na = 0, flag = 1;
    if (r >= 0) {
        const ListRef A{wa.w, wa.aux};
        if (mode[i] == 2 && old[i] >= 0) flag = differ_walk(c, list_ref(av, old[i]), A) ? 1 : 0;
        if (flag) {
            ne = shorten_walk(c, A, r, wb);
            na = wb.na;
            if (mode[i] == 0 && old[i] >= 0) flag = differ_walk(c, ListRef{wb.w, wb.aux}, list_ref(av, old[i])) ? 1 : 0;
        } else ne = 0;
    }
    res3[i] = ne; res3[n + i] = na; res3[2 * n + i] = flag;
}

template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(MAPLE_BLOCK) void k_update_items(MAPLE_UPDATE_ITEM_ARGS)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        update_item_lane(c, av, n, i, l1, b1, t1, l2, b2, t2, ud, mode, old, words, aux, woff, cap, res3);
}

// The same item by a whole wavefront (wave_update.h): what a level with a handful of items -- a single change walking up
// and down the tree -- waits for is one item's latency, not throughput.  One wavefront per workgroup, one item at a time;
// lists too long for the staged walk go through the one-lane code on lane 0.
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(64) void k_update_items_wave(MAPLE_UPDATE_ITEM_ARGS)
{
    __shared__ Lds lds;
    __shared__ WaveUpdLdsStd L;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    const int lane = threadIdx.x;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int id1 = l1[i], id2 = l2[i], idOld = old[i];
        const int n1 = av.n_ent[id1], n2 = av.n_ent[id2], nOld = idOld >= 0 ? av.n_ent[idOld] : 0;
        if (n1 > L.wuIn || n2 > L.wuIn || nOld > L.cap) {
            if (lane == 0) update_item_lane(c, av, n, i, l1, b1, t1, l2, b2, t2, ud, mode, old, words, aux, woff, cap, res3);
            continue;
        }
        wave_sync();                                                       // the item before is done with the LDS
        const ListRef Lo = idOld >= 0 ? list_ref(av, idOld) : ListRef{nullptr, nullptr};
        if (idOld >= 0) {
            const unsigned long long *wo = (const unsigned long long *)Lo.w;
            for (int k = lane; k < nOld; k += 64) L.old[k] = wo[k];
        }
        int naA = 0;
        const int r = wave_merge(c, list_ref(av, id1), n1, b1[i], t1[i] != 0, list_ref(av, id2), n2, b2[i], t2[i] != 0, ud[i] != 0, L, naA);
        int ne = r, na = 0, flag = 1;
        if (r >= 0) {
            const int md = mode[i];
            if (md == 2 && idOld >= 0) flag = wave_differ(c, L.old, Lo.aux, nOld, L.m, L.maux, r) ? 1 : 0;
            if (flag) {
                ne = wave_shorten(c, L, r, words + woff[i] + cap[i], aux + 5 * (woff[i] + cap[i]), na);
                if (md == 0 && idOld >= 0) flag = wave_differ(c, L.in, L.baux, ne, L.old, Lo.aux, nOld) ? 1 : 0;
            } else ne = 0;
        }
        if (lane == 0) { res3[i] = ne; res3[n + i] = na; res3[2 * n + i] = flag; }
    }
}

namespace {

struct UpdateScratch : ScratchBase, update_plan::Scratch {};   // per-context, persistent: the plan's per-node flags and node lists

}  // namespace

static UpdateScratch &update_scratch(maple_ctx *c)
{
    if (!c->upd) c->upd.reset(new UpdateScratch());
    return *static_cast<UpdateScratch *>(c->upd.get());
}

// One level's worth of items through k_update_items: merge, then shorten / compare as the item's mode says (see the
// kernel).  outList[i]: the new list (-1: None from the merge, or mode 2 and not different: nothing to replace);
// outNone[i] = 1 if the merge itself came out None; outDiff[i] = the areVectorsDifferent verdict (1 where none was asked).
// (batch_host.h: maple_debug_update_items of the debug library runs it on the caller's own lists)
int update_items(maple_ctx *c, int32_t n, const int32_t *l1, const double *b1, const uint8_t *t1, const int32_t *l2,
                        const double *b2, const uint8_t *t2, const uint8_t *ud, const uint8_t *mode, const int32_t *old,
                        int32_t *outList, uint8_t *outNone, uint8_t *outDiff)
{
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(check_ids(c, n, l1, false, "list1"));
    TRY(check_ids(c, n, l2, false, "list2"));
    TRY(check_ids(c, n, old, true, "old list"));
    std::vector<int64_t> woff(n), cap(n), woffB(n), aoffB(n);
    int64_t tot = 0;
    for (int i = 0; i < n; i++) {
        cap[i] = (int64_t)c->h_n_ent[l1[i]] + c->h_n_ent[l2[i]];
        woff[i] = tot; woffB[i] = tot + cap[i]; aoffB[i] = 5 * woffB[i];
        tot += 2 * cap[i];
    }
    HIPCK(c, c->s_words.reserve((size_t)tot));
    HIPCK(c, c->s_aux.reserve((size_t)(5 * tot)));
    TRY(stage_begin(c, (size_t)n * 128 + 1024));
    STAGE(dl1, c, l1, n); STAGE(dl2, c, l2, n); STAGE(db1, c, b1, n); STAGE(db2, c, b2, n);
    STAGE(dt1, c, t1, n); STAGE(dt2, c, t2, n); STAGE(dud, c, ud, n); STAGE(dmode, c, mode, n); STAGE(dold, c, old, n);
    STAGE(dwo, c, woff.data(), n); STAGE(dcap, c, cap.data(), n); STAGE(dwoB, c, woffB.data(), n); STAGE(daoB, c, aoffB.data(), n);
    TRY(stage_flush(c));
    HIPCK(c, c->s_i32[2].reserve((size_t)3 * n));
    int32_t *res3 = c->s_i32[2].p;
    // a level with few items waits for ONE item's latency: a wavefront per item (wave_update.h); many items: a lane each
    if (n <= wave_item_max(c, 4096))
        DISPATCH3(c, k_update_items_wave, <<<n, 64, 0, c->stream>>>(c->d_model, view(c), n, dl1, db1, dt1, dl2, db2, dt2, dud, dmode, dold,
                                                                     c->s_words.p, c->s_aux.p, dwo, dcap, res3));
    else
        DISPATCH3(c, k_update_items, <<<grid_for(n), MAPLE_BLOCK, 0, c->stream>>>(c->d_model, view(c), n, dl1, db1, dt1, dl2, db2, dt2, dud,
                                                                                    dmode, dold, c->s_words.p, c->s_aux.p, dwo, dcap, res3));
    HIPCK(c, hipGetLastError());
    HIPCK(c, c->pin_res.reserve((size_t)3 * n * sizeof(int32_t)));
    const int32_t *h3 = (const int32_t *)c->pin_res.p;
    HIPCK(c, hipMemcpyAsync(c->pin_res.p, res3, (size_t)3 * n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    std::vector<int32_t> ne(n), na(n);
    for (int i = 0; i < n; i++) {
        const int r = h3[i], flag = h3[(size_t)2 * n + i];
        outNone[i] = r == -1;
        outDiff[i] = (uint8_t)(flag != 0);
        ne[i] = (r >= 0 && !flag && mode[i] == 2) ? -1 : r;                // mode 2 and not different: nothing to commit
        na[i] = h3[(size_t)n + i];
    }
    return commit_known(c, n, dwoB, daoB, res3, res3 + n, ne, na, outList, nullptr, nullptr);
}

// the operations of update_plan.h on the device: the batch entry points of maple_hip.hip and update_items above
struct UpdateOps {
    maple_ctx *c;
    std::vector<uint8_t> dir;
    int pass(int32_t n, const int32_t *lists, const int32_t *mutLists, bool dirUp, int32_t *out)
    {
        dir.assign((size_t)n, dirUp ? 1 : 0);
        return maple_pass_branch_batch(c, n, lists, mutLists, dir.data(), out);
    }
    int items(update_plan::Batch &B, size_t i, size_t n)
    {
        return update_items(c, (int32_t)n, B.l1.data() + i, B.b1.data() + i, B.t1.data() + i, B.l2.data() + i, B.b2.data() + i, B.t2.data() + i,
                            B.ud.data() + i, B.mode.data() + i, B.old.data() + i, B.out.data() + i, B.none.data() + i, B.diff.data() + i);
    }
    int blen(int32_t upList, int32_t lowList, uint8_t tip, double *t, uint8_t *isFalse) { return maple_blen_batch(c, 1, &upList, &lowList, &tip, t, isFalse); }
    int rootVector(int32_t n, const int32_t *lists, const double *bLen, const uint8_t *tip, int32_t rootMut, int32_t *out)   // (n <= 2)
    {
        const int np = rootMut >= 0 ? 1 : 0;
        const int64_t pathOff[3] = {0, np, 2 * np};
        const int32_t pathMut[2] = {rootMut >= 0 ? rootMut : 0, rootMut >= 0 ? rootMut : 0};
        return maple_root_vector_batch(c, n, lists, bLen, tip, pathOff, pathMut, out);
    }
    int differ(int32_t a, int32_t b, uint8_t *different) { return maple_differ_batch(c, 1, &a, &b, different); }
};

// what a driver of update_plan.h returned: an operation's own error code (its message is already set), or the plan's error
static int plan_result(maple_ctx *c, int rc, const update_plan::Error &E)
{
    if (!E.kind) return rc;
    return fail(c, E.kind == update_plan::ERR_ARG ? MAPLE_ERR_ARG : MAPLE_ERR_FATAL, "%s", E.msg);
}

extern "C" int maple_update_partials(maple_ctx *c, int32_t n, int32_t root, const int32_t *up, const int32_t *c0, const int32_t *c1,
                                     const uint8_t *tip, const int32_t *mut, const int32_t *depth, double *dist, int32_t *lower,
                                     int32_t *upRight, int32_t *upLeft, int32_t *totUp, int32_t nChanged, const int32_t *changed,
                                     int32_t *nReplaced)
{
    if (!c || n <= 0 || !up || !c0 || !c1 || !tip || !mut || !depth || !dist || !lower || !upRight || !upLeft || !totUp
        || nChanged < 0 || (nChanged && !changed) || !nReplaced)
        return MAPLE_ERR_ARG;
    if (root < 0 || root >= n) return fail(c, MAPLE_ERR_ARG, "root %d is not a node", root);
    for (int i = 0; i < nChanged; i++)
        if (changed[i] < 0 || changed[i] >= n) return fail(c, MAPLE_ERR_ARG, "changed[%d] = %d is not a node", i, changed[i]);
    TRY(need_model(c));
    const update_plan::Tree T{n, root, up, c0, c1, tip, mut, depth, dist, lower, upRight, upLeft, totUp};
    UpdateOps ops{c};
    update_plan::Error E;
    return plan_result(c, update_plan::repair_drive(T, update_scratch(c), ops, nChanged, changed, c->tuning.verbose != 0, E, nReplaced), E);
}

// (batch_host.h) for the branch-length sweep, which calls maple_update_partials once per changed branch: what the last call
// visited, and the list maple_update_partials_touched reports, which the sweep replaces by the union over its repairs
const std::vector<int32_t> &update_partials_visited(maple_ctx *c) { return update_scratch(c).visitedNodes; }
std::vector<int32_t> &update_partials_replaced(maple_ctx *c) { return update_scratch(c).replacedNodes; }
void update_partials_keep_root_right(maple_ctx *c, bool keep) { update_scratch(c).keepRootRight = keep; }
// the counters of update_plan::Stats of the last maple_update_partials, in the order of UPDATE_PLAN_STATS: the first cap of them
int update_partials_stats(maple_ctx *c, int32_t cap, int64_t *counts)
{
    const update_plan::Stats &st = update_scratch(c).stats;
    const int64_t all[] = {
#define UPDATE_PLAN_STAT_VALUE(name) st.name,
        UPDATE_PLAN_STATS(UPDATE_PLAN_STAT_VALUE)
#undef UPDATE_PLAN_STAT_VALUE
    };
    const int32_t n = (int32_t)(sizeof all / sizeof all[0]);
    for (int32_t k = 0; k < n && k < cap; k++) counts[k] = all[k];
    return n;
}

// the nodes whose lists (or branch length) the last maple_update_partials replaced, each once, ascending: what a caller
// has to tell maple_tree_patch about besides its own tree edit
extern "C" int maple_update_partials_touched(maple_ctx *c, int32_t cap, int32_t *nodes, int32_t *n)
{
    if (!c || cap < 0 || !n || (cap && !nodes)) return MAPLE_ERR_ARG;
    UpdateScratch &S = update_scratch(c);
    std::vector<int32_t> u(S.replacedNodes);
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    *n = (int32_t)u.size();
    if ((int32_t)u.size() > cap) return fail(c, MAPLE_ERR_ARG, "%zu touched nodes do not fit in %d", u.size(), cap);
    for (size_t i = 0; i < u.size(); i++) nodes[i] = u[i];
    return MAPLE_OK;
}

// reCalculateAllGenomeLists (MAPLEv0.7.5.4.py:6013-6347) level by level inside the library: update_plan::rebuild_drive, each level
// ONE fused launch of k_update_items (mergeVectors -> shorten, above) on the caller's own tree columns: no Python in the loop, one
// synchronisation per level (the level's new list ids feed the next one).  bumpLen, badNodes, nBad: see update_plan.h.
extern "C" int maple_tree_rebuild_lists(maple_ctx *c, int32_t n, int32_t root, const int32_t *up, const int32_t *c0, const int32_t *c1,
                                        const uint8_t *tip, const int32_t *mut, double *dist, int32_t *lower, int32_t *upRight,
                                        int32_t *upLeft, int32_t *totUp, double bumpLen, int32_t capBad, int32_t *badNodes, int32_t *nBad)
{
    if (!c || n <= 0 || !up || !c0 || !c1 || !tip || !dist || !lower || !upRight || !upLeft || !totUp) return MAPLE_ERR_ARG;
    if (root < 0 || root >= n) return fail(c, MAPLE_ERR_ARG, "root %d is not a node", root);
    if (bumpLen > 0.0 && (!badNodes || !nBad || capBad < 4)) return MAPLE_ERR_ARG;
    TRY(need_model(c));
    std::vector<int32_t> noMut;
    if (!mut) { noMut.assign((size_t)n, -1); mut = noMut.data(); }
    const update_plan::Tree T{n, root, up, c0, c1, tip, mut, nullptr, dist, lower, upRight, upLeft, totUp};
    UpdateOps ops{c};
    update_plan::Error E;
    return plan_result(c, update_plan::rebuild_drive(T, ops, bumpLen, capBad, badNodes, nBad, E), E);
}
