// maple_amd/csrc/blen_sweep.hip -- traverseTreeToOptimizeBranchLengths (MAPLEv0.7.5.4.py:8727-8893) inside the library:
// maple_tree_optimize_blens.
//
// The reference visits the branches in a fixed LIFO order; at a dirty branch it estimates the length
// (estimateBranchLengthWithDerivative of the parent's upper vector, passed through the branch's MAT mutations where it has
// any, against the node's lower list) and, if the length moves by more than 1 %, repairs the genome lists around the branch at
// once (updatePartials) -- so every later estimate sees every earlier change.  Here the sweep's logic is the pure driver of
// sweep_plan.h; this unit plugs in its two callbacks: the estimates of a chunk of branches in ONE launch (k_sweep_estimate /
// k_sweep_estimate_wave: the pass through the mutation list is fused into the estimate and goes to per-item scratch, so a chunk
// costs no arena mark, commit or release and no second launch), and maple_update_partials (update.hip) as the repair.  The
// caller's columns stay authoritative, as for maple_update_partials.
// A translation unit of libmaple_hip.so (gfx950 only).
#include "../../include/maple_hip.h"
#include "genome_dev.h"
#include "wave_dev.h"
#include "wave_update.h"
#include "ctx_host.h"
#include "batch_host.h"
#include "sweep_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

// One estimate.  item = {upper list, mutation list of the branch or -1, lower list, isTip}.  With a mutation list the upper list
// is first re-expressed in the node's frame (pass_walk, dirIsUp = false) into the item's scratch: woff[i] words in `words`, five
// doubles of aux per word in `aux` (room: entries + 2 x mutations, the bound of maple_pass_branch_batch).  Then the walk of
// maple_blen_batch on the two lists, the same .inc bodies: t and isFalse are those of that call bit for bit.
// ais: aisOff[i] doubles of scratch per item for the one-lane walk (entries of both lists).
#define MAPLE_SWEEP_ARGS                                                                                                            \
    const DevModel *__restrict__ mp, ArenaView av, MutView mv, int n, const int4 *items, uint2 *words, double *aux,                  \
        const int64_t *woff, double *ais, const int64_t *aisOff, double *t, uint8_t *isFalse

#define MAPLE_SWEEP_WAVE_MAX 1024        // chunks up to this size go one wavefront per item (as the explicit-pair operators do)

// one lane per item (the occupancy of k_blen: the block size is the only bound)
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(MAPLE_BLOCK) void k_sweep_estimate(MAPLE_SWEEP_ARGS)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int4 it = items[i];
        ListRef P = list_ref(av, it.x);
        if (it.y >= 0) {
            Writer w;
            w.init(words + woff[i], aux + 5 * woff[i]);
            pass_walk(m.lRef, P, mv.mut3 + 3 * mv.off[it.y], mv.cnt[it.y], false, w);
            P = ListRef{w.w, w.aux};
        }
        bool f;
        t[i] = blen_walk(c, P, list_ref(av, it.z), it.w != 0, ais + aisOff[i], 1, &f);
        isFalse[i] = f ? 1 : 0;
    }
}

// one wavefront per item, as k_blen_wave: the two lists staged in LDS (WaveLdsStd, 8 KB) plus 128 doubles of terms; lists over
// capW entries go through the one-lane walk on lane 0.  The pass through a mutation list is one lane's work (lane 0 writes the
// scratch list, the wavefront then stages it like a stored one).
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(64) void k_sweep_estimate_wave(MAPLE_SWEEP_ARGS)
{
    __shared__ Lds lds;
    __shared__ WaveLdsStd W;
    __shared__ double terms[128];
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    const int lane = threadIdx.x;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int4 it = items[i];
        const int idC = it.z;
        const int nC = av.n_ent[idC];
        ListRef P = list_ref(av, it.x);
        int nP = av.n_ent[it.x];
        if (it.y >= 0) {
            uint2 *gw = words + woff[i];
            double *ga = aux + 5 * woff[i];
            int np = 0;
            if (lane == 0) {
                Writer w;
                w.init(gw, ga);
                np = pass_walk(m.lRef, P, mv.mut3 + 3 * mv.off[it.y], mv.cnt[it.y], false, w);
            }
            wave_sync();                                                   // lane 0's list is there for the other lanes
            nP = __builtin_amdgcn_readfirstlane(np);
            P = ListRef{gw, ga};
        }
        bool f = false;
        double v = 0.0;
        if (nP > W.capW || nC > W.capW) {
            if (lane == 0) v = blen_walk(c, P, list_ref(av, idC), it.w != 0, ais + aisOff[i], 1, &f);
        } else {
            wave_sync();                                                   // the item before is done with the LDS
            v = wave_blen(c, P, nP, list_ref(av, idC), nC, it.w != 0, W, terms, &f);
        }
        if (lane == 0) { t[i] = v; isFalse[i] = f ? 1 : 0; }
    }
}

namespace {

struct SweepScratch : ScratchBase {       // per-context: the counters of maple_tree_optimize_blens_stats, the call's host vectors
    int64_t launches = 0, computed = 0, used = 0, repairs = 0, sweeps = 0;
    std::vector<int4> items;
    std::vector<int64_t> woff, aisOff;
};

}  // namespace

static SweepScratch &sweep_scratch(maple_ctx *c)
{
    if (!c->sweep) c->sweep.reset(new SweepScratch());
    return *static_cast<SweepScratch *>(c->sweep.get());
}

// the estimates of one chunk: one launch, one copy back (declared in batch_host.h: maple_debug_sweep_estimate calls it too)
int sweep_estimate(maple_ctx *c, const std::vector<sweep_plan::SweepItem> &chunk, std::vector<double> &t, std::vector<uint8_t> &isFalse)
{
    SweepScratch &S = sweep_scratch(c);
    const int n = (int)chunk.size();
    if (n == 0) return MAPLE_OK;
    const int32_t nl = (int32_t)c->h_n_ent.size(), nml = (int32_t)c->h_mut_cnt.size();
    S.items.resize((size_t)n); S.woff.resize((size_t)n); S.aisOff.resize((size_t)n);
    int64_t totW = 0, totA = 0;
    for (int i = 0; i < n; i++) {
        const sweep_plan::SweepItem &it = chunk[i];
        if (it.upList < 0 || it.upList >= nl) return fail(c, MAPLE_ERR_ARG, "node %d: the upper vector of its parent, %d, is not a list id (have %d)", it.node, it.upList, nl);
        if (it.lowList < 0 || it.lowList >= nl) return fail(c, MAPLE_ERR_ARG, "node %d: lower[] = %d is not a list id (have %d)", it.node, it.lowList, nl);
        if (it.mutList >= nml) return fail(c, MAPLE_ERR_ARG, "node %d: mutList[] = %d is not a mutation-list id (have %d)", it.node, it.mutList, nml);
        S.items[i] = make_int4(it.upList, it.mutList < 0 ? -1 : it.mutList, it.lowList, it.tip ? 1 : 0);
        int64_t nP = c->h_n_ent[it.upList];
        S.woff[i] = totW;
        if (it.mutList >= 0) { nP += 2 * (int64_t)c->h_mut_cnt[it.mutList]; totW += nP; }
        S.aisOff[i] = totA;
        totA += nP + c->h_n_ent[it.lowList];
    }
    HIPCK(c, c->s_words.reserve((size_t)std::max<int64_t>(totW, 1)));
    HIPCK(c, c->s_aux.reserve((size_t)std::max<int64_t>(5 * totW, 1)));
    HIPCK(c, c->s_ais.reserve((size_t)std::max<int64_t>(totA, 1)));
    TRY(stage_begin(c, (size_t)n * 48 + 512));
    STAGE(dit, c, S.items.data(), n); STAGE(dwo, c, S.woff.data(), n); STAGE(dao, c, S.aisOff.data(), n);
    TRY(stage_flush(c));
    HIPCK(c, c->s_f64[0].reserve((size_t)n));
    HIPCK(c, c->s_u8[1].reserve((size_t)n));
    // few items: what the sweep waits for is one item's latency, a wavefront each; many: a lane each (as maple_blen_batch)
    if (n <= wave_item_max(c, MAPLE_SWEEP_WAVE_MAX))
        DISPATCH3(c, k_sweep_estimate_wave, <<<n, 64, 0, c->stream>>>(c->d_model, view(c), mview(c), n, dit, c->s_words.p, c->s_aux.p, dwo,
                                                                      c->s_ais.p, dao, c->s_f64[0].p, c->s_u8[1].p));
    else
        DISPATCH3(c, k_sweep_estimate, <<<grid_for(n), MAPLE_BLOCK, 0, c->stream>>>(c->d_model, view(c), mview(c), n, dit, c->s_words.p,
                                                                                     c->s_aux.p, dwo, c->s_ais.p, dao, c->s_f64[0].p,
                                                                                     c->s_u8[1].p));
    HIPCK(c, hipGetLastError());
    const size_t offF = ((size_t)n * sizeof(double) + 15) & ~(size_t)15;
    HIPCK(c, c->pin_res.reserve(offF + (size_t)n));
    HIPCK(c, hipMemcpyAsync(c->pin_res.p, c->s_f64[0].p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync((char *)c->pin_res.p + offF, c->s_u8[1].p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    memcpy(t.data(), c->pin_res.p, (size_t)n * sizeof(double));
    memcpy(isFalse.data(), (const char *)c->pin_res.p + offF, (size_t)n);
    return MAPLE_OK;
}

// The share of the root's two branches in their total length (M:8746-8784): the grid of half-mutation steps through the
// existing batch operators -- pass, merge with returnLK, pass through mutList[root], root probability -- under an arena mark.
// The first strict maximum wins (M:8780).
static int root_grid(maple_ctx *c, int32_t root, int a, int b, const uint8_t *tip, const int32_t *mut, const double *dist,
                     const int32_t *lower, double *best1)
{
    MarkGuard g{c};
    TRY(g.take());
    const double lRef = (double)c->lRef;
    const double totDist = (dist[a] + dist[b]) * lRef;
    const long long steps = std::max<long long>(1, (long long)std::nearbyint(totDist)) * 2 + 1;   // Python's round(): half to even
    if (steps > (1ll << 24)) return fail(c, MAPLE_ERR_ARG, "the root's two branches are %g substitutions long together", totDist);
    const int k = (int)steps;
    std::vector<double> b1((size_t)k), b2((size_t)k);
    for (int i = 0; i < k; i++) {
        const double l1 = std::min(totDist, (double)i / 2);
        const double l2 = std::max(totDist - l1, 0.0);
        b1[i] = l1 / lRef; b2[i] = l2 / lRef;
    }
    int32_t pv[2] = {lower[a], lower[b]};
    const int kid[2] = {a, b};
    for (int j = 0; j < 2; j++) {
        if (pv[j] < 0) return fail(c, MAPLE_ERR_ARG, "node %d (a child of the root) has no lower list", kid[j]);
        if (mut[kid[j]] >= 0) {
            const uint8_t upDir = 1;
            int32_t out = -1;
            TRY(maple_pass_branch_batch(c, 1, &pv[j], &mut[kid[j]], &upDir, &out));
            pv[j] = out;
        }
    }
    std::vector<int32_t> l1((size_t)k, pv[0]), l2((size_t)k, pv[1]), out((size_t)k, -1);
    std::vector<uint8_t> t1((size_t)k, tip[a]), t2((size_t)k, tip[b]), ud((size_t)k, 0);
    std::vector<double> lk((size_t)k, 0.0), rp((size_t)k, 0.0);
    TRY(maple_merge_batch(c, k, l1.data(), b1.data(), t1.data(), l2.data(), b2.data(), t2.data(), ud.data(), nullptr, nullptr, out.data(), lk.data()));
    for (int i = 0; i < k; i++)
        if (out[i] < 0) return fail(c, MAPLE_ERR_FATAL, "None root vector in the root branch-length grid (the reference fails here too)");
    if (mut[root] >= 0) {
        std::vector<int32_t> ml((size_t)k, mut[root]), passed((size_t)k, -1);
        std::vector<uint8_t> upDir((size_t)k, 1);
        TRY(maple_pass_branch_batch(c, k, out.data(), ml.data(), upDir.data(), passed.data()));
        out.swap(passed);
    }
    TRY(maple_root_prob_batch(c, k, out.data(), rp.data()));
    double bestCost = -INFINITY;
    bool have = false;
    for (int i = 0; i < k; i++) {
        const double cost = lk[i] + rp[i];
        if (cost > bestCost) { bestCost = cost; *best1 = b1[i]; have = true; }
    }
    TRY(g.release());
    if (!have) return fail(c, MAPLE_ERR_FATAL, "no finite likelihood in the root branch-length grid (the reference fails here too)");
    return MAPLE_OK;
}

extern "C" int maple_tree_optimize_blens(maple_ctx *c, int32_t n, int32_t root, const int32_t *up, const int32_t *c0, const int32_t *c1,
                                         const uint8_t *tip, const int32_t *mut, const int32_t *depth, double *dist, int32_t *lower,
                                         int32_t *upRight, int32_t *upLeft, int32_t *totUp, uint8_t *dirty,
                                         const maple_blen_sweep_params *params, int32_t *nUpdates, int32_t capOrder, int32_t *order,
                                         int32_t *nOrder)
{
    if (!c || n <= 0 || !up || !c0 || !c1 || !tip || !mut || !depth || !dist || !lower || !upRight || !upLeft || !totUp || !dirty
        || !params || !nUpdates || !nOrder || capOrder < 0 || (capOrder && !order))
        return MAPLE_ERR_ARG;
    if (params->structSize < sizeof(uint32_t))
        return fail(c, MAPLE_ERR_ARG, "maple_tree_optimize_blens: structSize is not set (sizeof(maple_blen_sweep_params) of the caller's header)");
    maple_blen_sweep_params P{};                                          // (what the caller's struct does not reach: 0)
    memcpy(&P, params, std::min<size_t>(params->structSize, sizeof(P)));
    if (P.chunk < 0) return fail(c, MAPLE_ERR_ARG, "maple_tree_optimize_blens: chunk %d", P.chunk);
    if (root < 0 || root >= n) return fail(c, MAPLE_ERR_ARG, "root %d is not a node", root);
    TRY(need_model(c));
    HIPCK(c, hipSetDevice(c->device));
    *nUpdates = 0;
    *nOrder = 0;
    std::vector<int32_t> visit, pos;
    if (!sweep_plan::sweep_order(n, root, c0, c1, visit, pos))
        return fail(c, MAPLE_ERR_ARG, "the children columns below root %d are no tree (an index out of range, one child only, or a node reached twice)", root);
    SweepScratch &S = sweep_scratch(c);
    std::vector<int32_t> &touchedOut = update_partials_replaced(c);
    S.sweeps++;
    if (c0[root] < 0) { touchedOut.clear(); return MAPLE_OK; }
    const int a = c0[root], b = c1[root];
    if (up[a] != root || up[b] != root) return fail(c, MAPLE_ERR_ARG, "a child of root %d does not point back to it", root);
    for (int v : visit) {
        const int p = up[v];
        if (p < 0 || p >= n || (c0[p] != v && c1[p] != v)) return fail(c, MAPLE_ERR_ARG, "node %d is a child of another node than its `up` entry %d", v, p);
    }
    const bool fast = P.fastPass != 0;
    std::vector<int32_t> handed, touched;     // nodes handed to a repair (fastPass: whose length changed) in order; the union of the repairs' touched nodes
    auto repair = [&](int v, std::vector<int32_t> &visited) -> int {
        int32_t nrep = 0;
        const int32_t one = v;
        const int rc = maple_update_partials(c, n, root, up, c0, c1, tip, mut, depth, dist, lower, upRight, upLeft, totUp, 1, &one, &nrep);
        const std::vector<int32_t> &vis = update_partials_visited(c);
        visited.insert(visited.end(), vis.begin(), vis.end());
        touched.insert(touched.end(), touchedOut.begin(), touchedOut.end());
        touched.push_back(v);
        return rc;
    };
    auto finish = [&](int rc) {
        touchedOut = touched;                 // maple_update_partials_touched: the union over the whole sweep
        *nOrder = (int32_t)handed.size();
        for (size_t i = 0; i < handed.size() && (int32_t)i < capOrder; i++) order[i] = handed[i];
        return rc;
    };
    // ---- the root's two branches ------------------------------------------------------------------------------------------------
    if (dist[a] > P.effectivelyNon0BLen || dist[b] > P.effectivelyNon0BLen) {
        double best1 = 0.0;
        const int rcGrid = root_grid(c, root, a, b, tip, mut, dist, lower, &best1);
        if (rcGrid) return finish(rcGrid);
        const double best2 = std::max(dist[a] + dist[b] - best1, 0.0);
        const int kid[2] = {a, b};
        const double len[2] = {best1, best2};
        std::vector<int32_t> visited;
        for (int j = 0; j < 2; j++) {
            const bool moved = dist[kid[j]] != len[j];
            dist[kid[j]] = len[j];
            if (fast) { if (moved) { handed.push_back(kid[j]); touched.push_back(kid[j]); } continue; }
            // (whether or not the length moved: the reference repairs, and the repair sets `dirty`)
            handed.push_back(kid[j]);
            visited.clear();
            // (the reference's work list is [(child, 2), (root, 0)] for BOTH children, M:8790 / 8796: after the second child's
            // repair the root's probVectUpRight, which depends on that child's length, is the one made with its old length)
            update_partials_keep_root_right(c, j == 1);
            const int rc = repair(kid[j], visited);
            update_partials_keep_root_right(c, false);
            S.repairs++;
            for (int w : visited) if (w >= 0 && w < n) dirty[w] = 1;
            if (rc) return finish(rc);
        }
    }
    // ---- every other branch -----------------------------------------------------------------------------------------------------
    const sweep_plan::SweepTree T{n, up, c0, mut, tip, dist, lower, upRight, upLeft, dirty};
    sweep_plan::SweepStats st;
    std::vector<int32_t> updated;
    const int rc = sweep_plan::sweep_drive(
        T, visit, pos, fast, P.chunk,
        [&](const std::vector<sweep_plan::SweepItem> &items, std::vector<double> &t, std::vector<uint8_t> &isFalse) {
            return sweep_estimate(c, items, t, isFalse);
        },
        repair, nUpdates, updated, st);
    S.launches += st.launches; S.computed += st.computed; S.used += st.used; S.repairs += st.repairs;
    handed.insert(handed.end(), updated.begin(), updated.end());
    if (fast) touched.insert(touched.end(), updated.begin(), updated.end());
    return finish(rc);
}

extern "C" int maple_tree_optimize_blens_stats(maple_ctx *c, int64_t *out5)
{
    if (!c || !out5) return MAPLE_ERR_ARG;
    const SweepScratch &S = sweep_scratch(c);
    out5[0] = S.launches; out5[1] = S.computed; out5[2] = S.used; out5[3] = S.repairs; out5[4] = S.sweeps;
    return MAPLE_OK;
}
