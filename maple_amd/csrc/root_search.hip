// maple_amd/csrc/root_search.hip -- the search of findBestRoot (MAPLEv0.7.5.4.py:7730-7848, without time trees and HnZ) inside the
// library: maple_tree_find_best_root.
//
// The score of re-rooting on a branch depends only on the path from the current root to it, so the scores of ALL branches are made
// level by level (root_search_plan.h: the internal nodes below the root, grouped by depth) and the reference's depth-first
// traversal with its stop rules is replayed over them on the host (root_search_plan::replay) -- what tree_host.find_best_root does
// with five maple_merge_batch(returnLK) launches, the passes through reference branches and one maple_root_prob_batch per level.
// Here a level is three launches on the context's stream and ONE synchronisation (the sizes of the lists to commit):
//   k_root_children  one lane per visited node t1: the merge of its children's lower lists (M:7797) into a CountSink; only the
//                    likelihood contribution is kept;
//   k_root_up        one lane per (t1, side): the merge of the other child's lower list with what t1 was handed from above
//                    (M:7804), written through a Writer into per-item scratch: upVect, the only list of a level that is read again
//                    (the next level is handed it) and the only merged list that is committed to the arena;
//   k_root_new       one lane per (t1, side): the merge of upVect with this child's lower list at half the branch each
//                    (M:7806-7807) into a RootProbSink (genome_dev.h), which runs findProbRoot over the entries as they are made:
//                    newRootProbVect is never stored.
// One lane per item, fp64, the step of merge_step_body.inc unchanged, for k_tree_lk's reason: the likelihood of a merge is an
// ORDERED product over the genome, so there is no wavefront-per-item form.
// MAT local references: findProbRoot(newRootProbVect, node = t1) passes the list up through every mutated branch between t1 and the
// root, so below (or at) a node with a mutation list the sink does not apply: those items write newRootProbVect
// (k_root_new_list), it is committed, passed up one mutated ancestor at a time (maple_pass_branch_batch) and summed by
// maple_root_prob_batch -- the Python path's steps.  Lower lists of children with a mutation list are passed up once per call
// (M:7795); an upVect handed to a child with a mutation list goes down through it and is shortened (M:7844-7845).
// The items carry branch lengths, tip flags and minor-sequence counts by value, taken from the host copy of the tree's columns,
// which maple_tree_patch keeps current: the flat device columns, stale after a patch, are not read.
// A translation unit of libmaple_hip.so (gfx950 only).
#include "batch_host.h"
#include "root_search_plan.h"

#include <cmath>
#include <limits>

// one visited node t1: its children's lower lists, what it was handed from above (list, the distance to it, whether that is a tip,
// its minor sequences), and whether newRootProbVect must be materialised
struct RsItem {
    int32_t l[2], passed, pmin;
    double d[2], dis;
    int32_t nm[2];
    uint8_t tip[2], ptip, mat;
};
// per-slot scratch of the list-writing kernels: slot k writes at words + woff[k] and aux + 5 * woff[k]
struct RsOut {
    uint2 *words;
    double *aux;
    const int64_t *woff;
    int32_t *n_ent, *n_aux;
};

template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(MAPLE_BLOCK) void k_root_children(const DevModel *__restrict__ mp, ArenaView av, int n, const RsItem *items,
                                                               double *outLK)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const RsItem &it = items[i];
        CountSink s;
        double lk = 0.0;
        (void)merge_walk(c, list_ref(av, it.l[0]), it.d[0], it.tip[0] != 0, list_ref(av, it.l[1]), it.d[1], it.tip[1] != 0, false, true,
                         it.nm[0], it.nm[1], s, &lk);
        outLK[i] = lk;
    }
}

// slot k = 2 * item + side: upVect for the child `side`, i.e. the OTHER child's lower list merged with what came from above
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(MAPLE_BLOCK) void k_root_up(const DevModel *__restrict__ mp, ArenaView av, int n2, const RsItem *items, RsOut o,
                                                         double *outLK)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n2; k += gridDim.x * blockDim.x) {
        const RsItem &it = items[k >> 1];
        const int a = 1 - (k & 1);
        Writer w;
        w.init(o.words + o.woff[k], o.aux + 5 * o.woff[k]);
        double lk = 0.0;
        const int r = merge_walk(c, list_ref(av, it.l[a]), it.d[a], it.tip[a] != 0, list_ref(av, it.passed), it.dis, it.ptip != 0, false,
                                 true, it.nm[a], it.pmin, w, &lk);
        o.n_ent[k] = r;
        o.n_aux[k] = w.na;
        outLK[k] = lk;
    }
}

// the new root in the middle of the branch above child `side`.  MATERIALISE = false: every slot of an item without `mat`, the root
// probability through the sink.  MATERIALISE = true: the slots sel[0..n), newRootProbVect written at nw's slot i.
template <bool RV, bool U, bool SS, bool MATERIALISE>
__device__ __forceinline__ void root_new_body(const DevModel *__restrict__ mp, ArenaView av, int n, const RsItem *items, const int32_t *sel,
                                              RsOut up, RsOut nw, int32_t *st, double *outLK, double *outRP)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int k = MATERIALISE ? sel[i] : i;
        const RsItem &it = items[k >> 1];
        if (!MATERIALISE && it.mat) continue;
        const int s = k & 1;
        if (up.n_ent[k] < 0) { st[k] = -1; if (MATERIALISE) { nw.n_aux[i] = 0; } continue; }   // "Stopping root search" (M:7838)
        const ListRef upVect{up.words + up.woff[k], up.aux + 5 * up.woff[k]};
        const double half = it.d[s] / 2;
        double lk = 0.0;
        if (MATERIALISE) {
            Writer w;
            w.init(nw.words + nw.woff[i], nw.aux + 5 * nw.woff[i]);
            st[k] = merge_walk(c, upVect, half, false, list_ref(av, it.l[s]), half, it.tip[s] != 0, false, true, 0, it.nm[s], w, &lk);
            nw.n_aux[i] = w.na;
        } else {
            RootProbSink<RV, U, SS> sink(c);
            st[k] = merge_walk(c, upVect, half, false, list_ref(av, it.l[s]), half, it.tip[s] != 0, false, true, 0, it.nm[s], sink, &lk);
            outRP[k] = sink.value();
        }
        outLK[k] = lk;
    }
}
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(MAPLE_BLOCK) void k_root_new(const DevModel *__restrict__ mp, ArenaView av, int n2, const RsItem *items, RsOut up,
                                                          int32_t *st, double *outLK, double *outRP)
{
    root_new_body<RV, U, SS, false>(mp, av, n2, items, nullptr, up, RsOut{}, st, outLK, outRP);
}
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(MAPLE_BLOCK) void k_root_new_list(const DevModel *__restrict__ mp, ArenaView av, int n, const RsItem *items,
                                                               const int32_t *sel, RsOut up, RsOut nw, int32_t *st, double *outLK)
{
    root_new_body<RV, U, SS, true>(mp, av, n, items, sel, up, nw, st, outLK, nullptr);
}

namespace {

struct RootSearchScratch : ScratchBase {
    // the plan of the tree as it stands (valid while maple_ctx::root_search_valid)
    root_search_plan::Levels lv;
    std::vector<int32_t> nearMut;        // per node with an item, and the root: the nearest node at or above it with a mutation list, -1 = none
    // per call
    std::vector<int32_t> low;            // per node: its lower list as its parent reads it (passed up where it has a mutation list)
    std::vector<int32_t> resUp;          // per (item, side): the list handed to that child's item, -1 = none (abandoned, or a leaf)
    std::vector<double> resRem, score;   // per (item, side): LKtoRemove for that child's item; per node: the default branchScore
    std::vector<uint8_t> matOf;          // per item
    std::vector<RsItem> items;
    std::vector<int64_t> woff;
    std::vector<int32_t> sel;
    DevBuf<RsItem> d_items;
    DevBuf<int64_t> d_woff;
    DevBuf<int32_t> d_sel, d_i32;
    DevBuf<double> d_f64;
    DevBuf<uint2> d_words;
    DevBuf<double> d_aux;
    PinBuf pin;
};

RootSearchScratch &scratch(maple_ctx *c)
{
    if (!c->rootsearch) { c->rootsearch.reset(new RootSearchScratch()); c->root_search_valid = false; }
    return *static_cast<RootSearchScratch *>(c->rootsearch.get());
}

int build_plan(maple_ctx *c, RootSearchScratch &S)
{
    const int32_t n = (int32_t)c->h_tree_up.size(), root = c->dtree.root;
    if (!root_search_plan::level_lists(n, root, c->h_tree_c0.data(), c->h_tree_c1.data(), S.lv))
        return fail(c, MAPLE_ERR_STATE, "the children columns below root %d are no tree", root);
    S.nearMut.assign((size_t)n, -1);
    if (c->h_tree_mut[root] >= 0) S.nearMut[(size_t)root] = root;
    for (const int32_t v : S.lv.node)                                     // (a parent's item comes before its children's)
        S.nearMut[(size_t)v] = c->h_tree_mut[v] >= 0 ? v : S.nearMut[(size_t)c->h_tree_up[v]];
    c->root_search_valid = true;
    return MAPLE_OK;
}

// lists through their mutation lists in one launch (maple_pass_branch_batch), in place
int pass_lists(maple_ctx *c, std::vector<int32_t> &lists, const std::vector<int32_t> &muts, bool up)
{
    if (lists.empty()) return MAPLE_OK;
    const std::vector<uint8_t> dir(lists.size(), up ? 1 : 0);
    std::vector<int32_t> out(lists.size(), -1);
    TRY(maple_pass_branch_batch(c, (int32_t)lists.size(), lists.data(), muts.data(), dir.data(), out.data()));
    for (size_t k = 0; k < out.size(); k++)
        if (out[k] < 0) return fail(c, MAPLE_ERR_FATAL, "a list could not be passed through the mutation list %d", muts[k]);
    lists.swap(out);
    return MAPLE_OK;
}

}  // namespace

extern "C" int maple_tree_find_best_root(maple_ctx *c, const int32_t *nMinor, const maple_root_search_params *params, int32_t *bestNode,
                                         double *bestLKdiff, int32_t *nodesVisited, double *branchScore, int32_t capBest,
                                         int32_t *bestNodes, double *bestScores, int32_t *nBest)
{
    if (!c || !params || !bestNode || !bestLKdiff || !nodesVisited || !nBest || capBest < 0 || (capBest > 0 && (!bestNodes || !bestScores)))
        return MAPLE_ERR_ARG;
    if (params->structSize < sizeof(uint32_t))
        return fail(c, MAPLE_ERR_ARG, "maple_tree_find_best_root: structSize is not set (sizeof(maple_root_search_params) of the caller's header)");
    maple_root_search_params P{};
    memcpy(&P, params, std::min<size_t>(params->structSize, sizeof(P)));
    TRY(begin_tree_call(c));
    RootSearchScratch &S = scratch(c);
    if (!c->root_search_valid) TRY(build_plan(c, S));
    const int32_t n = (int32_t)c->h_tree_up.size(), root = c->dtree.root;
    if (nMinor)
        for (int32_t v = 0; v < n; v++)
            if (nMinor[v] < 0) return fail(c, MAPLE_ERR_ARG, "nMinor[%d] = %d", v, nMinor[v]);
    const root_search_plan::Levels &lv = S.lv;
    const std::vector<int32_t> &C0 = c->h_tree_c0, &C1 = c->h_tree_c1, &MUT = c->h_tree_mut;
    const std::vector<double> &DIST = c->h_tree_dist;
    const std::vector<uint8_t> &TIP = c->h_tree_tip;
    auto nmOf = [&](int32_t v) { return nMinor ? nMinor[v] : 0; };
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double *score = branchScore;
    if (!score) { S.score.resize((size_t)n); score = S.score.data(); }
    for (int32_t v = 0; v < n; v++) score[v] = nan;
    const root_search_plan::Rules rules{P.strictTopologyStopRules != 0, P.allowedFailsTopology, P.thresholdLogLKtopology,
                                        P.thresholdLogLKoptimizationTopology, P.thresholdLogLKconsecutivePlacement};
    auto finish = [&]() {
        root_search_plan::Result R;
        root_search_plan::replay(root, C0.data(), C1.data(), score, rules, R);
        *bestNode = R.bestNode; *bestLKdiff = R.best; *nodesVisited = R.visited;
        *nBest = (int32_t)R.nodes.size();
        for (int32_t k = 0; k < capBest && k < *nBest; k++) { bestNodes[k] = R.nodes[(size_t)k]; bestScores[k] = R.scores[(size_t)k]; }
        return MAPLE_OK;
    };
    const size_t nI = lv.node.size();
    if (nI == 0) return finish();                                        // a root without children, or with two leaves: nothing to score

    // ---- the lower lists as the parents read them (M:7795): every node below the root, passed up where it has a mutation list
    const int32_t nl = (int32_t)c->h_n_ent.size(), nml = (int32_t)c->h_mut_cnt.size();
    S.low.assign((size_t)n, -1);
    std::vector<int32_t> pNode, pList, pMut;
    auto take = [&](int32_t v) -> int {
        const int32_t id = c->h_tree_lower[v], mu = MUT[v];
        if (id < 0 || id >= nl) return fail(c, MAPLE_ERR_STATE, "node %d has no lower list", v);
        if (mu >= nml) return fail(c, MAPLE_ERR_STATE, "node %d: mutList[] = %d is not a mutation-list id (have %d)", v, mu, nml);
        S.low[(size_t)v] = id;
        if (mu >= 0) { pNode.push_back(v); pList.push_back(id); pMut.push_back(mu); }
        return MAPLE_OK;
    };
    const int32_t r1 = C0[root], r2 = C1[root];
    TRY(take(r1)); TRY(take(r2));
    for (size_t k = 0; k < nI; k++) { TRY(take(C0[lv.node[k]])); TRY(take(C1[lv.node[k]])); }
    TRY(take(root));                                                     // (the root's own list through its own mutation list: M:7750)
    MarkGuard guard{c};                // the call's temporaries go on every path
    TRY(guard.take());
    TRY(pass_lists(c, pList, pMut, true));
    for (size_t k = 0; k < pNode.size(); k++) S.low[(size_t)pNode[k]] = pList[k];

    // ---- the root's own terms (M:7749-7778)
    double original = 0.0;
    TRY(maple_root_prob_batch(c, 1, &S.low[(size_t)root], &original));
    {
        RsItem it{};
        it.l[0] = S.low[(size_t)r2]; it.l[1] = S.low[(size_t)r1];
        it.d[0] = DIST[r2]; it.d[1] = DIST[r1];
        it.tip[0] = TIP[r2]; it.tip[1] = TIP[r1];
        it.nm[0] = nmOf(r2); it.nm[1] = nmOf(r1);
        TRY(h2d(c, S.d_items, &it, 1));
        HIPCK(c, S.d_f64.reserve(1));
        HIPCK(c, S.pin.reserve(sizeof(double)));
        DISPATCH3(c, k_root_children, <<<1, MAPLE_BLOCK, 0, c->stream>>>(c->d_model.p, view(c), 1, S.d_items.p, S.d_f64.p));
        HIPCK(c, hipGetLastError());
        HIPCK(c, hipMemcpyAsync(S.pin.p, S.d_f64.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        original += *(const double *)S.pin.p;
    }
    S.resUp.assign(2 * nI, -1);
    S.resRem.assign(2 * nI, 0.0);
    S.matOf.assign(nI, 0);
    struct Live { int32_t item, passed, pmin; double dis, rem; uint8_t ptip; };
    std::vector<Live> live;
    {   // level 0: what each of the root's children sees from above is the other child's lower list
        std::vector<int32_t> dn, dm; std::vector<size_t> at;
        for (size_t k = (size_t)lv.levelStart[0]; k < (size_t)lv.levelStart[1]; k++) {
            const int32_t v = lv.node[k], other = lv.side[k] ? r1 : r2;
            live.push_back(Live{(int32_t)k, S.low[(size_t)other], nmOf(other), DIST[v] + DIST[other], original, TIP[other]});
            S.matOf[k] = (MUT[root] >= 0 || MUT[v] >= 0) ? 1 : 0;
            if (MUT[v] >= 0) { at.push_back(live.size() - 1); dn.push_back(live.back().passed); dm.push_back(MUT[v]); }
        }
        TRY(pass_lists(c, dn, dm, false));
        for (size_t k = 0; k < at.size(); k++) live[at[k]].passed = dn[k];
    }

    std::vector<int64_t> cw, ca; std::vector<int32_t> cne, cna, cid, cslot;
    for (size_t level = 0;; level++) {
        const int32_t nL = (int32_t)live.size(), n2 = 2 * nL;
        if (nL > 0) {
            // ---- the items, their scratch, the slots that materialise newRootProbVect
            S.items.resize((size_t)nL);
            S.woff.assign((size_t)n2, 0);
            S.sel.clear();
            int64_t tot = 0;
            for (int32_t j = 0; j < nL; j++) {
                const Live &L = live[(size_t)j];
                const int32_t t = lv.node[(size_t)L.item], k0 = C0[t], k1 = C1[t];
                RsItem &it = S.items[(size_t)j];
                it.l[0] = S.low[(size_t)k0]; it.l[1] = S.low[(size_t)k1];
                it.passed = L.passed; it.pmin = L.pmin;
                it.d[0] = DIST[k0]; it.d[1] = DIST[k1]; it.dis = L.dis;
                it.nm[0] = nmOf(k0); it.nm[1] = nmOf(k1);
                it.tip[0] = TIP[k0]; it.tip[1] = TIP[k1]; it.ptip = L.ptip; it.mat = S.matOf[(size_t)L.item];
                for (int s = 0; s < 2; s++) {
                    S.woff[(size_t)(2 * j + s)] = tot;
                    tot += (int64_t)c->h_n_ent[it.l[1 - s]] + c->h_n_ent[it.passed];
                    if (it.mat) S.sel.push_back(2 * j + s);
                }
            }
            const int32_t nSel = (int32_t)S.sel.size();
            for (int32_t i = 0; i < nSel; i++) {                         // newRootProbVect: at most upVect's room + the child's list
                const int32_t k = S.sel[(size_t)i];
                const RsItem &it = S.items[(size_t)(k >> 1)];
                S.woff.push_back(tot);
                tot += (int64_t)c->h_n_ent[it.l[1 - (k & 1)]] + c->h_n_ent[it.passed] + c->h_n_ent[it.l[k & 1]];
            }
            HIPCK(c, S.d_words.reserve((size_t)tot));
            HIPCK(c, S.d_aux.reserve((size_t)(5 * tot)));
            TRY(h2d(c, S.d_items, S.items.data(), (size_t)nL));
            TRY(h2d(c, S.d_woff, S.woff.data(), S.woff.size()));
            TRY(h2d(c, S.d_sel, S.sel.data(), (size_t)nSel));
            // doubles: lkc [nL], lk [n2], lkRoot [n2], rp [n2]; words: n_ent [n2], n_aux [n2], st [n2], n_aux of the new lists [nSel]
            const size_t nF = (size_t)nL + 3 * (size_t)n2, nW = 3 * (size_t)n2 + (size_t)nSel;
            HIPCK(c, S.d_f64.reserve(nF));
            HIPCK(c, S.d_i32.reserve(nW));
            HIPCK(c, S.pin.reserve(nF * sizeof(double) + nW * sizeof(int32_t)));
            double *dLkc = S.d_f64.p, *dLk = dLkc + nL, *dLkRoot = dLk + n2, *dRp = dLkRoot + n2;
            int32_t *dNe = S.d_i32.p, *dNa = dNe + n2, *dSt = dNa + n2, *dNa2 = dSt + n2;
            const RsOut up{S.d_words.p, S.d_aux.p, S.d_woff.p, dNe, dNa};
            const RsOut nw{S.d_words.p, S.d_aux.p, S.d_woff.p + n2, nullptr, dNa2};
            DISPATCH3(c, k_root_children, <<<grid_for(nL), MAPLE_BLOCK, 0, c->stream>>>(c->d_model.p, view(c), nL, S.d_items.p, dLkc));
            HIPCK(c, hipGetLastError());
            DISPATCH3(c, k_root_up, <<<grid_for(n2), MAPLE_BLOCK, 0, c->stream>>>(c->d_model.p, view(c), n2, S.d_items.p, up, dLk));
            HIPCK(c, hipGetLastError());
            if (nSel < n2) {
                DISPATCH3(c, k_root_new, <<<grid_for(n2), MAPLE_BLOCK, 0, c->stream>>>(c->d_model.p, view(c), n2, S.d_items.p, up, dSt, dLkRoot, dRp));
                HIPCK(c, hipGetLastError());
            }
            if (nSel > 0) {
                DISPATCH3(c, k_root_new_list, <<<grid_for(nSel), MAPLE_BLOCK, 0, c->stream>>>(c->d_model.p, view(c), nSel, S.d_items.p, S.d_sel.p, up,
                                                                                            nw, dSt, dLkRoot));
                HIPCK(c, hipGetLastError());
            }
            double *hF = (double *)S.pin.p;
            int32_t *hW = (int32_t *)((char *)S.pin.p + nF * sizeof(double));
            HIPCK(c, hipMemcpyAsync(hF, S.d_f64.p, nF * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCK(c, hipMemcpyAsync(hW, S.d_i32.p, nW * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            HIPCK(c, hipStreamSynchronize(c->stream));
            const double *lkc = hF, *lk = lkc + nL, *lkRoot = lk + n2;
            double *rp = hF + nL + 2 * (size_t)n2;
            const int32_t *ne = hW, *na = ne + n2, *st = na + n2, *na2 = st + n2;

            // ---- what is committed: upVect where the child has an item of its own, newRootProbVect of the materialising slots
            cw.clear(); ca.clear(); cne.clear(); cna.clear(); cslot.clear();
            auto okSlot = [&](int32_t k) { return ne[k] >= 0 && st[k] >= 0; };
            for (int32_t k = 0; k < n2; k++) {
                const int32_t t = lv.node[(size_t)live[(size_t)(k >> 1)].item], b = (k & 1) ? C1[t] : C0[t];
                if (!okSlot(k) || C0[b] < 0) continue;
                cw.push_back(S.woff[(size_t)k]); ca.push_back(5 * S.woff[(size_t)k]); cne.push_back(ne[k]); cna.push_back(na[k]);
                cslot.push_back(k);
            }
            const size_t nUpC = cslot.size();
            for (int32_t i = 0; i < nSel; i++) {
                const int32_t k = S.sel[(size_t)i];
                if (!okSlot(k)) continue;
                cw.push_back(S.woff[(size_t)(n2 + i)]); ca.push_back(5 * S.woff[(size_t)(n2 + i)]); cne.push_back(st[k]); cna.push_back(na2[i]);
                cslot.push_back(k);
            }
            const int32_t nC = (int32_t)cslot.size();
            cid.assign((size_t)nC, -1);
            if (nC > 0) {
                TRY(stage_begin(c, (size_t)nC * 48 + 1024));
                STAGE(dcw, c, cw.data(), nC); STAGE(dca, c, ca.data(), nC); STAGE(dcne, c, cne.data(), nC); STAGE(dcna, c, cna.data(), nC);
                TRY(commit_known(c, nC, dcw, dca, dcne, dcna, cne, cna, cid.data(), S.d_words.p, S.d_aux.p));
            }
            // ---- the materialised lists into the root's frame, one mutated ancestor at a time, then their root probability
            if ((size_t)nC > nUpC) {
                std::vector<int32_t> lists(cid.begin() + (ptrdiff_t)nUpC, cid.end()), at((size_t)nC - nUpC);
                for (size_t q = 0; q < lists.size(); q++) at[q] = S.nearMut[(size_t)lv.node[(size_t)live[(size_t)(cslot[nUpC + q] >> 1)].item]];
                for (;;) {
                    std::vector<int32_t> pl, pm; std::vector<size_t> who;
                    for (size_t q = 0; q < lists.size(); q++)
                        if (at[q] >= 0) { pl.push_back(lists[q]); pm.push_back(MUT[at[q]]); who.push_back(q); }
                    if (who.empty()) break;
                    TRY(pass_lists(c, pl, pm, true));
                    for (size_t x = 0; x < who.size(); x++) {
                        const size_t q = who[x];
                        lists[q] = pl[x];
                        const int32_t above = c->h_tree_up[(size_t)at[q]];
                        at[q] = above < 0 ? -1 : S.nearMut[(size_t)above];  // the next node above with a mutation list
                    }
                }
                std::vector<double> val(lists.size());
                TRY(maple_root_prob_batch(c, (int32_t)lists.size(), lists.data(), val.data()));
                for (size_t q = 0; q < lists.size(); q++) rp[cslot[nUpC + q]] = val[q];
            }
            // ---- upVect down through the child's own mutation list, then shortened (M:7844-7845)
            {
                std::vector<int32_t> dl, dm; std::vector<size_t> who;
                for (size_t q = 0; q < nUpC; q++) {
                    const int32_t k = cslot[q], t = lv.node[(size_t)live[(size_t)(k >> 1)].item], b = (k & 1) ? C1[t] : C0[t];
                    if (MUT[b] >= 0) { dl.push_back(cid[q]); dm.push_back(MUT[b]); who.push_back(q); }
                }
                if (!who.empty()) {
                    TRY(pass_lists(c, dl, dm, false));
                    std::vector<int32_t> sh(dl.size(), -1);
                    TRY(maple_shorten_batch(c, (int32_t)dl.size(), dl.data(), sh.data()));
                    for (size_t x = 0; x < who.size(); x++) {
                        if (sh[x] < 0) return fail(c, MAPLE_ERR_FATAL, "a list handed down could not be shortened");
                        cid[who[x]] = sh[x];
                    }
                }
            }
            // ---- the scores (M:7808), term by term as the Python path adds them, and what the next level is handed
            for (int32_t k = 0; k < n2; k++) {
                if (!okSlot(k)) continue;
                const Live &L = live[(size_t)(k >> 1)];
                const int32_t t = lv.node[(size_t)L.item], b = (k & 1) ? C1[t] : C0[t];
                const double newRem = L.rem + lkc[k >> 1];
                double sc = rp[k] + lkRoot[k];
                sc = sc + lk[k];
                sc = sc - newRem;
                score[b] = sc;
                S.resRem[2 * (size_t)L.item + (size_t)(k & 1)] = newRem - lk[k];
            }
            for (size_t q = 0; q < nUpC; q++) S.resUp[2 * (size_t)live[(size_t)(cslot[q] >> 1)].item + (size_t)(cslot[q] & 1)] = cid[q];
        }
        if (level + 1 >= lv.levels()) break;
        live.clear();
        for (size_t k = (size_t)lv.levelStart[level + 1]; k < (size_t)lv.levelStart[level + 2]; k++) {
            const size_t from = 2 * (size_t)lv.parent[k] + lv.side[k];
            S.matOf[k] = (S.matOf[(size_t)lv.parent[k]] || MUT[lv.node[k]] >= 0) ? 1 : 0;
            if (S.resUp[from] < 0) continue;                             // a rooting above was abandoned: nothing below it is scored
            live.push_back(Live{(int32_t)k, S.resUp[from], 0, DIST[lv.node[k]], S.resRem[from], 0});
        }
    }
    HIPCK(c, hipStreamSynchronize(c->stream));                           // (the last commit reads this call's scratch)
    c->commit_pending = false;
    TRY(guard.release());
    return finish();
}
