// maple_amd/csrc/tree_lk.hip -- calculateTreeLikelihood (MAPLEv0.7.5.4.py:9721-9779, without checkCorrectness and HnZ) inside
// the library: maple_tree_log_lk.
//
// The reference walks the tree in post-order and, at every internal node, merges the two children's lower lists with returnLK
// (M:9756), keeps the likelihood contribution and throws the merged list away; findProbRoot of the root's list comes last.
// Here ONE LANE per internal node runs that merge (merge_walk with wantLK, the step of merge_step_body.inc: the arithmetic of
// maple_merge_batch's outLK, bit for bit) into a CountSink, so nothing but one double and one status per node is written.
// There is no wavefront-per-item form: the running factor of a merge is an ORDERED product over the genome (totalFactor, with
// its carry-over into the logarithm at minimumCarryOver), which one lane multiplies in genome order -- maple_merge_batch itself
// drops to the lane form when outLK is asked for.
// The items are the internal nodes in the reference's order (tree_lk_plan.h, kept per tree until maple_tree_upload or
// maple_tree_patch changes it), so the contributions come back in summation order and the host adds them front to back.
// MAT local references: a child with a mutation list is passed up first (M:9751-9755), and so is the root (M:9773): one
// maple_pass_branch_batch for all of them into lists under an arena mark of this call, as em.hip does for its branches; the
// items of such a call read the passed ids.
// A translation unit of libmaple_hip.so (gfx950 only).
#include "batch_host.h"
#include "tree_lk_plan.h"

#include <cmath>

// item = {children[v][0], children[v][1], list of child 0, list of child 1}; dist / tip / nMinor are columns by node
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(MAPLE_BLOCK) void k_tree_lk(const DevModel *__restrict__ mp, ArenaView av, int n, const int4 *items,
                                                         const double *dist, const uint8_t *tip, const int32_t *nMinor,
                                                         double *outLK, int32_t *status)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int4 it = items[i];
        CountSink s;
        double lk = 0.0;
        const int r = merge_walk(c, list_ref(av, it.z), dist[it.x], tip[it.x] != 0, list_ref(av, it.w), dist[it.y], tip[it.y] != 0,
                                 false, true, nMinor ? nMinor[it.x] : 0, nMinor ? nMinor[it.y] : 0, s, &lk);
        outLK[i] = lk;
        status[i] = r;
    }
}

// findProbRoot of the root's list (M:9772-9775): one lane
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(64) void k_tree_lk_root(const DevModel *__restrict__ mp, ArenaView av, int rootList, double *out)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    if (threadIdx.x == 0) *out = root_prob_walk(c, list_ref(av, rootList));
}

namespace {

struct TreeLkScratch : ScratchBase {
    // the plan of the tree as it stands (valid while maple_ctx::tree_lk_valid)
    std::vector<int32_t> order;          // internal nodes in the reference's order
    std::vector<int4> items;             // per entry of `order`
    std::vector<int32_t> passSlot, passList, passMut;   // children with a mutation list: 2 * item + side, their list, their mutation list
    DevBuf<int4> d_items;
    bool ownCols = false;                // the tree was patched since its upload: dist / tip come from the copies below
    DevBuf<double> d_dist;
    DevBuf<uint8_t> d_tip;
    // per call
    std::vector<int4> itemsCall;
    DevBuf<int4> d_itemsCall;
    DevBuf<int32_t> d_nm, d_status;
    DevBuf<double> d_lk;
    PinBuf pin;
};

TreeLkScratch &scratch(maple_ctx *c)
{
    if (!c->treelk) { c->treelk.reset(new TreeLkScratch()); c->tree_lk_valid = false; }
    return *static_cast<TreeLkScratch *>(c->treelk.get());
}

int build_plan(maple_ctx *c, TreeLkScratch &S)
{
    const int32_t n = (int32_t)c->h_tree_up.size(), root = c->dtree.root;
    const int32_t nl = (int32_t)c->h_n_ent.size(), nml = (int32_t)c->h_mut_cnt.size();
    if (!tree_lk_plan::lk_postorder(n, root, c->h_tree_c0.data(), c->h_tree_c1.data(), S.order))
        return fail(c, MAPLE_ERR_STATE, "the children columns below root %d are no tree", root);
    const size_t nI = S.order.size();
    S.items.resize(nI);
    S.passSlot.clear(); S.passList.clear(); S.passMut.clear();
    for (size_t i = 0; i < nI; i++) {
        const int32_t v = S.order[i];
        const int32_t kid[2] = {c->h_tree_c0[v], c->h_tree_c1[v]};
        int32_t lst[2];
        for (int j = 0; j < 2; j++) {
            lst[j] = c->h_tree_lower[kid[j]];
            if (lst[j] < 0 || lst[j] >= nl) return fail(c, MAPLE_ERR_STATE, "node %d: its child %d has no lower list", v, kid[j]);
            const int32_t mu = c->h_tree_mut[kid[j]];
            if (mu >= nml) return fail(c, MAPLE_ERR_STATE, "node %d: mutList[] = %d is not a mutation-list id (have %d)", kid[j], mu, nml);
            if (mu >= 0) { S.passSlot.push_back((int32_t)(2 * i + j)); S.passList.push_back(lst[j]); S.passMut.push_back(mu); }
        }
        S.items[i] = make_int4(kid[0], kid[1], lst[0], lst[1]);
    }
    if (c->h_tree_lower[root] < 0 || c->h_tree_lower[root] >= nl) return fail(c, MAPLE_ERR_STATE, "the root (%d) has no lower list", root);
    if (c->h_tree_mut[root] >= nml) return fail(c, MAPLE_ERR_STATE, "the root's mutList[] is not a mutation-list id");
    TRY(h2d(c, S.d_items, S.items.data(), nI));
    S.ownCols = c->tree_stale;           // (maple_tree_patch keeps the host copy of the columns, not the device's flat ones)
    if (S.ownCols) {
        TRY(h2d(c, S.d_dist, c->h_tree_dist.data(), (size_t)n));
        TRY(h2d(c, S.d_tip, c->h_tree_tip.data(), (size_t)n));
    }
    HIPCK(c, hipStreamSynchronize(c->stream));
    c->tree_lk_valid = true;
    return MAPLE_OK;
}

}  // namespace

extern "C" int maple_tree_log_lk(maple_ctx *c, const int32_t *nMinor, double *totalLK, double *rootLK, double *nodeLK)
{
    if (!c || !totalLK) return MAPLE_ERR_ARG;
    TRY(begin_tree_call(c));
    TreeLkScratch &S = scratch(c);
    if (!c->tree_lk_valid) TRY(build_plan(c, S));
    const int32_t n = (int32_t)c->h_tree_up.size(), root = c->dtree.root;
    const int32_t nI = (int32_t)S.order.size();
    if (nMinor)
        for (int32_t v = 0; v < n; v++)
            if (nMinor[v] < 0) return fail(c, MAPLE_ERR_ARG, "nMinor[%d] = %d", v, nMinor[v]);
    MarkGuard guard{c};                // the call's temporaries (the lists passed up through reference branches) go on every path
    TRY(guard.take());
    const int4 *dItems = S.d_items.p;
    int32_t rootList = c->h_tree_lower[root];
    const bool passRoot = c->h_tree_mut[root] >= 0;
    if (!S.passSlot.empty() || passRoot) {                               // M:9751-9755 and 9773, all in one launch
        std::vector<int32_t> pl(S.passList), pm(S.passMut);
        if (passRoot) { pl.push_back(rootList); pm.push_back(c->h_tree_mut[root]); }
        std::vector<uint8_t> upDir(pl.size(), 1);
        std::vector<int32_t> out(pl.size(), -1);
        TRY(maple_pass_branch_batch(c, (int32_t)pl.size(), pl.data(), pm.data(), upDir.data(), out.data()));
        for (size_t k = 0; k < out.size(); k++)
            if (out[k] < 0) return fail(c, MAPLE_ERR_FATAL, "a lower list could not be passed through the mutation list %d", pm[k]);
        if (passRoot) rootList = out.back();
        if (!S.passSlot.empty()) {
            S.itemsCall = S.items;
            for (size_t k = 0; k < S.passSlot.size(); k++) {
                int4 &it = S.itemsCall[(size_t)(S.passSlot[k] >> 1)];
                if (S.passSlot[k] & 1) it.w = out[k]; else it.z = out[k];
            }
            TRY(h2d(c, S.d_itemsCall, S.itemsCall.data(), (size_t)nI));
            dItems = S.d_itemsCall.p;
        }
    }
    const int32_t *dNm = nullptr;
    if (nMinor) { TRY(h2d(c, S.d_nm, nMinor, (size_t)n)); dNm = S.d_nm.p; }
    HIPCK(c, S.d_lk.reserve((size_t)nI + 1));
    HIPCK(c, S.d_status.reserve((size_t)nI + 1));
    const size_t offS = (((size_t)nI + 1) * sizeof(double) + 15) & ~(size_t)15;
    HIPCK(c, S.pin.reserve(offS + ((size_t)nI + 1) * sizeof(int32_t)));
    DISPATCH3(c, k_tree_lk_root, <<<1, 64, 0, c->stream>>>(c->d_model.p, view(c), rootList, S.d_lk.p + nI));
    HIPCK(c, hipGetLastError());
    if (nI > 0) {
        const double *dDist = S.ownCols ? S.d_dist.p : c->t_dist.p;
        const uint8_t *dTip = S.ownCols ? S.d_tip.p : c->t_tip.p;
        hipEvent_t e0, e1;
        TRY(ev_pair(c, &e0, &e1, MAPLE_K_OTHER, (double)nI, 0.0));
        HIPCK(c, hipEventRecord(e0, c->stream));
        DISPATCH3(c, k_tree_lk, <<<grid_for(nI), MAPLE_BLOCK, 0, c->stream>>>(c->d_model.p, view(c), nI, dItems, dDist, dTip, dNm, S.d_lk.p,
                                                                            S.d_status.p));
        HIPCK(c, hipGetLastError());
        HIPCK(c, hipEventRecord(e1, c->stream));
        HIPCK(c, hipMemcpyAsync((char *)S.pin.p + offS, S.d_status.p, (size_t)nI * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCK(c, hipMemcpyAsync(S.pin.p, S.d_lk.p, ((size_t)nI + 1) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    TRY(guard.release());
    const double *lk = (const double *)S.pin.p;
    const int32_t *st = (const int32_t *)((const char *)S.pin.p + offS);
    for (int32_t i = 0; i < nI; i++)
        if (st[i] < 0)
            return fail(c, MAPLE_ERR_FATAL, "node %d: the merge of its children's lower lists has no result, or its running factor "
                                            "underflowed (the reference raises here, M:9762)", S.order[i]);
    double total = 0.0;
    for (int32_t i = 0; i < nI; i++) total += lk[i];                     // in the reference's order (M:9757)
    total += lk[nI];                                                     // M:9775
    *totalLK = total;
    if (rootLK) *rootLK = lk[nI];
    if (nodeLK) {
        for (int32_t v = 0; v < n; v++) nodeLK[v] = 0.0;
        for (int32_t i = 0; i < nI; i++) nodeLK[S.order[i]] = lk[i];
    }
    return MAPLE_OK;
}
