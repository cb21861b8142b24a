// maple_amd/csrc/em.hip -- one expectation-maximisation step for the rates of the uploaded tree
// (expectationMaximizationCalculationRates, M:10077-10947; trackMutations=False -- the records of trackMutations=True are
// maple_tree_mutation_events, mat_events.hip, over the same step): maple_em_expectation, maple_em_rates.
//
// Expectation (M:10138-10850): for every non-root branch with dist != 0, or above a leaf under an error model (M:10146), ONE LANE
// walks the parent's upper list (upRight / upLeft of up[node], M:10150, passed down through mutList[node] first: one
// maple_pass_branch_batch for all such branches, under an arena mark of this call) against the node's lower list -- the step is
// em_step_body.inc, a restatement of M:10166-10790 arm for arm.  R / R runs touch no per-site table (the reference's
// totTreeLength + trackingNs bookkeeping), so a walk is O(list entries).
//   totals (counts, waitingTimes, errorCount, totTreeLength): each lane sums its own branch in a column of LDS, the block adds its
//     columns in a fixed tree order into one 22-double partial, the host adds the partials in block order: no float atomics, the
//     same bits on every call;
//   observedTotNucsSites, observedNucsSites: whole numbers, 64-bit integer atomics, exact; numTips is a property of the tree alone
//     (leaves and their minor sequences) and is counted on the host;
//   waitingTimesSites, countsSites, trackingNs, errorCountSites: fp64 atomic adds into tables of at most 7 x (lRef + 1) doubles --
//     their last bits can differ from call to call (DESIGN.md section 14 names the fix: per-branch records stably sorted by site).
// The MAT frame correction of the R / R arm (M:10233-10242) reads the accumulated (position, nucleotide) list of the node's
// reference frame (M:10107-10109, then passMutationListThroughBranch, M:10027, down the path): derived here once per uploaded
// tree, one list per reference node in CSR; a node's frame is its nearest ancestor-or-self with mutations.
// Maximisation (M:10852-10947): em_mstep.h on the host.
#include "branch_walk_host.h"
#include "em_mstep.h"

#include <utility>

#define EM_NACC 22                     // waitingTimes[4], counts[16], errorCount, totTreeLength

namespace {

struct EmOut {
    double *partials;                  // [blocks][EM_NACC]
    double *wts, *cs, *tn, *ecs;       // waitingTimesSites [lRef*4], countsSites [lRef], trackingNs [lRef+1], errorCountSites [lRef]
    unsigned long long *obs;           // observedNucsSites [lRef+1] then observedTotNucsSites (two's complement)
    int32_t *fatal;
};

struct EmScratch : ScratchBase {
    // frames of the uploaded tree (valid while maple_ctx::em_frames_valid)
    std::vector<int32_t> slotOfNode;   // per node at upload: CSR slot of a reference node's list, -1 otherwise
    branch_walk_plan::Rows rows;       // per call (kept for its memory)
    DevBuf<int2> d_fm;
    DevBuf<int32_t> d_fmOff;
    // per call
    DevBuf<int32_t> d_pl, d_cl, d_leafMinor, d_frame;
    DevBuf<double> d_dist, d_tables, d_partials;
    DevBuf<unsigned long long> d_obs;
    DevBuf<int32_t> d_fatal;
};

__device__ inline void em_add(double *p, double x) { unsafeAtomicAdd(p, x); }

template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(WALK_BLOCK) void k_em_walk(const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *pl,
                                                      const int32_t *cl, const double *distArr, const int32_t *leafMinor,
                                                      const int32_t *frame, const int2 *fmAll, const int32_t *fmOff,
                                                      const uint8_t *refIdx, EmOut o)
{
    __shared__ Lds lds;
    __shared__ double acc[EM_NACC * WALK_BLOCK];
    stage_model(*mp, lds);
    const int lane = threadIdx.x;
    for (int k = 0; k < EM_NACC; k++) acc[k * WALK_BLOCK + lane] = 0.0;
    const int b = blockIdx.x * WALK_BLOCK + lane;
    if (b < n) {
        Ctx<RV, U, SS> c(*mp, lds);
        const double *rf = c.rf;
        const int32_t *cb = mp->cumulativeBases;
        const int lRef = mp->lRef;
        const double dist = distArr[b];
        const bool leaf = leafMinor[b] >= 0;
        const int nMinor = leaf ? leafMinor[b] : 0;
        const int2 *fm = nullptr;
        int nFm = 0, iFm = 0;
        if (frame[b] >= 0) { fm = fmAll + fmOff[frame[b]]; nFm = fmOff[frame[b] + 1] - fmOff[frame[b]]; }
        long long obsTot = 0;
        bool fatal = false;
        if (RV) acc[21 * WALK_BLOCK + lane] = dist;                        // M:10148
#define WT(i, x) acc[(i) * WALK_BLOCK + lane] += (x)
#define CNT(i, j, x) acc[(4 + (i) * 4 + (j)) * WALK_BLOCK + lane] += (x)
#define ERRC(x) acc[20 * WALK_BLOCK + lane] += (x)
#define WTS_AT(p, i, x) do { if (RV) em_add(o.wts + (size_t)(p) * 4 + (i), (x)); } while (0)
#define WTS(i, x) WTS_AT(pos, i, x)
#define CS(x) do { if (RV) em_add(o.cs + pos, (x)); } while (0)
#define TN(p, x) do { if (RV) em_add(o.tn + (p), (x)); } while (0)
#define ECS(x) do { if (U && SS) em_add(o.ecs + pos, (x)); } while (0)
#define OBS(p, k) atomicAdd(o.obs + (p), (unsigned long long)(k))
#define OBSTOT(k) obsTot += (k)
#define NEG(x) do { if (RV && (x) < 0.0) fatal = true; } while (0)
#define MUT(i, j, x) ((void)0)         // trackMutations=False: the record hooks do nothing here (mat_events.hip feeds a sink)
#define MUT_SURE(i, j) ((void)0)
#define ERRREC(i, j, x) ((void)0)
#define NS_RUN(last) ((void)0)
#define NS_SITE() ((void)0)
        Cursor a, bb;
        a.init(list_ref(av, pl[b]));
        bb.init(list_ref(av, cl[b]));
        int pos = 0;
        for (;;) {
            const Ent &e1 = a.e, &e2 = bb.e;
#include "em_step_body.inc"
            if (pos == lRef) break;
            a.step(pos);
            bb.step(pos);
        }
#undef WT
#undef CNT
#undef ERRC
#undef WTS_AT
#undef WTS
#undef CS
#undef TN
#undef ECS
#undef OBS
#undef OBSTOT
#undef NEG
#undef MUT
#undef MUT_SURE
#undef ERRREC
#undef NS_RUN
#undef NS_SITE
        if (obsTot != 0) atomicAdd(o.obs + (lRef + 1), (unsigned long long)obsTot);
        if (fatal) *o.fatal = 1;
    }
    // the block's columns added in a fixed order: lane t takes lane t + stride, stride halving
    __syncthreads();
    for (int stride = WALK_BLOCK / 2; stride >= 1; stride >>= 1) {
        if (lane < stride)
            for (int k = 0; k < EM_NACC; k++) acc[k * WALK_BLOCK + lane] += acc[k * WALK_BLOCK + lane + stride];
        __syncthreads();
    }
    if (lane < EM_NACC) o.partials[(size_t)blockIdx.x * EM_NACC + lane] = acc[lane * WALK_BLOCK];
}

// passMutationListThroughBranch(list, mutations, dirIsUp=False), M:10027-10065, on (position, nucleotide) pairs
std::vector<int2> pass_mutation_list(const std::vector<int2> &m1, const int32_t *mut3, int nMut, const std::vector<uint8_t> &refIdx)
{
    std::vector<int2> out;
    size_t i1 = 0;
    int i2 = 0;
    for (;;) {
        if (i1 < m1.size()) {
            const int pos1 = m1[i1].x;
            if (i2 < nMut) {
                const int pos2 = mut3[i2 * 3];
                if (pos1 < pos2) out.push_back(m1[i1++]);
                else {
                    const int endNuc = mut3[i2 * 3 + 2];
                    if (endNuc != refIdx[pos2 - 1]) out.push_back(make_int2(pos2, endNuc));
                    i2++;
                    if (pos1 == pos2) i1++;
                }
            } else out.push_back(m1[i1++]);
        } else if (i2 < nMut) {
            const int pos2 = mut3[i2 * 3], endNuc = mut3[i2 * 3 + 2];
            if (endNuc != refIdx[pos2 - 1]) out.push_back(make_int2(pos2, endNuc));
            i2++;
        } else break;
    }
    return out;
}

EmScratch &scratch(maple_ctx *c)
{
    if (!c->em) { c->em.reset(new EmScratch()); c->em_frames_valid = false; }
    return *static_cast<EmScratch *>(c->em.get());
}

// the frames' accumulated mutation lists, once per uploaded tree
int derive_frames(maple_ctx *c, EmScratch &S)
{
    const int32_t n = (int32_t)c->h_tree_up.size(), root = c->dtree.root;
    S.slotOfNode.assign((size_t)n, -1);
    std::vector<int32_t> fmOff{0};
    std::vector<int2> fmAll;
    if (c->tree_has_mut) {
        std::vector<int32_t> mut3((size_t)c->used_mut * 3);             // the host's copy of the mutation lists' contents
        if (c->used_mut) HIPCK(c, hipMemcpy(mut3.data(), c->d_mut3.p, mut3.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::vector<std::vector<int2>> lists;                           // per slot
        std::vector<std::pair<int32_t, int32_t>> st{{root, -1}};        // (node, slot of the frame above it)
        while (!st.empty()) {
            const auto [v, above] = st.back();
            st.pop_back();
            int32_t mine = above;
            const int32_t id = c->h_tree_mut[v];
            if (id >= 0) {
                const int32_t *m = mut3.data() + 3 * c->h_mut_off[id];
                const int nm = c->h_mut_cnt[id];
                for (int k = 0; k < nm; k++)
                    if (m[k * 3] < 1 || m[k * 3] > c->lRef || m[k * 3 + 1] < 0 || m[k * 3 + 1] > 3 || m[k * 3 + 2] < 0 || m[k * 3 + 2] > 3
                        || (k && m[k * 3] <= m[(k - 1) * 3]))
                        return fail(c, MAPLE_ERR_ARG, "mutation list of node %d: entry %d is out of range or out of order", v, k);
                std::vector<int2> l;
                if (v == root) { for (int k = 0; k < nm; k++) l.push_back(make_int2(m[k * 3], m[k * 3 + 2])); }   // M:10107-10109
                else l = pass_mutation_list(above >= 0 ? lists[above] : std::vector<int2>(), m, nm, c->refIdx);
                mine = (int32_t)lists.size();
                lists.push_back(std::move(l));
                S.slotOfNode[v] = mine;
            }
            if (c->h_tree_c0[v] >= 0) { st.push_back({c->h_tree_c0[v], mine}); st.push_back({c->h_tree_c1[v], mine}); }
        }
        for (const auto &l : lists) { fmAll.insert(fmAll.end(), l.begin(), l.end()); fmOff.push_back((int32_t)fmAll.size()); }
    }
    HIPCK(c, S.d_fmOff.reserve(fmOff.size()));
    HIPCK(c, hipMemcpy(S.d_fmOff.p, fmOff.data(), fmOff.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCK(c, S.d_fm.reserve(fmAll.size() + 1));
    if (!fmAll.empty()) HIPCK(c, hipMemcpy(S.d_fm.p, fmAll.data(), fmAll.size() * sizeof(int2), hipMemcpyHostToDevice));
    c->em_frames_valid = true;
    return MAPLE_OK;
}

struct EmHost {                        // the statistics on the host, as they stand at M:10852
    maple_em_totals tot{};
    std::vector<double> wts, cs, tn, obs, ecs;
};

int expectation(maple_ctx *c, const int32_t *nMinorArr, EmHost &H)
{
    TRY(begin_tree_call(c));
    EmScratch &S = scratch(c);
    const int32_t n = (int32_t)c->h_tree_up.size(), lRef = c->lRef;
    const bool RV = c->dm.useRateVariation, U = c->dm.usingErrorRate, SS = c->dm.errorRateSiteSpecific;
    branch_walk_plan::Rows &rows = S.rows;
    TRY(gather_branches(c, branch_walk_plan::EM, nMinorArr, rows));     // (refuses columns that are no tree: the frames below trust them)
    if (!c->em_frames_valid) TRY(derive_frames(c, S));
    const int32_t nB = rows.size();
    std::vector<int32_t> frame((size_t)nB, -1);                          // the frame each branch lives in, in the tree as it stands
    for (int32_t k = 0; k < nB; k++) {
        const int32_t ref = rows.refNode[k];
        if (ref < 0) continue;
        if (ref >= (int32_t)S.slotOfNode.size() || S.slotOfNode[ref] < 0)
            return fail(c, MAPLE_ERR_STATE, "node %d has mutations the uploaded tree did not have", ref);
        frame[k] = S.slotOfNode[ref];
    }
    const uint8_t *d_refIdx = nullptr;
    TRY(device_ref_idx(c, &d_refIdx));
    MarkGuard guard{c};                // the call's temporaries (the parent lists passed through reference branches) go on every path
    TRY(guard.take());
    TRY(pass_parent_lists(c, rows, false));
    const size_t L1 = (size_t)lRef + 1;
    const size_t nTab = 4 * L1 + 3 * L1;                                 // wts, cs, tn, ecs: 7 x (lRef + 1) doubles
    const int blocks = std::max(1, (nB + WALK_BLOCK - 1) / WALK_BLOCK);
    HIPCK(c, S.d_tables.reserve(nTab));
    HIPCK(c, S.d_obs.reserve(L1 + 1));
    HIPCK(c, S.d_partials.reserve((size_t)blocks * EM_NACC));
    HIPCK(c, S.d_fatal.reserve(1));
    HIPCK(c, hipMemsetAsync(S.d_tables.p, 0, nTab * sizeof(double), c->stream));
    HIPCK(c, hipMemsetAsync(S.d_obs.p, 0, (L1 + 1) * sizeof(unsigned long long), c->stream));
    HIPCK(c, hipMemsetAsync(S.d_fatal.p, 0, sizeof(int32_t), c->stream));
    TRY(h2d(c, S.d_pl, rows.pList.data(), (size_t)nB));
    TRY(h2d(c, S.d_cl, rows.cList.data(), (size_t)nB));
    TRY(h2d(c, S.d_leafMinor, rows.leafMinor.data(), (size_t)nB));
    TRY(h2d(c, S.d_frame, frame.data(), (size_t)nB));
    TRY(h2d(c, S.d_dist, rows.dist.data(), (size_t)nB));
    EmOut o{S.d_partials.p, S.d_tables.p, S.d_tables.p + 4 * L1, S.d_tables.p + 5 * L1, S.d_tables.p + 6 * L1, S.d_obs.p, S.d_fatal.p};
    TRY(timed_launch(c, nB, [&] {
        DISPATCH3(c, k_em_walk, <<<dim3(blocks), dim3(WALK_BLOCK), 0, c->stream>>>(c->d_model.p, view(c), nB, S.d_pl.p, S.d_cl.p, S.d_dist.p,
                                                                                  S.d_leafMinor.p, S.d_frame.p, S.d_fm.p, S.d_fmOff.p,
                                                                                  d_refIdx, o));
    }));
    std::vector<double> partials((size_t)blocks * EM_NACC), tables(nTab);
    std::vector<unsigned long long> obs(L1 + 1);
    int32_t fatal = 0;
    HIPCK(c, hipMemcpyAsync(partials.data(), S.d_partials.p, partials.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (RV || SS) HIPCK(c, hipMemcpyAsync(tables.data(), S.d_tables.p, nTab * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(obs.data(), S.d_obs.p, obs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(&fatal, S.d_fatal.p, sizeof fatal, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (fatal) return fail(c, MAPLE_ERR_FATAL, "a negative probability in the EM walk (the reference raises, M:10293 and its kin)");
    double sum[EM_NACC] = {};
    for (int b = 0; b < blocks; b++)                                     // in block order
        for (int k = 0; k < EM_NACC; k++) sum[k] += partials[(size_t)b * EM_NACC + k];
    maple_em_totals &T = H.tot;
    for (int i = 0; i < 4; i++) T.waitingTimes[i] = sum[i];
    for (int i = 0; i < 16; i++) T.counts[i] = sum[4 + i];
    T.errorCount = U ? sum[20] : 0.0;
    T.totTreeLength = RV ? sum[21] : 0.0;
    T.numTips = rows.numTips;
    T.observedTotNucsSites = U ? (int64_t)obs[L1] : 0;
    H.wts.assign(tables.begin(), tables.begin() + 4 * (size_t)lRef);
    H.cs.assign(tables.begin() + 4 * L1, tables.begin() + 4 * L1 + lRef);
    H.tn.assign(tables.begin() + 5 * L1, tables.begin() + 6 * L1);
    H.ecs.assign(tables.begin() + 6 * L1, tables.begin() + 6 * L1 + lRef);
    H.obs.resize(L1);
    for (size_t i = 0; i < L1; i++) H.obs[i] = (double)(int64_t)obs[i];
    return MAPLE_OK;
}

} // namespace

extern "C" int maple_em_expectation(maple_ctx *c, const int32_t *nMinor, maple_em_totals *tot, double *waitingTimesSites,
                                    double *countsSites, double *trackingNs, double *observedNucsSites, double *errorCountSites)
{
    if (!c || !tot) return MAPLE_ERR_ARG;
    EmHost H;
    TRY(expectation(c, nMinor, H));
    *tot = H.tot;
    const size_t L = (size_t)c->lRef;
    if (waitingTimesSites) memcpy(waitingTimesSites, H.wts.data(), 4 * L * sizeof(double));
    if (countsSites) memcpy(countsSites, H.cs.data(), L * sizeof(double));
    if (trackingNs) memcpy(trackingNs, H.tn.data(), (L + 1) * sizeof(double));
    if (observedNucsSites) memcpy(observedNucsSites, H.obs.data(), (L + 1) * sizeof(double));
    if (errorCountSites) memcpy(errorCountSites, H.ecs.data(), L * sizeof(double));
    return MAPLE_OK;
}

extern "C" int maple_em_rates(maple_ctx *c, const int32_t *nMinor, int model, double *Q16, double *siteRates, double *errorRateGlobal,
                              double *siteErrRates)
{
    if (!c || !Q16) return MAPLE_ERR_ARG;
    if (!c->tree_set) return fail(c, MAPLE_ERR_STATE, "maple_tree_upload has not been called");
    TRY(need_model(c));
    const bool RV = c->dm.useRateVariation, U = c->dm.usingErrorRate, SS = c->dm.errorRateSiteSpecific;
    if (model != maple_em::EM_UNREST && model != maple_em::EM_GTR && !U)                 // M:10877-10879
        return fail(c, MAPLE_ERR_ARG, "expectation maximisation is implemented for models 0 (UNREST) and 1 (GTR), not %d", model);
    if ((RV && !siteRates) || (U && !errorRateGlobal) || (SS && !siteErrRates))
        return fail(c, MAPLE_ERR_ARG, "an output the current model has is missing (siteRates / errorRateGlobal / siteErrRates)");
    EmHost H;
    TRY(expectation(c, nMinor, H));
    maple_em::MStepStats s{};
    s.lRef = c->lRef; s.refIdx = c->refIdx.data(); s.rootFreqs = c->dm.rootFreqs;
    s.useRateVariation = RV; s.usingErrorRate = U; s.errorRateSiteSpecific = SS;
    for (int i = 0; i < 16; i++) s.counts[i] = H.tot.counts[i];
    for (int i = 0; i < 4; i++) s.waitingTimes[i] = H.tot.waitingTimes[i];
    s.errorCount = H.tot.errorCount; s.totTreeLength = H.tot.totTreeLength;
    s.observedTotNucsSites = H.tot.observedTotNucsSites; s.numTips = H.tot.numTips;
    s.waitingTimesSites = H.wts.data(); s.countsSites = H.cs.data(); s.trackingNs = H.tn.data();
    s.observedNucsSites = H.obs.data(); s.errorCountSites = H.ecs.data();
    if (maple_em::em_mstep(s, model, Q16, RV ? siteRates : nullptr, errorRateGlobal, SS ? siteErrRates : nullptr) != 0)
        return fail(c, MAPLE_ERR_ARG, "expectation maximisation is not implemented for model %d", model);
    return MAPLE_OK;
}
