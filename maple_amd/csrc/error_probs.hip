// maple_amd/csrc/error_probs.hip -- the per-sample report of probable sequencing errors (calculateErrorProbabilities,
// MAPLEv0.7.5.4.py:9783-10020, --estimateErrors) inside the library: maple_tree_error_probs.
//
// For every leaf without minor sequences the reference walks the parent's upper list (upRight / upLeft of up[leaf], M:9809-9812,
// passed down through mutList[leaf] first, M:9813-9814: one maple_pass_branch_batch for all such leaves, under an arena mark of this
// call, as em.hip does for its branches) against the leaf's lower list and writes one record per site whose posterior probability
// of being an error reaches minErrorProb.  Here ONE LANE walks each such leaf -- the step is err_step_body.inc, a restatement of
// M:9820-9988 arm for arm, over the Cursor / Ent / Ctx of the EM walk -- and the same kernel runs twice over a sink:
//   launch 1 counts each leaf's records; the host scans the counts into offsets (4 bytes per leaf down, 8 up);
//   launch 2 writes (position, allele, probability) at the leaf's offset, positions ascending as the walk meets them.
// Nothing is accumulated across lanes: no float atomics, no order that depends on scheduling, the same bytes on every call.
// A zero denominator (the reference's ZeroDivisionError) ends the lane's walk and notes (leaf, position) in one 64-bit word with an
// integer atomicMin, so that the first leaf of the report's order is the one named; nothing traps.
// A translation unit of libmaple_hip.so (gfx950 only).
#include "branch_walk_host.h"

#include <utility>

namespace {

struct ErrSink {                       // where the records go; pos == nullptr: they are only counted
    const int64_t *off;                // [items]: the item's first record
    int32_t *pos;
    uint8_t *allele;
    double *prob;
};

struct ErrScratch : ScratchBase {      // per call
    branch_walk_plan::Rows rows;       // (kept for its memory)
    DevBuf<int32_t> d_pl, d_cl, d_count, d_pos;
    DevBuf<double> d_dist, d_prob;
    DevBuf<int64_t> d_off;
    DevBuf<uint8_t> d_allele;
    DevBuf<unsigned long long> d_fatal;
};

// items = the leaves that are walked, in the report's order; count[b] = the records of item b (written when the sink only counts,
// the bound of what is written when it stores)
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(WALK_BLOCK) void k_err_walk(const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *pl,
                                                        const int32_t *cl, const double *distArr, double minErrorProb, int32_t *count,
                                                        ErrSink s, unsigned long long *fatal)
{
    __shared__ Lds lds;
    stage_model(*mp, lds);
    const int b = blockIdx.x * WALK_BLOCK + threadIdx.x;
    if (!U || b >= n) return;                                            // (the call refuses a model without error rates)
    Ctx<RV, U, SS> c(*mp, lds);
    const double *rf = c.rf;
    const int lRef = mp->lRef;
    const double dist = distArr[b];
    const bool store = s.pos != nullptr;
    const int64_t base = store ? s.off[b] : 0;
    const int room = store ? count[b] : 0;
    int nRec = 0, zeroAt = 0;
#define REC(al, x) do { if (store && nRec < room) { s.pos[base + nRec] = pos + 1; s.allele[base + nRec] = (uint8_t)(al); s.prob[base + nRec] = (x); } \
                        nRec++; } while (0)
#define DEN(x) if ((x) == 0.0) { zeroAt = pos + 1; break; }
    Cursor a, bb;
    a.init(list_ref(av, pl[b]));
    bb.init(list_ref(av, cl[b]));
    int pos = 0;
    for (;;) {
        const Ent &e1 = a.e, &e2 = bb.e;
#include "err_step_body.inc"
        if (pos == lRef) break;                                          // M:9990-10004
        a.step(pos);
        bb.step(pos);
    }
#undef REC
#undef DEN
    if (!store) count[b] = nRec;
    if (zeroAt) atomicMin(fatal, ((unsigned long long)(unsigned)b << 32) | (unsigned)zeroAt);
}

ErrScratch &scratch(maple_ctx *c)
{
    if (!c->errprob) c->errprob.reset(new ErrScratch());
    return *static_cast<ErrScratch *>(c->errprob.get());
}

}  // namespace

extern "C" int maple_tree_error_probs(maple_ctx *c, const int32_t *nMinorArr, double minErrorProb, int32_t capLeaves, int32_t *leafNode,
                                      int64_t *outOff, int32_t *nLeaves, int64_t cap, int32_t *outPos, uint8_t *outAllele,
                                      double *outProb, int64_t *nRecords)
{
    if (!c || !nLeaves || !nRecords || capLeaves < 0 || cap < 0 || (capLeaves > 0 && (!leafNode || !outOff))) return MAPLE_ERR_ARG;
    TRY(need_tree_and_model(c));
    if (!c->dm.usingErrorRate)
        return fail(c, MAPLE_ERR_STATE, "the model has no error rate (the reference reports errors only under an error model)");
    if (cap > 0 && (!outPos || !outAllele || !outProb)) return fail(c, MAPLE_ERR_ARG, "cap = %lld without the record arrays", (long long)cap);
    TRY(begin_tree_call(c));
    ErrScratch &S = scratch(c);
    // the leaves in the order the reference's traversal meets them (M:9801-10020); the walked ones -- no minor sequences, M:9805 --
    // are the kernel's items
    branch_walk_plan::Rows &rows = S.rows;
    TRY(gather_branches(c, branch_walk_plan::ERRORS, nMinorArr, rows));
    const std::vector<int32_t> &leaves = rows.leaves, &itemLeaf = rows.itemLeaf;
    const int32_t nL = (int32_t)leaves.size(), nI = rows.size();
    *nLeaves = nL;
    *nRecords = 0;
    if (nL > capLeaves) return fail(c, MAPLE_ERR_ARG, "capLeaves = %d, the tree has %d leaves", capLeaves, nL);
    for (int32_t k = 0; k < nL; k++) leafNode[k] = leaves[k];
    std::vector<int32_t> count((size_t)nI, 0);
    MarkGuard guard{c};                // the call's temporaries (the parent lists passed through reference branches) go on every path
    TRY(guard.take());
    const int blocks = (nI + WALK_BLOCK - 1) / WALK_BLOCK;
    const auto walk = [&](ErrSink sink) {                                // the one kernel: counting, then storing
        return timed_launch(c, nI, [&] {
            DISPATCH3(c, k_err_walk, <<<dim3(blocks), dim3(WALK_BLOCK), 0, c->stream>>>(c->d_model.p, view(c), nI, S.d_pl.p, S.d_cl.p,
                                                                                       S.d_dist.p, minErrorProb, S.d_count.p, sink, S.d_fatal.p));
        });
    };
    if (nI > 0) {
        TRY(pass_parent_lists(c, rows, true));
        const unsigned long long none = ~0ull;
        unsigned long long fatal = none;
        HIPCK(c, S.d_count.reserve((size_t)nI));
        HIPCK(c, S.d_fatal.reserve(1));
        HIPCK(c, hipMemcpyAsync(S.d_fatal.p, &none, sizeof none, hipMemcpyHostToDevice, c->stream));
        TRY(h2d(c, S.d_pl, rows.pList.data(), (size_t)nI));
        TRY(h2d(c, S.d_cl, rows.cList.data(), (size_t)nI));
        TRY(h2d(c, S.d_dist, rows.dist.data(), (size_t)nI));
        TRY(walk(ErrSink{}));
        HIPCK(c, hipMemcpyAsync(count.data(), S.d_count.p, (size_t)nI * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipMemcpyAsync(&fatal, S.d_fatal.p, sizeof fatal, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        if (fatal != none)
            return fail(c, MAPLE_ERR_FATAL, "node %d, position %d: a zero denominator in the error probability (the reference raises "
                                            "ZeroDivisionError: error rate 0 on a branch without length)",
                        leaves[itemLeaf[(size_t)(fatal >> 32)]], (int)(fatal & 0xffffffffu));
    }
    // offsets: the exclusive scan of the counts, leaves that are not walked have none
    std::vector<int64_t> itemOff((size_t)nI);
    int64_t total = 0;
    {
        int32_t i = 0;
        for (int32_t k = 0; k < nL; k++) {
            outOff[k] = total;
            if (i < nI && itemLeaf[i] == k) { itemOff[i] = total; total += count[i]; i++; }
        }
        outOff[nL] = total;
    }
    *nRecords = total;
    if (cap == 0 || total == 0) return guard.release();                  // counted only
    if (cap < total) return fail(c, MAPLE_ERR_ARG, "cap = %lld, the report has %lld records", (long long)cap, (long long)total);
    HIPCK(c, S.d_pos.reserve((size_t)total));
    HIPCK(c, S.d_allele.reserve((size_t)total));
    HIPCK(c, S.d_prob.reserve((size_t)total));
    TRY(h2d(c, S.d_off, itemOff.data(), (size_t)nI));
    TRY(walk(ErrSink{S.d_off.p, S.d_pos.p, S.d_allele.p, S.d_prob.p}));
    HIPCK(c, hipMemcpyAsync(outPos, S.d_pos.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(outAllele, S.d_allele.p, (size_t)total, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(outProb, S.d_prob.p, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.release();
}
