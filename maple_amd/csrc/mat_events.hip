// maple_amd/csrc/mat_events.hip -- the inferred mutation events of every branch of the uploaded tree: the record lists that
// expectationMaximizationCalculationRates(tree, root, trackMutations=True) leaves on the nodes (MAPLEv0.7.5.4.py:10077-10850,
// --estimateMAT: tree.mutationsInf, tree.Ns and, under an error model, tree.errors) inside the library: maple_tree_mutation_events.
//
// Every node the root reaches is an item of one of two kinds, the reference's if / else at M:10146 / M:10808:
//   pair items -- a non-root node with dist != 0, or a leaf under an error model: ONE LANE walks the parent's upper list (upRight /
//     upLeft of up[node], M:10150, passed down through mutList[node] first: one maple_pass_branch_batch for all such nodes, under an
//     arena mark of this call, as em.hip does) against the node's lower list.  The step is em_step_body.inc, the EM walk's own: its
//     accumulation macros are empty here and its record hooks (MUT, MUT_SURE, ERRREC, NS_RUN, NS_SITE) feed the sink; NEG stays;
//   single-list items -- everything else, the root included: the lane walks the lower list alone for the Ns records of
//     M:10810-10826.
// The same kernel runs twice over a sink, as in error_probs.hip:
//   launch 1 counts each item's records per stream; the host scans the counts, by node id, into the three offset arrays;
//   launch 2 writes each record at the item's offset in the order the walk meets it: a mutation or error record is one 16-byte
//     store (maple_mut_event), an Ns record one 8-byte store (maple_n_run), each stream bounded by the item's own count.
// Nothing is accumulated across lanes: no float atomics, no order that depends on scheduling, the same bytes on every call.
// A translation unit of libmaple_hip.so (gfx950 only).
#include "branch_walk_host.h"

#include <utility>

static_assert(sizeof(maple_mut_event) == 16 && sizeof(maple_n_run) == 8, "the records are one 16-byte / one 8-byte store");

namespace {

struct MatSink {                       // where the records go; off == nullptr: they are only counted
    const int64_t *off;                // [items][3]: the item's first record in mut / ns / err
    uint4 *mut;                        // maple_mut_event: {pos, from | to << 8, the probability's low word, its high word}
    int2 *ns;                          // maple_n_run: {first, last}
    uint4 *err;
};

struct MatScratch : ScratchBase {      // per call
    branch_walk_plan::Rows rows;       // (kept for its memory)
    DevBuf<int32_t> d_pl, d_cl, d_leafMinor, d_count, d_fatal;
    DevBuf<double> d_dist;
    DevBuf<int64_t> d_off;
    DevBuf<uint4> d_mut, d_err;
    DevBuf<int2> d_ns;
};

__device__ inline uint4 event_words(int pos, int from, int to, double x)
{
    return make_uint4((unsigned)pos, (unsigned)from | ((unsigned)to << 8), (unsigned)__double2loint(x), (unsigned)__double2hiint(x));
}

// items = the nodes the root reaches; pl[b] < 0: a single-list item; leafMinor[b] = nMinor of a leaf, -1 for an internal node;
// count[b * 3 + k] = the records of item b in stream k (written when the sink only counts, the bound of what is written when it
// stores)
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(WALK_BLOCK) void k_mat_walk(const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *pl,
                                                        const int32_t *cl, const double *distArr, const int32_t *leafMinor,
                                                        const uint8_t *refIdx, double minMutProb, int32_t *count, MatSink s,
                                                        int32_t *fatalOut)
{
    __shared__ Lds lds;
    stage_model(*mp, lds);
    const int b = blockIdx.x * WALK_BLOCK + threadIdx.x;
    if (b >= n) return;
    Ctx<RV, U, SS> c(*mp, lds);
    const double *rf = c.rf;
    const int32_t *cb = mp->cumulativeBases;
    const int lRef = mp->lRef;
    const double dist = distArr[b];
    const bool leaf = leafMinor[b] >= 0;
    const int nMinor = leaf ? leafMinor[b] : 0;
    const bool store = s.off != nullptr;
    const int64_t baseM = store ? s.off[(size_t)b * 3] : 0, baseN = store ? s.off[(size_t)b * 3 + 1] : 0,
                  baseE = store ? s.off[(size_t)b * 3 + 2] : 0;
    const int roomM = store ? count[(size_t)b * 3] : 0, roomN = store ? count[(size_t)b * 3 + 1] : 0,
              roomE = store ? count[(size_t)b * 3 + 2] : 0;
    int nM = 0, nN = 0, nE = 0;
    int lastRunEnd = 0;                                                  // the end of the Ns list's last record if it is a run, else 0
    bool fatal = false;
#define NSREC(first, last) do { if (nN < roomN) s.ns[baseN + nN] = make_int2((first), (last)); nN++; } while (0)
    Cursor bb;
    bb.init(list_ref(av, cl[b]));
    int pos = 0;
    if (pl[b] < 0) {                                                     // M:10810-10826
        for (;;) {
            const Ent &e2 = bb.e;
            if (e2.type == 5) {
                if (e2.pos > pos + 1) NSREC(pos + 1, e2.pos);
                else NSREC(pos + 1, 0);
                pos = e2.pos;
            } else if (e2.type == 4) pos = e2.pos;
            else {
                if (e2.type == 6 && leaf) NSREC(pos + 1, 0);
                pos += 1;
            }
            if (pos >= lRef) break;
            bb.next();
        }
    } else {
        const int2 *fm = nullptr;                                        // the frame's list corrects waiting times only (M:10233-10242)
        const int nFm = 0;
        int iFm = 0;
#define WT(i, x) ((void)0)
#define CNT(i, j, x) ((void)0)
#define ERRC(x) ((void)0)
#define WTS_AT(p, i, x) ((void)0)
#define WTS(i, x) ((void)0)
#define CS(x) ((void)0)
#define TN(p, x) ((void)0)
#define ECS(x) ((void)0)
#define OBS(p, k) ((void)0)
#define OBSTOT(k) ((void)0)
#define NEG(x) do { if (RV && (x) < 0.0) fatal = true; } while (0)
#define MUT_SURE(i, j) do { if (nM < roomM) s.mut[baseM + nM] = event_words(pos + 1, (i), (j), 1.0); nM++; } while (0)
#define MUT(i, j, x) do { if ((x) > minMutProb) { if (nM < roomM) s.mut[baseM + nM] = event_words(pos + 1, (i), (j), (x)); nM++; } } while (0)
#define ERRREC(i, j, x) do { if (U && (x) > minMutProb) { if (nE < roomE) s.err[baseE + nE] = event_words(pos + 1, (i), (j), (x)); nE++; } } while (0)
#define NS_RUN(last) do { if (lastRunEnd != (last)) { NSREC(pos + 1, (last)); lastRunEnd = (last); } } while (0)
#define NS_SITE() do { NSREC(pos + 1, 0); lastRunEnd = 0; } while (0)
        Cursor a;
        a.init(list_ref(av, pl[b]));
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
#undef MUT_SURE
#undef MUT
#undef ERRREC
#undef NS_RUN
#undef NS_SITE
        (void)fm; (void)iFm; (void)rf; (void)cb; (void)nMinor;
    }
#undef NSREC
    if (!store) { count[(size_t)b * 3] = nM; count[(size_t)b * 3 + 1] = nN; count[(size_t)b * 3 + 2] = nE; }
    if (fatal) *fatalOut = 1;
}

MatScratch &scratch(maple_ctx *c)
{
    if (!c->matevents) c->matevents.reset(new MatScratch());
    return *static_cast<MatScratch *>(c->matevents.get());
}

}  // namespace

extern "C" int maple_tree_mutation_events(maple_ctx *c, const int32_t *nMinorArr, double minMutProb, int64_t *mutOff, int64_t *nsOff,
                                          int64_t *errOff, int64_t capMut, maple_mut_event *mut, int64_t capNs, maple_n_run *ns,
                                          int64_t capErr, maple_mut_event *err, int64_t nRecords[3])
{
    if (!c || !mutOff || !nsOff || !errOff || !nRecords || capMut < 0 || capNs < 0 || capErr < 0) return MAPLE_ERR_ARG;
    TRY(need_tree_and_model(c));
    if ((capMut > 0 && !mut) || (capNs > 0 && !ns) || (capErr > 0 && !err))
        return fail(c, MAPLE_ERR_ARG, "a capacity without its record array");
    TRY(begin_tree_call(c));
    MatScratch &S = scratch(c);
    const int32_t n = (int32_t)c->h_tree_up.size();
    // the items, depth-first from the root (the order is the launch's only: the records are laid out by node id)
    branch_walk_plan::Rows &rows = S.rows;
    TRY(gather_branches(c, branch_walk_plan::EVENTS, nMinorArr, rows));
    const std::vector<int32_t> &node = rows.node;
    const int32_t nI = rows.size();
    for (int32_t v = 0; v <= n; v++) mutOff[v] = nsOff[v] = errOff[v] = 0;
    nRecords[0] = nRecords[1] = nRecords[2] = 0;
    MarkGuard guard{c};                // the call's temporaries (the parent lists passed through reference branches) go on every path
    TRY(guard.take());
    TRY(pass_parent_lists(c, rows, true));
    const int blocks = (nI + WALK_BLOCK - 1) / WALK_BLOCK;
    std::vector<int32_t> count((size_t)nI * 3, 0);
    int32_t fatal = 0;
    HIPCK(c, S.d_count.reserve((size_t)nI * 3));
    const uint8_t *d_refIdx = nullptr;
    TRY(device_ref_idx(c, &d_refIdx));
    HIPCK(c, S.d_fatal.reserve(1));
    HIPCK(c, hipMemsetAsync(S.d_fatal.p, 0, sizeof(int32_t), c->stream));
    TRY(h2d(c, S.d_pl, rows.pList.data(), (size_t)nI));
    TRY(h2d(c, S.d_cl, rows.cList.data(), (size_t)nI));
    TRY(h2d(c, S.d_leafMinor, rows.leafMinor.data(), (size_t)nI));
    TRY(h2d(c, S.d_dist, rows.dist.data(), (size_t)nI));
    const auto walk = [&](MatSink sink) {                                // the one kernel: counting, then storing
        return timed_launch(c, nI, [&] {
            DISPATCH3(c, k_mat_walk, <<<dim3(blocks), dim3(WALK_BLOCK), 0, c->stream>>>(c->d_model.p, view(c), nI, S.d_pl.p, S.d_cl.p, S.d_dist.p,
                                                                                       S.d_leafMinor.p, d_refIdx, minMutProb, S.d_count.p, sink,
                                                                                       S.d_fatal.p));
        });
    };
    TRY(walk(MatSink{}));
    HIPCK(c, hipMemcpyAsync(count.data(), S.d_count.p, (size_t)nI * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(&fatal, S.d_fatal.p, sizeof fatal, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (fatal) return fail(c, MAPLE_ERR_FATAL, "a negative probability in the EM walk (the reference raises, M:10293 and its kin)");
    // offsets: the exclusive scans of the counts by node id; slots the root does not reach have none
    std::vector<int32_t> itemOf((size_t)n, -1);
    for (int32_t i = 0; i < nI; i++) itemOf[node[i]] = i;
    std::vector<int64_t> itemOff((size_t)nI * 3);
    int64_t tot[3] = {0, 0, 0};
    int64_t *offs[3] = {mutOff, nsOff, errOff};
    for (int32_t v = 0; v < n; v++) {
        const int32_t i = itemOf[v];
        for (int k = 0; k < 3; k++) {
            offs[k][v] = tot[k];
            if (i >= 0) { itemOff[(size_t)i * 3 + k] = tot[k]; tot[k] += count[(size_t)i * 3 + k]; }
        }
    }
    for (int k = 0; k < 3; k++) { offs[k][n] = tot[k]; nRecords[k] = tot[k]; }
    if (capMut == 0 && capNs == 0 && capErr == 0) return guard.release();    // counted only
    if (capMut < tot[0] || capNs < tot[1] || capErr < tot[2])
        return fail(c, MAPLE_ERR_ARG, "capMut = %lld, capNs = %lld, capErr = %lld: the tree has %lld mutation, %lld Ns and %lld error records",
                    (long long)capMut, (long long)capNs, (long long)capErr, (long long)tot[0], (long long)tot[1], (long long)tot[2]);
    if (tot[0] + tot[1] + tot[2] == 0) return guard.release();
    HIPCK(c, S.d_mut.reserve((size_t)tot[0] + 1));
    HIPCK(c, S.d_ns.reserve((size_t)tot[1] + 1));
    HIPCK(c, S.d_err.reserve((size_t)tot[2] + 1));
    TRY(h2d(c, S.d_off, itemOff.data(), (size_t)nI * 3));
    TRY(walk(MatSink{S.d_off.p, S.d_mut.p, S.d_ns.p, S.d_err.p}));
    if (tot[0]) HIPCK(c, hipMemcpyAsync(mut, S.d_mut.p, (size_t)tot[0] * sizeof(maple_mut_event), hipMemcpyDeviceToHost, c->stream));
    if (tot[1]) HIPCK(c, hipMemcpyAsync(ns, S.d_ns.p, (size_t)tot[1] * sizeof(maple_n_run), hipMemcpyDeviceToHost, c->stream));
    if (tot[2]) HIPCK(c, hipMemcpyAsync(err, S.d_err.p, (size_t)tot[2] * sizeof(maple_mut_event), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return guard.release();
}
