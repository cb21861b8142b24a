// maple_amd/csrc/maple_hip.hip -- libmaple_hip.so: context, model, arena, the batched list operators over explicit pairs and their
// kernels, the RCCL arg-max, the timing readers (C ABI: include/maple_hip.h).  The dense query kernels live in append_queries.hip,
// the placement search in placement.hip, updatePartials and the list rebuild in update.hip, the tree mirror and the SPR search
// batch in spr_batch.hip, the frontier tier in frontier*.hip, the witness filter in witness.hip; the hooks of
// include/maple_hip_debug.h in debug_abi.hip.  What crosses units is declared in batch_host.h.
// gfx950 only.  One lane walks one (parent list, child list) pair; see genome_dev.h.
#include "../../include/maple_hip.h"
#include "genome_dev.h"
#include "search_dev.h"
#include "placement_dev.h"
#include "wave_dev.h"
#include "wave_update.h"

#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

using namespace maple;

// RCCL is used through dlopen only (maple_comm_*, below): types from the header, no link-time dependency
#include <dlfcn.h>
#include <hipcub/hipcub.hpp>
#include <rccl/rccl.h>
struct RcclApi {
    ncclResult_t (*GetUniqueId)(ncclUniqueId *);
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int);
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
    ncclResult_t (*CommDestroy)(ncclComm_t);
    const char *(*GetErrorString)(ncclResult_t);
};
static RcclApi g_rccl{};

#include "ctx_host.h"
#include "batch_host.h"
#include "frontier.h"
#include "witness.h"

// =================================================================================================
// kernels
// =================================================================================================

// appendProbNode over arbitrary pairs ----------------------------------------------------------
template <bool RV, bool U, bool SS>
__global__ MAPLE_APPEND_ATTR void k_append(const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *pl,
                                           const int32_t *cl, const uint8_t *tip, const double *bl, double *out)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        out[i] = append_walk(c, list_ref(av, pl[i]), list_ref(av, cl[i]), tip[i] != 0, bl[i]);
}

// per-item scratch placement for list-producing kernels
struct OutSpec {
    uint2 *words;                      // scratch words
    double *aux;                       // scratch aux
    const int64_t *woff;               // per item offset into words
    const int64_t *aoff;               // per item offset into aux
    int32_t *n_ent;                    // per item result: entries (or <0 status)
    int32_t *n_aux;
};

template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(MAPLE_BLOCK) void k_merge(const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *l1,
                                                       const double *b1, const uint8_t *t1, const int32_t *l2,
                                                       const double *b2, const uint8_t *t2, const uint8_t *ud,
                                                       const int32_t *nm1, const int32_t *nm2, OutSpec o, double *outLK)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        Writer w;
        w.init(o.words + o.woff[i], o.aux + o.aoff[i]);
        double lk = 0.0;
        int r = merge_walk(c, list_ref(av, l1[i]), b1[i], t1[i] != 0, list_ref(av, l2[i]), b2[i], t2[i] != 0,
                           ud[i] != 0, outLK != nullptr, nm1 ? nm1[i] : 0, nm2 ? nm2[i] : 0, w, &lk);
        o.n_ent[i] = r;
        o.n_aux[i] = w.na;
        if (outLK) outLK[i] = lk;
    }
}

template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(MAPLE_BLOCK) void k_blen(const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *pl,
                                                      const int32_t *cl, const uint8_t *tip, double *ais,
                                                      const int64_t *aisOff, double *t, uint8_t *isFalse)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        bool f;
        t[i] = blen_walk(c, list_ref(av, pl[i]), list_ref(av, cl[i]), tip[i] != 0, ais + aisOff[i], 1, &f);
        isFalse[i] = f ? 1 : 0;
    }
}

template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(MAPLE_BLOCK) void k_differ(const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *l1,
                                                        const int32_t *l2, uint8_t *out)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        out[i] = (l2[i] < 0) ? 1 : (differ_walk(c, list_ref(av, l1[i]), list_ref(av, l2[i])) ? 1 : 0);
}

template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(MAPLE_BLOCK) void k_root_prob(const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *l,
                                                           double *out)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        out[i] = root_prob_walk(c, list_ref(av, l[i]));
}

// One query against a resident candidate set: candidate k is scored against the query's list in ITS reference frame
// (frameLists[frameIdx[k]]), so trees with MAT local references need one launch per query, not one per frame.
template <bool RV, bool U, bool SS>
__global__ MAPLE_APPEND_ATTR void k_append_candset(const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *parent,
                                                   const int32_t *frameIdx, const int32_t *frameLists, int isTip, double bLen,
                                                   double *out)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        out[i] = append_walk(c, list_ref(av, parent[i]), list_ref(av, frameLists[frameIdx[i]]), isTip != 0, bLen);
}

__global__ __launch_bounds__(MAPLE_BLOCK) void k_minor_candset(int lRef, ArenaView av, int n, const int32_t *l1,
                                                               const int32_t *frameIdx, const int32_t *frameLists,
                                                               int onlyIdentical, uint8_t *out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        out[i] = (uint8_t)minor_walk(lRef, list_ref(av, l1[i]), list_ref(av, frameLists[frameIdx[i]]), onlyIdentical != 0);
}

__global__ __launch_bounds__(MAPLE_BLOCK) void k_minor(int lRef, ArenaView av, int n, const int32_t *l1, const int32_t *l2,
                                                       int onlyIdentical, uint8_t *out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        out[i] = (uint8_t)minor_walk(lRef, list_ref(av, l1[i]), list_ref(av, l2[i]), onlyIdentical != 0);
}

__global__ __launch_bounds__(MAPLE_BLOCK) void k_pass(int lRef, ArenaView av, MutView mv, int n, const int32_t *l,
                                                      const int32_t *ml, const uint8_t *up, OutSpec o)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        Writer w;
        w.init(o.words + o.woff[i], o.aux + o.aoff[i]);
        int id = ml[i];
        int r = pass_walk(lRef, list_ref(av, l[i]), mv.mut3 + 3 * mv.off[id], mv.cnt[id], up[i] != 0, w);
        o.n_ent[i] = r;
        o.n_aux[i] = w.na;
    }
}

template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(MAPLE_BLOCK) void k_shorten(const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *l, OutSpec o)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        Writer w;
        w.init(o.words + o.woff[i], o.aux + o.aoff[i]);
        o.n_ent[i] = shorten_walk(c, list_ref(av, l[i]), av.n_ent[l[i]], w);
        o.n_aux[i] = w.na;
    }
}


// The explicit-pair operators by one wavefront per pair, for the few pairs of a single reference call (mergeVectors without
// the likelihood, estimateBranchLengthWithDerivative; appendProbNode: k_wave_append below): same results, a fifth of the wait.
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(64) void k_merge_wave(const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *l1,
                                                   const double *b1, const uint8_t *t1, const int32_t *l2, const double *b2,
                                                   const uint8_t *t2, const uint8_t *ud, OutSpec o)
{
    __shared__ Lds lds;
    __shared__ WaveUpdLdsStd L;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    const int lane = threadIdx.x;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int id1 = l1[i], id2 = l2[i];
        const int n1 = av.n_ent[id1], n2 = av.n_ent[id2];
        uint2 *gw = o.words + o.woff[i];
        double *ga = o.aux + o.aoff[i];
        if (n1 > L.wuIn || n2 > L.wuIn) {
            if (lane == 0) {
                Writer w;
                w.init(gw, ga);
                double lk = 0.0;
                o.n_ent[i] = merge_walk(c, list_ref(av, id1), b1[i], t1[i] != 0, list_ref(av, id2), b2[i], t2[i] != 0, ud[i] != 0, false, 0, 0,
                                        w, &lk);
                o.n_aux[i] = w.na;
            }
            continue;
        }
        wave_sync();
        int na = 0;
        const int r = wave_merge(c, list_ref(av, id1), n1, b1[i], t1[i] != 0, list_ref(av, id2), n2, b2[i], t2[i] != 0, ud[i] != 0, L, na);
        if (r >= 0) {
            for (int k = lane; k < r; k += 64) { const unsigned long long w = L.m[k]; gw[k] = make_uint2((uint32_t)w, (uint32_t)(w >> 32)); }
            for (int k = lane; k < na; k += 64) ga[k] = L.maux[k];
        }
        if (lane == 0) { o.n_ent[i] = r; o.n_aux[i] = r >= 0 ? na : 0; }
    }
}

template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(64) void k_blen_wave(const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *pl,
                                                  const int32_t *cl, const uint8_t *tip, double *ais, const int64_t *aisOff,
                                                  double *t, uint8_t *isFalse)
{
    __shared__ Lds lds;
    __shared__ WaveLdsStd W;
    __shared__ double terms[128];
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int idP = pl[i], idC = cl[i];
        const int nP = av.n_ent[idP], nC = av.n_ent[idC];
        bool f = false;
        double v = 0.0;
        if (nP > W.capW || nC > W.capW) {
            if (threadIdx.x == 0) v = blen_walk(c, list_ref(av, idP), list_ref(av, idC), tip[i] != 0, ais + aisOff[i], 1, &f);
        } else {
            wave_sync();
            v = wave_blen(c, list_ref(av, idP), nP, list_ref(av, idC), nC, tip[i] != 0, W, terms, &f);
        }
        if (threadIdx.x == 0) { t[i] = v; isFalse[i] = f ? 1 : 0; }
    }
}

template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(64) void k_differ_wave(const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *l1, const int32_t *l2,
                                                    uint8_t *out)
{
    __shared__ Lds lds;
    constexpr int cap = WaveUpdLdsStd::cap;                               // (a list that is compared: as many entries as a merged one)
    __shared__ unsigned long long A[cap], B[cap];
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    const int lane = threadIdx.x;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int id1 = l1[i], id2 = l2[i];
        if (id2 < 0) { if (lane == 0) out[i] = 1; continue; }
        const int n1 = av.n_ent[id1], n2 = av.n_ent[id2];
        const ListRef L1 = list_ref(av, id1), L2 = list_ref(av, id2);
        if (n1 > cap || n2 > cap) {
            if (lane == 0) out[i] = differ_walk(c, L1, L2) ? 1 : 0;
            continue;
        }
        wave_sync();
        const unsigned long long *w1 = (const unsigned long long *)L1.w, *w2 = (const unsigned long long *)L2.w;
        for (int k = lane; k < n1; k += 64) A[k] = w1[k];
        for (int k = lane; k < n2; k += 64) B[k] = w2[k];
        wave_sync();
        const bool d = wave_differ(c, A, L1.aux, n1, B, L2.aux, n2);
        if (lane == 0) out[i] = d ? 1 : 0;
    }
}

// appendProbNode by a whole wavefront per pair (wave_dev.h), small batches of maple_append_batch and the hook of the parity tests
// (debug_abi.hip).  No launch bound: the __launch_bounds__(64) this definition used to carry never took effect (a declaration
// without it came first and instantiated the kernel), so the kernel has always been compiled for the default 1024; giving it the
// bound changes its code (the barriers go) and belongs in a change of its own.
template <bool RV, bool U, bool SS>
__global__ void k_wave_append(const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *pl, const int32_t *cl,
                              const uint8_t *tip, const double *bl, double *out)
{
    __shared__ Lds lds;
    __shared__ WaveLdsStd wl;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const double v = wave_append(c, list_ref(av, pl[i]), av.n_ent[pl[i]], list_ref(av, cl[i]), av.n_ent[cl[i]], tip[i] != 0, bl[i], wl);
        if (threadIdx.x == 0) out[i] = v;
        __builtin_amdgcn_wave_barrier();
    }
}
void launch_wave_append(maple_ctx *c, int grid, int n, const int32_t *pl, const int32_t *cl, const uint8_t *tip, const double *bl, double *out)
{
    DISPATCH3(c, k_wave_append, <<<grid, 64, 0, c->stream>>>(c->d_model, view(c), n, pl, cl, tip, bl, out));
}
#define MAPLE_WAVE_PAIRS_MAX 1024        // explicit-pair batches up to this size go one wavefront per pair

// shorten of ONE list per wavefront (wave_shorten, wave_update.h): for the handful of lists a single-query placement shortens
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(64) void k_shorten_wave(const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *l, OutSpec o)
{
    __shared__ Lds lds;
    __shared__ WaveUpdLdsStd L;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    const int lane = threadIdx.x;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int id = l[i], ne = av.n_ent[id], na = av.n_aux[id];
        if (ne > L.cap || na > 5 * L.cap) {
            if (lane == 0) {
                Writer w;
                w.init(o.words + o.woff[i], o.aux + o.aoff[i]);
                o.n_ent[i] = shorten_walk(c, list_ref(av, id), ne, w);
                o.n_aux[i] = w.na;
            }
            continue;
        }
        wave_sync();
        const ListRef src = list_ref(av, id);
        const unsigned long long *sw = (const unsigned long long *)src.w;
        for (int k = lane; k < ne; k += 64) L.m[k] = sw[k];
        for (int k = lane; k < na; k += 64) L.maux[k] = src.aux[k];
        wave_sync();
        int naOut = 0;
        const int r = wave_shorten(c, L, ne, o.words + o.woff[i], o.aux + o.aoff[i], naOut);
        if (lane == 0) { o.n_ent[i] = r; o.n_aux[i] = naOut; }
    }
}

// rootVector: frames up (node..root), root_walk, frames down (root..node), shorten.
// Each item owns 3 scratch lists of `cap` entries: A, B (ping-pong) and the final output slot.
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(MAPLE_BLOCK) void k_root_vector(const DevModel *__restrict__ mp, ArenaView av, MutView mv, int n,
                                                             const int32_t *l, const double *bl, const uint8_t *tip,
                                                             const int64_t *pathOff, const int32_t *pathMut,
                                                             const int64_t *capOff, OutSpec o)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int64_t cap = capOff[i + 1] - capOff[i];
        // o.woff[i] addresses 3*cap words; o.aoff[i] addresses 3*5*cap doubles
        uint2 *W[3] = {o.words + o.woff[i], o.words + o.woff[i] + cap, o.words + o.woff[i] + 2 * cap};
        double *A[3] = {o.aux + o.aoff[i], o.aux + o.aoff[i] + 5 * cap, o.aux + o.aoff[i] + 10 * cap};
        ListRef cur = list_ref(av, l[i]);
        int curN = av.n_ent[l[i]];
        int slot = 1;                  // next buffer to write (1 or 2); slot 0 is reserved for the result
        Writer w;
        for (int64_t k = pathOff[i]; k < pathOff[i + 1]; k++) {
            int id = pathMut[k];
            if (id < 0 || mv.cnt[id] == 0) continue;
            w.init(W[slot], A[slot]);
            curN = pass_walk(m.lRef, cur, mv.mut3 + 3 * mv.off[id], mv.cnt[id], true, w);
            cur = ListRef{W[slot], A[slot]};
            slot = 3 - slot;
        }
        w.init(W[slot], A[slot]);
        curN = root_walk(c, cur, bl[i], tip[i] != 0, w);
        cur = ListRef{W[slot], A[slot]};
        slot = 3 - slot;
        for (int64_t k = pathOff[i + 1] - 1; k >= pathOff[i]; k--) {
            int id = pathMut[k];
            if (id < 0 || mv.cnt[id] == 0) continue;
            w.init(W[slot], A[slot]);
            curN = pass_walk(m.lRef, cur, mv.mut3 + 3 * mv.off[id], mv.cnt[id], false, w);
            cur = ListRef{W[slot], A[slot]};
            slot = 3 - slot;
        }
        w.init(W[0], A[0]);
        o.n_ent[i] = shorten_walk(c, cur, curN, w);
        o.n_aux[i] = w.na;
    }
}

// evaluatePlacement (M:6790-6806): three branch-length solves around three merges, then one append.
// Each item owns 3 scratch lists (capacities capA/capB/capC packed back to back) and an `ais` strip.
#define MAPLE_EVALPLACE_ARGS                                                                                                    \
    const DevModel *__restrict__ mp, ArenaView av, int n, const int32_t *midTot, const int32_t *down, const int32_t *up,        \
        const double *dist, const int32_t *rem, const uint8_t *remTip, const uint8_t *fromTip1, uint2 *sw, double *sa,          \
        const int64_t *capOff, double *ais, const int64_t *aisOff, double *out4, int32_t *status, double *comp2

// comp2 (optional): what the caller compares the optimised placement with (M:8101-8187) -- appendProbNode of the node's
// lower list on its upper list at the branch's own length and at the sum of the two optimised halves.
template <bool RV, bool U, bool SS>
__device__ inline void evalplace_item_lane(const Ctx<RV, U, SS> &c, const ArenaView &av, int i, const int32_t *midTot, const int32_t *down,
                                           const int32_t *up, const double *dist, const int32_t *rem, const uint8_t *remTip,
                                           const uint8_t *fromTip1, uint2 *sw, double *sa, const int64_t *capOff, double *ais,
                                           const int64_t *aisOff, double *out4, int32_t *status, double *comp2)
{
    const DevModel &m = c.m;
    ListRef Lmid = list_ref(av, midTot[i]), Ldown = list_ref(av, down[i]), Lup = list_ref(av, up[i]), Lrem = list_ref(av, rem[i]);
    const int nDown = av.n_ent[down[i]], nUp = av.n_ent[up[i]], nRem = av.n_ent[rem[i]];
    const int64_t base = capOff[i];
    uint2 *wA = sw + base, *wB = wA + (nDown + nRem), *wC = wB + (nUp + nRem);
    double *aA = sa + 5 * base, *aB = aA + 5 * (int64_t)(nDown + nRem), *aC = aB + 5 * (int64_t)(nUp + nRem);
    double *myAis = ais + aisOff[i];
    const bool rt = remTip[i] != 0, ft = fromTip1[i] != 0;
    bool f;
    Writer w;
    status[i] = 0;
    double bestApp = blen_walk(c, Lmid, Lrem, rt, myAis, 1, &f);
    w.init(wA, aA);
    int r = merge_walk(c, Ldown, dist[i] / 2, ft, Lrem, bestApp, rt, false, false, 0, 0, w, nullptr);
    if (r < 0) { status[i] = -1; return; }
    ListRef midLower{wA, aA};
    double bestTop = blen_walk(c, Lup, midLower, false, myAis, 1, &f);
    w.init(wB, aB);
    r = merge_walk(c, Lup, bestTop, false, Lrem, bestApp, rt, true, false, 0, 0, w, nullptr);
    if (r == -1) {
        bestTop = m.defaultBLen * 0.1;
        w.init(wB, aB);
        r = merge_walk(c, Lup, bestTop, false, Lrem, bestApp, rt, true, false, 0, 0, w, nullptr);
    }
    if (r < 0) { status[i] = -1; return; }
    ListRef midTop{wB, aB};
    double bestBottom = blen_walk(c, midTop, Ldown, ft, myAis, 1, &f);
    w.init(wC, aC);
    r = merge_walk(c, Lup, bestTop, false, Ldown, bestBottom, ft, true, false, 0, 0, w, nullptr);
    if (r < 0) { status[i] = -1; return; }
    ListRef newMid{wC, aC};
    out4[i * 4 + 0] = append_walk(c, newMid, Lrem, rt, bestApp);
    out4[i * 4 + 1] = bestBottom;
    out4[i * 4 + 2] = bestTop;
    out4[i * 4 + 3] = bestApp;
    if (comp2) {
        comp2[2 * i] = append_walk(c, Lup, Ldown, ft, dist[i]);
        comp2[2 * i + 1] = append_walk(c, Lup, Ldown, ft, bestBottom + bestTop);
    }
}

template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(MAPLE_BLOCK) void k_evalplace(MAPLE_EVALPLACE_ARGS)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        evalplace_item_lane(c, av, i, midTot, down, up, dist, rem, remTip, fromTip1, sw, sa, capOff, ais, aisOff, out4, status, comp2);
}

// The same by a whole wavefront: the chain of seven list walks (three branch-length solves around three merges, one
// append) is what a single-query placement's refinement waits for -- 50 us per link for one lane, a few us for 64
// (wave_blen / wave_merge, wave_update.h; wave_append, wave_dev.h; every list in LDS).  One wavefront per workgroup.
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(64) void k_evalplace_wave(MAPLE_EVALPLACE_ARGS)
{
    __shared__ Lds lds;
    __shared__ WaveUpdLdsStd L;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    const int lane = threadIdx.x;
    WaveLdsStd &W = *reinterpret_cast<WaveLdsStd *>(L.baux);               // (baux and old are not used by the merges here)
    double *terms = reinterpret_cast<double *>(L.old);
    static_assert(sizeof(WaveLdsStd) <= sizeof(L.baux) && 128 * sizeof(double) <= sizeof(L.old), "LDS aliases");
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int idM = midTot[i], idD = down[i], idU = up[i], idR = rem[i];
        const int nMid = av.n_ent[idM], nDown = av.n_ent[idD], nUp = av.n_ent[idU], nRem = av.n_ent[idR];
        if (nMid > W.capW || nRem > W.capW || nDown + nRem > W.capW || nUp + nRem > W.capW || nUp + nDown > W.capW) {
            if (lane == 0)
                evalplace_item_lane(c, av, i, midTot, down, up, dist, rem, remTip, fromTip1, sw, sa, capOff, ais, aisOff, out4, status,
                                    comp2);
            continue;
        }
        wave_sync();
        const ListRef Lmid = list_ref(av, idM), Ldown = list_ref(av, idD), Lup = list_ref(av, idU), Lrem = list_ref(av, idR);
        const ListRef Lm{(const uint2 *)L.m, L.maux};                      // where the merges leave their result
        const bool rt = remTip[i] != 0, ft = fromTip1[i] != 0;
        const double d = dist[i];
        bool f;
        int na, st = 0;
        double bestApp = wave_blen(c, Lmid, nMid, Lrem, nRem, rt, W, terms, &f), bestTop = 0.0, bestBottom = 0.0, lk = 0.0;
        int r = wave_merge(c, Ldown, nDown, d / 2, ft, Lrem, nRem, bestApp, rt, false, L, na);
        if (r < 0) st = -1;
        if (!st) {
            bestTop = wave_blen(c, Lup, nUp, Lm, r, false, W, terms, &f);
            r = wave_merge(c, Lup, nUp, bestTop, false, Lrem, nRem, bestApp, rt, true, L, na);
            if (r == -1) {
                bestTop = m.defaultBLen * 0.1;
                r = wave_merge(c, Lup, nUp, bestTop, false, Lrem, nRem, bestApp, rt, true, L, na);
            }
            if (r < 0) st = -1;
        }
        if (!st) {
            bestBottom = wave_blen(c, Lm, r, Ldown, nDown, ft, W, terms, &f);
            r = wave_merge(c, Lup, nUp, bestTop, false, Ldown, nDown, bestBottom, ft, true, L, na);
            if (r < 0) st = -1;
        }
        if (!st) lk = wave_append(c, Lm, r, Lrem, nRem, rt, bestApp, W);
        if (lane == 0) {
            status[i] = st;
            if (!st) { out4[i * 4 + 0] = lk; out4[i * 4 + 1] = bestBottom; out4[i * 4 + 2] = bestTop; out4[i * 4 + 3] = bestApp; }
        }
        if (!st && comp2) {
            const double c0 = wave_append(c, Lup, nUp, Ldown, nDown, ft, d, W);
            const double c1 = wave_append(c, Lup, nUp, Ldown, nDown, ft, bestBottom + bestTop, W);
            if (lane == 0) { comp2[2 * i] = c0; comp2[2 * i + 1] = c1; }
        }
    }
}


// compaction of scratch lists into the arena: one wavefront per list, coalesced copies
__global__ __launch_bounds__(MAPLE_BLOCK) void k_commit(int n, const uint2 *sw, const double *sa, const int64_t *swoff,
                                                        const int64_t *saoff, const int32_t *n_ent, const int32_t *n_aux,
                                                        const int64_t *dst_w, const int64_t *dst_a, uint2 *words,
                                                        double *aux, const int32_t *rowId, int64_t *t_ent_off,
                                                        int64_t *t_aux_off, int32_t *t_n_ent, int32_t *t_n_aux)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int i = wave; i < n; i += nwaves) {
        if (n_ent[i] < 0) continue;
        if (rowId && lane == 0 && rowId[i] >= 0) {                         // the new list's row of the list table
            const int r = rowId[i];
            t_ent_off[r] = dst_w[i]; t_aux_off[r] = dst_a[i]; t_n_ent[r] = n_ent[i]; t_n_aux[r] = n_aux[i];
        }
        const uint2 *s = sw + swoff[i];
        uint2 *d = words + dst_w[i];
        for (int k = lane; k < n_ent[i]; k += 64) d[k] = s[k];
        const double *s2 = sa + saoff[i];
        double *d2 = aux + dst_a[i];
        for (int k = lane; k < n_aux[i]; k += 64) d2[k] = s2[k];
    }
}

// =================================================================================================
// host side
// =================================================================================================
extern "C" int maple_abi_version(void) { return MAPLE_ABI_VERSION; }

extern "C" const char *maple_last_error(maple_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

extern "C" int maple_create(maple_ctx **out, int device, int32_t lRef, const uint8_t *refIdx, const double *rootFreqs4,
                            const maple_params *params, uint64_t arena_bytes)
{
    if (!out || !refIdx || !rootFreqs4 || !params || lRef <= 0) return MAPLE_ERR_ARG;
    *out = nullptr;
    maple_ctx *c = new maple_ctx();
    if (const char *e = getenv("MAPLE_DEBUG")) c->tuning.verbose = atoi(e) > 1 ? atoi(e) : 1;   // (the one environment variable: progress lines)
    c->device = device;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0 || device >= ndev) {
        delete c;
        return MAPLE_ERR_HIP;          // no GPU: the product path fails loudly, there is no CPU fallback
    }
    if (hipSetDevice(device) != hipSuccess) { delete c; return MAPLE_ERR_HIP; }
    if (c->stream.create() != hipSuccess) { delete c; return MAPLE_ERR_HIP; }
    c->lRef = lRef;
    c->refIdx.assign(refIdx, refIdx + lRef);
    c->params = *params;
    DevModel &m = c->dm;
    memset(&m, 0, sizeof m);
    m.lRef = lRef;
    for (int i = 0; i < 4; i++) m.rootFreqs[i] = rootFreqs4[i];
    for (int i = 0; i < 4; i++) m.rootFreqsLog[i] = log(rootFreqs4[i]);  // M:3679
    m.globalTotRate = -(double)lRef;                                   // M:3607
    m.minimumCarryOver = DBL_MIN * (1e50);                             // M:3623
    m.thresholdProb = params->thresholdProb;
    double t2 = params->thresholdProb * params->thresholdProb;         // M:3692-3693
    m.thresholdProb4 = t2 * t2;
    m.minBLenSensitivity = params->minBLenSensitivity;
    m.thresholdDiffForUpdate = params->thresholdDiffForUpdate;
    m.thresholdFoldChangeUpdate = params->thresholdFoldChangeUpdate;
    m.defaultBLen = params->defaultBLen;
    if (arena_bytes == 0) arena_bytes = 1ull << 30;
    c->cap_ent = (int64_t)(arena_bytes / 24);
    c->cap_aux = 2 * c->cap_ent;
    c->cap_lists = c->cap_ent / 4 + 1024;
    c->cap_mut = c->cap_ent / 16 + 4096;
    c->cap_mut_lists = c->cap_lists / 4 + 1024;
    bool ok = c->d_words.reserve_exact(c->cap_ent + 64) == hipSuccess
              && c->d_aux.reserve_exact(c->cap_aux) == hipSuccess
              && c->d_ent_off.reserve_exact(c->cap_lists) == hipSuccess
              && c->d_aux_off.reserve_exact(c->cap_lists) == hipSuccess
              && c->d_n_ent.reserve_exact(c->cap_lists) == hipSuccess
              && c->d_n_aux.reserve_exact(c->cap_lists) == hipSuccess
              && c->d_mut3.reserve_exact(c->cap_mut * 3) == hipSuccess
              && c->d_mut_off.reserve_exact(c->cap_mut_lists) == hipSuccess
              && c->d_mut_cnt.reserve_exact(c->cap_mut_lists) == hipSuccess
              && c->d_cumRate.reserve_exact(lRef + 1) == hipSuccess
              && c->d_model.reserve_exact(1) == hipSuccess;
    ok = ok && c->d_cumBases.reserve_exact((size_t)(lRef + 1) * 4) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();       // (the status reports the refused request: left behind as the thread's last error, the next
        maple_destroy(c);              // launch check of another context would find it)
        return MAPLE_ERR_NOMEM;
    }
    {                                                                  // cumulativeBases, M:3669-3674
        std::vector<int32_t> cb((size_t)(lRef + 1) * 4, 0);
        for (int i = 0; i < lRef; i++) {
            for (int k = 0; k < 4; k++) cb[(size_t)(i + 1) * 4 + k] = cb[(size_t)i * 4 + k];
            cb[(size_t)(i + 1) * 4 + refIdx[i]] += 1;
        }
        if (hipMemcpy(c->d_cumBases, cb.data(), cb.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
            maple_destroy(c);
            return MAPLE_ERR_HIP;
        }
        m.cumulativeBases = c->d_cumBases;
    }
    *out = c;
    return MAPLE_OK;
}

extern "C" int maple_set_tuning(maple_ctx *c, const maple_tuning *t)
{
    if (!c || !t) return MAPLE_ERR_ARG;
    if (t->structSize < sizeof(uint32_t) + sizeof(int32_t)) return fail(c, MAPLE_ERR_ARG, "maple_set_tuning: structSize is not set (sizeof(maple_tuning) of the caller's header)");
    const int32_t verbose = c->tuning.verbose;
    maple_tuning mine{};                                              // (what the caller's struct does not reach keeps the library's choice)
    ahead_quiesce(c);
    memcpy(&mine, t, std::min<size_t>(t->structSize, sizeof(maple_tuning)));
    mine.structSize = (uint32_t)sizeof(maple_tuning);
    c->tuning = mine;
    if (!t->verbose && getenv("MAPLE_DEBUG")) c->tuning.verbose = verbose;   // (the environment variable keeps it on)
    return MAPLE_OK;
}

// What cannot be left to the members, before any of them goes: the library's own thread reads what they free, and nothing may be
// in flight on any stream of the context (the frontier tier's side streams live in its scratch: the device-wide wait).
maple_ctx::~maple_ctx()
{
    ahead_quiesce(this);
    if (!stream) return;                                                // (maple_create gave up before it had a device)
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);
    if (stream2) (void)hipStreamSynchronize(stream2);
    (void)hipDeviceSynchronize();
    if (rccl_comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy((ncclComm_t)rccl_comm);
}

extern "C" int maple_destroy(maple_ctx *c)
{
    delete c;
    return MAPLE_OK;
}

extern "C" int maple_set_model(maple_ctx *c, const double *Q16, const double *siteRates, int usingErrorRate,
                               double errorRateGlobal, const double *errorRates)
{
    if (!c || !Q16) return MAPLE_ERR_ARG;
    HIPCK(c, hipSetDevice(c->device));
    DevModel &m = c->dm;
    const int lRef = c->lRef;
    c->h_over_hint.clear();                                           // (which searches run over the budget is a property of the model too)
    ahead_quiesce(c);
    if (c->ahead) c->ahead->active = false;                             // (rows scored under another model)
    for (int i = 0; i < 16; i++) m.Q[i] = Q16[i];
    m.useRateVariation = siteRates ? 1 : 0;
    m.usingErrorRate = usingErrorRate ? 1 : 0;
    m.errorRateSiteSpecific = (usingErrorRate && errorRates) ? 1 : 0;
    m.errorRate = errorRateGlobal;
    // cumulativeRate, M:6350-6370
    c->h_cumRate.assign(lRef + 1, 0.0);
    for (int i = 0; i < lRef; i++) {
        double nm = Q16[c->refIdx[i] * 5];
        c->h_cumRate[i + 1] = siteRates ? c->h_cumRate[i] + nm * siteRates[i] : c->h_cumRate[i] + nm;
    }
    HIPCK(c, hipMemcpyAsync(c->d_cumRate, c->h_cumRate.data(), (lRef + 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    m.cumulativeRate = c->d_cumRate;
    if (siteRates) {
        HIPCK(c, c->d_siteRates.reserve_exact(lRef));
        HIPCK(c, hipMemcpyAsync(c->d_siteRates, siteRates, lRef * sizeof(double), hipMemcpyHostToDevice, c->stream));
        m.siteRates = c->d_siteRates;
    } else m.siteRates = nullptr;
    // cumulativeErrorRate / totError, M:6373-6390
    c->h_cumErr.clear();
    m.cumulativeErrorRate = nullptr;
    m.errorRates = nullptr;
    m.totError = 0.0;
    if (usingErrorRate) {
        if (errorRates) {
            c->h_cumErr.assign(lRef + 1, 0.0);
            for (int i = 0; i < lRef; i++) c->h_cumErr[i + 1] = c->h_cumErr[i] + errorRates[i];
            m.totError = -c->h_cumErr[lRef];
            HIPCK(c, c->d_errorRates.reserve_exact(lRef));
            HIPCK(c, c->d_cumErr.reserve_exact(lRef + 1));
            HIPCK(c, hipMemcpyAsync(c->d_errorRates, errorRates, lRef * sizeof(double), hipMemcpyHostToDevice, c->stream));
            HIPCK(c, hipMemcpyAsync(c->d_cumErr, c->h_cumErr.data(), (lRef + 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
            m.errorRates = c->d_errorRates;
            m.cumulativeErrorRate = c->d_cumErr;
        } else m.totError = -errorRateGlobal * lRef;
    }
    m.rootFreqsLogErrorCumulative = nullptr;
    if (usingErrorRate) {                                              // M:6380-6389 (note the 0.333333 of the table)
        std::vector<double> acc(lRef + 1, 0.0);
        for (int i = 0; i < lRef; i++) {
            double e = errorRates ? errorRates[i] : errorRateGlobal;
            acc[i + 1] = acc[i] + log(m.rootFreqs[c->refIdx[i]] * (1.0 - 1.33333 * e) + 0.333333 * e);
        }
        HIPCK(c, c->d_rflec.reserve_exact(lRef + 1));
        HIPCK(c, hipMemcpy(c->d_rflec, acc.data(), (lRef + 1) * sizeof(double), hipMemcpyHostToDevice));
        m.rootFreqsLogErrorCumulative = c->d_rflec;
    }
    HIPCK(c, hipMemcpyAsync(c->d_model, &c->dm, sizeof(DevModel), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    c->model_set = true;
    return MAPLE_OK;
}

extern "C" int maple_get_model(maple_ctx *c, double *cumulativeRate, double *cumulativeErrorRate, double *totError)
{
    if (!c) return MAPLE_ERR_ARG;
    if (!c->model_set) return fail(c, MAPLE_ERR_STATE, "model not set");
    if (cumulativeRate) memcpy(cumulativeRate, c->h_cumRate.data(), c->h_cumRate.size() * sizeof(double));
    if (cumulativeErrorRate && !c->h_cumErr.empty())
        memcpy(cumulativeErrorRate, c->h_cumErr.data(), c->h_cumErr.size() * sizeof(double));
    if (totError) *totError = c->dm.totError;
    return MAPLE_OK;
}

// ---- arena --------------------------------------------------------------------------------------
static int push_list_rows(maple_ctx *c, int32_t n, const int64_t *ent_off_abs, const int64_t *aux_off_abs,
                          const int32_t *n_ent, const int32_t *n_aux)
{
    int64_t first = (int64_t)c->h_n_ent.size();
    if (first + n > c->cap_lists) return fail(c, MAPLE_ERR_NOMEM, "list table full (%lld)", (long long)c->cap_lists);
    c->h_ent_off.insert(c->h_ent_off.end(), ent_off_abs, ent_off_abs + n);
    c->h_aux_off.insert(c->h_aux_off.end(), aux_off_abs, aux_off_abs + n);
    c->h_n_ent.insert(c->h_n_ent.end(), n_ent, n_ent + n);
    c->h_n_aux.insert(c->h_n_aux.end(), n_aux, n_aux + n);
    HIPCK(c, hipMemcpyAsync(c->d_ent_off + first, ent_off_abs, n * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(c->d_aux_off + first, aux_off_abs, n * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(c->d_n_ent + first, n_ent, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(c->d_n_aux + first, n_aux, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));   // source vectors are caller temporaries
    return MAPLE_OK;
}

extern "C" int maple_lists_upload(maple_ctx *c, int32_t n, const int64_t *ent_off, const int32_t *pos,
                                  const uint32_t *meta, const int64_t *aux_off, const double *aux, int32_t *first_id)
{
    if (!c || n < 0 || !ent_off || !aux_off || !first_id) return MAPLE_ERR_ARG;
    HIPCK(c, hipSetDevice(c->device));
    *first_id = (int32_t)c->h_n_ent.size();
    if (n == 0) return MAPLE_OK;
    const int64_t ne = ent_off[n] - ent_off[0], na = aux_off[n] - aux_off[0];
    if (c->used_ent + ne > c->cap_ent || c->used_aux + na > c->cap_aux)
        return fail(c, MAPLE_ERR_NOMEM, "arena full: need %lld entries / %lld aux", (long long)ne, (long long)na);
    std::vector<uint2> w((size_t)ne);
    for (int64_t k = 0; k < ne; k++) w[k] = make_uint2((uint32_t)pos[ent_off[0] + k], meta[ent_off[0] + k]);
    HIPCK(c, hipMemcpyAsync(c->d_words + c->used_ent, w.data(), ne * sizeof(uint2), hipMemcpyHostToDevice, c->stream));
    if (na) HIPCK(c, hipMemcpyAsync(c->d_aux + c->used_aux, aux + aux_off[0], na * sizeof(double), hipMemcpyHostToDevice, c->stream));
    std::vector<int64_t> eo(n), ao(n);
    std::vector<int32_t> cnt(n), cna(n);
    for (int i = 0; i < n; i++) {
        eo[i] = c->used_ent + (ent_off[i] - ent_off[0]);
        ao[i] = c->used_aux + (aux_off[i] - aux_off[0]);
        cnt[i] = (int32_t)(ent_off[i + 1] - ent_off[i]);
        cna[i] = (int32_t)(aux_off[i + 1] - aux_off[i]);
        if (cnt[i] <= 0) return fail(c, MAPLE_ERR_ARG, "list %d is empty", i);
    }
    int rc = push_list_rows(c, n, eo.data(), ao.data(), cnt.data(), cna.data());
    if (rc) return rc;
    c->used_ent += ne;
    c->used_aux += na;
    return MAPLE_OK;
}



extern "C" int maple_lists_sizes(maple_ctx *c, int32_t n, const int32_t *ids, int32_t *n_ent, int32_t *n_aux)
{
    if (!c || n < 0 || !ids) return MAPLE_ERR_ARG;
    int rc = check_ids(c, n, ids, false, "ids");
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
        if (n_ent) n_ent[i] = c->h_n_ent[ids[i]];
        if (n_aux) n_aux[i] = c->h_n_aux[ids[i]];
    }
    return MAPLE_OK;
}

extern "C" int maple_lists_download(maple_ctx *c, int32_t n, const int32_t *ids, const int64_t *ent_off, int32_t *pos,
                                    uint32_t *meta, const int64_t *aux_off, double *aux)
{
    if (!c || n < 0 || !ids || !ent_off || !aux_off) return MAPLE_ERR_ARG;
    HIPCK(c, hipSetDevice(c->device));
    int rc = check_ids(c, n, ids, false, "ids");
    if (rc) return rc;
    // lists that sit back to back in the arena AND in the caller's buffers (the usual case: a tree's lists, downloaded in id
    // order) move with one copy per run instead of one per list; the copies of up to 32 M entries are queued together and
    // awaited once (a tree whose four kinds of list are interleaved in the arena is millions of one-list runs)
    std::vector<uint2> w;
    struct Run { int first; int64_t ne, wOff; };
    std::vector<Run> runs;
    int i = 0;
    while (i < n) {
        runs.clear();
        int64_t tot = 0;
        const int chunkStart = i;
        while (i < n && tot < ((int64_t)32 << 20) && runs.size() < (size_t)1 << 16) {
            int j = i;
            int64_t ne = 0, na = 0;
            while (j < n) {
                const int id = ids[j];
                if (j > i) {
                    const int pid = ids[j - 1];
                    if (c->h_ent_off[id] != c->h_ent_off[pid] + c->h_n_ent[pid] || c->h_aux_off[id] != c->h_aux_off[pid] + c->h_n_aux[pid]
                        || ent_off[j] != ent_off[j - 1] + c->h_n_ent[pid] || aux_off[j] != aux_off[j - 1] + c->h_n_aux[pid])
                        break;
                }
                ne += c->h_n_ent[id]; na += c->h_n_aux[id];
                j++;
                if (ne > (int64_t)32 << 20) break;
            }
            runs.push_back(Run{i, ne, tot});
            tot += ne;
            const int id0 = ids[i];
            if (na) HIPCK(c, hipMemcpyAsync(aux + aux_off[i], c->d_aux + c->h_aux_off[id0], na * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            i = j;
        }
        (void)chunkStart;
        w.resize((size_t)tot);
        for (const Run &r : runs)
            if (r.ne) HIPCK(c, hipMemcpyAsync(w.data() + r.wOff, c->d_words + c->h_ent_off[ids[r.first]], r.ne * sizeof(uint2), hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        for (const Run &r : runs) {
            const int64_t o = ent_off[r.first];
            for (int64_t k = 0; k < r.ne; k++) { pos[o + k] = (int32_t)w[r.wOff + k].x; meta[o + k] = w[r.wOff + k].y; }
        }
    }
    return MAPLE_OK;
}

extern "C" int maple_set_fatal_policy(maple_ctx *c, int tolerate)
{
    if (!c) return MAPLE_ERR_ARG;
    c->tolerate_fatal = tolerate != 0;
    return MAPLE_OK;
}

// A mark is the number of genome lists in its low 40 bits and the number of MAT mutation lists above: releasing it drops
// both kinds of temporaries.
extern "C" int maple_arena_mark(maple_ctx *c, int64_t *mark)
{
    if (!c || !mark) return MAPLE_ERR_ARG;
    *mark = (int64_t)c->h_n_ent.size() | ((int64_t)c->h_mut_cnt.size() << 40);
    return MAPLE_OK;
}

extern "C" int maple_arena_release(maple_ctx *c, int64_t markBoth)
{
    if (!c || markBoth < 0) return MAPLE_ERR_ARG;
    const int64_t mark = markBoth & (((int64_t)1 << 40) - 1), mmark = markBoth >> 40;
    if (mark > (int64_t)c->h_n_ent.size() || mmark > (int64_t)c->h_mut_cnt.size()) return MAPLE_ERR_ARG;
    if (mmark < (int64_t)c->h_mut_cnt.size()) {
        c->used_mut = c->h_mut_off[mmark];
        c->h_mut_off.resize(mmark); c->h_mut_cnt.resize(mmark);
    }
    if (mark == (int64_t)c->h_n_ent.size()) return MAPLE_OK;
    if (c->ahead) {
        // the traversal made ahead reads its sample's list and the lists of the columns it scores: if one of them goes with the
        // release, the thread is joined before the room can be written again (a release above them -- the per-search mark of the
        // serial loop -- leaves it running)
        PlaceAhead &A = *c->ahead;
        bool reads = A.spec.row >= 0 && A.spec.row < (int32_t)A.q.size() && A.q[A.spec.row] >= mark;
        for (size_t i = 0; !reads && A.spec.row >= 0 && i < A.spec.lists.size(); i++) reads = A.spec.lists[i] >= mark;
        for (size_t i = 0; !reads && A.spec.row >= 0 && i < A.spec.leafLists.size(); i++) reads = A.spec.leafLists[i] >= mark;
        if (reads) ahead_quiesce(c);
        if (A.active)                                                   // (rows of samples whose lists go with the release)
            for (int32_t id : A.q) if (id >= mark) { A.active = false; ahead_quiesce(c); break; }
    }
    if (mark < c->cand_root_end) c->cand_root_end = -1;                 // (the candidates' root-frame copies go with the release)
    if (mark < c->cand_root_top) c->cand_root_mark = c->cand_root_top = -1;
    int64_t ue = c->h_ent_off[mark], ua = c->h_aux_off[mark];
    {   // a list below the mark that maple_lists_update moved to the end of the arena keeps its (new) room
        size_t k = 0;
        for (int32_t id : c->relocated) {
            if (id >= mark) continue;
            ue = std::max<int64_t>(ue, c->h_ent_off[id] + c->h_n_ent[id]);
            ua = std::max<int64_t>(ua, c->h_aux_off[id] + c->h_n_aux[id]);
            c->relocated[k++] = id;
        }
        c->relocated.resize(k);
    }
    c->used_ent = ue;
    c->used_aux = ua;
    c->h_ent_off.resize(mark); c->h_aux_off.resize(mark); c->h_n_ent.resize(mark); c->h_n_aux.resize(mark);
    if (c->place && c->place->rootVect >= mark) c->place->rootVect = -1;     // the cached root vector went with the release
    return MAPLE_OK;
}

// Keep only the lists `live` (ids in any order, no duplicates, -1 entries allowed and kept as -1): they are copied to the
// bottom of the arena in the order given and renumbered 0, 1, 2, ...; newIds[i] = the new id of live[i].  Everything else
// -- every other list id, every arena mark, resident candidate sets and the uploaded tree -- is gone: upload the tree again
// with the new ids.  What a long run of maple_update_partials / single-sample placements needs from time to time: every
// replaced list keeps its room until then.
extern "C" int maple_arena_compact(maple_ctx *c, int64_t nLive, const int32_t *live, int32_t *newIds)
{
    ahead_quiesce(c);
    if (c && c->ahead) c->ahead->active = false;
    if (!c || nLive < 0 || (nLive && (!live || !newIds))) return MAPLE_ERR_ARG;
    HIPCK(c, hipSetDevice(c->device));
    TRY(settle(c));
    const int64_t nl = (int64_t)c->h_n_ent.size();
    std::vector<uint8_t> seen((size_t)nl, 0);
    int64_t totE = 0, totA = 0, m = 0;
    for (int64_t i = 0; i < nLive; i++) {
        if (live[i] == -1) continue;
        if (live[i] < 0 || live[i] >= nl) return fail(c, MAPLE_ERR_ARG, "live[%lld] = %d is not a list id", (long long)i, live[i]);
        if (seen[live[i]]) return fail(c, MAPLE_ERR_ARG, "list %d is named twice", live[i]);
        seen[live[i]] = 1;
        totE += c->h_n_ent[live[i]]; totA += c->h_n_aux[live[i]];
        m++;
    }
    // gather into scratch (one wavefront per list), then one straight copy back to the bottom of the arena
    std::vector<int64_t> srcW((size_t)m), srcA((size_t)m), dstW((size_t)m), dstA((size_t)m);
    std::vector<int32_t> ne((size_t)m), na((size_t)m);
    int64_t e = 0, a = 0, k = 0;
    for (int64_t i = 0; i < nLive; i++) {
        if (live[i] == -1) { newIds[i] = -1; continue; }
        const int32_t id = live[i];
        srcW[k] = c->h_ent_off[id]; srcA[k] = c->h_aux_off[id]; dstW[k] = e; dstA[k] = a; ne[k] = c->h_n_ent[id]; na[k] = c->h_n_aux[id];
        e += ne[k]; a += na[k];
        newIds[i] = (int32_t)k++;
    }
    if (m) {
        HIPCK(c, c->s_words.reserve((size_t)totE));
        HIPCK(c, c->s_aux.reserve((size_t)std::max<int64_t>(totA, 1)));
        for (int b = 0; b < 6; b++) HIPCK(c, c->s_i64[b].reserve((size_t)m));
        HIPCK(c, c->s_i32[2].reserve((size_t)m));
        HIPCK(c, c->s_i32[3].reserve((size_t)m));
        HIPCK(c, hipMemcpyAsync(c->s_i64[0].p, srcW.data(), (size_t)m * 8, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(c->s_i64[1].p, srcA.data(), (size_t)m * 8, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(c->s_i64[2].p, dstW.data(), (size_t)m * 8, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(c->s_i64[3].p, dstA.data(), (size_t)m * 8, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(c->s_i32[2].p, ne.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(c->s_i32[3].p, na.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
        // (k_commit: list i of the source (words, aux) at swoff / saoff -> destination arrays at dst_w / dst_a)
        hipLaunchKernelGGL(k_commit, dim3(grid_for((int)std::min<int64_t>(m, 1 << 20) * 64)), dim3(MAPLE_BLOCK), 0, c->stream, (int)m, c->d_words,
                           c->d_aux, c->s_i64[0].p, c->s_i64[1].p, c->s_i32[2].p, c->s_i32[3].p, c->s_i64[2].p, c->s_i64[3].p, c->s_words.p,
                           c->s_aux.p, (const int32_t *)nullptr, (int64_t *)nullptr, (int64_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr);
        HIPCK(c, hipGetLastError());
        HIPCK(c, hipMemcpyAsync(c->d_words, c->s_words.p, (size_t)totE * sizeof(uint2), hipMemcpyDeviceToDevice, c->stream));
        if (totA) HIPCK(c, hipMemcpyAsync(c->d_aux, c->s_aux.p, (size_t)totA * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(c->d_ent_off, dstW.data(), (size_t)m * 8, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(c->d_aux_off, dstA.data(), (size_t)m * 8, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(c->d_n_ent, ne.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(c->d_n_aux, na.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
    }
    c->h_ent_off.assign(dstW.begin(), dstW.end()); c->h_aux_off.assign(dstA.begin(), dstA.end());
    c->h_n_ent.assign(ne.begin(), ne.end()); c->h_n_aux.assign(na.begin(), na.end());
    c->used_ent = totE; c->used_aux = totA;
    c->relocated.clear();
    c->tree_set = false; c->tree_stale = false; c->nodes_current = false; c->scan_valid = false; c->cand_root_end = -1;
    c->cand_root_mark = c->cand_root_top = -1;                          // (the lists were renumbered)
    if (c->place) { c->place->valid = false; c->place->rootVect = -1; }
    for (auto &cs : c->candsets) cs = maple_ctx::CandSet{};
    return MAPLE_OK;
}

extern "C" int maple_arena_stats(maple_ctx *c, int64_t *n_lists, int64_t *n_entries, int64_t *n_aux, int64_t *cap_entries)
{
    if (!c) return MAPLE_ERR_ARG;
    if (n_lists) *n_lists = (int64_t)c->h_n_ent.size();
    if (n_entries) *n_entries = c->used_ent;
    if (n_aux) *n_aux = c->used_aux;
    if (cap_entries) *cap_entries = c->cap_ent;
    return MAPLE_OK;
}

extern "C" int maple_mutations_upload(maple_ctx *c, int32_t n, const int64_t *off, const int32_t *mut3, int32_t *first_id)
{
    if (!c || n < 0 || !off || !first_id) return MAPLE_ERR_ARG;
    HIPCK(c, hipSetDevice(c->device));
    *first_id = (int32_t)c->h_mut_cnt.size();
    if (n == 0) return MAPLE_OK;
    const int64_t nm = off[n] - off[0];
    if (c->used_mut + nm > c->cap_mut || (int64_t)c->h_mut_cnt.size() + n > c->cap_mut_lists)
        return fail(c, MAPLE_ERR_NOMEM, "mutation arena full");
    if (nm) HIPCK(c, hipMemcpyAsync(c->d_mut3 + 3 * c->used_mut, mut3 + 3 * off[0], nm * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    std::vector<int64_t> o(n);
    std::vector<int32_t> cnt(n);
    for (int i = 0; i < n; i++) { o[i] = c->used_mut + (off[i] - off[0]); cnt[i] = (int32_t)(off[i + 1] - off[i]); }
    int64_t first = *first_id;
    HIPCK(c, hipMemcpyAsync(c->d_mut_off + first, o.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(c->d_mut_cnt + first, cnt.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    c->h_mut_off.insert(c->h_mut_off.end(), o.begin(), o.end());
    c->h_mut_cnt.insert(c->h_mut_cnt.end(), cnt.begin(), cnt.end());
    c->used_mut += nm;
    return MAPLE_OK;
}

// ---- helpers for batch calls -----------------------------------------------------------------------
// Move freshly produced scratch lists into the arena and hand out ids (or -1 for None).  d_woff / d_aoff: the per-item
// scratch offsets, already on the device.  One synchronisation (the sizes come back), then one staged copy (destinations and
// list ids) and the copy kernel, which also writes the new rows of the device-side list table; nothing waits for it.
int commit_lists(maple_ctx *c, int32_t n, const int64_t *d_woff, const int64_t *d_aoff, int32_t *d_n_ent, int32_t *d_n_aux,
                 int32_t *outList, const uint2 *srcW, const double *srcA)
{
    HIPCK(c, c->pin_res.reserve((size_t)2 * n * sizeof(int32_t)));
    int32_t *h = (int32_t *)c->pin_res.p;
    HIPCK(c, hipMemcpyAsync(h, d_n_ent, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(h + n, d_n_aux, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    const std::vector<int32_t> ne(h, h + n), na(h + n, h + 2 * (size_t)n);
    return commit_known(c, n, d_woff, d_aoff, d_n_ent, d_n_aux, ne, na, outList, srcW, srcA);
}

// ... with the sizes already on the host (ne[i] == -1: nothing to commit for item i)
int commit_known(maple_ctx *c, int32_t n, const int64_t *d_woff, const int64_t *d_aoff, const int32_t *d_n_ent,
                        const int32_t *d_n_aux, const std::vector<int32_t> &ne, const std::vector<int32_t> &na, int32_t *outList,
                        const uint2 *srcW, const double *srcA)
{
    if (!srcW) { srcW = c->s_words.p; srcA = c->s_aux.p; }             // the batch operators' shared scratch
    std::vector<int64_t> dw(n, -1), da(n, -1);
    std::vector<int32_t> rowId(n, -1);
    int64_t ue = c->used_ent, ua = c->used_aux;
    const int64_t first = (int64_t)c->h_n_ent.size();
    int32_t next_id = (int32_t)first;
    for (int i = 0; i < n; i++) {
        if (ne[i] == -1) { outList[i] = -1; continue; }
        if (ne[i] < 0) {
            if (c->tolerate_fatal) { outList[i] = -2; continue; }
            return fail(c, MAPLE_ERR_FATAL, "item %d hit a state the reference treats as fatal (%d)", i, ne[i]);
        }
        dw[i] = ue; da[i] = ua;
        ue += ne[i]; ua += na[i];
        rowId[i] = next_id;
        outList[i] = next_id++;
    }
    if (ue > c->cap_ent || ua > c->cap_aux) return fail(c, MAPLE_ERR_NOMEM, "arena full while committing %d lists", n);
    if (next_id > c->cap_lists) return fail(c, MAPLE_ERR_NOMEM, "list table full (%lld)", (long long)c->cap_lists);
    for (int i = 0; i < n; i++) {
        if (rowId[i] < 0) continue;
        c->h_ent_off.push_back(dw[i]); c->h_aux_off.push_back(da[i]); c->h_n_ent.push_back(ne[i]); c->h_n_aux.push_back(na[i]);
    }
    STAGE(d_dw, c, dw.data(), n);
    STAGE(d_da, c, da.data(), n);
    STAGE(d_row, c, rowId.data(), n);
    TRY(stage_flush(c));
    int waves_per_block = MAPLE_BLOCK / 64;
    int g = (n + waves_per_block - 1) / waves_per_block;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_commit, dim3(g), dim3(MAPLE_BLOCK), 0, c->stream, n, srcW, srcA, d_woff, d_aoff, d_n_ent, d_n_aux, d_dw,
                       d_da, c->d_words, c->d_aux, d_row, c->d_ent_off, c->d_aux_off, c->d_n_ent, c->d_n_aux);
    HIPCK(c, hipGetLastError());
    c->used_ent = ue;
    c->used_aux = ua;
    c->commit_pending = true;
    return MAPLE_OK;
}

// lists committed on the library's stream are not yet visible to work on another stream: wait once
int settle(maple_ctx *c)
{
    if (c->commit_pending) { HIPCK(c, hipStreamSynchronize(c->stream)); c->commit_pending = false; }
    return MAPLE_OK;
}

__global__ void k_set_rows(int n, const int32_t *ids, const int64_t *eo, const int64_t *ao, const int32_t *ne, const int32_t *na,
                           int64_t *t_ent_off, int64_t *t_aux_off, int32_t *t_n_ent, int32_t *t_n_aux)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const int r = ids[i]; t_ent_off[r] = eo[i]; t_aux_off[r] = ao[i]; t_n_ent[r] = ne[i]; t_n_aux[r] = na[i]; }
}

// maple_lists_update keeps ids: the placement search's columns that read one of the rewritten lists score something new.  Score rows
// made ahead note them as changed (maple_tree_patch does the same for the nodes it is given), and the root vector of a rewritten
// root list is made again.
static void lists_update_mark_rows(maple_ctx *c, int32_t n, const int32_t *ids)
{
    if (!c->place || !c->place->valid || !c->tree_set) return;
    PlaceMeta &M = *c->place;
    std::vector<int32_t> s(ids, ids + n);
    std::sort(s.begin(), s.end());
    auto has = [&](int32_t id) { return id >= 0 && std::binary_search(s.begin(), s.end(), id); };
    PlaceAhead *const ah = (c->ahead && c->ahead->active) ? c->ahead.get() : nullptr;
    const int32_t root = c->dtree.root;
    if (root >= 0 && (size_t)root < c->h_tree_lower.size() && has(c->h_tree_lower[root])) {
        M.rootVect = -1;
        if (ah) ah->rootDirty = true;
    }
    if (!ah) return;
    for (size_t col = 0; col < M.h_candList.size(); col++)
        if (has(M.h_candList[col])) { if ((int64_t)col >= ah->ld - 1) ah->active = false; else ah->dirtyCols.push_back((int32_t)col); }
    for (size_t lc = 0; lc < M.h_leafList.size(); lc++)
        if (has(M.h_leafList[lc])) { if ((int64_t)lc >= ah->ldL) ah->active = false; else ah->dirtyLeaves.push_back((int32_t)lc); }
}

// New contents for EXISTING lists: ids[i] keeps its number (every table that refers to it -- tree columns, candidate sets,
// an uploaded tree -- stays valid) and from now on names the new words.  A list that fits in the room of the old one is
// overwritten in place; otherwise it gets fresh room at the end of the arena (the old room is given back by the next
// maple_arena_release past it, like everything else in a bump arena).
extern "C" int maple_lists_update(maple_ctx *c, int32_t n, const int32_t *ids, const int64_t *ent_off, const int32_t *pos,
                                  const uint32_t *meta, const int64_t *aux_off, const double *aux)
{
    if (!c || n < 0 || !ids || !ent_off || !aux_off || (n && (!pos || !meta))) return MAPLE_ERR_ARG;
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(check_ids(c, n, ids, false, "list"));
    ahead_quiesce(c);                                                   // (the words of a list the library's thread may be reading)
    lists_update_mark_rows(c, n, ids);
    std::vector<int64_t> eo(n), ao(n);
    std::vector<int32_t> cnt(n), cna(n);
    int64_t ue = c->used_ent, ua = c->used_aux;
    for (int i = 0; i < n; i++) {
        cnt[i] = (int32_t)(ent_off[i + 1] - ent_off[i]);
        cna[i] = (int32_t)(aux_off[i + 1] - aux_off[i]);
        if (cnt[i] <= 0) return fail(c, MAPLE_ERR_ARG, "list %d is empty", i);
        const int32_t id = ids[i];
        if (cnt[i] <= c->h_n_ent[id] && cna[i] <= c->h_n_aux[id]) { eo[i] = c->h_ent_off[id]; ao[i] = c->h_aux_off[id]; }
        else { eo[i] = ue; ao[i] = ua; ue += cnt[i]; ua += cna[i]; }
    }
    if (ue > c->cap_ent || ua > c->cap_aux) return fail(c, MAPLE_ERR_NOMEM, "arena full while updating %d lists", n);
    // (maple_arena_release must not free their room; a list relocated again and again is listed once: the list is kept sorted)
    for (int i = 0; i < n; i++)
        if (eo[i] >= c->used_ent) {
            auto at = std::lower_bound(c->relocated.begin(), c->relocated.end(), ids[i]);
            if (at == c->relocated.end() || *at != ids[i]) c->relocated.insert(at, ids[i]);
        }
    TRY(settle(c));
    std::vector<uint2> w;
    for (int i = 0; i < n; i++) {
        w.resize((size_t)cnt[i]);
        for (int k = 0; k < cnt[i]; k++) w[k] = make_uint2((uint32_t)pos[ent_off[i] + k], meta[ent_off[i] + k]);
        HIPCK(c, hipMemcpyAsync(c->d_words + eo[i], w.data(), (size_t)cnt[i] * sizeof(uint2), hipMemcpyHostToDevice, c->stream));
        if (cna[i]) HIPCK(c, hipMemcpyAsync(c->d_aux + ao[i], aux + aux_off[i], (size_t)cna[i] * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));                       // (w is reused)
        const int32_t id = ids[i];
        c->h_ent_off[id] = eo[i]; c->h_aux_off[id] = ao[i]; c->h_n_ent[id] = cnt[i]; c->h_n_aux[id] = cna[i];
    }
    TRY(stage_begin(c, (size_t)n * 32 + 256));
    STAGE(dids, c, ids, n); STAGE(deo, c, eo.data(), n); STAGE(dao, c, ao.data(), n); STAGE(dne, c, cnt.data(), n); STAGE(dna, c, cna.data(), n);
    TRY(stage_flush(c));
    hipLaunchKernelGGL(k_set_rows, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, dids, deo, dao, dne, dna, c->d_ent_off,
                       c->d_aux_off, c->d_n_ent, c->d_n_aux);
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipStreamSynchronize(c->stream));
    c->used_ent = ue;
    c->used_aux = ua;
    return MAPLE_OK;
}

// ---- batched operators -----------------------------------------------------------------------------
extern "C" int maple_append_batch(maple_ctx *c, int32_t n, const int32_t *pl, const int32_t *cl, const uint8_t *tip,
                                  const double *bl, double *out)
{
    if (!c || n < 0 || !pl || !cl || !tip || !bl || !out) return MAPLE_ERR_ARG;
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(need_model(c));
    TRY(check_ids(c, n, pl, false, "parentList"));
    TRY(check_ids(c, n, cl, false, "childList"));
    TRY(stage_begin(c, (size_t)n * 32 + 256));
    STAGE(dpl, c, pl, n); STAGE(dcl, c, cl, n); STAGE(dtip, c, tip, n); STAGE(dbl, c, bl, n);
    TRY(stage_flush(c));
    HIPCK(c, c->s_f64[1].reserve(n));
    if (n <= wave_item_max(c, MAPLE_WAVE_PAIRS_MAX))
        launch_wave_append(c, n, n, dpl, dcl, dtip, dbl, c->s_f64[1].p);
    else
        DISPATCH3(c, k_append, <<<grid_for(n), MAPLE_BLOCK, 0, c->stream>>>(c->d_model, view(c), n, dpl, dcl, dtip, dbl, c->s_f64[1].p));
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(out, c->s_f64[1].p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return MAPLE_OK;
}

extern "C" int maple_merge_batch(maple_ctx *c, int32_t n, const int32_t *l1, const double *b1, const uint8_t *t1,
                                 const int32_t *l2, const double *b2, const uint8_t *t2, const uint8_t *ud,
                                 const int32_t *nm1, const int32_t *nm2, int32_t *outList, double *outLK)
{
    if (!c || n < 0 || !l1 || !b1 || !t1 || !l2 || !b2 || !t2 || !ud || !outList) return MAPLE_ERR_ARG;
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(need_model(c));
    TRY(check_ids(c, n, l1, false, "list1"));
    TRY(check_ids(c, n, l2, false, "list2"));
    std::vector<int64_t> woff(n), aoff(n);
    int64_t tot = 0;
    for (int i = 0; i < n; i++) {
        woff[i] = tot; aoff[i] = 5 * tot;
        tot += (int64_t)c->h_n_ent[l1[i]] + c->h_n_ent[l2[i]];
    }
    HIPCK(c, c->s_words.reserve((size_t)tot));
    HIPCK(c, c->s_aux.reserve((size_t)(5 * tot)));
    TRY(stage_begin(c, (size_t)n * 96 + 512));
    STAGE(dl1, c, l1, n); STAGE(dl2, c, l2, n); STAGE(db1, c, b1, n); STAGE(db2, c, b2, n);
    STAGE(dt1, c, t1, n); STAGE(dt2, c, t2, n); STAGE(dud, c, ud, n);
    const int32_t *dnm1 = nullptr, *dnm2 = nullptr;
    if (nm1) { STAGE(p1, c, nm1, n); dnm1 = p1; }
    if (nm2) { STAGE(p2, c, nm2, n); dnm2 = p2; }
    STAGE(dwo, c, woff.data(), n); STAGE(dao, c, aoff.data(), n);
    TRY(stage_flush(c));
    HIPCK(c, c->s_i32[2].reserve(n));
    HIPCK(c, c->s_i32[3].reserve(n));
    double *dlk = nullptr;
    if (outLK) { HIPCK(c, c->s_f64[2].reserve(n)); dlk = c->s_f64[2].p; }
    OutSpec o{c->s_words.p, c->s_aux.p, dwo, dao, c->s_i32[2].p, c->s_i32[3].p};
    if (!outLK && n <= wave_item_max(c, MAPLE_WAVE_PAIRS_MAX))
        DISPATCH3(c, k_merge_wave, <<<n, 64, 0, c->stream>>>(c->d_model, view(c), n, dl1, db1, dt1, dl2, db2, dt2, dud, o));
    else
        DISPATCH3(c, k_merge, <<<grid_for(n), MAPLE_BLOCK, 0, c->stream>>>(c->d_model, view(c), n, dl1, db1, dt1, dl2, db2, dt2, dud, dnm1,
                                                                             dnm2, o, dlk));
    HIPCK(c, hipGetLastError());
    if (outLK) HIPCK(c, hipMemcpyAsync(outLK, dlk, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return commit_lists(c, n, dwo, dao, c->s_i32[2].p, c->s_i32[3].p, outList);
}

extern "C" int maple_blen_batch(maple_ctx *c, int32_t n, const int32_t *pl, const int32_t *cl, const uint8_t *tip,
                                double *t, uint8_t *isFalse)
{
    if (!c || n < 0 || !pl || !cl || !tip || !t || !isFalse) return MAPLE_ERR_ARG;
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(need_model(c));
    TRY(check_ids(c, n, pl, false, "parentList"));
    TRY(check_ids(c, n, cl, false, "childList"));
    std::vector<int64_t> aoff(n);
    int64_t tot = 0;
    for (int i = 0; i < n; i++) { aoff[i] = tot; tot += (int64_t)c->h_n_ent[pl[i]] + c->h_n_ent[cl[i]]; }
    HIPCK(c, c->s_ais.reserve((size_t)tot));
    TRY(stage_begin(c, (size_t)n * 32 + 256));
    STAGE(dpl, c, pl, n); STAGE(dcl, c, cl, n); STAGE(dtip, c, tip, n); STAGE(dao, c, aoff.data(), n);
    TRY(stage_flush(c));
    HIPCK(c, c->s_f64[0].reserve(n));
    HIPCK(c, c->s_u8[1].reserve(n));
    if (n <= wave_item_max(c, MAPLE_WAVE_PAIRS_MAX))
        DISPATCH3(c, k_blen_wave, <<<n, 64, 0, c->stream>>>(c->d_model, view(c), n, dpl, dcl, dtip, c->s_ais.p, dao, c->s_f64[0].p,
                                                             c->s_u8[1].p));
    else
        DISPATCH3(c, k_blen, <<<grid_for(n), MAPLE_BLOCK, 0, c->stream>>>(c->d_model, view(c), n, dpl, dcl, dtip, c->s_ais.p, dao,
                                                                            c->s_f64[0].p, c->s_u8[1].p));
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(t, c->s_f64[0].p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(isFalse, c->s_u8[1].p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return MAPLE_OK;
}

extern "C" int maple_differ_batch(maple_ctx *c, int32_t n, const int32_t *l1, const int32_t *l2, uint8_t *out)
{
    if (!c || n < 0 || !l1 || !l2 || !out) return MAPLE_ERR_ARG;
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(need_model(c));
    TRY(check_ids(c, n, l1, false, "list1"));
    TRY(check_ids(c, n, l2, true, "list2"));
    TRY(stage_begin(c, (size_t)n * 8 + 128));
    STAGE(dl1, c, l1, n); STAGE(dl2, c, l2, n);
    TRY(stage_flush(c));
    HIPCK(c, c->s_u8[0].reserve(n));
    if (n <= wave_item_max(c, MAPLE_WAVE_PAIRS_MAX))
        DISPATCH3(c, k_differ_wave, <<<n, 64, 0, c->stream>>>(c->d_model, view(c), n, dl1, dl2, c->s_u8[0].p));
    else
        DISPATCH3(c, k_differ, <<<grid_for(n), MAPLE_BLOCK, 0, c->stream>>>(c->d_model, view(c), n, dl1, dl2, c->s_u8[0].p));
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(out, c->s_u8[0].p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return MAPLE_OK;
}

// ---- resident candidate sets (placement of one query at a time against the whole tree) --------------------------
extern "C" int maple_candset_create(maple_ctx *c, int32_t n, const int32_t *lists, const int32_t *frameIdx, int32_t nFrames,
                                    int32_t *setId)
{
    if (!c || n <= 0 || !lists || !frameIdx || nFrames <= 0 || !setId) return MAPLE_ERR_ARG;
    HIPCK(c, hipSetDevice(c->device));
    TRY(check_ids(c, n, lists, false, "lists"));
    for (int i = 0; i < n; i++)
        if (frameIdx[i] < 0 || frameIdx[i] >= nFrames) return fail(c, MAPLE_ERR_ARG, "frameIdx[%d] out of range", i);
    maple_ctx::CandSet cs;
    cs.n = n; cs.nFrames = nFrames;
    HIPCK(c, cs.lists.reserve_exact(n));
    HIPCK(c, cs.frame.reserve_exact(n));
    HIPCK(c, hipMemcpy(cs.lists, lists, n * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCK(c, hipMemcpy(cs.frame, frameIdx, n * sizeof(int32_t), hipMemcpyHostToDevice));
    *setId = (int32_t)c->candsets.size();
    c->candsets.push_back(std::move(cs));
    return MAPLE_OK;
}

extern "C" int maple_candset_destroy(maple_ctx *c, int32_t setId)
{
    if (!c || setId < 0 || setId >= (int32_t)c->candsets.size()) return MAPLE_ERR_ARG;
    HIPCK(c, hipSetDevice(c->device));
    auto &cs = c->candsets[setId];
    cs.lists.release(); cs.frame.release();
    cs.n = 0;
    return MAPLE_OK;
}

extern "C" int maple_append_candset(maple_ctx *c, int32_t setId, const int32_t *frameLists, int isTipC, double bLen, double *out)
{
    if (!c || setId < 0 || setId >= (int32_t)c->candsets.size() || !frameLists || !out) return MAPLE_ERR_ARG;
    HIPCK(c, hipSetDevice(c->device));
    TRY(need_model(c));
    const auto &cs = c->candsets[setId];
    if (!cs.lists) return fail(c, MAPLE_ERR_ARG, "candidate set %d has been destroyed", setId);
    TRY(check_ids(c, cs.nFrames, frameLists, false, "frameLists"));
    TRY(h2d(c, c->s_i32[0], frameLists, (size_t)cs.nFrames));
    HIPCK(c, c->s_f64[0].reserve(cs.n));
    hipEvent_t e0, e1;
    TRY(ev_pair(c, &e0, &e1, MAPLE_K_OTHER, (double)cs.n, 0.0));
    HIPCK(c, hipEventRecord(e0, c->stream));
    DISPATCH3(c, k_append_candset, <<<grid_for(cs.n), MAPLE_BLOCK, 0, c->stream>>>(c->d_model, view(c), cs.n, cs.lists, cs.frame,
                                                                                  c->s_i32[0].p, isTipC, bLen, c->s_f64[0].p));
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipEventRecord(e1, c->stream));
    HIPCK(c, hipMemcpyAsync(out, c->s_f64[0].p, cs.n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return MAPLE_OK;
}

extern "C" int maple_minor_candset(maple_ctx *c, int32_t setId, const int32_t *frameLists, int onlyFindIdentical, uint8_t *out)
{
    if (!c || setId < 0 || setId >= (int32_t)c->candsets.size() || !frameLists || !out) return MAPLE_ERR_ARG;
    HIPCK(c, hipSetDevice(c->device));
    const auto &cs = c->candsets[setId];
    if (!cs.lists) return fail(c, MAPLE_ERR_ARG, "candidate set %d has been destroyed", setId);
    TRY(check_ids(c, cs.nFrames, frameLists, false, "frameLists"));
    TRY(h2d(c, c->s_i32[0], frameLists, (size_t)cs.nFrames));
    HIPCK(c, c->s_u8[0].reserve(cs.n));
    hipLaunchKernelGGL(k_minor_candset, dim3(grid_for(cs.n)), dim3(MAPLE_BLOCK), 0, c->stream, c->lRef, view(c), cs.n, cs.lists,
                       cs.frame, c->s_i32[0].p, onlyFindIdentical, c->s_u8[0].p);
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(out, c->s_u8[0].p, cs.n, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return MAPLE_OK;
}

extern "C" int maple_root_prob_batch(maple_ctx *c, int32_t n, const int32_t *l, double *out)
{
    if (!c || n < 0 || !l || !out) return MAPLE_ERR_ARG;
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(need_model(c));
    TRY(check_ids(c, n, l, false, "list"));
    TRY(h2d(c, c->s_i32[0], l, (size_t)n));
    HIPCK(c, c->s_f64[0].reserve(n));
    DISPATCH3(c, k_root_prob, <<<grid_for(n), MAPLE_BLOCK, 0, c->stream>>>(c->d_model, view(c), n, c->s_i32[0].p, c->s_f64[0].p));
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(out, c->s_f64[0].p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return MAPLE_OK;
}

extern "C" int maple_minor_batch(maple_ctx *c, int32_t n, const int32_t *l1, const int32_t *l2, int onlyFindIdentical,
                                 uint8_t *out)
{
    if (!c || n < 0 || !l1 || !l2 || !out) return MAPLE_ERR_ARG;
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(check_ids(c, n, l1, false, "list1"));
    TRY(check_ids(c, n, l2, false, "list2"));
    TRY(h2d(c, c->s_i32[0], l1, (size_t)n));
    TRY(h2d(c, c->s_i32[1], l2, (size_t)n));
    HIPCK(c, c->s_u8[0].reserve(n));
    hipLaunchKernelGGL(k_minor, dim3(grid_for(n)), dim3(MAPLE_BLOCK), 0, c->stream, c->lRef, view(c), n, c->s_i32[0].p,
                       c->s_i32[1].p, onlyFindIdentical, c->s_u8[0].p);
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(out, c->s_u8[0].p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return MAPLE_OK;
}

extern "C" int maple_pass_branch_batch(maple_ctx *c, int32_t n, const int32_t *l, const int32_t *ml, const uint8_t *up,
                                       int32_t *outList)
{
    if (!c || n < 0 || !l || !ml || !up || !outList) return MAPLE_ERR_ARG;
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(check_ids(c, n, l, false, "list"));
    const int32_t nml = (int32_t)c->h_mut_cnt.size();
    std::vector<int64_t> woff(n), aoff(n);
    int64_t tot = 0;
    for (int i = 0; i < n; i++) {
        if (ml[i] < 0 || ml[i] >= nml) return fail(c, MAPLE_ERR_ARG, "mutList[%d] = %d is not a mutation-list id", i, ml[i]);
        woff[i] = tot; aoff[i] = 5 * tot;
        tot += (int64_t)c->h_n_ent[l[i]] + 2 * (int64_t)c->h_mut_cnt[ml[i]];
    }
    HIPCK(c, c->s_words.reserve((size_t)tot));
    HIPCK(c, c->s_aux.reserve((size_t)(5 * tot)));
    TRY(stage_begin(c, (size_t)n * 64 + 256));
    STAGE(dl, c, l, n); STAGE(dml, c, ml, n); STAGE(dup, c, up, n); STAGE(dwo, c, woff.data(), n); STAGE(dao, c, aoff.data(), n);
    TRY(stage_flush(c));
    HIPCK(c, c->s_i32[2].reserve(n));
    HIPCK(c, c->s_i32[3].reserve(n));
    OutSpec o{c->s_words.p, c->s_aux.p, dwo, dao, c->s_i32[2].p, c->s_i32[3].p};
    hipLaunchKernelGGL(k_pass, dim3(grid_for(n)), dim3(MAPLE_BLOCK), 0, c->stream, c->lRef, view(c), mview(c), n, dl, dml, dup, o);
    HIPCK(c, hipGetLastError());
    return commit_lists(c, n, dwo, dao, c->s_i32[2].p, c->s_i32[3].p, outList);
}

extern "C" int maple_shorten_batch(maple_ctx *c, int32_t n, const int32_t *l, int32_t *outList)
{
    if (!c || n < 0 || !l || !outList) return MAPLE_ERR_ARG;
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(need_model(c));
    TRY(check_ids(c, n, l, false, "list"));
    std::vector<int64_t> woff(n), aoff(n);
    int64_t tot = 0;
    for (int i = 0; i < n; i++) { woff[i] = tot; aoff[i] = 5 * tot; tot += c->h_n_ent[l[i]]; }
    HIPCK(c, c->s_words.reserve((size_t)tot));
    HIPCK(c, c->s_aux.reserve((size_t)(5 * tot)));
    TRY(stage_begin(c, (size_t)n * 56 + 256));
    STAGE(dl, c, l, n); STAGE(dwo, c, woff.data(), n); STAGE(dao, c, aoff.data(), n);
    TRY(stage_flush(c));
    HIPCK(c, c->s_i32[2].reserve(n));
    HIPCK(c, c->s_i32[3].reserve(n));
    OutSpec o{c->s_words.p, c->s_aux.p, dwo, dao, c->s_i32[2].p, c->s_i32[3].p};
    if (n <= wave_item_max(c, 1024))
        DISPATCH3(c, k_shorten_wave, <<<n, 64, 0, c->stream>>>(c->d_model, view(c), n, dl, o));
    else
        DISPATCH3(c, k_shorten, <<<grid_for(n), MAPLE_BLOCK, 0, c->stream>>>(c->d_model, view(c), n, dl, o));
    HIPCK(c, hipGetLastError());
    return commit_lists(c, n, dwo, dao, c->s_i32[2].p, c->s_i32[3].p, outList);
}

extern "C" int maple_root_vector_batch(maple_ctx *c, int32_t n, const int32_t *l, const double *bl, const uint8_t *tip,
                                       const int64_t *pathOff, const int32_t *pathMut, int32_t *outList)
{
    if (!c || n < 0 || !l || !bl || !tip || !pathOff || !outList) return MAPLE_ERR_ARG;
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(need_model(c));
    TRY(check_ids(c, n, l, false, "list"));
    const int32_t nml = (int32_t)c->h_mut_cnt.size();
    std::vector<int64_t> capOff(n + 1), woff(n), aoff(n);
    int64_t tot = 0;
    for (int i = 0; i < n; i++) {
        int64_t cap = c->h_n_ent[l[i]];
        for (int64_t k = pathOff[i]; k < pathOff[i + 1]; k++) {
            if (pathMut[k] >= nml) return fail(c, MAPLE_ERR_ARG, "pathMutLists[%lld] is not a mutation-list id", (long long)k);
            if (pathMut[k] >= 0) cap += 4 * (int64_t)c->h_mut_cnt[pathMut[k]];
        }
        capOff[i] = tot; woff[i] = 3 * tot; aoff[i] = 15 * tot;
        tot += cap;
    }
    capOff[n] = tot;
    HIPCK(c, c->s_words.reserve((size_t)(3 * tot)));
    HIPCK(c, c->s_aux.reserve((size_t)(15 * tot)));
    const int64_t np = pathOff[n];
    TRY(stage_begin(c, (size_t)n * 96 + (size_t)np * 4 + 512));
    STAGE(dl, c, l, n); STAGE(dbl, c, bl, n); STAGE(dtip, c, tip, n); STAGE(dwo, c, woff.data(), n); STAGE(dao, c, aoff.data(), n);
    STAGE(dpo, c, pathOff, n + 1); STAGE(dpm, c, pathMut, np); STAGE(dco, c, capOff.data(), n + 1);
    TRY(stage_flush(c));
    HIPCK(c, c->s_i32[2].reserve(n));
    HIPCK(c, c->s_i32[3].reserve(n));
    OutSpec o{c->s_words.p, c->s_aux.p, dwo, dao, c->s_i32[2].p, c->s_i32[3].p};
    DISPATCH3(c, k_root_vector, <<<grid_for(n), MAPLE_BLOCK, 0, c->stream>>>(c->d_model, view(c), mview(c), n, dl, dbl, dtip, dpo, dpm,
                                                                               dco, o));
    HIPCK(c, hipGetLastError());
    return commit_lists(c, n, dwo, dao, c->s_i32[2].p, c->s_i32[3].p, outList);
}

// comp2 (optional, 2 doubles per item): see k_evalplace
int evaluate_placement_items(maple_ctx *c, int32_t n, const int32_t *midTot, const int32_t *down, const int32_t *up,
                                    const double *dist, const int32_t *rem, const uint8_t *remTip, const uint8_t *fromTip1,
                                    double *out4, double *comp2)
{
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(need_model(c));
    TRY(check_ids(c, n, midTot, false, "midTot"));
    TRY(check_ids(c, n, down, false, "downVect"));
    TRY(check_ids(c, n, up, false, "upVect"));
    TRY(check_ids(c, n, rem, false, "removedPartials"));
    std::vector<int64_t> capOff(n), aisOff(n);
    int64_t tot = 0, totA = 0;
    for (int i = 0; i < n; i++) {
        int64_t nd = c->h_n_ent[down[i]], nu = c->h_n_ent[up[i]], nr = c->h_n_ent[rem[i]], nm = c->h_n_ent[midTot[i]];
        capOff[i] = tot;
        tot += (nd + nr) + (nu + nr) + (nu + nd);
        aisOff[i] = totA;
        int64_t mx = nm + nr;
        if (nu + nd + nr > mx) mx = nu + nd + nr;
        if (nu + nr + nd > mx) mx = nu + nr + nd;
        totA += mx;
    }
    HIPCK(c, c->s_words.reserve((size_t)tot));
    HIPCK(c, c->s_aux.reserve((size_t)(5 * tot)));
    HIPCK(c, c->s_ais.reserve((size_t)totA));
    TRY(stage_begin(c, (size_t)n * 64 + 1024));
    STAGE(dMid, c, midTot, n); STAGE(dDown, c, down, n); STAGE(dUp, c, up, n); STAGE(dRem, c, rem, n); STAGE(dDist, c, dist, n);
    STAGE(dRt, c, remTip, n); STAGE(dFt, c, fromTip1, n); STAGE(dCap, c, capOff.data(), n); STAGE(dAis, c, aisOff.data(), n);
    TRY(stage_flush(c));
    HIPCK(c, c->s_f64[1].reserve((size_t)6 * n));
    HIPCK(c, c->s_i32[4].reserve(n));
    double *d4 = c->s_f64[1].p, *d2 = comp2 ? d4 + (size_t)4 * n : nullptr;
    // a handful of items (a single query's short list) wait for ONE item's chain of walks: a wavefront per item
    if (n <= wave_item_max(c, 2048))
        DISPATCH3(c, k_evalplace_wave, <<<n, 64, 0, c->stream>>>(c->d_model, view(c), n, dMid, dDown, dUp, dDist, dRem, dRt, dFt, c->s_words.p,
                                                                  c->s_aux.p, dCap, c->s_ais.p, dAis, d4, c->s_i32[4].p, d2));
    else
        DISPATCH3(c, k_evalplace, <<<grid_for(n), MAPLE_BLOCK, 0, c->stream>>>(c->d_model, view(c), n, dMid, dDown, dUp, dDist, dRem, dRt, dFt,
                                                                                 c->s_words.p, c->s_aux.p, dCap, c->s_ais.p, dAis, d4,
                                                                                 c->s_i32[4].p, d2));
    HIPCK(c, hipGetLastError());
    const size_t nD = (size_t)(comp2 ? 6 : 4) * n;
    HIPCK(c, c->pin_res.reserve(nD * sizeof(double) + (size_t)n * sizeof(int32_t)));
    double *hD = (double *)c->pin_res.p;
    int32_t *st = (int32_t *)(hD + nD);
    HIPCK(c, hipMemcpyAsync(hD, d4, nD * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(st, c->s_i32[4].p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    memcpy(out4, hD, (size_t)4 * n * sizeof(double));
    if (comp2) memcpy(comp2, hD + (size_t)4 * n, (size_t)2 * n * sizeof(double));
    for (int i = 0; i < n; i++)
        if (st[i]) return fail(c, MAPLE_ERR_FATAL, "evaluatePlacement item %d: a merge returned None", i);
    return MAPLE_OK;
}

extern "C" int maple_evaluate_placement_batch(maple_ctx *c, int32_t n, const int32_t *midTot, const int32_t *down,
                                              const int32_t *up, const double *dist, const int32_t *rem,
                                              const uint8_t *remTip, const uint8_t *fromTip1, double *out4)
{
    if (!c || n < 0 || !midTot || !down || !up || !dist || !rem || !remTip || !fromTip1 || !out4) return MAPLE_ERR_ARG;
    return evaluate_placement_items(c, n, midTot, down, up, dist, rem, remTip, fromTip1, out4, nullptr);
}

// ---- device-resident forms ---------------------------------------------------------------------------
int maple_internal_ev_pair(maple_ctx *c, hipEvent_t *a, hipEvent_t *b, int kind, double units, double bytes, size_t *slotOut)
{
    if (c->ev_used >= 65536) c->ev_used = 0;      // nobody is reading these timings: recycle the event pairs
    const size_t slot = c->ev_used / 2;
    if (c->ev_kind.size() <= slot) { c->ev_kind.resize(slot + 1); c->ev_units.resize(slot + 1); c->ev_bytes.resize(slot + 1); }
    c->ev_kind[slot] = kind; c->ev_units[slot] = units; c->ev_bytes[slot] = bytes;
    if (c->ev_used + 2 > c->evs.size()) {
        Event e0, e1;
        HIPCK(c, e0.create());
        HIPCK(c, e1.create());
        c->evs.push_back(std::move(e0));
        c->evs.push_back(std::move(e1));
    }
    *a = c->evs[c->ev_used];
    *b = c->evs[c->ev_used + 1];
    c->ev_used += 2;
    if (slotOut) *slotOut = slot;
    return MAPLE_OK;
}

extern "C" int maple_append_batch_dev(maple_ctx *c, int32_t n, const int32_t *pl, const int32_t *cl, const uint8_t *tip,
                                      const double *bl, double *out, void *stream)
{
    if (!c || n < 0 || !pl || !cl || !tip || !bl || !out) return MAPLE_ERR_ARG;
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(need_model(c));
    TRY(settle(c));
    hipStream_t s = (hipStream_t)stream;                               // the caller's stream, verbatim (NULL = the legacy default stream)
    hipEvent_t e0, e1;
    TRY(ev_pair(c, &e0, &e1, MAPLE_K_APPEND_PAIRS, (double)n, 0.0));
    HIPCK(c, hipEventRecord(e0, s));
    DISPATCH3(c, k_append, <<<grid_for(n), MAPLE_BLOCK, 0, s>>>(c->d_model, view(c), n, pl, cl, tip, bl, out));
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipEventRecord(e1, s));
    return MAPLE_OK;
}


// ---- RCCL: the arg-max over the ranks' candidate shards (SURVEY 8b / 8e level 2) -----------------------------------------
// RCCL is loaded at run time (dlopen: the copy the process already has, e.g. PyTorch's, is reused), so the library itself
// links against nothing but the HIP runtime.  The communicator's unique id travels out of band (the host broadcasts the
// 128 bytes, e.g. with torch.distributed).
static int rccl_load(maple_ctx *c)
{
    if (c->rccl_lib) return MAPLE_OK;
    void *h = nullptr;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (h) break;
    }
    if (!h) return fail(c, MAPLE_ERR_STATE, "RCCL (librccl.so) cannot be loaded: %s", dlerror());
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(h, "ncclCommInitRank");
    g_rccl.AllReduce = (decltype(g_rccl.AllReduce))dlsym(h, "ncclAllReduce");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(h, "ncclCommDestroy");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.CommDestroy)
        return fail(c, MAPLE_ERR_STATE, "librccl.so lacks the expected entry points");
    c->rccl_lib = h;
    return MAPLE_OK;
}
#define NCCLCK(c, call)                                                                                     \
    do {                                                                                                    \
        ncclResult_t r_ = (call);                                                                           \
        if (r_ != ncclSuccess)                                                                              \
            return fail((c), MAPLE_ERR_HIP, "%s failed: %s", #call, g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "?"); \
    } while (0)

extern "C" int maple_comm_unique_id(maple_ctx *c, uint8_t *id128)
{
    if (!c || !id128) return MAPLE_ERR_ARG;
    TRY(rccl_load(c));
    ncclUniqueId id;
    NCCLCK(c, g_rccl.GetUniqueId(&id));
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    memcpy(id128, &id, 128);
    return MAPLE_OK;
}

extern "C" int maple_comm_init(maple_ctx *c, int32_t world, int32_t rank, const uint8_t *id128)
{
    if (!c || world < 1 || rank < 0 || rank >= world || !id128) return MAPLE_ERR_ARG;
    HIPCK(c, hipSetDevice(c->device));
    TRY(rccl_load(c));
    if (c->rccl_comm) { NCCLCK(c, g_rccl.CommDestroy((ncclComm_t)c->rccl_comm)); c->rccl_comm = nullptr; }
    ncclUniqueId id;
    memcpy(&id, id128, 128);
    ncclComm_t comm;
    NCCLCK(c, g_rccl.CommInitRank(&comm, world, id, rank));
    c->rccl_comm = comm; c->rccl_world = world; c->rccl_rank = rank;
    return MAPLE_OK;
}

// order-preserving image of a double in an unsigned 64-bit integer (so that an integer max IS the float max), and back
__device__ inline unsigned long long f64_key(double x)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__global__ void k_argmax_pack(int n, const double *score, unsigned long long *key)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) key[i] = f64_key(score[i]);
}
// after the max all-reduce of the keys: ranks that hold the winning score offer their visit index, the others "infinity"
__global__ void k_argmax_offer(int n, const double *score, const unsigned long long *best, const int32_t *idx, unsigned long long *offer)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) offer[i] = (f64_key(score[i]) == best[i]) ? (unsigned long long)(uint32_t)idx[i] : ~0ull;
}
__global__ void k_argmax_unpack(int n, const unsigned long long *best, const unsigned long long *offer, double *score, int32_t *idx)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const unsigned long long k = best[i];
        const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
        score[i] = __longlong_as_double((long long)b);
        idx[i] = (int32_t)(uint32_t)offer[i];
    }
}

// In place, on `stream`: score[i] = max over ranks, idx[i] = the SMALLEST idx among the ranks that hold that score (the
// earliest depth-first visit wins an exact tie, like the reference's strict >, M:7083 / 8065).  Two all-reduces of n
// 8-byte words over xGMI (max of the order-preserving keys, then min of the offered indices).
extern "C" int maple_argmax_allreduce_dev(maple_ctx *c, int32_t n, double *score_dev, int32_t *idx_dev, void *stream)
{
    if (!c || n < 0 || !score_dev || !idx_dev) return MAPLE_ERR_ARG;
    if (n == 0) return MAPLE_OK;
    if (!c->rccl_comm) return fail(c, MAPLE_ERR_STATE, "maple_comm_init has not been called");
    HIPCK(c, hipSetDevice(c->device));
    HIPCK(c, c->s_comm_u64.reserve((size_t)2 * n));
    unsigned long long *key = c->s_comm_u64.p, *offer = key + n;
    hipStream_t s = (hipStream_t)stream;
    const int g = (n + 255) / 256;
    hipLaunchKernelGGL(k_argmax_pack, dim3(g), dim3(256), 0, s, n, score_dev, key);
    NCCLCK(c, g_rccl.AllReduce(key, key, (size_t)n, ncclUint64, ncclMax, (ncclComm_t)c->rccl_comm, s));
    hipLaunchKernelGGL(k_argmax_offer, dim3(g), dim3(256), 0, s, n, score_dev, key, idx_dev, offer);
    NCCLCK(c, g_rccl.AllReduce(offer, offer, (size_t)n, ncclUint64, ncclMin, (ncclComm_t)c->rccl_comm, s));
    hipLaunchKernelGGL(k_argmax_unpack, dim3(g), dim3(256), 0, s, n, key, offer, score_dev, idx_dev);
    HIPCK(c, hipGetLastError());
    return MAPLE_OK;
}


extern "C" int maple_timing_reset(maple_ctx *c)
{
    if (!c) return MAPLE_ERR_ARG;
    c->ev_used = 0;
    return MAPLE_OK;
}

extern "C" int maple_timing_read_each(maple_ctx *c, int32_t cap, float *ms, int32_t *n_launches)
{
    if (!c || cap < 0 || !ms || !n_launches) return MAPLE_ERR_ARG;
    int k = 0;
    for (size_t i = 0; i + 1 < c->ev_used && k < cap; i += 2, k++) {
        HIPCK(c, hipEventSynchronize(c->evs[i + 1]));
        HIPCK(c, hipEventElapsedTime(&ms[k], c->evs[i], c->evs[i + 1]));
    }
    *n_launches = k;
    return MAPLE_OK;
}

extern "C" int maple_timing_read(maple_ctx *c, int32_t *n_launches, double *total_ms)
{
    if (!c || !n_launches || !total_ms) return MAPLE_ERR_ARG;
    double tot = 0.0;
    for (size_t k = 0; k + 1 < c->ev_used; k += 2) {
        float ms = 0.f;
        HIPCK(c, hipEventSynchronize(c->evs[k + 1]));
        HIPCK(c, hipEventElapsedTime(&ms, c->evs[k], c->evs[k + 1]));
        tot += ms;
    }
    *n_launches = (int32_t)(c->ev_used / 2);
    *total_ms = tot;
    return MAPLE_OK;
}

extern "C" int maple_timing_read_kind(maple_ctx *c, int32_t kind, int32_t *n_launches, double *total_ms, double *units,
                                      double *alg_bytes)
{
    if (!c || !n_launches || !total_ms) return MAPLE_ERR_ARG;
    double tot = 0.0, u = 0.0, b = 0.0;
    int32_t n = 0;
    for (size_t k = 0; k + 1 < c->ev_used; k += 2) {
        if (c->ev_kind[k / 2] != kind) continue;
        float ms = 0.f;
        HIPCK(c, hipEventSynchronize(c->evs[k + 1]));
        HIPCK(c, hipEventElapsedTime(&ms, c->evs[k], c->evs[k + 1]));
        tot += ms; u += c->ev_units[k / 2]; b += c->ev_bytes[k / 2];
        n++;
    }
    *n_launches = n; *total_ms = tot;
    if (units) *units = u;
    if (alg_bytes) *alg_bytes = b;
    return MAPLE_OK;
}

extern "C" int maple_append_algorithmic_bytes(maple_ctx *c, int32_t n, const int32_t *pl, const int32_t *cl,
                                              int child_once, uint64_t *bytes)
{
    if (!c || n < 0 || !pl || !bytes) return MAPLE_ERR_ARG;
    TRY(check_ids(c, n, pl, false, "parentList"));
    uint64_t b = 0;
    // 8 B per entry word + 8 B per aux double (d0/d1 scalars, 4 per O vector) + 8 B result   
    for (int i = 0; i < n; i++) b += 8ull * c->h_n_ent[pl[i]] + 8ull * c->h_n_aux[pl[i]] + 8ull;
    if (cl) {
        if (child_once) b += 8ull * c->h_n_ent[cl[0]] + 8ull * c->h_n_aux[cl[0]];
        else {
            TRY(check_ids(c, n, cl, false, "childList"));
            for (int i = 0; i < n; i++) b += 8ull * c->h_n_ent[cl[i]] + 8ull * c->h_n_aux[cl[i]];
        }
    }
    *bytes = b;
    return MAPLE_OK;
}
