// maple_amd/csrc/debug_abi.hip -- the measurement aids and test hooks of include/maple_hip_debug.h.  Compiled like every other
// unit and linked into libmaple_hip_debug.so only (the product library's objects plus this one).  gfx950 only.
#include "../../include/maple_hip_debug.h"
#include "genome_dev.h"
#include "ctx_host.h"
#include "batch_host.h"
#include "frontier.h"
#include "frontier_dev.h"
#include "witness.h"
#include "update_plan.h"
#include "sweep_plan.h"

#include <algorithm>

using namespace frt;

// Calibration of the FETCH_SIZE counter for THIS library's access pattern (MI355X_MICROARCH.md, HBM section: the
// counter is only calibrated for 16 B/lane coalesced streams).  Every lane walks its own contiguous 512-byte "list"
// with dependent 8-byte loads, exactly like a genome-list walk, over a buffer far larger than the 256 MiB Infinity
// Cache; the byte count is known, so FETCH_SIZE / bytes is the correction factor for k_append*.
__global__ __launch_bounds__(MAPLE_BLOCK) void k_calib_walk(const unsigned long long *buf, long long nLists, unsigned long long *sink)
{
    unsigned long long acc = 0;
    for (long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x; l < nLists; l += (long long)gridDim.x * blockDim.x) {
        const unsigned long long *p = buf + l * 64;
        unsigned idx = 0;
        for (int k = 0; k < 64; k++) {
            unsigned long long w = p[idx];
            acc += w;
            idx = (idx + 1 + (unsigned)(w & 0)) & 63;                    // data-dependent next index, like a cursor
        }
    }
    if (acc == 0x123456789abcdefull) *sink = acc;
}

// WRITE_SIZE calibration: mode 1 writes `bytes` as a coalesced 8-byte-per-lane stream, mode 2 writes ONE 8-byte value into
// every 64-byte line of the buffer (the score-matrix pattern of k_append_queries: a lane's score lands in a line of its own)
__global__ __launch_bounds__(MAPLE_BLOCK) void k_calib_write(unsigned long long *buf, long long nWords, int strideWords)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i * strideWords < nWords; i += (long long)gridDim.x * blockDim.x)
        buf[i * strideWords] = (unsigned long long)i;
}

extern "C" int maple_debug_calib_write(maple_ctx *c, uint64_t bytes, int32_t mode, int32_t repeats, float *ms)
{
    if (!c || bytes < 512 || repeats <= 0 || mode < 1 || mode > 2) return MAPLE_ERR_ARG;
    HIPCK(c, hipSetDevice(c->device));
    DevBuf<unsigned long long> buf;
    HIPCK(c, buf.reserve_exact((size_t)((bytes + 7) / 8)));
    HIPCK(c, hipMemset(buf, 0, bytes));
    HIPCK(c, hipDeviceSynchronize());
    Event e0, e1;
    HIPCK(c, e0.create());
    HIPCK(c, e1.create());
    HIPCK(c, hipEventRecord(e0, c->stream));
    for (int r = 0; r < repeats; r++)
        hipLaunchKernelGGL(k_calib_write, dim3(4096), dim3(MAPLE_BLOCK), 0, c->stream, buf.p, (long long)(bytes / 8), mode == 1 ? 1 : 8);
    HIPCK(c, hipEventRecord(e1, c->stream));
    HIPCK(c, hipEventSynchronize(e1));
    if (ms) HIPCK(c, hipEventElapsedTime(ms, e0, e1));
    return MAPLE_OK;
}

extern "C" int maple_debug_calib_walk(maple_ctx *c, uint64_t bytes, int32_t repeats, float *ms)
{
    if (!c || bytes < 512 || repeats <= 0) return MAPLE_ERR_ARG;
    HIPCK(c, hipSetDevice(c->device));
    DevBuf<unsigned long long> buf, sink;
    HIPCK(c, buf.reserve_exact((size_t)((bytes + 7) / 8)));
    HIPCK(c, sink.reserve_exact(1));
    HIPCK(c, hipMemset(buf, 1, bytes));
    HIPCK(c, hipDeviceSynchronize());
    Event e0, e1;
    HIPCK(c, e0.create());
    HIPCK(c, e1.create());
    HIPCK(c, hipEventRecord(e0, c->stream));
    for (int r = 0; r < repeats; r++)
        hipLaunchKernelGGL(k_calib_walk, dim3(2048), dim3(MAPLE_BLOCK), 0, c->stream, buf.p, (long long)(bytes / 512), sink.p);
    HIPCK(c, hipEventRecord(e1, c->stream));
    HIPCK(c, hipEventSynchronize(e1));
    if (ms) HIPCK(c, hipEventElapsedTime(ms, e0, e1));
    return MAPLE_OK;
}

// Parity hooks for the two innermost device functions, which no batched operator exposes on their own: getPartialVec
// (M:4073-4141) with the caller's matrix (the reference passes mutMatrices[pos] = Q * siteRates[pos]) and simplify
// (M:3697-3717).  One lane per call.
struct MatCtx {                        // what gpv_vec / gpv_nuc need from a context: q(r, i, j) of THIS call's matrix
    const double *M;
    __device__ inline double q(double, int i, int j) const { return M[i * 4 + j]; }
};
struct ThrCtx { struct { double thresholdProb, thresholdProb4; } m; };

__global__ __launch_bounds__(MAPLE_BLOCK) void k_debug_gpv(int n, int usingErrorRate, const int32_t *i12, const double *totLen,
                                                           const double *M16, const double *errorRate, const double *vect,
                                                           const uint8_t *upNode, const uint8_t *flag, double *out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        MatCtx c{M16 + 16 * (size_t)i};
        double o[4];
        if (i12[i] == 6) gpv_vec(c, 1.0, vect + 4 * (size_t)i, totLen[i], upNode[i] != 0, o);
        else if (usingErrorRate) gpv_nuc<MatCtx, true>(c, 1.0, i12[i], totLen[i], errorRate[i], upNode[i] != 0, flag[i] != 0, o);
        else gpv_nuc<MatCtx, false>(c, 1.0, i12[i], totLen[i], errorRate[i], upNode[i] != 0, false, o);
        for (int k = 0; k < 4; k++) out[4 * (size_t)i + k] = o[k];
    }
}

__global__ __launch_bounds__(MAPLE_BLOCK) void k_debug_simplify(int n, double thresholdProb, double thresholdProb4, const double *vec,
                                                                const int32_t *refA, int32_t *out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        ThrCtx c;
        c.m.thresholdProb = thresholdProb; c.m.thresholdProb4 = thresholdProb4;
        out[i] = simplify(c, vec + 4 * (size_t)i, refA[i]);
    }
}

extern "C" int maple_debug_gpv_batch(maple_ctx *c, int32_t n, const int32_t *i12, const double *totLen, const double *M16,
                                     const double *errorRate, const double *vect4, const uint8_t *upNode, const uint8_t *flag,
                                     double *out4)
{
    if (!c || n < 0 || !i12 || !totLen || !M16 || !errorRate || !vect4 || !upNode || !flag || !out4) return MAPLE_ERR_ARG;
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(need_model(c));
    TRY(h2d(c, c->s_i32[0], i12, (size_t)n));
    TRY(h2d(c, c->s_f64[0], totLen, (size_t)n));
    TRY(h2d(c, c->s_f64[1], M16, (size_t)16 * n));
    TRY(h2d(c, c->s_f64[2], errorRate, (size_t)n));
    TRY(h2d(c, c->s_f64[3], vect4, (size_t)4 * n));
    TRY(h2d(c, c->s_u8[0], upNode, (size_t)n));
    TRY(h2d(c, c->s_u8[1], flag, (size_t)n));
    HIPCK(c, c->s_aux.reserve((size_t)4 * n));
    hipLaunchKernelGGL(k_debug_gpv, dim3(grid_for(n)), dim3(MAPLE_BLOCK), 0, c->stream, n, c->dm.usingErrorRate, c->s_i32[0].p,
                       c->s_f64[0].p, c->s_f64[1].p, c->s_f64[2].p, c->s_f64[3].p, c->s_u8[0].p, c->s_u8[1].p, c->s_aux.p);
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(out4, c->s_aux.p, (size_t)4 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return MAPLE_OK;
}

extern "C" int maple_debug_simplify_batch(maple_ctx *c, int32_t n, const double *vec4, const int32_t *refA, int32_t *out)
{
    if (!c || n < 0 || !vec4 || !refA || !out) return MAPLE_ERR_ARG;
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(h2d(c, c->s_f64[0], vec4, (size_t)4 * n));
    TRY(h2d(c, c->s_i32[0], refA, (size_t)n));
    HIPCK(c, c->s_i32[1].reserve(n));
    hipLaunchKernelGGL(k_debug_simplify, dim3(grid_for(n)), dim3(MAPLE_BLOCK), 0, c->stream, n, c->dm.thresholdProb,
                       c->dm.thresholdProb4, c->s_f64[0].p, c->s_i32[0].p, c->s_i32[1].p);
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(out, c->s_i32[1].p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return MAPLE_OK;
}

// debugging aid: record the visit sequence (t1, direction, needsUpdating, failedPasses, lastLK, midProb) of one query
extern "C" int maple_debug_wave_append_batch(maple_ctx *c, int32_t n, const int32_t *pl, const int32_t *cl, const uint8_t *tip,
                                             const double *bl, double *out, float *ms)
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
    hipEvent_t e0, e1;
    TRY(ev_pair(c, &e0, &e1, MAPLE_K_OTHER, (double)n, 0.0));
    HIPCK(c, hipEventRecord(e0, c->stream));
    launch_wave_append(c, std::min(n, 256 * 16), n, dpl, dcl, dtip, dbl, c->s_f64[1].p);
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipEventRecord(e1, c->stream));
    HIPCK(c, hipMemcpyAsync(out, c->s_f64[1].p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (ms) HIPCK(c, hipEventElapsedTime(ms, e0, e1));
    return MAPLE_OK;
}

extern "C" int maple_debug_live_resources(int64_t *allocs, int64_t *bytes, int64_t *handles)
{
    if (!allocs || !bytes || !handles) return MAPLE_ERR_ARG;
    const DevBufStats &s = devbuf_stats();
    *allocs = s.live_allocs; *bytes = s.live_bytes; *handles = s.live_handles;
    return MAPLE_OK;
}

extern "C" int maple_debug_trace_query(maple_ctx *c, int32_t query)
{
    if (!c) return MAPLE_ERR_ARG;
    c->trace_query = query;
    if (query >= 0) {
        HIPCK(c, c->s_trace_i.reserve(4 * 4096 + 4));
        HIPCK(c, c->s_trace_d.reserve(2 * 4096));
        HIPCK(c, hipMemset(c->s_trace_i.p, 0, (4 * 4096 + 4) * sizeof(int32_t)));
    }
    return MAPLE_OK;
}

extern "C" int maple_debug_trace_read(maple_ctx *c, int32_t *n, int32_t *items4, double *vals2)
{
    if (!c || !n || !items4 || !vals2 || !c->s_trace_i.p) return MAPLE_ERR_ARG;
    HIPCK(c, hipMemcpy(n, c->s_trace_i.p + 4 * 4096, sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCK(c, hipMemcpy(items4, c->s_trace_i.p, 4 * 4096 * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCK(c, hipMemcpy(vals2, c->s_trace_d.p, 2 * 4096 * sizeof(double), hipMemcpyDeviceToHost));
    return MAPLE_OK;
}

extern "C" int maple_debug_frontier_levels(maple_ctx *c, int32_t cap, int64_t *itemsUpdating, int64_t *itemsCached, float *msUpdating,
                                           float *msCached, int32_t *n, int64_t *waveItemsSmall, int64_t *waveItemsBig)
{
    if (!c || cap < 0 || !itemsUpdating || !itemsCached || !msUpdating || !msCached || !n) return MAPLE_ERR_ARG;
    HIPCK(c, hipSetDevice(c->device));
    int nn = 0;
    const int rc = frontier_level_profile(c, cap, (long long *)itemsUpdating, (long long *)itemsCached, msUpdating, msCached, &nn,
                                          (long long *)waveItemsSmall, (long long *)waveItemsBig);
    *n = nn;
    return rc;
}

extern "C" int maple_debug_frontier_wave_paths(maple_ctx *c, int64_t *counts, int32_t cap, float *levelSlowestMs, int32_t *levelSlowestSlot,
                                               double *slots, int32_t *profiled)
{
    if (!c || !counts || cap < 0 || (cap > 0 && (!levelSlowestMs || !levelSlowestSlot)) || !slots || !profiled) return MAPLE_ERR_ARG;
    int prof = 0;
    const int rc = frontier_wave_paths(c, (long long *)counts, cap, levelSlowestMs, (int *)levelSlowestSlot, slots, &prof);
    *profiled = prof;
    return rc;
}

extern "C" int maple_debug_frontier_handbacks(maple_ctx *c, int64_t *reasons, int64_t *searchesHandedBack)
{
    if (!c || !reasons || !searchesHandedBack) return MAPLE_ERR_ARG;
    long long r[8] = {}, n = 0;
    const int rc = frontier_handbacks(c, r, &n);
    for (int k = 0; k < 8; k++) reasons[k] = r[k];
    *searchesHandedBack = n;
    return rc;
}

// ---- passGenomeListThroughBranch of a removed list as the frontier tier of the SPR search runs it (frontier_dev.h) ---------------
// The tier's two forms -- one lane per item (fpass_removed: fpass_store + shorten_would_merge) and one wavefront per item
// (wave_pass with `removed` set) -- are reached in the product only from inside a search on a tree with MAT local references.
// These two kernels call them as k_fr_pass / k_fr_pass_wave (frontier.hip) do, on n items of the caller, over the least of an
// FPools they read: the temporary lists' pool with its records, flags and counters, a scratch slab per lane, the mutation view.
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(FR_BLOCK) void k_debug_fpass_lane(const DevModel *__restrict__ mp, ArenaViewS av, FPools fp, int n, const int32_t *l,
                                                               const int32_t *ml, const uint8_t *up, int32_t *handle)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    const long long laneId = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long i = laneId; i < n; i += (long long)gridDim.x * blockDim.x)
        handle[i] = fpass_removed(c, fp, av, laneId, ftree(l[i]), ml[i], up[i] != 0);
}

template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(FR_BLOCK) void k_debug_fpass_wave(const DevModel *__restrict__ mp, ArenaViewS av, FPools fp, int n, const int32_t *l,
                                                               const int32_t *ml, const uint8_t *up, int32_t *handle)
{
    __shared__ Lds lds;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nWaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63;
    for (long long i = wave; i < n; i += nWaves) {
        const int h = wave_pass(c, fp, av, ftree(l[i]), ml[i], up[i] != 0, true);
        if (lane == 0) handle[i] = h;
    }
}

// where each item's new temporary list lies, for commit_lists (n_ent -1: the item got its own handle back, or none), and its grade
__global__ __launch_bounds__(FR_BLOCK) void k_debug_fpass_out(FPools fp, int n, const int32_t *handle, int64_t *woff, int64_t *aoff, int32_t *nEnt,
                                                              int32_t *nAux, uint8_t *grade)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int h = handle[i];
        if (h >= 0 && h < fp.capL) {
            const LRec r = fp.trec[h];
            woff[i] = LREC_OFF(r.x); aoff[i] = LREC_OFF(r.y); nEnt[i] = LREC_N(r.x); nAux[i] = LREC_N(r.y); grade[i] = fp.tflag[h];
        } else { woff[i] = 0; aoff[i] = 0; nEnt[i] = -1; nAux[i] = 0; grade[i] = 0; }
    }
}

extern "C" int maple_debug_frontier_pass_batch(maple_ctx *c, int32_t n, const int32_t *list, const int32_t *mutList, const uint8_t *dirIsUp,
                                               int32_t waveForm, int32_t *outList, uint8_t *grade, uint8_t *sameHandle)
{
    if (!c || n < 0 || n > (1 << 20) || !list || !mutList || !dirIsUp || !outList || !grade || !sameHandle) return MAPLE_ERR_ARG;
    if (n == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(need_model(c));
    TRY(check_ids(c, n, list, false, "list"));
    TRY(settle(c));
    const int32_t nml = (int32_t)c->h_mut_cnt.size();
    // the most a pass writes: two entries per mutation, each with the tail of the run it splits (<= 2 doubles)
    long long capW = 0, capA = 0;
    int capE = 1;
    for (int i = 0; i < n; i++) {
        if (mutList[i] < -1 || mutList[i] >= nml) return fail(c, MAPLE_ERR_ARG, "mutList[%d] = %d is not a mutation-list id", i, mutList[i]);
        const long long cnt = mutList[i] < 0 ? 0 : c->h_mut_cnt[mutList[i]];
        const long long ne = c->h_n_ent[list[i]] + 2 * cnt, na = c->h_n_aux[list[i]] + 4 * cnt;
        capW += ne; capA += na;
        capE = std::max(capE, (int)ne);
    }
    const int threads = waveForm ? 64 * std::min(n, 1024) : std::min(1024, (n + FR_BLOCK - 1) / FR_BLOCK * FR_BLOCK);
    const int grid = (threads + FR_BLOCK - 1) / FR_BLOCK;
    const long long lanes = (long long)grid * FR_BLOCK;
    HIPCK(c, c->s_words.reserve((size_t)capW));
    HIPCK(c, c->s_aux.reserve((size_t)capA));
    // one allocation for the rest: list records, flags, counters, the lanes' scratch slabs, the items' results
    auto up16 = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t oRec = 0, oCtr = up16(oRec + (size_t)n * sizeof(LRec)), oSw = up16(oCtr + sizeof(FCtr)),
                 oSa = up16(oSw + (waveForm ? 0 : (size_t)lanes * capE * sizeof(uint2))),
                 oWoff = up16(oSa + (waveForm ? 0 : (size_t)lanes * 5 * capE * sizeof(double))), oAoff = up16(oWoff + (size_t)n * 8),
                 oHandle = up16(oAoff + (size_t)n * 8), oNe = up16(oHandle + (size_t)n * 4), oNa = up16(oNe + (size_t)n * 4),
                 oFlag = up16(oNa + (size_t)n * 4), oGrade = up16(oFlag + (size_t)n), total = up16(oGrade + (size_t)n);
    DevBuf<uint8_t> own;
    HIPCK(c, own.reserve_exact(total));
    uint8_t *const buf = own.p;
    int rc = MAPLE_OK;
    std::vector<int32_t> handle(n);
    do {
        if (hipMemsetAsync(buf, 0, oSw, c->stream) != hipSuccess) { rc = fail(c, MAPLE_ERR_HIP, "hipMemsetAsync"); break; }
        FPools fp;
        memset(&fp, 0, sizeof fp);
        fp.tw = c->s_words.p; fp.ta = c->s_aux.p;
        fp.trec = (LRec *)(buf + oRec); fp.tflag = buf + oFlag;
        fp.capW = capW; fp.capA = capA; fp.capL = n;
        fp.sw = (uint2 *)(buf + oSw); fp.sa = (double *)(buf + oSa); fp.capE = capE;
        fp.ctr = (FCtr *)(buf + oCtr);
        fp.mat = 1;
        fp.mv = MutViewS{c->d_mut3, c->d_mut_off, c->d_mut_cnt};
        const ArenaViewS av{c->d_words, c->d_aux, c->d_ent_off, c->d_aux_off, c->d_n_ent, c->d_n_aux};
        if ((rc = stage_begin(c, (size_t)n * 64 + 256)) != MAPLE_OK) break;
        auto *dl = stage_put(c, list, (size_t)n);
        auto *dml = stage_put(c, mutList, (size_t)n);
        auto *dup = stage_put(c, dirIsUp, (size_t)n);
        if (!dl || !dml || !dup) { rc = fail(c, MAPLE_ERR_NOMEM, "argument staging overflow"); break; }
        if ((rc = stage_flush(c)) != MAPLE_OK) break;
        int32_t *dHandle = (int32_t *)(buf + oHandle), *dNe = (int32_t *)(buf + oNe), *dNa = (int32_t *)(buf + oNa);
        int64_t *dWoff = (int64_t *)(buf + oWoff), *dAoff = (int64_t *)(buf + oAoff);
        if (waveForm) DISPATCH3(c, k_debug_fpass_wave, <<<grid, FR_BLOCK, 0, c->stream>>>(c->d_model, av, fp, n, dl, dml, dup, dHandle));
        else DISPATCH3(c, k_debug_fpass_lane, <<<grid, FR_BLOCK, 0, c->stream>>>(c->d_model, av, fp, n, dl, dml, dup, dHandle));
        hipLaunchKernelGGL(k_debug_fpass_out, dim3(grid_for(n)), dim3(FR_BLOCK), 0, c->stream, fp, n, dHandle, dWoff, dAoff, dNe, dNa, buf + oGrade);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(handle.data(), dHandle, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess
            || hipMemcpyAsync(grade, buf + oGrade, (size_t)n, hipMemcpyDeviceToHost, c->stream) != hipSuccess
            || hipStreamSynchronize(c->stream) != hipSuccess) { rc = fail(c, MAPLE_ERR_HIP, "the frontier pass hook's launch failed"); break; }
        for (int i = 0; i < n && rc == MAPLE_OK; i++) {
            sameHandle[i] = handle[i] == -(list[i] + 10);
            if (!sameHandle[i] && handle[i] < 0) rc = fail(c, MAPLE_ERR_NOMEM, "item %d: no room for the new list (%d)", i, handle[i]);
        }
        if (rc != MAPLE_OK) break;
        if ((rc = commit_lists(c, n, dWoff, dAoff, dNe, dNa, outList, fp.tw, fp.ta)) != MAPLE_OK) break;
        if (hipStreamSynchronize(c->stream) != hipSuccess) { rc = fail(c, MAPLE_ERR_HIP, "hipStreamSynchronize"); break; }
        for (int i = 0; i < n; i++) if (sameHandle[i]) outList[i] = list[i];
    } while (0);
    return rc;
}

// ---- score rows of the whole-tree searches from explicit lists (spr_batch.hip's pre_rows makes them from a tree) --------------------
// form 0: the dense kernel with bitmap (launch_append_queries(..., finMask)), form 1: the witness filter (witness_score); then the
// prefix counts the replay kernels index by (launch_finite_prefix).  The product's launches on the caller's lists; only the fill of
// the table beforehand is the hook's own -- the product leaves the cells of -inf scores as they are.
__global__ __launch_bounds__(MAPLE_BLOCK) void k_debug_fill(long long n, double v, double *out)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = v;
}

extern "C" int maple_debug_score_rows(maple_ctx *c, int32_t form, int32_t nQ, const int32_t *qList, const uint8_t *qTip, const double *qBLen,
                                      int32_t nC, const int32_t *cand, const int32_t *outCol, int64_t ldOut, double fill, double *out,
                                      uint64_t *finMask, int32_t *prefix, int64_t *pairsWalked)
{
    if (!c || form < 0 || form > 1 || nQ <= 0 || nC <= 0 || !qList || !qTip || !qBLen || !cand || ldOut < nC || !out || !finMask || !prefix)
        return MAPLE_ERR_ARG;
    if ((long long)nQ * ldOut > (1ll << 28)) return fail(c, MAPLE_ERR_ARG, "maple_debug_score_rows: a table of %lld scores", (long long)nQ * ldOut);
    HIPCK(c, hipSetDevice(c->device));
    TRY(need_model(c));
    TRY(check_ids(c, nQ, qList, false, "qList"));
    TRY(check_ids(c, nC, cand, true, "cand"));
    for (int k = 0; k < nC; k++) {
        if (cand[k] < -1) return fail(c, MAPLE_ERR_ARG, "cand[%d] = %d", k, cand[k]);
        if (outCol && (outCol[k] < 0 || outCol[k] >= ldOut)) return fail(c, MAPLE_ERR_ARG, "outCol[%d] = %d is outside a row of %lld", k, outCol[k], (long long)ldOut);
    }
    TRY(settle(c));
    const int nWords = (nC + 63) / 64;
    const size_t nOut = (size_t)nQ * (size_t)ldOut, nMask = (size_t)nQ * nWords, nPre = (size_t)nQ * (nWords + 1);
    DevBuf<double> dOut;
    DevBuf<unsigned long long> dMask;
    DevBuf<int32_t> dPre;
    HIPCK(c, dOut.reserve_exact(nOut));
    HIPCK(c, dMask.reserve_exact(nMask));
    HIPCK(c, dPre.reserve_exact(nPre));
    TRY(stage_begin(c, (size_t)nQ * 16 + (size_t)nC * 8 + 256));
    STAGE(dq, c, qList, nQ); STAGE(dtip, c, qTip, nQ); STAGE(dbl, c, qBLen, nQ); STAGE(dcand, c, cand, nC);
    const int32_t *dcol = nullptr;
    if (outCol) { STAGE(dc, c, outCol, nC); dcol = dc; }
    TRY(stage_flush(c));
    hipLaunchKernelGGL(k_debug_fill, dim3(grid_for((int)nOut)), dim3(MAPLE_BLOCK), 0, c->stream, (long long)nOut, fill, dOut.p);
    HIPCK(c, hipGetLastError());
    // (both forms write every word of the bitmap themselves, and the prefix kernel every count: they start from a pattern)
    HIPCK(c, hipMemsetAsync(dMask.p, 0xA5, nMask * sizeof(unsigned long long), c->stream));
    HIPCK(c, hipMemsetAsync(dPre.p, 0xA5, nPre * sizeof(int32_t), c->stream));
    long long pairs = -1;
    if (form == 1)
        TRY(witness_score(c, c->stream, nQ, dq, dtip, dbl, nC, dcand, dcol, dOut.p, ldOut, dMask.p, nWords, 0.0, 0.0, &pairs));
    else
        TRY(launch_append_queries(c, c->stream, nQ, dq, nC, dcand, 0, 0.0, dOut.p, ldOut, dcol, dtip, dbl, MAPLE_K_OTHER, 0.0, nullptr, nullptr,
                                  nullptr, 0, 1, dMask.p));
    TRY(launch_finite_prefix(c, c->stream, (size_t)nQ, nWords, dMask.p, dPre.p));
    HIPCK(c, hipMemcpyAsync(out, dOut.p, nOut * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(finMask, dMask.p, nMask * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(prefix, dPre.p, nPre * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (pairsWalked) *pairsWalked = pairs;
    return MAPLE_OK;
}

// ---- the repair's fused item kernels on explicit lists, and the arms the last repair took -------------------------------------
// update_items of update.hip itself (staging, the choice of kernel by wave_item_max, commit_known): nothing of it is repeated here.
extern "C" int maple_debug_update_items(maple_ctx *c, int32_t n, const int32_t *l1, const double *b1, const uint8_t *t1, const int32_t *l2,
                                        const double *b2, const uint8_t *t2, const uint8_t *upDown, const uint8_t *mode, const int32_t *old,
                                        int32_t *outList, uint8_t *outNone, uint8_t *outDiff)
{
    if (!c || n < 0 || !l1 || !b1 || !t1 || !l2 || !b2 || !t2 || !upDown || !mode || !old || !outList || !outNone || !outDiff) return MAPLE_ERR_ARG;
    for (int i = 0; i < n; i++)
        if (mode[i] > 2) return fail(c, MAPLE_ERR_ARG, "mode[%d] = %d", i, mode[i]);
    TRY(need_model(c));
    return update_items(c, n, l1, b1, t1, l2, b2, t2, upDown, mode, old, outList, outNone, outDiff);
}

// ---- the branch-length sweep's fused estimate kernels on explicit items ---------------------------------------------------------
// sweep_estimate of blen_sweep.hip itself (the id checks, the scratch offsets, the choice of kernel by wave_item_max, the copy back).
extern "C" int maple_debug_sweep_estimate(maple_ctx *c, int32_t n, const int32_t *upList, const int32_t *mutList, const int32_t *lowList,
                                          const uint8_t *tip, double *t, uint8_t *isFalse)
{
    if (!c || n < 0 || !upList || !mutList || !lowList || !tip || !t || !isFalse) return MAPLE_ERR_ARG;
    std::vector<sweep_plan::SweepItem> items((size_t)n);
    for (int i = 0; i < n; i++) {
        if (mutList[i] < -1) return fail(c, MAPLE_ERR_ARG, "mutList[%d] = %d", i, mutList[i]);
        items[i] = sweep_plan::SweepItem{i, upList[i], mutList[i], lowList[i], (uint8_t)(tip[i] != 0)};
    }
    TRY(need_model(c));
    HIPCK(c, hipSetDevice(c->device));
    std::vector<double> tv((size_t)n, 0.0);
    std::vector<uint8_t> fv((size_t)n, 0);
    TRY(sweep_estimate(c, items, tv, fv));
    for (int i = 0; i < n; i++) { t[i] = tv[i]; isFalse[i] = fv[i]; }
    return MAPLE_OK;
}

extern "C" int maple_debug_update_partials_stats(maple_ctx *c, int64_t *counts, int32_t cap, int32_t *n)
{
    if (!c || cap < 0 || !n || (cap && !counts)) return MAPLE_ERR_ARG;
    *n = update_partials_stats(c, cap, counts);
    return MAPLE_OK;
}

// the nodes the last maple_update_partials visited, with repeats and in the order of the visits (update_partials_visited of update.hip:
// what the branch-length sweep sets `dirty` from)
extern "C" int maple_debug_update_partials_visited(maple_ctx *c, int32_t cap, int32_t *nodes, int32_t *n)
{
    if (!c || cap < 0 || !n || (cap && !nodes)) return MAPLE_ERR_ARG;
    const std::vector<int32_t> &vis = update_partials_visited(c);
    *n = (int32_t)vis.size();
    if ((int32_t)vis.size() > cap) return fail(c, MAPLE_ERR_ARG, "%zu visited nodes do not fit in %d", vis.size(), cap);
    for (size_t i = 0; i < vis.size(); i++) nodes[i] = vis[i];
    return MAPLE_OK;
}

extern "C" const char *maple_debug_update_partials_stat_names(void)
{
#define UPDATE_PLAN_STAT_NAME(name) #name " "
    return UPDATE_PLAN_STATS(UPDATE_PLAN_STAT_NAME);
#undef UPDATE_PLAN_STAT_NAME
}
