// maple_amd/csrc/debug_abi.hip -- the measurement aids and test hooks of include/maple_hip_debug.h.  Compiled like every other
// unit and linked into libmaple_hip_debug.so only (the product library's objects plus this one).  gfx950 only.
#include "../../include/maple_hip_debug.h"
#include "genome_dev.h"
#include "ctx_host.h"
#include "batch_host.h"
#include "frontier.h"

#include <algorithm>

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
    unsigned long long *buf = nullptr;
    HIPCK(c, hipMalloc((void **)&buf, bytes));
    HIPCK(c, hipMemset(buf, 0, bytes));
    HIPCK(c, hipDeviceSynchronize());
    hipEvent_t e0, e1;
    HIPCK(c, hipEventCreate(&e0));
    HIPCK(c, hipEventCreate(&e1));
    HIPCK(c, hipEventRecord(e0, c->stream));
    for (int r = 0; r < repeats; r++)
        hipLaunchKernelGGL(k_calib_write, dim3(4096), dim3(MAPLE_BLOCK), 0, c->stream, buf, (long long)(bytes / 8), mode == 1 ? 1 : 8);
    HIPCK(c, hipEventRecord(e1, c->stream));
    HIPCK(c, hipEventSynchronize(e1));
    if (ms) HIPCK(c, hipEventElapsedTime(ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(buf);
    return MAPLE_OK;
}

extern "C" int maple_debug_calib_walk(maple_ctx *c, uint64_t bytes, int32_t repeats, float *ms)
{
    if (!c || bytes < 512 || repeats <= 0) return MAPLE_ERR_ARG;
    HIPCK(c, hipSetDevice(c->device));
    unsigned long long *buf = nullptr, *sink = nullptr;
    HIPCK(c, hipMalloc((void **)&buf, bytes));
    HIPCK(c, hipMalloc((void **)&sink, 8));
    HIPCK(c, hipMemset(buf, 1, bytes));
    HIPCK(c, hipDeviceSynchronize());
    hipEvent_t e0, e1;
    HIPCK(c, hipEventCreate(&e0));
    HIPCK(c, hipEventCreate(&e1));
    HIPCK(c, hipEventRecord(e0, c->stream));
    for (int r = 0; r < repeats; r++)
        hipLaunchKernelGGL(k_calib_walk, dim3(2048), dim3(MAPLE_BLOCK), 0, c->stream, buf, (long long)(bytes / 512), sink);
    HIPCK(c, hipEventRecord(e1, c->stream));
    HIPCK(c, hipEventSynchronize(e1));
    if (ms) HIPCK(c, hipEventElapsedTime(ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(buf); (void)hipFree(sink);
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
