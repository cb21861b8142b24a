// maple_amd/csrc/append_queries.hip -- the dense query path of libmaple_hip.so: appendProbNode of Q queries x C candidates
// (k_append_queries, k_append_queries_lds), the per-query arg-max over their tiles, and the maple_append_queries*_dev entry
// points.  launch_append_queries (declared in batch_host.h) is what the SPR search batch and the placement search call.
// gfx950 only.
#include "../../include/maple_hip.h"
#include "genome_dev.h"
#include "append_lds.h"
#include "ctx_host.h"
#include "batch_host.h"

#include <cmath>

#define MAPLE_QLDS 192                 // query-list words staged in LDS per wavefront (longer lists are read from HBM/L2)

// Q queries x C candidates, query-major output out[q*C + k]: pair (q, k) is handled by one lane.  A tile is one query x
// 64 consecutive candidates and every WAVEFRONT pulls its next tile from an atomic counter, so there is no barrier
// anywhere and a wavefront that drew short lists never idles behind its workgroup's longest lane.  Tiles are numbered
// candidate-chunk-major: the ~4 000 wavefronts in flight sweep the same few candidate chunks (hot in L1/L2) with
// different queries.  Callers pass the candidates SORTED BY LIST LENGTH so that the 64 lanes of a wavefront finish
// together.  Measured on the 10 000-sample bench tree (256 queries x 14 878 branches), ms per launch:
//   static 256-candidate tiles, query-major 2.56 | chunk-major 2.29 | dynamic 64-candidate tiles, query-major 2.30 |
//   dynamic + chunk-major 1.85 | + candidates sorted by length 1.53.
// (Staging the query in LDS behind __syncthreads() was 1.4x slower; several queries per tile lost balance: 2.06 at 4.)

template <bool RV, bool U, bool SS>
__global__ MAPLE_APPEND_ATTR void k_append_queries(const DevModel *__restrict__ mp, ArenaView av, int nQ,
                                                   const int32_t *qList, int nC, const int32_t *cand, int isTip,
                                                   double bLen, double *out, long long ldOut, const int32_t *outCol,
                                                   const uint8_t *qTip, const double *qBLen, int *counter,
                                                   TileBest *tileBest, const int32_t *visitRank, unsigned long long *finMask)
{
    __shared__ Lds lds;
    __shared__ unsigned long long qlds[MAPLE_BLOCK / 64][MAPLE_QLDS];   // the tile's query list, one copy per wavefront
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    const int lane = threadIdx.x & 63;
    unsigned long long *myq = qlds[threadIdx.x >> 6];
    const int nChunks = (nC + 63) / 64;
    const long long tiles = (long long)nQ * nChunks;
    double tbScore = -INFINITY;
    int tbRank = 0x7fffffff, tbIdx = -1;
    for (;;) {
        int j = 0;
        if (lane == 0) j = atomicAdd(counter, 1);
        j = __builtin_amdgcn_readfirstlane(j);
        if (j >= tiles) break;
        const int ch = j / nQ;
        const int q = j - ch * nQ;
        const int k = ch * 64 + lane;
        const int ql = qList[q];
        const int nq = av.n_ent[ql];
        const ListRef qref = list_ref(av, ql);
        const bool staged = nq <= MAPLE_QLDS;                             // wave-uniform
        if (staged) {
            // all 64 lanes walk the same query: its words go to LDS once per tile (no workgroup barrier: the LDS
            // pipeline serves one wavefront's requests in order) and every step's query load is a ds_read
            for (int i = lane; i < nq; i += 64) myq[i] = ((const unsigned long long *)qref.w)[i];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        const int cl = k < nC ? cand[k] : -1;                             // -1: this column has no list (score unused)
        bool finite = false;
        if (cl >= 0) {
            const bool tipq = qTip ? qTip[q] != 0 : isTip != 0;
            const double blq = qBLen ? qBLen[q] : bLen;
            double lk;
            if (staged) {
                PairWalk<RV, U, SS> w(c, qref, tipq, blq, myq);
                w.start(list_ref(av, cl));
                while (!w.step()) {}
                lk = w.finish();
            } else lk = append_walk(c, list_ref(av, cl), qref, tipq, blq);
            if (!tileBest) { if (!finMask || lk > -INFINITY) out[(long long)q * ldOut + (outCol ? outCol[k] : k)] = lk; }   // (see the LDS kernel)
            else { tbScore = lk; tbRank = visitRank ? visitRank[k] : k; tbIdx = k; }
            finite = lk > -INFINITY;
        }
        if (finMask) {
            const unsigned long long fm = __ballot(finite);
            if (lane == 0) finMask[(long long)q * nChunks + ch] = fm;
        }
        if (tileBest) {
            // the wavefront reduction of north_star: best score of the tile's 64 candidates, exact ties to the EARLIEST visit
            // (the reference keeps the first of equal scores: strict >, M:7083 / 8065); one 16-byte record per (query, tile)
            // instead of 64 scores
            for (int m2 = 32; m2 >= 1; m2 >>= 1) {
                const double os = __shfl_xor(tbScore, m2, 64);
                const int orank = __shfl_xor(tbRank, m2, 64), oidx = __shfl_xor(tbIdx, m2, 64);
                if (os > tbScore || (os == tbScore && orank < tbRank)) { tbScore = os; tbRank = orank; tbIdx = oidx; }
            }
            if (lane == 0) tileBest[(long long)q * nChunks + ch] = TileBest{tbScore, tbRank, tbIdx};
            tbScore = -INFINITY; tbRank = 0x7fffffff; tbIdx = -1;
        }
        __builtin_amdgcn_wave_barrier();
    }
}


// The same Q x C scoring with the tile's 64 candidate lists staged in LDS (append_lds.h): a workgroup of 16 wavefronts (one
// per CU) takes a unit = (chunk of 64 candidates, block of MAPLE_LDS_QB queries), copies the chunk's words and aux doubles into
// LDS with coalesced loads -- and, with per-site rates, the rate of every entry's last site next to it -- and its
// wavefronts then pull the block's queries from an LDS counter: one query x the 64 staged candidates per tile, candidate
// words / stored lengths / O vectors / site rates and the query's words and rates all read with ds_read.  Chunks too long for
// the LDS budget, and queries longer than the strip, are walked from global memory as before.
#define MAPLE_LDS_BLOCK 1024
#define MAPLE_LDS_CAPW 4096            // candidate words per staged chunk (32 KB, + 32 KB of site rates with rate variation)
#define MAPLE_LDS_CAPA 1536            // candidate aux doubles per staged chunk (12 KB)
#ifndef MAPLE_LDS_QB
#define MAPLE_LDS_QB 512               // queries per unit: 128 / 256 / 512 measured 549 / 544 / 538 ms per launch at 100k tips
#endif
template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(MAPLE_LDS_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_append_queries_lds(const DevModel *__restrict__ mp, ArenaView av, int nQ, const int32_t *qList, int nC, const int32_t *cand,
                          int isTip, double bLen, double *out, long long ldOut, const int32_t *outCol, const uint8_t *qTip,
                          const double *qBLen, int *counter, TileBest *tileBest, const int32_t *visitRank,
                          const int4 *chunkTab, int nChunkTab, int nF, unsigned long long *finMask)
{
    // chunkTab (trees with MAT local references): the chunks are given as {first candidate, candidates (<= 64), reference
    // frame, -}, each within ONE frame, and query q's list is qList[q * nF + frame] -- the query expressed in that frame
    constexpr int NW = MAPLE_LDS_BLOCK / 64;
    __shared__ Lds lds;
    __shared__ int cwoff[65], caoff[65];
    __shared__ int sUnit, sNext, sStaged;
    extern __shared__ unsigned long long dynU64[];
    // dynamic LDS: candidate words | candidate aux | [candidate rates] | per-wavefront query words | [per-wavefront query rates]
    unsigned long long *cW = dynU64;
    double *cA = (double *)(cW + MAPLE_LDS_CAPW);
    double *cR = cA + MAPLE_LDS_CAPA;
    unsigned long long *qW = (unsigned long long *)(cR + (RV ? MAPLE_LDS_CAPW : 0));
    double *qR = (double *)(qW + NW * MAPLE_QLDS);
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nChunks = chunkTab ? nChunkTab : (nC + 63) / 64, nQB = (nQ + MAPLE_LDS_QB - 1) / MAPLE_LDS_QB;
    const long long units = (long long)nChunks * nQB;
    unsigned long long *myq = qW + wave * MAPLE_QLDS;
    double *myqR = qR + wave * MAPLE_QLDS;
    double tbScore = -INFINITY;
    int tbRank = 0x7fffffff, tbIdx = -1;
    for (;;) {
        if (tid == 0) sUnit = atomicAdd(counter, 1);
        __syncthreads();
        const int unit = sUnit;
        if (unit >= units) break;
        const int ch = unit / nQB, qb = unit - ch * nQB;
        int c0 = ch * 64, nCk = min(64, nC - ch * 64), frame = 0;
        if (chunkTab) { const int4 u = chunkTab[ch]; c0 = u.x; nCk = u.y; frame = u.z; }
        // this lane's candidate and where its list sits in the staged chunk
        const int k = c0 + lane;
        const int cl = lane < nCk ? cand[k] : -1;
        if (wave == 0) {
            int ne = cl >= 0 ? av.n_ent[cl] : 0, na = cl >= 0 ? av.n_aux[cl] : 0;
            int pw = ne, pa = na;                                          // inclusive prefix sums over the 64 lists
            for (int d = 1; d < 64; d <<= 1) {
                const int ow = __shfl_up(pw, d, 64), oa = __shfl_up(pa, d, 64);
                if (lane >= d) { pw += ow; pa += oa; }
            }
            cwoff[lane] = pw - ne; caoff[lane] = pa - na;
            if (lane == 63) { cwoff[64] = pw; caoff[64] = pa; sStaged = (pw <= MAPLE_LDS_CAPW && pa <= MAPLE_LDS_CAPA) ? 1 : 0; sNext = 0; }
        }
        __syncthreads();
        const bool stagedC = sStaged != 0;
        if (stagedC) {                                                     // 4 lists per wavefront, coalesced within a list
            constexpr int perWave = (64 + NW - 1) / NW;
            for (int i = wave * perWave; i < min(64, wave * perWave + perWave); i++) {
                if (i >= nCk) break;
                const int li = cand[c0 + i];
                const unsigned long long *sw = (const unsigned long long *)(av.words + av.ent_off[li]);
                const double *sa = av.aux + av.aux_off[li];
                const int w0 = cwoff[i], nw = cwoff[i + 1] - w0, a0 = caoff[i], na2 = caoff[i + 1] - a0;
#ifndef MAPLE_DENSE_PLAIN
                // (staged in the SKIPPING form of append_lds.h: the tail-less reference runs in front of single-site entries are left
                // out -- half the entries, and with them half the steps of every walk over the chunk)
                int kept = 0;
                for (int j0 = 0; j0 < nw; j0 += 64) {
                    const int j = j0 + lane;
                    unsigned long long w = 0;
                    bool keep = false;
                    if (j < nw) { w = sw[j]; keep = !skip_form_drops(w, j + 1 < nw ? sw[j + 1] : 0ull, j + 1 == nw); }
                    const unsigned long long bal = __ballot(keep);
                    if (keep) {
                        const int d = w0 + kept + __popcll(bal & ((1ull << lane) - 1ull));
                        cW[d] = w;
                        if (RV) cR[d] = c.rate((int)(uint32_t)w - 1);
                    }
                    kept += __popcll(bal);
                }
#else
                for (int j = lane; j < nw; j += 64) {
                    const unsigned long long w = sw[j];
                    cW[w0 + j] = w;
                    if (RV) cR[w0 + j] = c.rate((int)(uint32_t)w - 1);
                }
#endif
                for (int j = lane; j < na2; j += 64) cA[a0 + j] = sa[j];
            }
        }
        __syncthreads();
        const int myW = cwoff[lane], myA = caoff[lane];
        for (;;) {
            int qi = 0;
            if (lane == 0) qi = atomicAdd(&sNext, 1);
            qi = __builtin_amdgcn_readfirstlane(qi);
            const int q = qb * MAPLE_LDS_QB + qi;
            if (qi >= MAPLE_LDS_QB || q >= nQ) break;
            const int ql = chunkTab ? qList[(long long)q * nF + frame] : qList[q];
            const int nq = av.n_ent[ql];
            const ListRef qref = list_ref(av, ql);
            const bool stagedQ = nq <= MAPLE_QLDS;                          // wave-uniform
            if (stagedQ) {
#ifndef MAPLE_DENSE_PLAIN
                const unsigned long long *qsrc = (const unsigned long long *)qref.w;
                int kept = 0;
                for (int j0 = 0; j0 < nq; j0 += 64) {
                    const int j = j0 + lane;
                    unsigned long long w = 0;
                    bool keep = false;
                    if (j < nq) { w = qsrc[j]; keep = !skip_form_drops(w, j + 1 < nq ? qsrc[j + 1] : 0ull, j + 1 == nq); }
                    const unsigned long long bal = __ballot(keep);
                    if (keep) {
                        const int d = kept + __popcll(bal & ((1ull << lane) - 1ull));
                        myq[d] = w;
                        if (RV) myqR[d] = c.rate((int)(uint32_t)w - 1);
                    }
                    kept += __popcll(bal);
                }
#else
                for (int i = lane; i < nq; i += 64) {
                    const unsigned long long w = ((const unsigned long long *)qref.w)[i];
                    myq[i] = w;
                    if (RV) myqR[i] = c.rate((int)(uint32_t)w - 1);
                }
#endif
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            bool finite = false;
#ifndef MAPLE_DENSE_PLAIN
            // (the walk in skipping form votes over the whole wavefront, append_lds.h: every lane calls, those without a candidate
            // with valid = false)
            const bool validL = cl >= 0;
            double lkAll;
            {
                const bool tipq = qTip ? qTip[q] != 0 : isTip != 0;
                const double blq = qBLen ? qBLen[q] : bLen;
                const MemLG qL{(lds_u64p)myq, qref.aux, (lds_f64p)myqR};
                const MemG qG{(const unsigned long long *)qref.w, qref.aux};
                if (stagedC) {                                              // (block-uniform; stagedQ is wave-uniform)
                    const MemL pL{(lds_u64p)(cW + myW), (lds_f64p)(cA + myA), (lds_f64p)(cR + myW)};
                    lkAll = stagedQ ? append_walk_c(c, pL, qL, tipq, blq, validL) : append_walk_c(c, pL, qG, tipq, blq, validL);
                } else {
                    const ListRef pr = validL ? list_ref(av, cl) : qref;
                    const MemG pG{(const unsigned long long *)pr.w, pr.aux};
                    lkAll = stagedQ ? append_walk_c(c, pG, qL, tipq, blq, validL) : append_walk_c(c, pG, qG, tipq, blq, validL);
                }
            }
#endif
            if (cl >= 0) {
#ifndef MAPLE_DENSE_PLAIN
                const double lk = lkAll;
#else
                const bool tipq = qTip ? qTip[q] != 0 : isTip != 0;
                const double blq = qBLen ? qBLen[q] : bLen;
                const MemLG qL{(lds_u64p)myq, qref.aux, (lds_f64p)myqR};
                const MemG qG{(const unsigned long long *)qref.w, qref.aux};
                double lk;
                if (stagedC) {
                    const MemL pL{(lds_u64p)(cW + myW), (lds_f64p)(cA + myA), (lds_f64p)(cR + myW)};
                    lk = stagedQ ? append_walk_m(c, pL, qL, tipq, blq) : append_walk_m(c, pL, qG, tipq, blq);
                } else {
                    const ListRef pr = list_ref(av, cl);
                    const MemG pG{(const unsigned long long *)pr.w, pr.aux};
                    lk = stagedQ ? append_walk_m(c, pG, qL, tipq, blq) : append_walk_m(c, pG, qG, tipq, blq);
                }
#endif
                // finMask: which of the tile's 64 scores are finite goes out as ONE word per (query, tile) and only the finite
                // scores are stored -- the searches these rows are for are the ones whose scores are nearly all -inf (a mismatch
                // over a zero-length branch), and an 8-byte store into every line of a row was most of the kernel's HBM traffic
                if (!tileBest) { if (!finMask || lk > -INFINITY) out[(long long)q * ldOut + (outCol ? outCol[k] : k)] = lk; }
                else { tbScore = lk; tbRank = visitRank ? visitRank[k] : k; tbIdx = k; }
                finite = lk > -INFINITY;
            }
            if (finMask) {
                const unsigned long long fm = __ballot(finite);
                if (lane == 0) finMask[(long long)q * nChunks + ch] = fm;
            }
            if (tileBest) {
                for (int m2 = 32; m2 >= 1; m2 >>= 1) {
                    const double os = __shfl_xor(tbScore, m2, 64);
                    const int orank = __shfl_xor(tbRank, m2, 64), oidx = __shfl_xor(tbIdx, m2, 64);
                    if (os > tbScore || (os == tbScore && orank < tbRank)) { tbScore = os; tbRank = orank; tbIdx = oidx; }
                }
                if (lane == 0) tileBest[(long long)q * nChunks + ch] = TileBest{tbScore, tbRank, tbIdx};
                tbScore = -INFINITY; tbRank = 0x7fffffff; tbIdx = -1;
            }
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();                                                   // nobody may still read the chunk when it is restaged
    }
}
template <bool RV> static size_t lds_kernel_dyn_bytes()
{
    constexpr int NW = MAPLE_LDS_BLOCK / 64;
    return (size_t)MAPLE_LDS_CAPW * 8 + (size_t)MAPLE_LDS_CAPA * 8 + (RV ? (size_t)MAPLE_LDS_CAPW * 8 : 0)
           + (size_t)NW * MAPLE_QLDS * 8 * (RV ? 2 : 1);
}

// per query: the best of its tiles (same order: score, then earliest visit)
__global__ __launch_bounds__(64) void k_argmax_reduce(int nQ, int nChunks, const TileBest *tb, double *bestScore, int32_t *bestIdx)
{
    const int q = blockIdx.x;
    if (q >= nQ) return;
    TileBest b{-INFINITY, 0x7fffffff, -1};
    for (int i = threadIdx.x; i < nChunks; i += 64) {
        const TileBest t = tb[(long long)q * nChunks + i];
        if (t.score > b.score || (t.score == b.score && t.rank < b.rank)) b = t;
    }
    for (int m2 = 32; m2 >= 1; m2 >>= 1) {
        const double os = __shfl_xor(b.score, m2, 64);
        const int orank = __shfl_xor(b.rank, m2, 64), oidx = __shfl_xor(b.idx, m2, 64);
        if (os > b.score || (os == b.score && orank < b.rank)) { b.score = os; b.rank = orank; b.idx = oidx; }
    }
    if (threadIdx.x == 0) { bestScore[q] = b.score; bestIdx[q] = b.idx; }
}

// one launch of k_append_queries on stream s (timed with an event pair): out[q * ldOut + (outCol ? outCol[k] : k)]
int launch_append_queries(maple_ctx *c, hipStream_t s, int nQ, const int32_t *qList, int nC, const int32_t *cand,
                          int isTip, double bLen, double *out, long long ldOut, const int32_t *outCol,
                          const uint8_t *qTip, const double *qBLen, int kind, double algBytes, TileBest *tileBest,
                          const int32_t *visitRank, const int4 *chunkTab, int nChunkTab, int nF,
                          unsigned long long *finMask, bool lanesOnly)
{
    const long long tiles = (long long)nQ * (chunkTab ? nChunkTab : (nC + 63) / 64);
    if (tiles > 0x7fffffffLL - (1 << 20)) return fail(c, MAPLE_ERR_ARG, "nQ x nC too large for one launch");
    HIPCK(c, c->d_tile_counters.reserve_exact(64));
    int32_t *counter = c->d_tile_counters + (c->tile_counter_next++ & 63);
    HIPCK(c, hipMemsetAsync(counter, 0, sizeof(int32_t), s));
    const long long waves = (tiles + 3) / 4;
    const int grid = waves < 256 * MAPLE_APPEND_WAVES ? (int)waves : 256 * MAPLE_APPEND_WAVES;   // workgroups of 4 wavefronts, MAPLE_APPEND_WAVES per CU = the occupancy limit
    hipEvent_t e0, e1;
    TRY(ev_pair(c, &e0, &e1, kind, (double)nQ * (double)nC, algBytes));
    HIPCK(c, hipEventRecord(e0, s));
    // (lanesOnly: many queries against a HANDFUL of candidates -- the columns a placement changed, for every sample still waiting,
    // placement.hip: the LDS kernel would be one workgroup with a few lanes of each wavefront at work)
    if (!lanesOnly && (chunkTab || nQ >= 32)) {
        // enough queries to reuse a staged candidate chunk: the LDS kernel, one workgroup of 16 wavefronts per CU
        const long long units = (long long)(chunkTab ? nChunkTab : (nC + 63) / 64) * ((nQ + MAPLE_LDS_QB - 1) / MAPLE_LDS_QB);
        const int gridL = units < 256 ? (int)units : 256;
        const bool rv_ = c->dm.useRateVariation;
        const size_t dyn = rv_ ? lds_kernel_dyn_bytes<true>() : lds_kernel_dyn_bytes<false>();
        static bool attrSet = false;
        if (!attrSet) {                                                // more than 64 KB of LDS per workgroup has to be asked for
#define MAPLE_SET_LDS(RV_, U_, SS_) HIPCK(c, hipFuncSetAttribute((const void *)k_append_queries_lds<RV_, U_, SS_>, \
                                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_kernel_dyn_bytes<RV_>()))
            MAPLE_SET_LDS(false, false, false); MAPLE_SET_LDS(true, false, false); MAPLE_SET_LDS(false, true, false);
            MAPLE_SET_LDS(false, true, true); MAPLE_SET_LDS(true, true, false); MAPLE_SET_LDS(true, true, true);
#undef MAPLE_SET_LDS
            attrSet = true;
        }
        DISPATCH3(c, k_append_queries_lds, <<<gridL, MAPLE_LDS_BLOCK, dyn, s>>>(c->d_model, view(c), nQ, qList, nC, cand, isTip, bLen, out,
                                                                              ldOut, outCol, qTip, qBLen, counter, tileBest, visitRank,
                                                                              chunkTab, nChunkTab, nF, finMask));
    } else
    DISPATCH3(c, k_append_queries, <<<grid, MAPLE_BLOCK, 0, s>>>(c->d_model, view(c), nQ, qList, nC, cand, isTip, bLen, out, ldOut,
                                                                  outCol, qTip, qBLen, counter, tileBest, visitRank, finMask));
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipEventRecord(e1, s));
    return MAPLE_OK;
}

extern "C" int maple_append_queries_dev(maple_ctx *c, int32_t nQ, const int32_t *qList_dev, int32_t nC,
                                        const int32_t *cand_dev, int isTipC, double bLen, double *out_dev, void *stream)
{
    if (!c || nQ < 0 || nC < 0 || !qList_dev || !cand_dev || !out_dev) return MAPLE_ERR_ARG;
    if (nQ == 0 || nC == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(need_model(c));
    TRY(settle(c));
    return launch_append_queries(c, (hipStream_t)stream, nQ, qList_dev, nC, cand_dev, isTipC, bLen, out_dev,
                                 nC, nullptr, nullptr, nullptr, MAPLE_K_APPEND_QUERIES, 0.0);
}

// Q queries x C candidates without the score matrix: per query the best score and the candidate that has it (exact
// ties to the smallest visitRank, or to the smallest index when visitRank is NULL).
extern "C" int maple_append_queries_argmax_dev(maple_ctx *c, int32_t nQ, const int32_t *qList_dev, int32_t nC,
                                               const int32_t *cand_dev, const int32_t *visitRank_dev, int isTipC, double bLen,
                                               double *bestScore_dev, int32_t *bestIdx_dev, void *stream)
{
    if (!c || nQ < 0 || nC < 0 || !qList_dev || !cand_dev || !bestScore_dev || !bestIdx_dev) return MAPLE_ERR_ARG;
    if (nQ == 0 || nC == 0) return MAPLE_OK;
    HIPCK(c, hipSetDevice(c->device));
    TRY(need_model(c));
    TRY(settle(c));
    const int nChunks = (nC + 63) / 64;
    HIPCK(c, c->s_tilebest.reserve((size_t)nQ * nChunks * sizeof(TileBest)));
    TileBest *tb = (TileBest *)c->s_tilebest.p;
    TRY(launch_append_queries(c, (hipStream_t)stream, nQ, qList_dev, nC, cand_dev, isTipC, bLen, nullptr, 0, nullptr, nullptr, nullptr,
                              MAPLE_K_APPEND_QUERIES, 0.0, tb, visitRank_dev));
    hipLaunchKernelGGL(k_argmax_reduce, dim3(nQ), dim3(64), 0, (hipStream_t)stream, nQ, nChunks, tb, bestScore_dev, bestIdx_dev);
    HIPCK(c, hipGetLastError());
    return MAPLE_OK;
}
