// maple_amd/csrc/branch_walk_host.h -- the host side the three calls that walk every branch of the uploaded tree share (em.hip,
// error_probs.hip, mat_events.hip): the rows of branch_walk_plan.h from the context's columns, the parent lists of reference
// branches passed down in one launch, the reference nucleotides on the device, the walks' block size and a launch bracketed by
// its timing pair.  Each entry function then reads: prologue (begin_tree_call, batch_host.h), gather,
// pass, upload the rows, launch, scan / copy back.
#pragma once
#include "batch_host.h"
#include "branch_walk_plan.h"

#define WALK_BLOCK 256                 // k_em_walk, k_err_walk, k_mat_walk: ONE LANE per branch, 256 branches per block

static int gather_branches(maple_ctx *c, branch_walk_plan::Rule rule, const int32_t *nMinor, branch_walk_plan::Rows &rows)
{
    const branch_walk_plan::Columns t{(int32_t)c->h_tree_up.size(), c->dtree.root, c->h_tree_up.data(), c->h_tree_c0.data(),
                                      c->h_tree_c1.data(), c->h_tree_dist.data(), c->h_tree_lower.data(), c->h_tree_upLeft.data(),
                                      c->h_tree_upRight.data(), c->h_tree_mut.data(), nMinor, (int32_t)c->h_n_ent.size(),
                                      (int32_t)c->h_mut_cnt.size(), c->dm.usingErrorRate != 0};
    const branch_walk_plan::Status s = branch_walk_plan::gather(rule, t, rows);
    if (s == branch_walk_plan::OK) return MAPLE_OK;
    return fail(c, s == branch_walk_plan::BAD_ARG ? MAPLE_ERR_ARG : MAPLE_ERR_STATE, "%s", rows.message.c_str());
}

// M:10154-10155 / M:9813-9814: the parent lists of the rows above a reference branch go down through the node's mutation list,
// all in one maple_pass_branch_batch; the new lists (the caller holds an arena mark) replace rows.pList.  timed: the pass, its
// commit and their waits are bracketed by an event pair like the walks (maple_timing_*).
static int pass_parent_lists(maple_ctx *c, branch_walk_plan::Rows &rows, bool timed)
{
    const size_t n = rows.passIdx.size();
    if (!n) return MAPLE_OK;
    std::vector<int32_t> list(n), mut(n), out(n, -1);
    const std::vector<uint8_t> down(n, 0);
    for (size_t k = 0; k < n; k++) { list[k] = rows.pList[rows.passIdx[k]]; mut[k] = rows.mut[rows.passIdx[k]]; }
    hipEvent_t p0, p1;
    if (timed) {
        TRY(ev_pair(c, &p0, &p1, MAPLE_K_OTHER, (double)n, 0.0));
        HIPCK(c, hipEventRecord(p0, c->stream));
    }
    const int rc = maple_pass_branch_batch(c, (int32_t)n, list.data(), mut.data(), down.data(), out.data());
    if (timed) HIPCK(c, hipEventRecord(p1, c->stream));                  // (also when the pass failed: a pair is read as a pair)
    TRY(rc);
    for (size_t k = 0; k < n; k++) {
        if (out[k] < 0)
            return fail(c, MAPLE_ERR_FATAL, "node %d: its parent's upper list could not be passed through its mutation list",
                        rows.node[rows.passIdx[k]]);
        rows.pList[rows.passIdx[k]] = out[k];
    }
    return MAPLE_OK;
}

// the reference nucleotides on the device, one copy per context, uploaded on the call's stream on first use
static int device_ref_idx(maple_ctx *c, const uint8_t **refIdx)
{
    if (!c->d_refIdx.p) {
        HIPCK(c, c->d_refIdx.reserve_exact((size_t)c->lRef));
        const hipError_t e = hipMemcpyAsync(c->d_refIdx.p, c->refIdx.data(), (size_t)c->lRef, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) c->d_refIdx.release();                      // (a buffer that was never filled is not kept)
        HIPCK(c, e);
    }
    *refIdx = c->d_refIdx.p;
    return MAPLE_OK;
}

// one walk launch bracketed by an event pair of its own (maple_timing_*: the kernel's time, what tools/*_stats.py report);
// units = the items walked
template <class Launch> static int timed_launch(maple_ctx *c, int32_t units, Launch launch)
{
    hipEvent_t e0, e1;
    TRY(ev_pair(c, &e0, &e1, MAPLE_K_OTHER, (double)units, 0.0));
    HIPCK(c, hipEventRecord(e0, c->stream));
    launch();
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipEventRecord(e1, c->stream));
    return MAPLE_OK;
}
