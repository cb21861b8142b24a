// maple_amd/csrc/branch_walk_plan.h -- which branches of the uploaded tree the EM step (em.hip), the error report (error_probs.hip)
// and the mutation events (mat_events.hip) walk, and in which order, as pure host code: no HIP, no context, nothing but the
// standard library, so that it compiles on its own and is tested on the CPU (tests/branch_walk_plan_main.cpp,
// tests/test_branch_walk_plan.py).  Each of the three calls walks one item per row of what gather() returns: the parent's upper
// list (pList) against the node's lower list (cList), one lane per row.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace branch_walk_plan {

enum Rule {
    // expectationMaximizationCalculationRates, M:10140-10155: a node is an item iff up >= 0 && (dist != 0.0 || (U && leaf));
    // numTips = the sum over the leaves of 1 + nMinor.  Preorder with the children[1] subtree BEFORE the children[0] subtree:
    // the totals do not depend on the order as numbers, but k_em_walk adds them block by block, so their bits do -- this is the
    // order the call has always had.
    EM = 0,
    // the same loop under trackMutations: every node the root reaches is an item and needs a lower list; pList = -1 (a
    // single-list item, M:10808-10826) where the EM rule says no.  Preorder, children[0] first (the order is the launch's only).
    EVENTS = 1,
    // calculateErrorProbabilities, M:9801-9812: `leaves` = all leaves in the order the reference's traversal meets them
    // (children[0] first); a leaf is an item iff nMinor == 0 && up >= 0; itemLeaf = the item's index into `leaves`.
    ERRORS = 2,
};

enum Status { OK = 0, BAD_ARG = 1, BAD_STATE = 2 };   // (the caller's MAPLE_ERR_ARG / MAPLE_ERR_STATE)

struct Columns {                       // the host's copy of the uploaded tree, n nodes
    int32_t n, root;
    const int32_t *up, *c0, *c1;
    const double *dist;
    const int32_t *lower, *upLeft, *upRight, *mut;
    const int32_t *nMinor;             // len(minorSequences[v]); null: none anywhere
    int32_t nLists, nMutLists;         // list ids are 0 .. nLists - 1, mutation-list ids 0 .. nMutLists - 1
    bool usingErrorRate;               // U
};

struct Rows {
    std::vector<int32_t> node, pList, cList, mut, leafMinor;   // leafMinor: nMinor of a leaf, -1 for an internal node
    std::vector<int32_t> refNode;      // the node's nearest ancestor-or-self with a mutation list (the reference frame it lives in
                                       // as the columns stand now, whatever a patch has moved), -1 where there is none
    std::vector<double> dist;
    std::vector<int32_t> passIdx;      // the rows with mut >= 0 (their pList goes down through the mutation list first)
    int64_t numTips = 0;               // EM
    std::vector<int32_t> leaves, itemLeaf;   // ERRORS
    std::string message;               // of a status other than OK
    int32_t size() const { return (int32_t)node.size(); }
    // gather()'s own: a caller that keeps its Rows from call to call keeps their memory too (a tree's worth of fresh pages per
    // column costs more than the traversal)
    std::vector<int32_t> stack, refOf;   // refOf: per node reached its refNode, UNSEEN before
    void clear()
    {
        for (auto *c : {&node, &pList, &cList, &mut, &leafMinor, &refNode, &passIdx, &leaves, &itemLeaf}) c->clear();
        dist.clear(); stack.clear(); message.clear();
        numTips = 0;
    }
};

// Iterative (an explicit stack: a caterpillar of any length costs heap, not call frames).  Columns that are no tree below the
// root are refused (as tree_lk_plan::lk_postorder refuses them), so no index taken from them is used unchecked.
inline Status gather(Rule rule, const Columns &t, Rows &r)
{
    r.clear();
    char buf[256];
    auto fail = [&](Status s, const char *fmt, int32_t a, int32_t b = 0, int32_t c = 0) {
        snprintf(buf, sizeof buf, fmt, a, b, c);
        r.message = buf;
        return s;
    };
    const char *noTree = "node %d: the columns are no tree (an index out of range, one child only, a node reached twice)";
    if (t.n <= 0 || t.root < 0 || t.root >= t.n || t.up[t.root] >= 0) return fail(BAD_STATE, noTree, t.root);
    const bool U = t.usingErrorRate;
    const int32_t UNSEEN = -2;
    std::vector<int32_t> &refOf = r.refOf, &st = r.stack;
    refOf.assign((size_t)t.n, UNSEEN);
    st.push_back(t.root);
    while (!st.empty()) {
        const int32_t v = st.back();
        st.pop_back();
        const int32_t a = t.c0[v], b = t.c1[v];
        const bool leaf = a < 0 && b < 0;
        if (refOf[v] != UNSEEN || (!leaf && (a < 0 || b < 0 || a >= t.n || b >= t.n || a == b || t.up[a] != v || t.up[b] != v)))
            return fail(BAD_STATE, noTree, v);
        const int32_t p = t.up[v], mu = t.mut[v], ref = mu >= 0 ? v : (p < 0 ? -1 : refOf[p]);   // (p was reached first)
        refOf[v] = ref;
        if (!leaf) {
            st.push_back(rule == EM ? a : b);
            st.push_back(rule == EM ? b : a);
        }
        const int32_t nm = t.nMinor ? t.nMinor[v] : 0;
        if (nm < 0) return fail(BAD_ARG, "nMinor[%d] = %d", v, nm);
        if (leaf) r.numTips += 1 + nm;                                   // M:10140-10142
        if (rule == ERRORS && !leaf) continue;
        const bool pair = rule == ERRORS ? (nm == 0 && p >= 0)           // M:9805 (a root without children: the reference fails on up[root])
                                         : (p >= 0 && (t.dist[v] != 0.0 || (U && leaf)));   // M:10146
        if (pair || rule == EVENTS) {
            int32_t pList = -1;
            const int32_t cList = t.lower[v];
            if (pair) {
                pList = (t.c0[p] == v) ? t.upRight[p] : t.upLeft[p];     // M:10150-10153, M:9809-9812
                if (pList < 0 || pList >= t.nLists) return fail(BAD_STATE, "node %d: the branch above it has no upper list of its parent", v);
                if (mu >= t.nMutLists)                                   // (of the pairs only: maple_tree_upload refuses such an id on any
                    return fail(BAD_STATE, "node %d: mutList[] = %d is not a mutation-list id (have %d)", v, mu, t.nMutLists);   // node)
                if (mu >= 0) r.passIdx.push_back(r.size());
            }
            if (cList < 0 || cList >= t.nLists) return fail(BAD_STATE, "node %d has no lower list", v);
            if (rule == ERRORS) r.itemLeaf.push_back((int32_t)r.leaves.size());
            r.node.push_back(v); r.pList.push_back(pList); r.cList.push_back(cList); r.mut.push_back(pair ? mu : -1);
            r.dist.push_back(t.dist[v]); r.leafMinor.push_back(leaf ? nm : -1); r.refNode.push_back(ref);
        }
        if (rule == ERRORS) r.leaves.push_back(v);
    }
    return OK;
}

}  // namespace branch_walk_plan
