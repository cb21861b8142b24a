// maple_amd/csrc/update_plan.h -- the level loops of updatePartials (MAPLEv0.7.5.4.py:5479-5815) and of reCalculateAllGenomeLists
// (M:6013-6347) as pure host code: no HIP, no context, nothing but the standard library, so that it compiles on its own and is
// tested on the CPU (tests/update_plan_main.cpp, tests/test_update_plan.py).  maple_update_partials and maple_tree_rebuild_lists
// (update.hip) are repair_drive() and rebuild_drive() below with the batch entry points of the library plugged in as `Ops`:
//   ops.pass(n, lists, mutLists, dirUp, out)          passGenomeListThroughBranch of n lists (M:3749-3877)
//   ops.items(B, first, n)                            items [first, first + n) of a Batch -> B.out / B.none / B.diff (see Batch)
//   ops.blen(upList, lowList, tip, &t, &isFalse)      estimateBranchLengthWithDerivative of one branch
//   ops.rootVector(n, lists, bLen, tip, rootMut, out) rootVector of n (<= 2) lists below the root (rootMut: its mutation list or -1)
//   ops.differ(a, b, &different)                      areVectorsDifferent(a, b)
// each returning 0 or an error code of its own, which the drivers hand on unchanged.
//
// The reference repairs the genome lists around ONE change with a LIFO work list of (node, direction) items, one mergeVectors at
// a time.  Here the lists invalidated by ANY number of simultaneous changes are repaired level by level -- phase A up (lower
// lists, deepest level first), phase B down (probVectTotUp / probVectUpRight / probVectUpLeft, shallowest first) -- every level
// one Batch, with the reference's own stop rule (areVectorsDifferent, M:5645-5658 / 5793) deciding where the repair ends.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace update_plan {

constexpr int ERR_ARG = 1, ERR_FATAL = 2;         // Error::kind: the caller's columns are wrong / the lists are
constexpr int FAILED = INT_MIN;                   // what a driver returns after Error::fail
#define UP_TRY(x) do { const int rc_ = (x); if (rc_) return rc_; } while (0)

struct Error {                                    // an error of the plan's own (an operation's error code is handed on as it is)
    int kind = 0;
    char msg[512] = "";
    int fail(int k, const char *fmt, ...) __attribute__((format(printf, 3, 4)))
    {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof msg, fmt, ap);
        va_end(ap);
        kind = k;
        return FAILED;
    }
};

struct Tree {                                     // the caller's columns, updated in place (depth: the repair only)
    int32_t n, root;
    const int32_t *up, *c0, *c1;
    const uint8_t *tip;
    const int32_t *mut, *depth;
    double *dist;
    int32_t *lower, *upRight, *upLeft, *totUp;
    int32_t upListOf(int v) const { const int p = up[v]; return c0[p] == v ? upRight[p] : upLeft[p]; }
};

// lists[i] passed through the branch above nodes[i] (up or down) where that branch carries mutations, M:3749-3877 (nodes[i] < 0: no branch)
template <class Ops>
int passed(const Tree &T, Ops &ops, int32_t *ids, const int32_t *nodes, size_t n, bool dirUp)
{
    std::vector<int32_t> src, ml, where;
    for (size_t i = 0; i < n; i++)
        if (nodes[i] >= 0 && T.mut[nodes[i]] >= 0 && ids[i] >= 0) { src.push_back(ids[i]); ml.push_back(T.mut[nodes[i]]); where.push_back((int32_t)i); }
    if (src.empty()) return 0;
    std::vector<int32_t> out(src.size());
    UP_TRY(ops.pass((int32_t)src.size(), src.data(), ml.data(), dirUp, out.data()));
    for (size_t i = 0; i < where.size(); i++) ids[where[i]] = out[i];
    return 0;
}
// the upper vector seen by each node, in the node's own reference frame (M:5503-5513)
template <class Ops>
int vect_up_of(const Tree &T, Ops &ops, const std::vector<int32_t> &nodes, std::vector<int32_t> &out)
{
    out.resize(nodes.size());
    for (size_t i = 0; i < nodes.size(); i++) out[i] = T.upListOf(nodes[i]);
    return passed(T, ops, out.data(), nodes.data(), nodes.size(), false);
}

enum Kind : uint8_t { TOT_UP = 0, UP_RIGHT = 1, UP_LEFT = 2, LOWER = 3 };

// One level's items: mergeVectors(l1, b1, t1, l2, b2, t2, ud), then what the item's mode says -- mode 0 (a lower list,
// M:5760-5800): shorten(), then areVectorsDifferent(new, old); mode 1: shorten(); mode 2 (probVectUpRight / UpLeft, M:5559-5660):
// areVectorsDifferent(old, new), and shorten() only if they differ.  out[i]: the new list (-1: None from the merge, or mode 2
// and not different: nothing to replace); none[i] = 1 if the merge itself came out None; diff[i] = the areVectorsDifferent
// verdict (1 where none was asked).  The new lists take their arena room in item order.
struct Batch {
    std::vector<int32_t> l1, l2, old, node, kid1, kid2, out;   // kid1 / kid2: the child whose lower list l1 / l2 is (-1: none)
    std::vector<double> b1, b2;
    std::vector<uint8_t> t1, t2, ud, mode, kind, none, diff;
    size_t n = 0;                                 // items; the columns keep their largest size so far
    size_t size() const { return n; }

    // The columns as plain pointers and the next free item: a local of the loop that fills a batch, so that the stores of one
    // item make nothing be read again for the next (a byte store may alias any vector's bookkeeping, never a local).
    struct Fill {
        int32_t *l1, *l2, *old, *node, *kid1, *kid2;
        double *b1, *b2;
        uint8_t *t1, *t2, *ud, *mode, *kind;
        size_t n;
        void add(int32_t L1, double B1, uint8_t T1, int32_t K1, int32_t L2, double B2, uint8_t T2, int32_t K2, uint8_t upDown, uint8_t md,
                 int32_t oldList, int32_t v, Kind k)
        {
            l1[n] = L1; b1[n] = B1; t1[n] = T1; kid1[n] = K1; l2[n] = L2; b2[n] = B2; t2[n] = T2; kid2[n] = K2;
            ud[n] = upDown; mode[n] = md; old[n] = oldList; node[n] = v; kind[n] = k;
            n++;
        }
        // the lower list of v from its two children (M:5760-5800 / 6031-6200); md 0: compared with the list v has; false: v has no two children
        bool lower(const Tree &T, int v, uint8_t md)
        {
            const int a = T.c0[v], b = T.c1[v];
            if (a < 0 || b < 0 || a >= T.n || b >= T.n) return false;
            add(T.lower[a], T.dist[a], T.tip[a], a, T.lower[b], T.dist[b], T.tip[b], b, 0, md, md == 0 ? T.lower[v] : -1, v, LOWER);
            return true;
        }
        // probVectTotUp of v: its upper vector and its lower list, half the branch each (M:5525-5557 / 6262-6275)
        void totUp(const Tree &T, int v, int32_t vectUp) { add(vectUp, T.dist[v] / 2, 0, -1, T.lower[v], T.dist[v] / 2, T.tip[v], -1, 1, 1, -1, v, TOT_UP); }
        // probVectUpRight (which = 1: upper vector + child 1, for child 0) / probVectUpLeft (which = 0: upper vector + child 0, for
        // child 1) of v (M:5559-5660 / 6277-6345); compare: replaced only where areVectorsDifferent(old, new)
        void upper(const Tree &T, int v, int which, int32_t vectUp, bool compare)
        {
            const int kd = which == 1 ? T.c1[v] : T.c0[v];
            add(vectUp, T.dist[v], 0, -1, T.lower[kd], T.dist[kd], T.tip[kd], kd, 1, compare ? 2 : 1,
                compare ? (which == 1 ? T.upRight[v] : T.upLeft[v]) : -1, v, which == 1 ? UP_RIGHT : UP_LEFT);
        }
    };
    // start a batch of at most `room` items (the columns grow geometrically and are never shrunk); done(F) ends it
    Fill fill(size_t room)
    {
        if (l1.size() < room) {
            room = std::max(room, 2 * l1.size());
            for (auto *c : {&l1, &l2, &old, &node, &kid1, &kid2, &out}) c->resize(room);
            for (auto *c : {&t1, &t2, &ud, &mode, &kind, &none, &diff}) c->resize(room);
            b1.resize(room); b2.resize(room);
        }
        return Fill{l1.data(), l2.data(), old.data(), node.data(), kid1.data(), kid2.data(), b1.data(), b2.data(),
                    t1.data(), t2.data(), ud.data(), mode.data(), kind.data(), 0};
    }
    void done(const Fill &F) { n = F.n; }
    // the children's lower lists go through their own branches first where those carry mutations; then the whole batch
    template <class Ops> int run(const Tree &T, Ops &ops)
    {
        if (n && kind[0] == LOWER) UP_TRY(passed(T, ops, l1.data(), kid1.data(), n, true));   // (a batch is of lower or of upper items)
        UP_TRY(passed(T, ops, l2.data(), kid2.data(), n, true));
        std::fill_n(out.begin(), n, -1); std::fill_n(none.begin(), n, 0); std::fill_n(diff.begin(), n, 0);
        return ops.items(*this, (size_t)0, n);
    }
};

// Which arms the last repair took, for the tests (maple_debug_update_partials_stats): the names once, in the order of the counters.
// rounds: rounds of phase A + phase B; phaseA_none: a lower merge that came out None between two zero-length branches, and the
// branch re-estimated first / second for it; upper_none_*: a None upper merge by kind, the ones skipped because the node's other
// merge had dealt with it, and the re-estimates of the node's / the merged child's branch; root_*: the root's upper lists made
// (probVectUpRight / UpLeft) or kept because rootVector came out as it was; totup_cleared: a probVectTotUp dropped over length 0;
// items_*: the items of the level batches by mode, and those of mode 0 / 2 that had no old list to compare with.
#define UPDATE_PLAN_STATS(X)                                                                                                     \
    X(rounds) X(phaseA_none) X(phaseA_reest_first) X(phaseA_reest_second)                                                        \
    X(upper_none_totup) X(upper_none_upright) X(upper_none_upleft) X(upper_deferred_skip) X(upper_reest_node) X(upper_reest_child) \
    X(root_right_made) X(root_left_made) X(root_kept) X(totup_cleared)                                                           \
    X(items_mode0) X(items_mode1) X(items_mode2) X(items_old_absent)
struct Stats {
#define UPDATE_PLAN_STAT_FIELD(name) int64_t name = 0;
    UPDATE_PLAN_STATS(UPDATE_PLAN_STAT_FIELD)
#undef UPDATE_PLAN_STAT_FIELD
};

struct Scratch {                                  // persistent between calls: flags per node, cleared through the touched list
    std::vector<uint8_t> dLow, dUp, dDist, dCh0, dCh1, inFrontier, inTodo;
    std::vector<int32_t> touched;
    Batch batch;                          // the level's items of the repair (kept: a call allocates nothing once it is warm)
    std::vector<int32_t> replacedNodes;   // nodes one of whose four lists (or whose branch length) the last call replaced
    std::vector<int32_t> visitedNodes;    // nodes the last call visited (with repeats): the changed nodes, every node that entered
                                          // phase A's frontier or phase B's todo list, the nodes whose length was re-estimated --
                                          // the ones the reference's updatePartials sets `dirty` for (M:5499-5500, 5410-5411)
    Stats stats;                          // the arms the last call took
    bool keepRootRight = false;           // the caller's, kept across calls: the root's probVectUpRight is not made again although the
                                          // root's child 1 changed -- the reference's sweep repairs BOTH children of the root with the
                                          // work list [(child, 2), (root, 0)] (M:8790, 8796), which for child 1 makes the root's lower
                                          // list again and leaves the list child 0 sees as it was (maple_tree_optimize_blens sets it)
    void fit(size_t n)
    {
        if (dLow.size() < n) {
            dLow.assign(n, 0); dUp.assign(n, 0); dDist.assign(n, 0); dCh0.assign(n, 0); dCh1.assign(n, 0);
            inFrontier.assign(n, 0); inTodo.assign(n, 0);
            touched.clear();
        }
    }
    void touch(int v) { touched.push_back(v); visitedNodes.push_back(v); }   // (every touched node ends up in phase B's todo list)
    void clear()
    {
        for (int v : touched) dLow[v] = dUp[v] = dDist[v] = dCh0[v] = dCh1[v] = inFrontier[v] = inTodo[v] = 0;
        touched.clear();
    }
};

// One call of the repair: what the rounds share (replaced, the nodes an earlier round left undone) and one round's work lists.
template <class Ops> struct Repair {
    const Tree &T;
    Scratch &S;
    Ops &ops;
    Error &E;
    bool verbose;
    int replaced = 0, roundNo = 0;
    bool badNode = false;                         // (the caller's columns are trusted only as far as they are read: every relative
                                                  // that enters the work lists is range-checked)
    std::vector<int32_t> redoNow, redoNext;       // nodes whose upper vectors an earlier round left undone
    std::vector<int32_t> next;                    // nodes whose length a re-estimate made non-zero: the next round's changes
    std::vector<int32_t> frontier, todo, nodes, rest, vu, deferred;
    Batch &B = S.batch;

    bool okNode(int v) { if (v < -1 || v >= T.n) { badNode = true; return false; } return v >= 0; }
    void markChild(int p, int which) { (which == 0 ? S.dCh0 : S.dCh1)[p] = 1; S.touch(p); }
    // v's lower list or length changed: its parent's lower list is to be made again
    void toParent(int v)
    {
        const int p = T.up[v];
        if (!okNode(p)) return;
        markChild(p, T.c0[p] == v ? 0 : 1);
        if (!S.inFrontier[p]) { S.inFrontier[p] = 1; frontier.push_back(p); }
    }
    // the level's batch, counted by mode, then run
    int runBatch()
    {
        for (size_t k = 0; k < B.size(); k++) {
            (B.mode[k] == 0 ? S.stats.items_mode0 : B.mode[k] == 1 ? S.stats.items_mode1 : S.stats.items_mode2)++;
            if (B.mode[k] != 1 && B.old[k] < 0) S.stats.items_old_absent++;
        }
        return B.run(T, ops);
    }
    void addTodo(int v) { if (!S.inTodo[v]) { S.inTodo[v] = 1; S.touch(v); todo.push_back(v); } }
    // the nodes of `work` at its deepest / shallowest depth, ascending, into `nodes`; the others stay
    void takeLevel(std::vector<int32_t> &work, bool deepest, std::vector<uint8_t> &flag)
    {
        int d = deepest ? -1 : 1 << 30;
        for (int v : work) d = deepest ? std::max(d, T.depth[v]) : std::min(d, T.depth[v]);
        nodes.clear(); rest.clear();
        for (int v : work) (T.depth[v] == d ? nodes : rest).push_back(v);
        work.swap(rest);
        std::sort(nodes.begin(), nodes.end());
        for (int v : nodes) flag[v] = 0;
    }
    // updateBLen (M:5385-5414): the branch above w estimated again from the lists on its two sides
    int reestimate(int w)
    {
        std::vector<int32_t> one{w}, vu1;
        UP_TRY(vect_up_of(T, ops, one, vu1));
        double t = 0.0;
        uint8_t isFalse = 0;
        UP_TRY(ops.blen(vu1[0], T.lower[w], T.tip[w], &t, &isFalse));
        T.dist[w] = isFalse ? 0.0 : t;
        S.replacedNodes.push_back(w);
        return 0;
    }
    // a new probVectUpRight / probVectUpLeft of v: the child that sees it is next
    void newUpper(int v, int kind, int32_t id)
    {
        (kind == UP_RIGHT ? T.upRight : T.upLeft)[v] = id;
        S.replacedNodes.push_back(v);
        replaced++;
        const int target = kind == UP_RIGHT ? T.c0[v] : T.c1[v];
        S.dUp[target] = 1; S.touch(target);
        addTodo(target);
    }

    void seed(const std::vector<int32_t> &chg)
    {
        frontier.clear();
        for (int v : chg) { S.dLow[v] = 1; S.dDist[v] = 1; S.touch(v); toParent(v); }
    }

    // ---- phase A: lower lists, deepest first ------------------------------------------------------------------------------
    int phaseA()
    {
        while (!frontier.empty()) {
            takeLevel(frontier, true, S.inFrontier);
            Batch::Fill F = B.fill(nodes.size());
            for (int v : nodes)
                if (!F.lower(T, v, 0)) return E.fail(ERR_ARG, "node %d has a changed child but no two (valid) children", v);
            B.done(F);
            UP_TRY(runBatch());
            for (size_t k = 0; k < B.size(); k++) {
                if (!B.none[k]) continue;
                S.stats.phaseA_none++;
                // None between two zero-length branches: re-estimate the branch above the changed child, like updateBLen
                // (M:5385-5414, 5689-5701)
                const int p = nodes[k];
                if (B.b1[k] != 0.0 || B.b2[k] != 0.0)
                    return E.fail(ERR_FATAL, "None vector from non-zero distances in the lower merge at node %d (the reference raises too)", p);
                const int first = S.dCh0[p] ? 0 : 1;
                for (int oi = 0; oi < 2; oi++) {
                    const int which = oi == 0 ? first : 1 - first;
                    const int ch = which == 0 ? T.c0[p] : T.c1[p];
                    UP_TRY(reestimate(ch));
                    (oi == 0 ? S.stats.phaseA_reest_first : S.stats.phaseA_reest_second)++;
                    S.dLow[ch] = 1; S.dDist[ch] = 1; S.touch(ch);
                    markChild(p, which);
                    if (T.dist[ch] != 0.0) break;
                }
                B.b1[k] = T.dist[B.kid1[k]]; B.b2[k] = T.dist[B.kid2[k]];
                UP_TRY(ops.items(B, k, (size_t)1));
                if (B.none[k]) return E.fail(ERR_FATAL, "None vector after updateBLen at node %d", p);
                // (after updateBLen the reference goes on to p's parent whatever the new list looks like -- madeChange, M:5694,
                // 5808-5812 -- and sets `dirty` for it; here the new list decides below, and the parent counts as visited)
                if (okNode(T.up[p])) S.visitedNodes.push_back(T.up[p]);
            }
            for (size_t k = 0; k < B.size(); k++) {
                const int v = nodes[k];
                T.lower[v] = B.out[k];
                S.replacedNodes.push_back(v);
                replaced++;
                if (!B.diff[k]) continue;
                S.dLow[v] = 1; S.touch(v);
                toParent(v);
            }
        }
        return 0;
    }

    // the root's probVectUpRight / probVectUpLeft: rootVector of the other child's lower list (M:5715-5735)
    int rootLevel()
    {
        const int r = T.root;
        if (T.c0[r] < 0) return 0;
        for (int which = 1; which >= 0; which--) {                         // upRight merges child 1, upLeft child 0
            if (!(which == 0 ? S.dCh0[r] : S.dCh1[r])) continue;
            if (which == 1 && S.keepRootRight) continue;
            const int k = which == 1 ? T.c1[r] : T.c0[r];
            std::vector<int32_t> one{k}, pl{T.lower[k]};
            UP_TRY(passed(T, ops, pl.data(), one.data(), 1, true));
            int32_t res = -1;
            UP_TRY(ops.rootVector(1, pl.data(), &T.dist[k], &T.tip[k], T.mut[r], &res));
            const int32_t have = which == 1 ? T.upRight[r] : T.upLeft[r];
            uint8_t df = 1;
            if (have >= 0) UP_TRY(ops.differ(have, res, &df));
            if (df) { newUpper(r, which == 1 ? UP_RIGHT : UP_LEFT, res); (which == 1 ? S.stats.root_right_made : S.stats.root_left_made)++; }
            else S.stats.root_kept++;
        }
        return 0;
    }

    // An inconsistency between zero-length branches in item i (M:5522-5528, 5568-5600): the reference re-estimates the branch
    // above the node (updateBLen) and, if that stays at zero, the branch above the child that was being merged, then repairs from
    // there.  Here: the same estimates, and the node whose length changed starts another round of the level loops.
    int noneUpper(size_t i)
    {
        const int v = B.node[i], kd = B.kid2[i];
        if (verbose)
            fprintf(stderr, "[maple] updatePartials round %d: None %s at node %d (length %.3g), child %d (length %.3g), merged with b1 %.3g b2 %.3g\n",
                    roundNo, B.kind[i] == TOT_UP ? "probVectTotUp" : (B.kind[i] == UP_RIGHT ? "probVectUpRight" : "probVectUpLeft"), v, T.dist[v], kd,
                    kd >= 0 ? T.dist[kd] : -1.0, B.b1[i], B.b2[i]);
        (B.kind[i] == TOT_UP ? S.stats.upper_none_totup : B.kind[i] == UP_RIGHT ? S.stats.upper_none_upright : S.stats.upper_none_upleft)++;
        if (std::find(deferred.begin(), deferred.end(), v) != deferred.end()) { S.stats.upper_deferred_skip++; return 0; }   // (its other merge already dealt with it)
        if (B.kind[i] != TOT_UP && (T.dist[v] != 0.0 || T.dist[kd] != 0.0))
            return E.fail(ERR_FATAL, "None upper vector from non-zero distances at node %d (the reference raises too)", v);
        deferred.push_back(v);
        redoNext.push_back(v);
        for (int w : {v, kd}) {
            if (w < 0 || T.up[w] < 0) continue;
            UP_TRY(reestimate(w));
            (w == v ? S.stats.upper_reest_node : S.stats.upper_reest_child)++;
            S.visitedNodes.push_back(w);
            S.visitedNodes.push_back(T.up[w]);
            if (T.dist[w] != 0.0) { next.push_back(w); return 0; }
        }
        return E.fail(ERR_FATAL, "None upper vector at node %d and no branch length to lengthen", v);
    }

    // ---- phase B: upper lists, shallowest first ---------------------------------------------------------------------------
    int phaseB()
    {
        todo.clear();
        {
            std::vector<int32_t> seen(S.touched);
            std::sort(seen.begin(), seen.end());
            seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
            for (int v : seen)
                if ((S.dLow[v] || S.dCh0[v] || S.dCh1[v]) && !S.inTodo[v]) { S.inTodo[v] = 1; todo.push_back(v); }
        }
        for (int v : redoNow) { S.dUp[v] = 1; S.touch(v); addTodo(v); }
        while (!todo.empty()) {
            takeLevel(todo, false, S.inTodo);
            if (nodes[0] == T.root) {
                UP_TRY(rootLevel());
                if (nodes.size() == 1) continue;
                nodes.erase(nodes.begin());                                // (only the root has depth 0)
            }
            for (int v : nodes) if (T.up[v] < 0 || T.up[v] >= T.n) return E.fail(ERR_ARG, "node %d: parent index out of range", v);
            UP_TRY(vect_up_of(T, ops, nodes, vu));
            // One batch for the level, node by node: probVectTotUp where the node's lower list, length or upper vector changed,
            // probVectUpRight and probVectUpLeft where the upper vector, the length or that child changed
            Batch::Fill F = B.fill(3 * nodes.size());
            for (size_t k = 0; k < nodes.size(); k++) {
                const int v = nodes[k];
                if (S.dUp[v] || S.dLow[v]) {
                    if (T.dist[v] == 0.0) { if (T.totUp[v] != -1) S.replacedNodes.push_back(v); T.totUp[v] = -1; S.stats.totup_cleared++; }
                    else F.totUp(T, v, vu[k]);
                }
                if (T.c0[v] < 0) continue;
                if (T.c0[v] >= T.n || T.c1[v] < 0 || T.c1[v] >= T.n) return E.fail(ERR_ARG, "node %d: child index out of range", v);
                for (int which = 1; which >= 0; which--)
                    if (S.dUp[v] || S.dDist[v] || (which == 0 ? S.dCh0[v] : S.dCh1[v])) F.upper(T, v, which, vu[k], true);
            }
            B.done(F);
            if (B.size() == 0) continue;
            UP_TRY(runBatch());
            deferred.clear();                                              // nodes of this level that met an inconsistency
            for (size_t i = 0; i < B.size(); i++) if (B.none[i]) UP_TRY(noneUpper(i));
            // (the reference recomputes ALL of such a node's vectors with the new length before anything goes on to its children,
            // M:5575-5600: none of what this level computed for it with the old length is used; the next round redoes the node)
            for (size_t i = 0; i < B.size(); i++) {
                const int v = B.node[i];
                if (B.none[i] || std::find(deferred.begin(), deferred.end(), v) != deferred.end()) continue;
                if (B.kind[i] == TOT_UP) { T.totUp[v] = B.out[i]; S.replacedNodes.push_back(v); replaced++; }
                else if (B.diff[i]) newUpper(v, B.kind[i], B.out[i]);
            }
        }
        return 0;
    }

    int round(const std::vector<int32_t> &chg)
    {
        seed(chg);
        UP_TRY(phaseA());
        UP_TRY(phaseB());
        if (badNode) return E.fail(ERR_ARG, "a relative index of a touched node is out of range");
        return 0;
    }
};

// updatePartials around changed[0 .. nChanged): rounds of phase A + phase B until no zero-length branch is left inconsistent
template <class Ops>
int repair_drive(const Tree &T, Scratch &S, Ops &ops, int32_t nChanged, const int32_t *changed, bool verbose, Error &E, int32_t *nReplaced)
{
    S.fit((size_t)T.n);
    S.clear();
    S.replacedNodes.clear();
    S.visitedNodes.clear();
    S.stats = Stats{};
    Repair<Ops> R{T, S, ops, E, verbose};
    std::vector<int32_t> chg(changed, changed + nChanged);
    int rc = 0;
    for (int round = 0; !rc && (!chg.empty() || !R.redoNext.empty()); round++) {
        if (round >= 64) { rc = E.fail(ERR_FATAL, "updatePartials keeps finding inconsistent zero-length branches"); break; }
        R.next.clear();
        R.roundNo = round;
        S.stats.rounds++;
        R.redoNow.swap(R.redoNext);
        R.redoNext.clear();
        rc = R.round(chg);
        S.clear();
        chg.swap(R.next);
    }
    if (!rc) *nReplaced = R.replaced;
    return rc;
}

// reCalculateAllGenomeLists (M:6013-6347) level by level: given the tips' lower lists, every internal node's probVect (pass 1,
// M:6031-6200: deepest level first) and every node's probVectUpRight / probVectUpLeft / probVectTotUp (pass 2, M:6226-6345: from
// the root down), each level ONE Batch.
// bumpLen = 0: a None between two zero-length branches is fatal, as in the reference (M:6087 / 6279: it would call updateBLen);
// bumpLen > 0 (building a synthetic tree): in pass 1 the two child branches are lengthened to bumpLen and merged again; a None
// that remains, or one in pass 2, is reported in badNodes (the caller lengthens those branches and starts over): *nBad > 0.
template <class Ops> struct Rebuild {
    const Tree &T;
    Ops &ops;
    Error &E;
    double bumpLen;
    int32_t capBad, *badNodes, *nBad;
    std::vector<std::vector<int32_t>> byDepth;    // the nodes reachable from the root, by depth, ascending within a depth
    Batch B;

    // (*nBad counts every bad node, also those beyond capBad: a caller that sees *nBad > capBad knows the list is cut short)
    void bad(int v) { if (nBad) { if (*nBad < capBad) badNodes[*nBad] = v; (*nBad)++; } }

    int levels()
    {
        std::vector<int32_t> depth((size_t)T.n, -1), order;
        order.reserve((size_t)T.n);
        order.push_back(T.root);
        depth[T.root] = 0;
        int maxd = 0;
        for (size_t h = 0; h < order.size(); h++) {
            const int v = order[h];
            for (int k = 0; k < 2; k++) {
                const int ch = k == 0 ? T.c0[v] : T.c1[v];
                if (ch < 0) continue;
                if (ch >= T.n || depth[ch] >= 0) return E.fail(ERR_ARG, "node %d: child %d out of range or reached twice", v, ch);
                if (T.up[ch] != v) return E.fail(ERR_ARG, "node %d is a child of %d but its `up` entry says %d", ch, v, T.up[ch]);   // (pass 2 reads `up`)
                if ((T.c0[v] < 0) != (T.c1[v] < 0)) return E.fail(ERR_ARG, "node %d has one child", v);
                depth[ch] = depth[v] + 1;
                maxd = std::max(maxd, depth[ch]);
                order.push_back(ch);
            }
        }
        byDepth.assign((size_t)maxd + 1, {});
        for (int v : order) byDepth[depth[v]].push_back(v);                // (breadth-first: ascending depth; sorted below)
        for (auto &lv : byDepth) std::sort(lv.begin(), lv.end());
        for (int v : order) {
            if (T.c0[v] >= 0) T.lower[v] = -1;
            else if (T.lower[v] < 0) return E.fail(ERR_ARG, "tip %d has no lower list", v);
            T.upRight[v] = T.upLeft[v] = T.totUp[v] = -1;
        }
        return 0;
    }

    // ---- pass 1: lower lists, deepest level first -------------------------------------------------------------------------
    int pass1()
    {
        const Tree t = T;                         // (a local copy: its pointers stay in registers while a level is filled)
        for (size_t d = byDepth.size(); d-- > 0;) {
            Batch::Fill F = B.fill(byDepth[d].size());
            for (int v : byDepth[d]) if (t.c0[v] >= 0) F.lower(t, v, 1);
            B.done(F);
            if (!B.size()) continue;
            UP_TRY(B.run(T, ops));
            for (size_t k = 0; k < B.size(); k++) {
                if (!B.none[k]) continue;
                if (bumpLen <= 0.0)
                    return E.fail(ERR_FATAL, "inconsistent lower lists at node %d (the reference would call updateBLen here)", B.node[k]);
                // (a child's branch length does not enter the child's own lower list: lengthen the two branches, merge this pair again)
                const int a = B.kid1[k], b = B.kid2[k];
                B.b1[k] = T.dist[a] = std::max(T.dist[a], bumpLen);
                B.b2[k] = T.dist[b] = std::max(T.dist[b], bumpLen);
                UP_TRY(ops.items(B, k, (size_t)1));
                if (B.none[k]) { bad(a); bad(b); }
            }
            if (nBad && *nBad) return 0;
            for (size_t k = 0; k < B.size(); k++) T.lower[B.node[k]] = B.out[k];
        }
        return 0;
    }

    // ---- pass 2: upper lists from the root down ---------------------------------------------------------------------------
    int pass2()
    {
        const Tree t = T;
        const int r = T.root;
        if (T.c0[r] >= 0) {
            const std::vector<int32_t> kids{T.c1[r], T.c0[r]};
            std::vector<int32_t> pl{T.lower[kids[0]], T.lower[kids[1]]};
            UP_TRY(passed(T, ops, pl.data(), kids.data(), 2, true));
            const double bl[2] = {T.dist[kids[0]], T.dist[kids[1]]};
            const uint8_t tp[2] = {T.tip[kids[0]], T.tip[kids[1]]};
            int32_t rv[2] = {-1, -1};
            UP_TRY(ops.rootVector(2, pl.data(), bl, tp, T.mut[r], rv));
            T.upRight[r] = rv[0]; T.upLeft[r] = rv[1];
        }
        std::vector<int32_t> vu;
        for (size_t d = 1; d < byDepth.size(); d++) {
            const std::vector<int32_t> &lv = byDepth[d];
            if (lv.empty()) continue;
            UP_TRY(vect_up_of(T, ops, lv, vu));
            // (kind by kind: the new lists take their room in item order, so the level's probVectTotUp lists -- the candidate lists of
            // every search -- end up next to each other in the arena, and a download of one kind moves in long runs)
            Batch::Fill F = B.fill(3 * lv.size());
            for (size_t k = 0; k < lv.size(); k++) if (t.dist[lv[k]] != 0.0) F.totUp(t, lv[k], vu[k]);   // M:6262-6275
            for (int which = 1; which >= 0; which--)                        // probVectUpRight (child 1), then probVectUpLeft (child 0)
                for (size_t k = 0; k < lv.size(); k++) if (t.c0[lv[k]] >= 0) F.upper(t, lv[k], which, vu[k], false);
            B.done(F);
            if (!B.size()) continue;
            UP_TRY(B.run(T, ops));
            for (size_t i = 0; i < B.size(); i++) {
                const int v = B.node[i];
                if (B.kind[i] == TOT_UP) { T.totUp[v] = B.none[i] ? -1 : B.out[i]; continue; }   // (a None probVectTotUp stays None, M:6270)
                if (B.none[i]) {
                    if (bumpLen <= 0.0)
                        return E.fail(ERR_FATAL, "inconsistent upper lists at node %d (the reference would call updateBLen here)", v);
                    bad(v); bad(B.kid2[i]);
                    continue;
                }
                (B.kind[i] == UP_RIGHT ? T.upRight : T.upLeft)[v] = B.out[i];
            }
            // (bad nodes of this level: the levels below a node without its upper lists cannot be made, but every other node of THIS
            // level has been looked at -- the caller lengthens all of them before it starts over)
            if (nBad && *nBad) return 0;
        }
        return 0;
    }
};

template <class Ops>
int rebuild_drive(const Tree &T, Ops &ops, double bumpLen, int32_t capBad, int32_t *badNodes, int32_t *nBad, Error &E)
{
    if (nBad) *nBad = 0;
    Rebuild<Ops> R{T, ops, E, bumpLen, capBad, badNodes, nBad};
    UP_TRY(R.levels());
    UP_TRY(R.pass1());
    if (nBad && *nBad) return 0;
    return R.pass2();
}

#undef UP_TRY
}  // namespace update_plan
