// maple_amd/csrc/sweep_plan.h -- the logic of the branch-length sweep, traverseTreeToOptimizeBranchLengths
// (MAPLEv0.7.5.4.py:8727-8893), as pure host code: no HIP, no context, nothing but the standard library, so that it compiles on
// its own and is tested on the CPU (tests/sweep_plan_main.cpp, tests/test_sweep_plan.py).  maple_tree_optimize_blens
// (blen_sweep.hip) is sweep_drive() below with the estimate kernels and maple_update_partials plugged in.
//
//   blen_verdict  the rule that decides whether a branch takes its new estimate (M:8835 / 8869-8883)
//   sweep_order   the order in which the reference visits the branches (M:8812-8823 / 8884-8885); static, the topology is fixed
//   next_chunk    how many estimates the next launch computes (scheduling only: no result depends on it)
//   sweep_drive   the sweep itself over two callbacks: estimate(items) and repair(node)
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace sweep_plan {

// M:8835 / 8869-8883 with Python's truthiness: estimateBranchLengthWithDerivative returns a float or False, and `False`, `0.0`
// (and the None of a missing length: 0.0 in the columns) are all falsy.  `best` is what dist[node] becomes when the verdict is
// true; when it is false the branch keeps its length and its dirty flag is cleared.  The ratio tests are the reference's own
// fp64 expressions (cur / best, compared with the doubles 1.01 and 0.99).
inline bool blen_verdict(double cur, double t, bool isFalse, double *best)
{
    const double b = isFalse ? 0.0 : t;
    *best = b;
    if (!(b != 0.0 || cur != 0.0)) return false;                           // `if bestLength or dist[node]`
    if (b == 0.0 || cur == 0.0) return true;                               // (not bestLength) or (not dist[node])
    const double ratio = cur / b;
    return ratio > 1.01 || ratio < 0.99;
}

// The visiting order: the stack starts with the children of root child 0, then those of root child 1; pop; push child0, child1.
// pos[v] = index of v in `order`, -1 for the root, its children and every node not below them.  False if the children columns
// are no tree (an index out of range, one child only, a node reached twice).
inline bool sweep_order(int32_t n, int32_t root, const int32_t *c0, const int32_t *c1, std::vector<int32_t> &order, std::vector<int32_t> &pos)
{
    order.clear();
    pos.assign((size_t)(n > 0 ? n : 0), -1);
    if (n <= 0 || root < 0 || root >= n) return false;
    auto kidsOk = [&](int v) { return (c0[v] < 0 && c1[v] < 0) || (c0[v] >= 0 && c1[v] >= 0 && c0[v] < n && c1[v] < n && c0[v] != c1[v]); };
    if (!kidsOk(root)) return false;
    if (c0[root] < 0) return true;
    std::vector<int32_t> stack;
    std::vector<uint8_t> seen((size_t)n, 0);
    seen[root] = 1;
    for (int k = 0; k < 2; k++) {
        const int ch = k == 0 ? c0[root] : c1[root];
        if (ch == root || seen[ch] || !kidsOk(ch)) return false;
        seen[ch] = 1;
        if (c0[ch] >= 0) { stack.push_back(c0[ch]); stack.push_back(c1[ch]); }
    }
    while (!stack.empty()) {
        const int v = stack.back();
        stack.pop_back();
        if (seen[v] || !kidsOk(v)) return false;
        seen[v] = 1;
        pos[v] = (int32_t)order.size();
        order.push_back(v);
        if (c0[v] >= 0) { stack.push_back(c0[v]); stack.push_back(c1[v]); }
    }
    return true;
}

// The adaptive chunk size.  A repair at v replaces the upper vectors of v's children, and the reference's LIFO order visits them
// right after v: on a tree where most branches move, most of a large chunk is thrown away, and on a converged one nearly all of
// it is used.  So: start at CHUNK_START (the fixed size of the Python sweep); after a chunk that was cut short (a repair made one
// of its remaining estimates stale, or dirtied a branch it does not hold), twice the run length that was used, never more than
// the size before; after a chunk used in full, twice the size.  CHUNK_MIN: a launch and its copy back cost the same whatever
// the launch holds, and up to a few hundred wavefront estimates run side by side, so three estimates that may be thrown away
// are cheaper than a launch that may be saved (a choice, not a measurement; measured: DESIGN.md section 15, 1.8-2.7 estimates
// computed per estimate used where nearly every branch moves).  CHUNK_MAX: the largest batch that still goes one
// wavefront per item (the explicit-pair operators' default), so the adaptive policy never changes the kernel form by itself.
constexpr int CHUNK_START = 256, CHUNK_MIN = 4, CHUNK_MAX = 1024;
inline int next_chunk(int cur, int used, bool broke)
{
    if (broke) return std::max(CHUNK_MIN, std::min(cur, 2 * std::max(used, 1)));
    if (used >= cur) return std::min(CHUNK_MAX, std::max(cur, 2 * cur));
    return cur;                                                            // (the order ran out before the chunk was full)
}

struct SweepItem {                       // one estimate: the two lists it reads, as they were when the chunk was formed
    int32_t node, upList, mutList, lowList;
    uint8_t tip;
};

struct SweepStats { int64_t launches = 0, computed = 0, used = 0, repairs = 0; };

struct SweepTree {                       // the caller's columns (maple_update_partials' meaning); the id columns are re-read after every repair
    int32_t n;
    const int32_t *up, *c0, *mut;
    const uint8_t *tip;
    double *dist;
    const int32_t *lower, *upRight, *upLeft;
    uint8_t *dirty;
};

// The sweep over the nodes of `order` (pos = their indices, sweep_order above).
//   estimate(items, t, isFalse) -> 0 or an error code: estimateBranchLengthWithDerivative of every item
//   repair(node, visited)       -> 0 or an error code: updatePartials around `node` (its length already in dist[]); it updates
//                                  the id columns and names every node it visited (dirty[] is set here)
// A chunk is the next k nodes in visiting order that are dirty when it is formed.  An estimate is used when the node's turn
// comes only if both ids it was computed from are still the node's; otherwise the chunk ends there and the next one starts at
// that node.  dirty[node] is read at the node's turn: a node that is clean when a chunk passes over it and that a repair later in
// the same chunk dirties has no estimate in the chunk, so the chunk is cut before it (`limit`).  A node's flag is only ever
// cleared at its own turn, so a node of the chunk is still dirty when its turn comes.
// chunk: 0 = next_chunk's policy (with fastPass: one launch, nothing can go stale), k > 0 = exactly k.
template <class Est, class Rep>
int sweep_drive(const SweepTree &T, const std::vector<int32_t> &order, const std::vector<int32_t> &pos, bool fastPass, int chunk,
                Est &&estimate, Rep &&repair, int32_t *nUpdates, std::vector<int32_t> &updated, SweepStats &st)
{
    const size_t N = order.size();
    auto upListOf = [&](int v) { const int p = T.up[v]; return T.c0[p] == v ? T.upRight[p] : T.upLeft[p]; };
    long long cur = chunk > 0 ? chunk : (fastPass ? (long long)N + 1 : CHUNK_START);
    std::vector<SweepItem> items;
    std::vector<double> t;
    std::vector<uint8_t> isFalse, inChunk((size_t)T.n, 0);
    std::vector<int32_t> visited;
    size_t at = 0;
    while (at < N) {
        items.clear();
        size_t p = at;
        for (; p < N && (long long)items.size() < cur; p++) {
            const int v = order[p];
            if (T.dirty[v]) items.push_back(SweepItem{v, upListOf(v), T.mut[v], T.lower[v], T.tip[v]});
        }
        if (items.empty()) break;
        for (const SweepItem &it : items) inChunk[it.node] = 1;
        t.assign(items.size(), 0.0);
        isFalse.assign(items.size(), 0);
        int rc = estimate(items, t, isFalse);
        st.launches++;
        st.computed += (int64_t)items.size();
        size_t limit = p, next = p;
        int used = 0;
        bool broke = false;
        for (size_t k = 0; k < items.size() && !rc; k++) {
            const SweepItem &it = items[k];
            const int v = it.node;
            if ((size_t)pos[v] >= limit) { broke = true; next = limit; break; }
            if (upListOf(v) != it.upList || T.lower[v] != it.lowList) { broke = true; next = (size_t)pos[v]; break; }
            used++;
            st.used++;
            double best;
            if (!blen_verdict(T.dist[v], t[k], isFalse[k] != 0, &best)) { T.dirty[v] = 0; continue; }
            T.dist[v] = best;
            (*nUpdates)++;
            updated.push_back(v);
            if (fastPass) continue;
            visited.clear();
            rc = repair(v, visited);
            st.repairs++;
            for (int w : visited) {
                if (w < 0 || w >= T.n) continue;
                T.dirty[w] = 1;
                if (pos[w] > pos[v] && (size_t)pos[w] < limit && !inChunk[w]) limit = (size_t)pos[w];
            }
        }
        for (const SweepItem &it : items) inChunk[it.node] = 0;
        if (rc) return rc;
        if (!broke) next = limit;
        if (next < p) broke = true;                                        // (cut after its last usable item)
        at = next;
        if (chunk <= 0 && !fastPass) cur = next_chunk((int)cur, used, broke);
    }
    return 0;
}

}  // namespace sweep_plan
