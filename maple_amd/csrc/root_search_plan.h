// maple_amd/csrc/root_search_plan.h -- the two host-only halves of the search of findBestRoot (MAPLEv0.7.5.4.py:7730-7848) as
// pure host code: no HIP, no context, nothing but the standard library, so that it compiles on its own and is tested on the CPU
// (tests/root_search_plan_main.cpp, tests/test_root_search_plan.py).  tree_lk_plan.h's sibling.
//   level_lists: the nodes whose two child branches get a score, grouped by depth -- maple_tree_find_best_root (root_search.hip)
//                runs one batch of lanes per level, a level's items reading what their parents' items made;
//   replay:      the reference's depth-first traversal with its stop rules (M:7782-7848) over the table of scores.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace root_search_plan {

// The items of the search: every internal node below the root (the root's internal children are level 0), level by level; within a
// level in the order of the parents' items, side 0 before side 1.  parent[k] = the item (an index into node[]) of node[k]'s parent,
// -1 for level 0; side[k] = which child of its parent node[k] is.  Level l = [levelStart[l], levelStart[l + 1]); no level is empty.
struct Levels {
    std::vector<int32_t> node, parent;
    std::vector<uint8_t> side;
    std::vector<int32_t> levelStart;
    size_t levels() const { return levelStart.empty() ? 0 : levelStart.size() - 1; }
};

// Breadth-first from the root, iterative (a caterpillar of any length costs heap, not call frames).  False if the children columns
// below `root` are no tree (an index out of range, one child only, a node reached twice -- lk_postorder's cases); `out` is then
// unspecified.
inline bool level_lists(int32_t n, int32_t root, const int32_t *c0, const int32_t *c1, Levels &out)
{
    out.node.clear(); out.parent.clear(); out.side.clear(); out.levelStart.clear();
    if (n <= 0 || root < 0 || root >= n) return false;
    auto kidsOk = [&](int32_t v) {
        return (c0[v] < 0 && c1[v] < 0) || (c0[v] >= 0 && c1[v] >= 0 && c0[v] < n && c1[v] < n && c0[v] != c1[v]);
    };
    std::vector<uint8_t> seen((size_t)n, 0);
    struct Todo { int32_t v, parent; uint8_t side; };
    std::vector<Todo> cur, next;
    if (!kidsOk(root)) return false;
    seen[root] = 1;
    if (c0[root] >= 0) { cur.push_back({c0[root], -1, 0}); cur.push_back({c1[root], -1, 1}); }
    out.levelStart.push_back(0);
    while (!cur.empty()) {
        next.clear();
        for (const Todo &t : cur) {
            if (seen[t.v] || !kidsOk(t.v)) return false;
            seen[t.v] = 1;
            if (c0[t.v] < 0) continue;
            const int32_t k = (int32_t)out.node.size();
            out.node.push_back(t.v); out.parent.push_back(t.parent); out.side.push_back(t.side);
            next.push_back({c0[t.v], k, 0});
            next.push_back({c1[t.v], k, 1});
        }
        if ((int32_t)out.node.size() > out.levelStart.back()) out.levelStart.push_back((int32_t)out.node.size());
        cur.swap(next);
    }
    if (out.node.empty()) out.levelStart.clear();
    return true;
}

struct Rules {
    bool strictTopologyStopRules;
    int32_t allowedFailsTopology;
    double thresholdLogLKtopology, thresholdLogLKoptimizationTopology, thresholdLogLKconsecutivePlacement;
};

struct Result {
    int32_t bestNode = -1, visited = 0;
    double best = 0.0;
    std::vector<int32_t> nodes;          // the reference's bestNodes dict in insertion order, the root (0.0) first
    std::vector<double> scores;
};

// M:7782-7848 over score[v] = the `score` of M:7808 for rooting on the branch above v; a NaN is "no score": the branch does not
// compete and the traversal does not go below it (the reference's `except:`, M:7838).  The stack is the reference's LIFO
// nodesToVisit, seeded with the root's internal children in its order; at a node side 0 comes before side 1.  The comparisons are
// the reference's: > for a new best, < for a failed pass, >= for bestNodes, > for "within thresholdLogLKtopology".
inline void replay(int32_t root, const int32_t *c0, const int32_t *c1, const double *score, const Rules &r, Result &out)
{
    out.bestNode = root; out.best = 0.0; out.visited = 1;
    out.nodes.assign(1, root); out.scores.assign(1, 0.0);
    struct Visit { int32_t t1; double lastLK; int32_t fails; };
    std::vector<Visit> stack;
    if (c0[root] < 0) return;
    for (const int32_t ch : {c0[root], c1[root]})
        if (c0[ch] >= 0) stack.push_back({ch, 0.0, 0});
    while (!stack.empty()) {
        out.visited++;
        const Visit v = stack.back();
        stack.pop_back();
        for (int i = 0; i < 2; i++) {
            const int32_t kid = i ? c1[v.t1] : c0[v.t1];
            const double sc = score[kid];
            if (sc != sc) continue;
            int32_t fails = v.fails;
            if (sc > out.best) { out.best = sc; out.bestNode = kid; fails = 0; }
            else if (sc < v.lastLK - r.thresholdLogLKconsecutivePlacement) fails++;
            if (sc >= out.best - r.thresholdLogLKoptimizationTopology) { out.nodes.push_back(kid); out.scores.push_back(sc); }
            if (c0[kid] < 0) continue;
            const bool within = sc > out.best - r.thresholdLogLKtopology;
            const bool go = r.strictTopologyStopRules ? (fails <= r.allowedFailsTopology && within)
                                                      : (fails <= r.allowedFailsTopology || within);
            if (go) stack.push_back({kid, sc, fails});
        }
    }
}

}  // namespace root_search_plan
