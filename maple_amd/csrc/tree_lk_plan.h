// maple_amd/csrc/tree_lk_plan.h -- the order in which calculateTreeLikelihood (MAPLEv0.7.5.4.py:9721-9779) adds the
// contributions of the internal nodes, as pure host code: no HIP, no context, nothing but the standard library, so that it
// compiles on its own and is tested on the CPU (tests/tree_lk_plan_main.cpp, tests/test_tree_lk_plan.py).  maple_tree_log_lk
// (tree_lk.hip) walks one item per entry of this order and sums what comes back front to back.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tree_lk_plan {

// The loop of M:9735-9770 visits a node's children[0] subtree, then its children[1] subtree, then merges at the node: the
// internal nodes reachable from `root` in post-order.  Iterative (an explicit stack of nodes whose second child is still to
// come, so a caterpillar of any length costs heap, not call frames).  False if the children columns below `root` are no tree
// (an index out of range, one child only, a node reached twice); `order` is then unspecified.
inline bool lk_postorder(int32_t n, int32_t root, const int32_t *c0, const int32_t *c1, std::vector<int32_t> &order)
{
    order.clear();
    if (n <= 0 || root < 0 || root >= n) return false;
    auto kidsOk = [&](int32_t v) {
        return (c0[v] < 0 && c1[v] < 0) || (c0[v] >= 0 && c1[v] >= 0 && c0[v] < n && c1[v] < n && c0[v] != c1[v]);
    };
    std::vector<uint8_t> seen((size_t)n, 0);
    std::vector<int32_t> path;           // the internal nodes above the current one, the root first
    std::vector<uint8_t> second;         // per entry of `path`: its children[1] subtree is the one being walked
    int32_t v = root;
    for (;;) {
        // direction 0 (M:9736-9738): down through children[0] to a leaf
        for (;;) {
            if (seen[v] || !kidsOk(v)) return false;
            seen[v] = 1;
            if (c0[v] < 0) break;
            path.push_back(v);
            second.push_back(0);
            v = c0[v];
        }
        // direction 1 (M:9745-9770): up while we come from a children[1]; the first node we reach from its children[0] sends us
        // down its children[1]
        for (;;) {
            if (path.empty()) return true;
            const int32_t p = path.back();
            if (!second.back()) { second.back() = 1; v = c1[p]; break; }
            order.push_back(p);
            path.pop_back();
            second.pop_back();
        }
    }
}

}  // namespace tree_lk_plan
