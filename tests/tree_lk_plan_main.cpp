// tests/tree_lk_plan_main.cpp -- maple_amd/csrc/tree_lk_plan.h on the CPU, compiled on its own (tests/test_tree_lk_plan.py).
// One command per line on stdin, one answer per line on stdout:
//   P n root c0[n] c1[n]      -> "P ok order..."     lk_postorder (ok = 0: the columns are no tree, no order follows)
#include "../maple_amd/csrc/tree_lk_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char cmd = 0;
        in >> cmd;
        if (!cmd) continue;
        if (cmd != 'P') { fprintf(stderr, "unknown command %c\n", cmd); return 2; }
        int32_t n = 0, root = 0;
        in >> n >> root;
        std::vector<int32_t> c0((size_t)(n > 0 ? n : 0)), c1(c0.size()), order;
        for (auto &x : c0) in >> x;
        for (auto &x : c1) in >> x;
        if (!in) { fprintf(stderr, "short line\n"); return 2; }
        const bool ok = tree_lk_plan::lk_postorder(n, root, c0.data(), c1.data(), order);
        std::string out = ok ? "P 1" : "P 0";
        if (ok) for (int32_t v : order) { out += ' '; out += std::to_string(v); }
        puts(out.c_str());
    }
    return 0;
}
