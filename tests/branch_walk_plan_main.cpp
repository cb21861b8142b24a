// tests/branch_walk_plan_main.cpp -- maple_amd/csrc/branch_walk_plan.h on the CPU, compiled on its own
// (tests/test_branch_walk_plan.py).  One command per line on stdin, one answer per line on stdout:
//   G n root U nLists nMutLists hasMinor up[n] c0[n] c1[n] dist[n] lower[n] upLeft[n] upRight[n] mut[n] (nMinor[n])
// and per rule (EM, EVENTS, ERRORS, in this order)
//     -> "G 0 numTips nRows nPass nLeaves  (node pList cList mut dist leafMinor refNode) x nRows  passIdx x nPass  leaves x nLeaves
//         itemLeaf x (ERRORS ? nRows : 0)"           dist as a hexadecimal float
//     -> "G status message"                          status 1 / 2: gather() refused the columns
#include "../maple_amd/csrc/branch_walk_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

int main()
{
    using namespace branch_walk_plan;
    std::string line;
    Rows r;                              // one for every call, as the library keeps one per context: gather() must leave nothing behind
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char cmd = 0;
        in >> cmd;
        if (!cmd) continue;
        if (cmd != 'G') { fprintf(stderr, "unknown command %c\n", cmd); return 2; }
        int U = 0, hasMinor = 0;
        Columns t{};
        in >> t.n >> t.root >> U >> t.nLists >> t.nMutLists >> hasMinor;
        const size_t n = (size_t)(t.n > 0 ? t.n : 0);
        std::vector<int32_t> col[8];     // up c0 c1 lower upLeft upRight mut nMinor
        std::vector<double> dist(n);
        auto ints = [&](int k) { col[k].resize(n); for (auto &x : col[k]) in >> x; };
        ints(0); ints(1); ints(2);
        for (auto &x : dist) in >> x;
        ints(3); ints(4); ints(5); ints(6);
        if (hasMinor) ints(7);
        if (!in) { fprintf(stderr, "short line\n"); return 2; }
        t.up = col[0].data(); t.c0 = col[1].data(); t.c1 = col[2].data(); t.dist = dist.data(); t.lower = col[3].data();
        t.upLeft = col[4].data(); t.upRight = col[5].data(); t.mut = col[6].data(); t.nMinor = hasMinor ? col[7].data() : nullptr;
        t.usingErrorRate = U != 0;
        for (Rule rule : {EM, EVENTS, ERRORS}) {
            const Status s = gather(rule, t, r);
            if (s != OK) { printf("G %d %s\n", (int)s, r.message.c_str()); continue; }
            std::string out = "G 0 " + std::to_string(r.numTips) + " " + std::to_string(r.size()) + " " + std::to_string(r.passIdx.size()) + " "
                              + std::to_string(r.leaves.size());
            char buf[64];
            for (int32_t k = 0; k < r.size(); k++) {
                for (int32_t x : {r.node[k], r.pList[k], r.cList[k], r.mut[k]}) { out += ' '; out += std::to_string(x); }
                snprintf(buf, sizeof buf, " %a ", r.dist[k]);
                out += buf;
                out += std::to_string(r.leafMinor[k]) + " " + std::to_string(r.refNode[k]);
            }
            for (int32_t x : r.passIdx) { out += ' '; out += std::to_string(x); }
            for (int32_t x : r.leaves) { out += ' '; out += std::to_string(x); }
            for (int32_t x : r.itemLeaf) { out += ' '; out += std::to_string(x); }
            puts(out.c_str());
        }
    }
    return 0;
}
