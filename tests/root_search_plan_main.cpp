// tests/root_search_plan_main.cpp -- maple_amd/csrc/root_search_plan.h on the CPU, compiled on its own
// (tests/test_root_search_plan.py).  One command per line on stdin, one answer per line on stdout; doubles travel as C99
// hexadecimal floats (or nan / inf / -inf), so no bit is lost either way:
//   L n root c0[n] c1[n]                                  -> "L ok K node[K] parent[K] side[K] M levelStart[M]"   level_lists
//                                                            (ok = 0: the columns are no tree, nothing follows)
//   R n root c0[n] c1[n] strict fails thrTopology thrOptimization thrConsecutive score[n]
//                                                         -> "R bestNode best visited k nodes[k] scores[k]"        replay
#include "../maple_amd/csrc/root_search_plan.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

static bool read_double(std::istringstream &in, double &x)
{
    std::string w;
    if (!(in >> w)) return false;
    char *end = nullptr;
    x = strtod(w.c_str(), &end);
    return end && *end == 0;
}

static std::string hex(double x)
{
    char buf[64];
    snprintf(buf, sizeof buf, "%a", x);
    return buf;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char cmd = 0;
        in >> cmd;
        if (!cmd) continue;
        if (cmd != 'L' && cmd != 'R') { fprintf(stderr, "unknown command %c\n", cmd); return 2; }
        int32_t n = 0, root = 0;
        in >> n >> root;
        std::vector<int32_t> c0((size_t)(n > 0 ? n : 0)), c1(c0.size());
        for (auto &x : c0) in >> x;
        for (auto &x : c1) in >> x;
        if (!in) { fprintf(stderr, "short line\n"); return 2; }
        std::string out;
        if (cmd == 'L') {
            root_search_plan::Levels lv;
            const bool ok = root_search_plan::level_lists(n, root, c0.data(), c1.data(), lv);
            out = ok ? "L 1" : "L 0";
            if (ok) {
                if (lv.parent.size() != lv.node.size() || lv.side.size() != lv.node.size()) { fprintf(stderr, "ragged levels\n"); return 2; }
                out += ' ' + std::to_string(lv.node.size());
                for (int32_t v : lv.node) out += ' ' + std::to_string(v);
                for (int32_t v : lv.parent) out += ' ' + std::to_string(v);
                for (uint8_t v : lv.side) out += ' ' + std::to_string((int)v);
                out += ' ' + std::to_string(lv.levelStart.size());
                for (int32_t v : lv.levelStart) out += ' ' + std::to_string(v);
            }
        } else {
            int strict = 0;
            root_search_plan::Rules r{};
            in >> strict >> r.allowedFailsTopology;
            r.strictTopologyStopRules = strict != 0;
            bool ok = (bool)in && read_double(in, r.thresholdLogLKtopology) && read_double(in, r.thresholdLogLKoptimizationTopology)
                      && read_double(in, r.thresholdLogLKconsecutivePlacement);
            std::vector<double> score(c0.size());
            for (auto &x : score) ok = ok && read_double(in, x);
            if (!ok) { fprintf(stderr, "short or malformed line\n"); return 2; }
            root_search_plan::Result res;
            root_search_plan::replay(root, c0.data(), c1.data(), score.data(), r, res);
            if (res.nodes.size() != res.scores.size()) { fprintf(stderr, "ragged bestNodes\n"); return 2; }
            out = "R " + std::to_string(res.bestNode) + ' ' + hex(res.best) + ' ' + std::to_string(res.visited) + ' '
                  + std::to_string(res.nodes.size());
            for (int32_t v : res.nodes) out += ' ' + std::to_string(v);
            for (double x : res.scores) out += ' ' + hex(x);
        }
        puts(out.c_str());
    }
    return 0;
}
