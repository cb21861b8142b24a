// tests/search_route_main.cpp -- the routing rules of maple_amd/csrc/search_plan.h (which search of a round goes where) on their
// own: scenarios as lines of numbers on stdin, what the rules say on stdout (test_search_route.py compiles this with the host
// sanitizers and compares with tests/golden/search_route_cases.json, whose "in" / "out" entries name the numbers of a line in order).
#include "../maple_amd/csrc/search_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace maple::plan;

static bool route_in(std::istringstream &is, RouteIn &r)
{
    int uer, mt, uf, sv, hp, hc, ncs, dws, wof, noh;
    is >> r.wideBudget >> uer >> mt >> uf >> sv >> hp >> hc >> ncs >> dws >> wof >> noh;
    r.usingErrorRate = uer != 0; r.matTree = mt != 0; r.useFrontier = uf != 0; r.scanValid = sv != 0; r.havePlace = hp != 0; r.hintsCoverTree = hc != 0;
    r.noCladeScan = ncs != 0; r.denseWideScoring = dws != 0; r.wideOutsideFrontier = wof != 0; r.noOverHint = noh != 0;
    return (bool)is;
}

static int one_case(const std::string &kind, std::istringstream &is)
{
    if (kind == "P") {                     // patched_only
        int nc, mt, n, tier, tracing, lists, requested, uer, anyZero;
        if (!(is >> nc >> mt >> n >> tier >> tracing >> lists >> requested >> uer >> anyZero)) return 1;
        printf("P %d\n", (int)patched_only(nc != 0, mt != 0, n, tier, tracing != 0, lists != 0, requested, uer != 0, anyZero != 0));
    } else if (kind == "B") {              // wide_budget, frontier_budget (MAPLE_WIDE_BUDGET_DEFAULT is 256)
        int requested, nScored, uer, patchedOnly;
        if (!(is >> requested >> nScored >> uer >> patchedOnly)) return 1;
        const int wb = wide_budget(requested, nScored, uer != 0, patchedOnly != 0, 256);
        printf("B %d %d\n", wb, frontier_budget(wb, requested, nScored, uer != 0));
    } else if (kind == "S") {              // score_rows_max
        int known, nNodes;
        size_t freeB, capB;
        if (!(is >> known >> freeB >> capB >> nNodes)) return 1;
        printf("S %zu\n", score_rows_max(known != 0, freeB, capB, nNodes));
    } else if (kind == "K") {              // pre_rows_kind, pre_rows_fit, pre_rows_spare
        RouteIn r;
        size_t nCand, rowsMax;
        if (!route_in(is, r) || !(is >> nCand >> rowsMax)) return 1;
        const PreRowsKind k = pre_rows_kind(r);
        const bool fit = k != PRE_NONE && pre_rows_fit(nCand, rowsMax);
        printf("K %d %d %d\n", (int)k, (int)fit, fit ? pre_rows_spare(nCand, rowsMax, k == PRE_WITNESS) : 0);
    } else if (kind == "R") {              // root_rows_ok
        RouteIn r;
        int nF;
        size_t nWide;
        if (!route_in(is, r) || !(is >> nF >> nWide)) return 1;
        printf("R %d\n", (int)root_rows_ok(r, nF, nWide));
    } else if (kind == "W") {              // split_wide
        int mZ, spare, mt, nBatch, nWide;
        if (!(is >> mZ >> spare >> mt >> nBatch >> nWide)) return 1;
        std::vector<int32_t> wide(nWide), rowOf(nBatch);
        for (auto &v : wide) is >> v;
        for (auto &v : rowOf) is >> v;
        if (!is) return 1;
        const WideSplit s = split_wide(wide, rowOf, mZ, spare, mt != 0);
        if (s.take.size() != s.row.size()) return 1;
        printf("W %zu", s.take.size());
        for (int32_t v : s.take) printf(" %d", v);
        for (int32_t v : s.row) printf(" %d", v);
        printf(" %zu", s.rest.size());
        for (int32_t v : s.rest) printf(" %d", v);
        printf(" %d\n", s.nSpare);
    } else if (kind == "C") {              // frame_chunk; the removed lists offered as runs of (count, entries, aux values)
        int nF, nRuns;
        long long freeEnt, freeAux;
        if (!(is >> nF >> freeEnt >> freeAux >> nRuns)) return 1;
        std::vector<int32_t> nEnt, nAux;
        for (int r = 0, cnt, e, a; r < nRuns && (is >> cnt >> e >> a); r++) { nEnt.insert(nEnt.end(), cnt, e); nAux.insert(nAux.end(), cnt, a); }
        if (!is) return 1;
        const int m = (int)nEnt.size();
        const FrameChunk f = frame_chunk(m, nF, freeEnt, freeAux, nEnt.data(), nAux.data());
        printf("C %d %d\n", f.m, (int)f.laneOnly);
    } else if (kind == "G") {              // cache_reserve
        size_t need, cap, chunkRows;
        int nNodes;
        if (!(is >> need >> cap >> chunkRows >> nNodes)) return 1;
        printf("G %zu\n", cache_reserve(need, cap, chunkRows, nNodes));
    } else if (kind == "H") {              // the four hint rules
        int hintBudget, wideBudget, hinted, row, status, nAppend;
        double hintEff0, eff0;
        if (!(is >> hintBudget >> hintEff0 >> wideBudget >> eff0 >> hinted >> row >> status >> nAppend)) return 1;
        const bool sentOn = hint_sends_on(hinted != 0, row);
        printf("H %d %d %d %d\n", (int)hints_stale(hintBudget, hintEff0, wideBudget, eff0), (int)sentOn, (int)hint_set(status, nAppend, sentOn),
               (int)hint_clear(hinted != 0, status, nAppend, wideBudget));
    } else
        return 1;
    return 0;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string kind;
        if (!(is >> kind)) continue;
        if (one_case(kind, is)) { fprintf(stderr, "bad scenario: %.200s\n", line.c_str()); return 2; }
    }
    return 0;
}
