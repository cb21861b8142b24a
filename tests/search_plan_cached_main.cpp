// tests/search_plan_cached_main.cpp -- the cached launches the frontier plan queues behind an updating level
// (maple_amd/csrc/search_plan.h: FrontierPlan::cachedBehind / cachedBehindEarly / cachedEarlyLevels, cached_behind): the frontier
// scenarios of tests/golden/search_plan_cases.json on stdin ("F" lines as tests/search_plan_main.cpp reads them; only the numbers
// the plan's launch geometry depends on are used), per line "m cachedBehind cachedBehindEarly cachedEarlyLevels" and
// cached_behind(level) for levels 0..11 on stdout.  test_search_plan_cached.py compiles this with the host sanitizers.
#include "../maple_amd/csrc/search_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace maple::plan;

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string kind;
        if (!(is >> kind) || kind != "F") continue;
        FrontierPlanIn in;
        int uer, fw, mt;
        is >> in.m >> in.budget >> in.itemsHint >> uer >> fw >> mt >> in.nLists >> in.usedEnt >> in.treeMaxEnt >> in.freeBytes >> in.waveAllBelow;
        if (!is) { fprintf(stderr, "bad scenario: %s\n", line.c_str()); return 2; }
        in.usingErrorRate = uer != 0; in.forceWide = fw != 0; in.matTree = mt != 0;
        if (in.budget < 1) in.budget = 1 << 30;
        in.szItem = 96; in.szVisit = 32; in.szRec = 48; in.frBlock = 256; in.heavyMult = 24; in.bigMin = 176;
        const FrontierPlan p = plan_frontier(in);
        printf("%d %d %d %d", in.m, p.cachedBehind, p.cachedBehindEarly, p.cachedEarlyLevels);
        for (int level = 0; level < 12; level++) printf(" %d", cached_behind(p, level));
        printf("\n");
    }
    return 0;
}
