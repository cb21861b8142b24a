// tests/search_plan_main.cpp -- maple_amd/csrc/search_plan.h on its own: scenarios as lines of numbers on stdin, the plans on
// stdout (test_search_plan.py compiles this with the host sanitizers and compares with tests/golden/search_plan_cases.json,
// whose "frontier_in" / "frontier_out" / "lane_in" / "lane_out" name the numbers of a line in order).
#include "../maple_amd/csrc/search_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace maple::plan;

// a buffer after reserve_exact(n): grow-only (DevBuf, ctx_host.h)
static size_t reserved(size_t cap, size_t n) { return n > cap ? n : cap; }

static int frontier_case(std::istringstream &is)
{
    FrontierPlanIn in;
    FrontierCaps &F = in.cap;
    int uer, fw, mt, lo, anyWide, overflow;
    unsigned long long usedU, usedC, usedR, usedLists, usedW, usedA;
    is >> in.m >> in.budget >> in.itemsHint >> uer >> fw >> mt >> in.nLists >> in.usedEnt >> in.treeMaxEnt >> in.freeBytes >> in.waveAllBelow;
    is >> F.itemsU >> F.itemsC >> F.tw >> F.ta >> F.trec >> F.tflag >> F.arec >> F.sw >> F.sa >> F.sais >> F.bw >> F.bw2 >> F.recs >> F.perm >> F.perm2
       >> F.perm3 >> F.perm4 >> F.visit >> F.lsize >> F.lpos >> F.lpar >> F.passList >> F.passListR;
    is >> in.capE >> in.need.needU >> in.need.needC >> in.need.needR >> in.need.needL >> in.need.needW >> in.need.needA >> in.need.needM >> lo;
    is >> anyWide >> usedU >> usedC >> usedR >> usedLists >> usedW >> usedA >> overflow;
    if (!is) return 1;
    in.usingErrorRate = uer != 0; in.forceWide = fw != 0; in.matTree = mt != 0; in.need.lastOverflow = lo != 0;
    if (in.budget < 1) in.budget = 1 << 30;                                // (as frontier_search does)
    in.szItem = 96; in.szVisit = 32; in.szRec = 48; in.frBlock = 256; in.heavyMult = 24; in.bigMin = 176;
    const FrontierPlan p = plan_frontier(in);
    FrontierCaps A = F;
    A.itemsU = reserved(F.itemsU, p.resItemsU); A.itemsC = reserved(F.itemsC, p.resItemsC); A.recs = reserved(F.recs, p.resRecs);
    A.tw = reserved(F.tw, p.resTw); A.ta = reserved(F.ta, p.resTa); A.trec = reserved(F.trec, p.resTrec); A.arec = reserved(F.arec, p.resArec);
    A.tflag = reserved(F.tflag, p.resTflag); A.sw = reserved(F.sw, p.resSw); A.sa = reserved(F.sa, p.resSa); A.sais = reserved(F.sais, p.resSais);
    A.bw = reserved(F.bw, p.resBw); A.bw2 = reserved(F.bw2, p.resBw2);
    const FrontierBound b = bind_frontier(in, p, A);
    const FrontierNeeds n = remember_frontier(in.need, in.m, anyWide && in.forceWide, usedU, usedC, usedR, usedLists, usedW, usedA, overflow != 0);
    printf("F %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", p.resItemsU, p.resItemsC, p.resRecs, p.resTw, p.resTa, p.resTrec, p.resArec,
           p.resTflag, p.resSw, p.resSa, p.resSais, p.resBw, p.resBa, p.resBw2, p.resBa2);
    printf(" %lld %lld %lld %lld %lld %lld %d", p.capU, p.capC, p.capR, p.capL, p.capW, p.capA, (int)p.growthCut);
    printf(" %d %lld %lld %d %lld %lld %lld %lld", p.capE, p.scratchLanes, p.extraSlabs, p.gridUpd, p.capBig, p.capBig2, p.capRecs, (long long)(2.0 * p.room));
    printf(" %d %d %d %d %d %d %d %d %d", p.gridN, p.gridCached, p.heavyMin, p.bigMin, p.gridWave, p.gridWaveSmall, p.groupLevels, p.gridLayout, p.waveAllBelow);
    printf(" %lld %lld %lld %lld %lld %lld %lld %lld %lld %d", b.capU, b.capC, b.capCC, b.capW, b.capA, b.capL, b.capBig, b.capRecs, b.capVisit, (int)b.layoutOK);
    printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", b.resPerm, b.resPerm2, b.resPerm3, b.resPerm4, b.resVisit, b.resLsize, b.resLpos, b.resLpar,
           b.resPassList, b.resPassListR, b.resDeferred);
    printf(" %lld %lld %lld %lld %lld %lld %lld %d\n", n.needU, n.needC, n.needR, n.needL, n.needW, n.needA, n.needM, (int)n.lastOverflow);
    return 0;
}

static int lane_case(std::istringstream &is)
{
    LanePlanIn in;
    int wsEntriesPerLane, treeMaxEnt, heavy, cached, strict, assist, freeKnown;
    is >> wsEntriesPerLane >> treeMaxEnt >> heavy >> in.attempt >> cached >> strict >> assist >> freeKnown >> in.freeBytes >> in.wsCap >> in.m;
    if (!is) return 1;
    in.cached = cached != 0; in.strict = strict != 0; in.assist = assist != 0; in.freeKnown = freeKnown != 0;
    in.szList = 24; in.szStack = 32; in.szBest = 40;
    const int capW0 = lane_cap_w0(wsEntriesPerLane, treeMaxEnt);
    in.capW = lane_start_cap_w(capW0, in.cached, heavy != 0);
    for (int a = 0; a < in.attempt; a++) in.capW *= 8;                     // (as run_queries does from pass to pass)
    const LanePlan p = plan_lane_launch(in);
    printf("L %d %d %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu %lld %lld %d %d %d %d %zu\n", capW0, p.capW, p.capA, p.capH, p.capS, p.capB, p.capAis, p.w, p.aux,
           p.h, p.st, p.best, p.ais, p.total, p.wsBudget, p.maxLanes, p.lanesWanted, p.activeLanes, p.nWaves, p.lanes, p.reserve);
    return 0;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string kind;
        if (!(is >> kind)) continue;
        const int bad = kind == "F" ? frontier_case(is) : kind == "L" ? lane_case(is) : 1;
        if (bad) { fprintf(stderr, "bad scenario: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
