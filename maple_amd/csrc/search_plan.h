// maple_amd/csrc/search_plan.h -- how large the pools of the two SPR tiers are, how many lanes, wavefronts and scratch slabs a
// launch gets, what is remembered for the next call, and which search of a round goes to which tier: functions of numbers and
// flags, nothing else.  No HIP, nothing of the project (record sizes come in as fields, filled by the caller with sizeof), so it
// compiles and is tested on its own (tests/search_plan_main.cpp, tests/test_search_plan.py; the routing rules:
// tests/search_route_main.cpp, tests/test_search_route.py).  frontier_search (frontier.hip), run_queries and
// maple_spr_search_batch (spr_batch.hip) fill the input, reserve what the plan says and launch.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#ifndef MAPLE_FR_CACHED_EARLY
#define MAPLE_FR_CACHED_EARLY 4        // cached launches behind each of a whole round's first updating levels (FrontierPlan::cachedBehindEarly)
#endif

namespace maple {
namespace plan {

// ---- the frontier tier (frontier.hip) ------------------------------------------------------------------------------------

// what the last call that counts asked of the pools, and its searches
struct FrontierNeeds {
    long long needU = 0, needC = 0, needR = 0, needL = 0, needW = 0, needA = 0, needM = 0;
    bool lastOverflow = false;         // ... and whether one of them ran over
};

// the capacities of the scratch's buffers, in elements of each (FrontierScratch: itemsU, itemsC, recs, visit in bytes)
struct FrontierCaps {
    size_t itemsU = 0, itemsC = 0, tw = 0, ta = 0, trec = 0, tflag = 0, arec = 0, sw = 0, sa = 0, sais = 0, bw = 0, bw2 = 0, recs = 0;
    size_t perm = 0, perm2 = 0, perm3 = 0, perm4 = 0, visit = 0, lsize = 0, lpos = 0, lpar = 0, passList = 0, passListR = 0;
};

struct FrontierPlanIn {
    int m = 0, budget = 0;             // searches of the batch; items a search may expand (>= 1)
    long long itemsHint = 0;
    bool usingErrorRate = false, forceWide = false, matTree = false;
    size_t nLists = 0;                 // lists in the arena
    long long usedEnt = 0;             // ... and their entries
    int treeMaxEnt = 0;
    size_t freeBytes = 0;              // free on the device (8 GB where the runtime does not say)
    int waveAllBelow = 0;              // the tuning's
    size_t szItem = 0, szVisit = 0, szRec = 0;   // sizeof(FItem), sizeof(FVisit), sizeof(FRec)
    int frBlock = 0, heavyMult = 0, bigMin = 0;  // FR_BLOCK, FR_HEAVY_MULT, FR_BIG_MIN
    FrontierCaps cap;                  // what the scratch holds ...
    int capE = 0;                      // ... and remembers: entries of a per-lane scratch slab,
    FrontierNeeds need;                // the asks
};

struct FrontierPlan {
    // what to pass to reserve_exact, buffer by buffer (0: nothing to reserve)
    size_t resItemsU, resItemsC, resRecs, resTw, resTa, resTrec, resArec, resTflag, resSw, resSa, resSais, resBw, resBa, resBw2, resBa2;
    // the pools as planned, before a pool that grows is given half as much again: the cached pool splits capC : capR
    long long capU, capC, capR, capL, capW, capA;
    bool growthCut;                    // what the pools would grow by did not fit and was cut down
    int capE;
    long long scratchLanes, extraSlabs;
    int gridUpd;
    long long capBig, capBig2, capRecs;
    double room;
    // launch geometry
    int gridN, gridCached, heavyMin, bigMin, gridWave, gridWaveSmall, groupLevels, gridLayout, waveAllBelow;
    // cached-regime launches queued behind the publication of an updating level: cachedBehindEarly behind each of the first
    // cachedEarlyLevels levels, cachedBehind behind every later one (cached_behind below)
    int cachedBehind, cachedBehindEarly, cachedEarlyLevels;
};

// Every cached launch takes a snapshot of what is complete when it starts, so any count >= 1 gives the same searches; a launch more
// is two more layout launches at the end of the round.
static inline int cached_behind(const FrontierPlan &p, int level)
{
    return level < p.cachedEarlyLevels ? p.cachedBehindEarly : p.cachedBehind;
}

static inline size_t grow(size_t want, size_t cap) { return want <= cap ? cap : std::max(want, cap + cap / 2); }

// pools, sized for the batch and bounded by what the device has free
static inline FrontierPlan plan_frontier(const FrontierPlanIn &in)
{
    FrontierPlan p;
    const FrontierCaps &F = in.cap;
    const int m = in.m, budget = in.budget;
    const size_t held = F.itemsU + F.itemsC + F.tw * 8 + F.ta * sizeof(double)
                        + F.sw * 8 + F.sa * sizeof(double) + F.sais * sizeof(double) + F.bw * 48 + F.bw2 * 48;
    const double room = 0.5 * (double)(in.freeBytes + held);
    p.room = room;
    // (first guesses, for a context's first batch: afterwards the pools go by what the batch before used.  With an error model a fifth
    // of the searches runs to the budget -- a quarter of it per search on average, and three times the temporary lists: measured 1 500
    // cached items and 61 lists per search at 1 000 000 tips, where a first call that ran over took 2.9-5.3 s and the two calls
    // after it 2.3-3.1 s before the pools had grown)
    const bool longSearches = in.usingErrorRate && !in.forceWide;
    const long long perSearchC = longSearches ? std::min<long long>(budget, std::max<long long>(768, budget / 4)) : std::min<long long>(budget, 768);
    long long capC = std::max<long long>(1 << 16, std::max((long long)m * perSearchC, in.itemsHint));
    long long capU = std::max<long long>(1 << 14, (long long)m * std::min<long long>(budget, 16));
    // (roots: the cached-regime items the list-updating items push -- the upper part of the cached pool)
    long long capR = std::max<long long>(1 << 16, std::min(capC, (long long)m * std::min<long long>(budget, 32)));
    const long long meanEnt = std::max<long long>(16, in.nLists == 0 ? 64 : in.usedEnt / (long long)in.nLists);   // entries per list in the arena
    long long capL = (longSearches ? 6 : 2) * capU;
    long long capW = 2 * capL * meanEnt, capA = capW;
    if (in.need.needM > 0 && !in.forceWide) {
        // what the last batch asked for, scaled to this one: with an error model the searches are several times as long as the
        // first guess, and a pool that runs over hands its searches back
        // (after an overflow the asks themselves are too low -- the searches that were handed back stopped asking: twice, not 1.25 x)
        const double f = (in.need.lastOverflow ? 2.0 : 1.25) * std::min(16.0, (double)m / (double)in.need.needM);   // (a far smaller batch is no measure: capped)
        capU = std::max(capU, (long long)(f * in.need.needU)); capC = std::max(capC, (long long)(f * in.need.needC)); capR = std::max(capR, (long long)(f * in.need.needR));
        capL = std::max(capL, (long long)(f * in.need.needL));
        // (the words' first guess goes with the arena's mean list length, which moves by an entry when the tree is uploaded again:
        // 47 -> 48 made two 5 GB pools "grow" by half -- 0.73 s of the first round on a changed tree.  Once a batch has said what it
        // used, that alone sizes them.)
        capW = std::max<long long>(1 << 20, (long long)(f * in.need.needW)); capA = std::max<long long>(1 << 20, (long long)(f * in.need.needA));
    }
    // per-lane scratch for lists of up to capE entries (two average lists merged, with room); the few longer ones -- near the
    // root -- take pieces of a shared region.  As many lanes as the GPU holds at once at this kernel's occupancy.
    // (in steps of 32 and never below what the slabs were cut for: they are 6 GB, and 282 -> 288 entries would allocate them again)
    const int capE = std::max(in.capE, std::max(256, std::min(1024, (6 * (int)meanEnt + 31) / 32 * 32)));
    p.capE = capE;
    long long scratchLanes = m <= 64 ? 16384 : 256ll * 4 * 4 * 64;         // 256 CUs x 4 SIMDs x 4 wavefronts (a handful of searches: what they can use)
    // slabs beyond the lanes' own: one per wavefront of the two wavefront-wide kernels (256 + 1 280 <= 2 048) and, on a tree with MAT
    // local references, one per lane of k_fr_pass (256 workgroups), which runs next to k_fr_updating
    const long long extraSlabs = 2048 + (in.matTree ? 256ll * in.frBlock : 0);
    while (scratchLanes > 16384 && (double)(scratchLanes + extraSlabs) * capE * 64 > 0.25 * room) scratchLanes /= 2;
    p.scratchLanes = scratchLanes; p.extraSlabs = extraSlabs;
    p.gridUpd = (int)(scratchLanes / in.frBlock);
    const long long capBig = std::max<long long>(1 << 20, 64ll * 1024 * std::max(1, in.treeMaxEnt));
    const long long capBig2 = in.matTree ? std::max<long long>(1 << 20, capBig / 4) : 0;
    p.capBig = capBig; p.capBig2 = capBig2;
    {   // What a pool already holds it keeps (a request below its capacity costs nothing, and a pool that shrinks and grows from
        // call to call is freed and allocated again -- tens of GB: 1.3 s of a 1 000 000-tip step); what a pool would GROW by is cut
        // down proportionally if the total would not fit.  (The temporary lists' pools used to be set back to their first guess
        // whenever the total met the room -- always, at 1 000 000 tips: the list words overflowed on EVERY step and sent 15 000
        // of 131 072 searches to the one-lane kernel, 550 ms.)
        const long long curU = (long long)(F.itemsU / in.szItem), curCR = (long long)(F.itemsC / in.szItem);
        const long long curL = (long long)std::min(F.trec, F.tflag);
        const long long curW = (long long)F.tw, curA = (long long)F.ta;
        const double perItem = (double)(in.szItem + in.szVisit + 12);
        const double fixed = (double)(scratchLanes + extraSlabs) * capE * 64 + (double)(capBig + capBig2) * 48;
        const double base = (double)(curCR + curU) * perItem + (double)(curW + curA) * 8 + (double)curL * 24 + fixed;
        const double gCR = std::max<double>(0.0, (double)(capC + capR - curCR)), gU = std::max<double>(0.0, (double)(capU - curU));
        const double gL = std::max<double>(0.0, (double)(capL - curL)), gW = std::max<double>(0.0, (double)(capW - curW)), gA = std::max<double>(0.0, (double)(capA - curA));
        const double growth = (gCR + gU) * perItem + (gW + gA) * 8 + gL * 24;
        double f = 1.0;
        if (base + growth > room && growth > 0) f = std::max(0.0, (room - base) / growth);
        p.growthCut = f < 1.0;
        const double wantCR = std::max<double>((double)curCR, (double)curCR + f * gCR);
        const double shareR = (double)capR / (double)(capC + capR);
        capR = std::max<long long>(1 << 16, (long long)(wantCR * shareR)); capC = std::max<long long>(1 << 16, (long long)wantCR - capR);
        capU = std::max<long long>(1 << 14, std::max(curU, (long long)(curU + f * gU)));
        capL = std::max<long long>(2 * (1 << 14), std::max(curL, (long long)(curL + f * gL)));
        capW = std::max<long long>(1 << 20, std::max(curW, (long long)(curW + f * gW)));
        capA = std::max<long long>(1 << 20, std::max(curA, (long long)(curA + f * gA)));
    }
    p.capU = capU; p.capC = capC; p.capR = capR; p.capL = capL; p.capW = capW; p.capA = capA;
    const long long capRecs = std::max<long long>(1 << 14, (long long)m * 16);
    p.capRecs = capRecs;
    p.resItemsU = grow((size_t)capU * in.szItem, F.itemsU);
    p.resItemsC = grow((size_t)(capC + capR) * in.szItem, F.itemsC);
    p.resRecs = grow((size_t)capRecs * in.szRec, F.recs);
    p.resTw = grow((size_t)capW, F.tw);
    p.resTa = grow((size_t)capA, F.ta);
    p.resTrec = grow((size_t)capL, F.trec);
    p.resArec = grow(in.nLists, F.arec);
    p.resTflag = grow((size_t)capL, F.tflag);
    p.resSw = (size_t)(scratchLanes + extraSlabs) * capE;
    p.resSa = (size_t)(scratchLanes + extraSlabs) * capE * 5;
    p.resSais = (size_t)(scratchLanes + extraSlabs) * capE * 2;
    p.resBw = (size_t)capBig;
    p.resBa = (size_t)capBig * 5;
    p.resBw2 = (size_t)capBig2;
    p.resBa2 = (size_t)capBig2 * 5;
    p.gridN = std::max(1, std::min(2048, (m + in.frBlock - 1) / in.frBlock));
    // (many short-lived workgroups rather than a grid-stride loop over few long-lived ones: wavefront slots come free all the
    // time, and the dispatcher hands them to the higher-priority stream first)
    // (a launch of 16 384 workgroups costs 0.4-0.5 ms even when it finds ten thousand items: the grid goes with the batch -- a
    // round's largest launch holds ~21 items per search)
    p.gridCached = (int)std::min<long long>(16384, std::max<long long>(512, (long long)m / 12));
    // items whose two lists add up to this many entries are walked by a wavefront each, in two size classes (frontier_dev.h):
    // k_fr_updating_wave_s, sizeof(WaveUpdLds<128>) = 27 680 bytes of LDS per wavefront, five wavefronts per compute unit, and
    // k_fr_updating_wave, sizeof(WaveUpdLds<512>) = 110 720 bytes, one per compute unit (+ 160 bytes of model constants each)
    // (a handful of searches -- the re-search of a proposed move -- wait for every single item: all of them by wavefronts)
    p.heavyMin = m <= 64 ? 1 : std::max(256, in.heavyMult * (int)meanEnt / 4); p.gridWave = 256; p.gridWaveSmall = 1280;
    p.bigMin = m <= 64 ? (1 << 30) : in.bigMin;                             // (lists of this many entries together: 16 items to a wavefront)
    // the host looks at the counters every few levels: a handful of searches (the re-search of a proposed move) is over after a few
    // levels and each look costs them less than the levels it saves; a whole round runs ~20 updating levels
    p.groupLevels = m <= 64 ? 2 : 8;
    // two cached launches behind every level: the cached subtrees are deeper than the updating chain is long.  The first six levels
    // of a whole round hold 95 % of its updating items, last 6-9 ms each, and a cached launch next to them is over in 0.5-2 ms:
    // the stream then idles until the next level publishes its roots.  MAPLE_FR_CACHED_EARLY launches behind each of those
    // (measured on the headline, medians of 8 runs each in two sessions: 2 -> 121.2 ms per step, 3 -> 118.5, 4 -> 118.2, the same
    // order in both sessions; profiles/late_levels_bench.md); a handful of searches keeps two throughout.
    p.cachedBehind = 2; p.cachedBehindEarly = m <= 64 ? 2 : MAPLE_FR_CACHED_EARLY; p.cachedEarlyLevels = 6;
    p.gridLayout = (int)std::min<long long>(1024, std::max<long long>(64, (long long)m / 64));   // (~100 small launches: the grid goes with the batch)
    p.waveAllBelow = in.waveAllBelow > 0 ? in.waveAllBelow : (in.waveAllBelow < 0 ? 0 : 49152);
    return p;
}

// what follows from the capacities the buffers ended up with (`after`: the scratch's once the plan's sizes are reserved)
struct FrontierBound {
    long long capU, capC, capCC, capW, capA, capL, capBig, capRecs, capVisit;
    bool layoutOK;                     // the visiting-order layout of the items (k_fr_layout_*) is made
    // what to pass to reserve_exact (0: nothing to reserve); the pass lists' are their capacities afterwards
    size_t resPerm, resPerm2, resPerm3, resPerm4, resVisit, resLsize, resLpos, resLpar, resPassList, resPassListR, resDeferred;
};

static inline FrontierBound bind_frontier(const FrontierPlanIn &in, const FrontierPlan &p, const FrontierCaps &after)
{
    FrontierBound b;
    b.capU = (long long)(after.itemsU / in.szItem); b.capC = (long long)(after.itemsC / in.szItem);
    // (a buffer kept from a larger call: both parts grow with it)
    b.capCC = b.capC - std::max(p.capR, (long long)((double)b.capC * p.capR / (double)(p.capC + p.capR)));
    b.capW = (long long)after.tw; b.capA = (long long)after.ta;
    b.capL = (long long)std::min(after.trec, after.tflag);
    b.resPerm = std::max(after.perm, (size_t)b.capU);
    b.resPerm2 = std::max(after.perm2, (size_t)b.capU);
    b.resPerm3 = std::max(after.perm3, (size_t)b.capU);
    b.resPerm4 = std::max(after.perm4, (size_t)b.capU);
    b.capVisit = b.capU + b.capC;
    b.layoutOK = in.m > 64 && b.capVisit < (1ll << 31) - 64;               // (ranks are 32-bit; a handful of searches is not worth 90 launches)
    b.resVisit = b.resLsize = b.resLpos = b.resLpar = 0;
    if (b.layoutOK) {
        b.resVisit = std::max(after.visit, (size_t)b.capVisit * in.szVisit);
        b.resLsize = std::max(after.lsize, (size_t)b.capVisit);
        b.resLpos = std::max(after.lpos, (size_t)b.capVisit);
        b.resLpar = std::max(after.lpar, (size_t)b.capVisit);
    }
    b.capBig = (long long)after.bw;
    b.capRecs = (long long)(after.recs / in.szRec);
    // trees with MAT local references: the lists a search carries go through the reference branches it crosses
    b.resPassList = b.resPassListR = b.resDeferred = 0;
    if (in.matTree) {
        b.resPassList = std::max(after.passList, (size_t)std::max<long long>(1 << 16, b.capC / 8));
        b.resPassListR = std::max(after.passListR, (size_t)std::max<long long>(1 << 16, (b.capC - b.capCC) / 4));
        b.resDeferred = b.resPassList + b.resPassListR;
    }
    return b;
}

// (a batch of whole-tree searches only says nothing about the next full one -- and neither does a handful of searches: the
// re-searches of the apply phase, one to 32 at a time, used to leave their asks behind, the next ROUND scaled them up by
// 200 000 / 1 and grew the pools to whatever fitted: 1.8 s of hipMalloc in the first search after the moves, round 6)
static inline FrontierNeeds remember_frontier(const FrontierNeeds &before, int m, bool wideOnly, unsigned long long usedU, unsigned long long usedC,
                                       unsigned long long usedR, unsigned long long nLists, unsigned long long usedW, unsigned long long usedA,
                                       bool overflow)
{
    FrontierNeeds n = before;
    if (!wideOnly && (m >= 1024 || m >= before.needM)) {
        n.needU = (long long)usedU; n.needC = (long long)usedC; n.needR = (long long)usedR; n.needL = (long long)nLists; n.needW = (long long)usedW;
        n.needA = (long long)usedA; n.needM = m; n.lastOverflow = overflow;
    }
    return n;
}

// ---- the one-lane-per-search tier (spr_batch.hip) ------------------------------------------------------------------------

// per-lane list workspace: a search near the root of a tree with long lists (rate variation: many O vectors) merges
// lists of several hundred entries a few hundred times before it is handed over or done
static inline int lane_cap_w0(int wsEntriesPerLane, int treeMaxEnt) { return wsEntriesPerLane > 0 ? wsEntriesPerLane : std::max(16384, 64 * treeMaxEnt); }
// the few cached (whole-tree) searches get room up front; more when the budgeted pass already ran out of it
static inline int lane_start_cap_w(int capW0, bool cached, bool heavyQueries) { return cached ? (heavyQueries ? 8 : 4) * capW0 : capW0; }

struct LanePlanIn {
    int m = 0, attempt = 0, capW = 0;  // searches of the launch; 0, 1, 2: the pass; list entries per lane (x 8 from pass to pass)
    bool cached = false, strict = false, assist = false;   // with a score table; P.strict; wave-assisted, few searching lanes
    bool freeKnown = false;
    size_t freeBytes = 0, wsCap = 0;   // free on the device, where the runtime says; bytes the workspace holds
    size_t szList = 0, szStack = 0, szBest = 0;   // sizeof(TList), sizeof(StackItem), sizeof(BestRec)
};

struct LanePlan {
    int32_t capW, capA, capH, capS, capB, capAis;            // WsLayout: per-lane capacities
    size_t w, aux, h, st, best, ais, total;                  // ... and their bytes, each a multiple of 64
    long long wsBudget, maxLanes;
    int lanesWanted, activeLanes, nWaves, lanes;
    size_t reserve;                                          // bytes to reserve for the workspace
};

static inline LanePlan plan_lane_launch(const LanePlanIn &in)
{
    LanePlan p;
    const int m = in.m, attempt = in.attempt;
    p.capW = in.capW;
    p.capA = 5 * p.capW;                                        // O-vector-heavy lists (rate variation) carry up to 4-5 aux doubles per entry
    p.capH = p.capW / 8 + 256;
    p.capS = 1024 * (attempt + 1);
    p.capB = (in.cached ? 4096 : 1024) * (attempt + 1);         // whole-tree (cached) searches short-list far more branches
    p.capAis = 8192 * (attempt + 1);
    auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };
    p.w = al((size_t)p.capW * 8);
    p.aux = al((size_t)p.capA * sizeof(double));
    p.h = al((size_t)p.capH * in.szList);
    p.st = al((size_t)p.capS * in.szStack);
    p.best = al((size_t)p.capB * in.szBest);
    p.ais = al((size_t)p.capAis * sizeof(double));
    p.total = p.w + p.aux + p.h + p.st + p.best + p.ais;
    // lanes: one query per lane while they last; at most 4 wavefronts per SIMD (the kernel's occupancy) and a
    // workspace footprint bounded to ~96 GB of the 288 GB
    long long wsBudget = 96ll << 30;
    if (in.freeKnown) {   // ... and to 70 % of what is free on the device right now (plus what this buffer already holds)
        const long long avail = (long long)((double)(in.freeBytes + in.wsCap) * 0.7);
        if (avail < wsBudget) wsBudget = avail;
    }
    long long maxLanes = wsBudget / (long long)p.total;
    if (maxLanes > 4096 * 64) maxLanes = 4096 * 64;
    // lanes pull searches from a counter: more wavefronts than the GPU holds at once (4 per SIMD) only cost workspace
    if (in.cached && maxLanes > 8192) maxLanes = 8192;
    if (maxLanes < 64) maxLanes = 64;
    const int lanesWanted = (int)(m < maxLanes ? m : maxLanes);
    // searching lanes per wavefront (measured at 20k queries: the long searches of a non-strict round like 2 lanes,
    // 42 vs 46 ms with 1; the short ones of a strict round like 1, 31 vs 37 ms with 2; more is always worse)
    // (at 200k queries with the budget of a 100 000-tip tree: 2 / 4 / 8 / 13 / 24 lanes -> 825 / 645 / 512 / 424 / 417 ms)
    const int lanesDiv = in.strict ? 32768 : (lanesWanted > 65536 ? 8192 : 16384);
    int activeLanes = (lanesWanted + lanesDiv - 1) / lanesDiv;
    if (activeLanes < 1) activeLanes = 1;
    if (activeLanes > 64) activeLanes = 64;
    // wave-assisted lane searches: the wavefront serves its lanes' score requests one after the other, so few
    // searching lanes per wavefront (100 000 tips, budget 2 132: 2 / 4 / 6 / 8 / 16 / 24 lanes -> 298 / 281 / 279 / 289 /
    // 394 / 345 ms; without the assistance 375)
    if (!in.cached && in.assist && activeLanes > 4) activeLanes = 4;
    int nWaves = (lanesWanted + activeLanes - 1) / activeLanes;
    if (nWaves > 8192) nWaves = 8192;
    const int lanes = nWaves * activeLanes;
    p.wsBudget = wsBudget; p.maxLanes = maxLanes; p.lanesWanted = lanesWanted; p.activeLanes = activeLanes; p.nWaves = nWaves; p.lanes = lanes;
    {   // grow-only and at least doubling (a 20 GB hipMalloc costs ~0.7 s): batches of slowly growing size must not
        // reallocate every time
        size_t need = (size_t)lanes * p.total;
        if (need > in.wsCap) {
            const size_t top = (size_t)maxLanes * p.total;
            need = std::min(std::max(need, 2 * in.wsCap), std::max(top, need));
        }
        p.reserve = need;
    }
    return p;
}

// ---- which search of a round goes where (maple_spr_search_batch, spr_batch.hip) -------------------------------------------

// The tree was patched since its tables were built.  A small batch (the re-search of proposed moves before they are
// applied) runs on the patched node records alone, through the frontier tier with no hand-over to the dense tier -- unless
// one of its searches is a whole-tree search by construction (a zero-length branch without an error model); everything
// else rebuilds the tables first.
static inline bool patched_only(bool nodesCurrent, bool matTree, int n, int searchTier, bool tracing, bool wantsLists, int requested,
                                bool usingErrorRate, bool anyZeroLength)
{
    if (!(nodesCurrent && !matTree && n <= 64 && searchTier == 0 && !tracing && !wantsLists)) return false;
    return !(requested >= 0 && !usingErrorRate && anyZeroLength);
}

// A search that scores more branches than the budget is handed to the dense path, which costs it one appendProbNode per
// branch of the tree -- so the budget that pays grows with the tree: 1/64 of the scored branches, measured best at 10 000
// tips (256: 91 ms per round; 128: 100, 384: 97) and at 100 000 (2 048: 1.08 s; 256: 2.69, 1 024: 1.13, 4 096: 1.20)
// (requested: the caller's wideSearchBudget -- 0: this rule, negative: no dense tier; budgetDefault: MAPLE_WIDE_BUDGET_DEFAULT)
static inline int wide_budget(int requested, int nScored, bool usingErrorRate, bool patchedOnly, int budgetDefault)
{
    int wideBudget = requested == 0 ? std::max(budgetDefault, std::min(8192, nScored / 64)) : requested;
    if (patchedOnly) wideBudget = -1;                                   // (no tree-sized table is current)
    // (a long search costs the wave-assisted lane tier a tenth of what it cost one lane: twice the budget pays -- 100 000 tips:
    // 2 132 / 3 072 / 4 096 / 6 144 -> 693 / 688 / 668 / 692 ms per round; 10 000 tips: 256 / 384 / 512 -> 75 / 72 / 72)
    // (with an error model too, since the frontier tier: 100 000 tips, budget 2 132 / 3 000 / 4 264 / 8 528 -> 532 / 447 / 420 / 441 ms
    // per round -- the searches between 2 000 and 4 000 items are the ones with the longest removed lists, which the dense kernel
    // walks slowest: 28 116 rows take it 260 ms, 25 785 rows 114)
    // (1 000 000 tips, 8 192 / 16 384: 2.32 / 2.73 s per 131 072 searches -- the pools of the longer searches are reallocated on
    // the way: with an error model the doubling stops at 8 192)
    if (requested == 0) wideBudget = usingErrorRate ? std::min(2 * wideBudget, std::max(wideBudget, 8192)) : 2 * wideBudget;
    return wideBudget;                                                  // (> 0: searches over it go to the dense tier, "hybrid")
}

// An item of the frontier tier costs about what half a (search, branch) pair costs the dense tier on full walks (1.1e9
// items/s against 2.3e9 pairs/s), so a search only pays for a row of the whole tree once it has expanded half a tree's
// worth of items; the searches from zero-length branches (whole-tree searches without an error model) never start here.
// (With an error model there are no searches known to be whole-tree ones beforehand, a fifth of all searches is long, and
// half a tree's worth of items each does not fit any pool -- 5e8 items at 100 000 tips and counting: those searches
// leave at the lane tiers' budget.)
static inline int frontier_budget(int wideBudget, int requested, int nScored, bool usingErrorRate)
{
    if (wideBudget <= 0) return 0;
    return usingErrorRate ? wideBudget : std::max(wideBudget, requested == 0 ? nScored / 2 : 0);
}

// rows the (query x node) score table may have: 4 GiB, more on big trees -- a row of a 1 000 000-tip tree is 16 MB and every
// launch over the table wants thousands of searches (one per wavefront): up to half of what is free (plus what the table
// already holds), 96 GiB at most.  Never below one row: a chunk of the dense tier is at least one search, and the rows made
// ahead want 64 searches (pre_rows_fit), which neither 0 nor 1 row takes.
static inline size_t score_rows_max(bool freeKnown, size_t freeBytes, size_t cacheCapBytes, int nNodes)
{
    size_t budget = (size_t)4ull << 30;
    if (freeKnown) budget = std::max(budget, std::min((freeBytes + cacheCapBytes) / 2, (size_t)96ull << 30));
    return std::max<size_t>(1, budget / ((size_t)nNodes * sizeof(double)));
}

// what the tuning and the state of the context say about a call's whole-tree searches
struct RouteIn {
    int wideBudget = 0;                // wide_budget()
    bool usingErrorRate = false, matTree = false, useFrontier = false;
    bool scanValid = false, havePlace = false;   // the clade-scan tables and the frames' tables exist
    bool hintsCoverTree = false;       // the hints of the call before are as long as the tree
    bool noCladeScan = false, denseWideScoring = false, wideOutsideFrontier = false, noOverHint = false;   // the tuning's
};

// Rows of the score table made ahead, on a side stream next to the budgeted pass: for the searches from zero-length branches
// (no error model: the witness filter's) or for those that ran over the budget the last time (error model: the hinted ones)
enum PreRowsKind { PRE_NONE = 0, PRE_WITNESS = 1, PRE_HINTED = 2 };
static inline PreRowsKind pre_rows_kind(const RouteIn &r)
{
    const bool hybrid = r.wideBudget > 0;
    if (hybrid && !r.usingErrorRate && r.wideBudget > 16
        && (!r.matTree || (r.scanValid && r.havePlace && !r.noCladeScan && !r.denseWideScoring && !r.wideOutsideFrontier)))
        return PRE_WITNESS;
    if (hybrid && r.usingErrorRate && r.useFrontier && !r.noOverHint && r.hintsCoverTree && r.wideBudget > 16 && r.scanValid && r.havePlace
        && !r.noCladeScan && !r.wideOutsideFrontier)
        return PRE_HINTED;
    return PRE_NONE;
}
// ... are made for 64 searches or more, as many as the table takes
static inline bool pre_rows_fit(size_t nCand, size_t rowsMax) { return nCand >= 64 && nCand <= rowsMax; }
// ... with rows to spare for searches that run over their budget unannounced (the witness filter's only)
static inline int pre_rows_spare(size_t nCand, size_t rowsMax, bool witness) { return witness ? (int)std::min<size_t>(4096, rowsMax - nCand) : 0; }

// Trees with local references: the rows of the searches that ran over their budget are made in the ROOT's frame as well
// (appendProbNode does not depend on the frame) and replayed inside the frontier tier; only what the tier hands back goes the
// frame-by-frame way.
static inline bool root_rows_ok(const RouteIn &r, int nF, size_t nWide)
{
    return nF > 1 && r.useFrontier && r.scanValid && r.havePlace && !r.noCladeScan && !r.wideOutsideFrontier && nWide >= 64;
}

// The searches that left the budgeted pass (`wide`: positions in the batch) when rows were made ahead: `take` are replayed over
// row `row` each -- their own (rowOf >= 0) or, for the unannounced ones, the next of the `spare` rows behind the mZ made ahead
// (nSpare handed out) -- and `rest` go on to the dense tier's chunks.  (A tree with local references: what the tier did not finish
// over these rows goes frame by frame -- the one-wavefront-per-search replay wants the removed list in every frame.)
struct WideSplit { std::vector<int32_t> take, row, rest; int nSpare = 0; };
static inline WideSplit split_wide(const std::vector<int32_t> &wide, const std::vector<int32_t> &rowOf, int mZ, int spare, bool matTree)
{
    WideSplit s;
    for (int32_t i : wide) {
        if (matTree) { s.rest.push_back(i); continue; }
        if (rowOf[i] >= 0) { s.take.push_back(i); s.row.push_back(rowOf[i]); }
        else if (s.nSpare < spare) { s.take.push_back(i); s.row.push_back(mZ + s.nSpare++); }
        else s.rest.push_back(i);
    }
    return s;
}

// The frame-by-frame chunk: the removed list goes into EVERY reference frame, so the batch is bounded by what the arena can
// take (a third of its free entries and aux values; nEnt, nAux: the removed lists of the m searches offered) and by 8 Mi
// (query, frame) items.  laneOnly: too many frames for this arena (a 100 000-tip tree has ~2 000) -- batches this small would
// turn the replay into a chain of one-lane launches, the remaining wide searches run lane-only instead.
struct FrameChunk { int m; bool laneOnly; };
static inline FrameChunk frame_chunk(int m, int nF, int64_t arenaFreeEnt, int64_t arenaFreeAux, const int32_t *nEnt, const int32_t *nAux)
{
    const int64_t freeEnt = arenaFreeEnt / 3, freeAux = arenaFreeAux / 3;
    int64_t needEnt = 0, needAux = 0;
    int k = 0;
    for (; k < m; k++) {
        needEnt += (int64_t)nF * (nEnt[k] + 24);
        needAux += (int64_t)nF * (nAux[k] + 8);
        if (needEnt > freeEnt || needAux > freeAux || (int64_t)(k + 1) * nF > (8ll << 20)) break;
    }
    return FrameChunk{k, k < m && k < 2048};
}

// the score table for a chunk of `need` scores: grow-only and at least doubling, up to a full chunk's rows
static inline size_t cache_reserve(size_t need, size_t cap, size_t chunkRows, int nNodes)
{
    if (need > cap) need = std::min(std::max(need, 2 * cap), std::max(chunkRows * (size_t)nNodes, need));
    return need;
}

// The routing hint of searches with an error model (the node's search ran over the budget the last time it was searched on
// this tree).  Hints taken under another budget or threshold say nothing about this one: all are dropped
static inline bool hints_stale(int hintBudget, double hintEff0, int wideBudget, double eff0) { return hintBudget != wideBudget || hintEff0 != eff0; }
// a hinted search leaves the budgeted pass at once -- unless it has a row made ahead: a whole-tree search inside the pass
static inline bool hint_sends_on(bool hinted, int row) { return hinted && !(row >= 0); }
// what the pass saw: over the budget -> the hint is set (nAppend -1: left for shorten(), k_fr_begin -- not over the budget;
// a search the hint sent on says nothing new)
static inline bool hint_set(int status, int nAppend, bool sentOn) { return status == -5 && nAppend >= 0 && !sentOn; }
// (a hinted search that turned out short -- the tree changed around it -- is tried within the budget again next time)
static inline bool hint_clear(bool hinted, int status, int nAppend, int wideBudget) { return hinted && status == 0 && nAppend <= wideBudget / 4; }

}  // namespace plan
}  // namespace maple
