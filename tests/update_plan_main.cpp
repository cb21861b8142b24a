// tests/update_plan_main.cpp -- maple_amd/csrc/update_plan.h on the CPU, compiled on its own (tests/test_update_plan.py).
// Commands on stdin, answers on stdout (doubles as C hex floats).  A toy model of lists is plugged into the plan: a list id is an
// index, its content a 64-bit value; merge, pass-through-branch and root-vector make a new id whose content is a hash of the
// inputs' contents and arguments, shorten keeps the content, areVectorsDifferent compares contents (exactly, or modulo `coarse`).
// A merge comes out None where a scripted rule says so; estimates come from a scripted queue, then from a hash.
//   tree n root coarse / up.. / c0.. / c1.. / tip.. / mut.. / depth.. / dist.. / low..   (9 lines; low: the tips' contents, 0 = no list)
//        the columns; the four id columns start empty but for the tips' lower lists
//   rebuild bumpLen         rebuild_drive on the current lengths -> result line, state line, log line
//   save / reset            keep the current state / go back to it
//   dist v x | low v c      change a length / give node v a new lower list of content c
//   col name v x            write x into column `name` (up c0 c1 lower) at v: malformed input
//   rules k (udMask zeroOnly halves mod rem)*k     a merge is None if a rule matches: its isUpDown bit in udMask, zeroOnly -> both
//                           lengths 0, halves -> the two lengths equal, and content % mod == rem  (not applied by `rebuild` / `check`)
//   blen k (t isFalse)*k    the next k estimates
//   repair k v*k            repair_drive -> result line "ok replaced" or "err kind|message", state line, log line, "B ..." line:
//                           replaced nodes | visited nodes | 1 if every flag is zero again
//   keepright 0|1           set Scratch::keepRootRight: the root's probVectUpRight is left alone where only the root's child 1 changed
//   check                   "same 1" if a rebuild on the current lengths gives the contents of the current state
// state line: "S lower.. | upRight.. | upLeft.. | totUp.. | dist.." (contents, - for none); log line: "L" and per items call
// " I node:kind.." (kind 0 totUp, 1 upRight, 2 upLeft, 3 lower), per estimate " E", per pass " P<n>", root vectors " R<n>", differ " D".
#include "../maple_amd/csrc/update_plan.h"

#include <cinttypes>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

using namespace update_plan;

static uint64_t bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }
static uint64_t hashOf(std::initializer_list<uint64_t> xs)           // (the test computes the same in Python: kept cheap)
{
    uint64_t h = 0x9e3779b97f4a7c15ull;
    for (uint64_t x : xs) { h = (h ^ x) * 0xbf58476d1ce4e5b9ull; h ^= h >> 32; }
    return h;
}

struct Rule { int udMask, zeroOnly, halves; uint64_t mod, rem; };

struct ToyOps {
    std::vector<uint64_t> content;                // per list id
    uint64_t coarse = 0;
    std::vector<Rule> rules;
    bool rulesOn = true;
    std::vector<std::pair<double, int>> blenQueue;
    size_t blenAt = 0;
    std::string log;

    int32_t make(uint64_t c) { content.push_back(c); return (int32_t)content.size() - 1; }
    bool isNone(uint64_t h, double b1, double b2, int ud) const
    {
        if (!rulesOn) return false;
        for (const Rule &r : rules)
            if (((r.udMask >> ud) & 1) && (!r.zeroOnly || (b1 == 0.0 && b2 == 0.0)) && (!r.halves || b1 == b2) && h % r.mod == r.rem) return true;
        return false;
    }
    bool different(uint64_t a, uint64_t b) const { return coarse ? a % coarse != b % coarse : a != b; }
    int pass(int32_t n, const int32_t *lists, const int32_t *mutLists, bool dirUp, int32_t *out)
    {
        log += " P" + std::to_string(n);
        for (int i = 0; i < n; i++) out[i] = make(hashOf({2, content.at(lists[i]), (uint64_t)mutLists[i], dirUp ? 1u : 0u}));
        return 0;
    }
    int items(Batch &B, size_t first, size_t n)
    {
        log += " I";
        for (size_t i = first; i < first + n; i++) {
            log += " " + std::to_string(B.node.at(i)) + ":" + std::to_string(B.kind.at(i));
            const uint64_t h = hashOf({1, content.at(B.l1.at(i)), bits(B.b1.at(i)), B.t1.at(i), content.at(B.l2.at(i)), bits(B.b2.at(i)), B.t2.at(i), B.ud.at(i)});
            B.none.at(i) = isNone(h, B.b1[i], B.b2[i], B.ud[i]);
            B.diff.at(i) = 1;
            B.out.at(i) = -1;
            if (B.none[i]) continue;
            const int32_t old = B.old.at(i);
            if (B.mode.at(i) == 2 && old >= 0) B.diff[i] = different(content.at(old), h);            // (old, new), unshortened
            if (B.mode[i] == 2 && !B.diff[i]) continue;                                              // nothing to replace
            B.out[i] = make(h);                                                                      // shorten keeps the content
            if (B.mode[i] == 0 && old >= 0) B.diff[i] = different(h, content.at(old));
        }
        return 0;
    }
    int blen(int32_t upList, int32_t lowList, uint8_t tip, double *t, uint8_t *isFalse)
    {
        log += " E";
        const uint64_t h = hashOf({4, content.at(upList), content.at(lowList), tip});
        if (blenAt < blenQueue.size()) { *t = blenQueue[blenAt].first; *isFalse = (uint8_t)blenQueue[blenAt].second; blenAt++; return 0; }
        *isFalse = (h & 7) == 0;
        *t = 1e-4 * (double)(1 + ((h >> 8) & 3));
        return 0;
    }
    int rootVector(int32_t n, const int32_t *lists, const double *bLen, const uint8_t *tip, int32_t rootMut, int32_t *out)
    {
        log += " R" + std::to_string(n);
        for (int i = 0; i < n; i++) out[i] = make(hashOf({3, content.at(lists[i]), bits(bLen[i]), tip[i], (uint64_t)(int64_t)rootMut}));
        return 0;
    }
    int differ(int32_t a, int32_t b, uint8_t *d) { log += " D"; *d = different(content.at(a), content.at(b)); return 0; }
};

struct State {
    int32_t n = 0, root = 0;
    std::vector<int32_t> up, c0, c1, mut, depth, lower, upRight, upLeft, totUp;
    std::vector<uint8_t> tip;
    std::vector<double> dist;
    Tree view() { return Tree{n, root, up.data(), c0.data(), c1.data(), tip.data(), mut.data(), depth.data(), dist.data(), lower.data(),
                              upRight.data(), upLeft.data(), totUp.data()}; }
};

static void printState(const State &s, const ToyOps &ops)
{
    printf("S");
    for (const std::vector<int32_t> *col : {&s.lower, &s.upRight, &s.upLeft, &s.totUp}) {
        for (int32_t id : *col) if (id < 0) printf(" -"); else printf(" %" PRIu64, ops.content.at(id));
        printf(" |");
    }
    for (double d : s.dist) printf(" %a", d);
    printf("\n");
}
static void printResult(int rc, const Error &E, int32_t value)
{
    if (!rc) printf("ok %d\n", value);
    else if (E.kind) printf("err %d|%s\n", E.kind, E.msg);
    else printf("err 0|operation failed with %d\n", rc);
}
static bool sameContents(const State &a, const State &b, const ToyOps &ops)
{
    auto eq = [&](const std::vector<int32_t> &x, const std::vector<int32_t> &y) {
        for (size_t i = 0; i < x.size(); i++)
            if ((x[i] < 0) != (y[i] < 0) || (x[i] >= 0 && ops.content.at(x[i]) != ops.content.at(y[i]))) return false;
        return true;
    };
    return eq(a.lower, b.lower) && eq(a.upRight, b.upRight) && eq(a.upLeft, b.upLeft) && eq(a.totUp, b.totUp);
}

int main()
{
    State cur, saved;
    ToyOps ops;
    Scratch scratch;                              // persistent across the repairs of a run, like the context's
    std::string line;
    auto readRow = [&](auto &col, size_t n, bool hex) {
        std::getline(std::cin, line);
        std::istringstream in(line);
        col.resize(n);
        for (auto &x : col) { std::string w; in >> w; x = hex ? (decltype(+x))strtod(w.c_str(), nullptr) : (decltype(+x))strtoll(w.c_str(), nullptr, 10); }
        if (!in) { fprintf(stderr, "short row\n"); exit(2); }
    };
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "tree") {
            cur = State();
            ops = ToyOps();
            in >> cur.n >> cur.root >> ops.coarse;
            const size_t n = (size_t)cur.n;
            std::vector<int> tip;
            std::vector<unsigned long long> low;
            readRow(cur.up, n, false); readRow(cur.c0, n, false); readRow(cur.c1, n, false); readRow(tip, n, false);
            readRow(cur.mut, n, false); readRow(cur.depth, n, false); readRow(cur.dist, n, true);
            std::getline(std::cin, line);
            std::istringstream lin(line);
            cur.tip.assign(tip.begin(), tip.end());
            cur.lower.assign(n, -1); cur.upRight.assign(n, -1); cur.upLeft.assign(n, -1); cur.totUp.assign(n, -1);
            for (size_t v = 0; v < n; v++) { unsigned long long c = 0; lin >> c; if (c) cur.lower[v] = ops.make(c); }
            if (!lin) { fprintf(stderr, "short low row\n"); return 2; }
        } else if (cmd == "rebuild") {
            std::string b;
            in >> b;
            int32_t bad[8], nBad = 0;
            Error E;
            ops.log.clear();
            ops.rulesOn = false;
            const Tree T = cur.view();
            const int rc = rebuild_drive(T, ops, strtod(b.c_str(), nullptr), 8, bad, &nBad, E);
            ops.rulesOn = true;
            printResult(rc, E, nBad);
            printState(cur, ops);
            printf("L%s\n", ops.log.c_str());
        } else if (cmd == "save") saved = cur;
        else if (cmd == "reset") cur = saved;
        else if (cmd == "dist") { int v; std::string x; in >> v >> x; cur.dist.at(v) = strtod(x.c_str(), nullptr); }
        else if (cmd == "low") { int v; unsigned long long c; in >> v >> c; cur.lower.at(v) = ops.make(c); }
        else if (cmd == "col") {
            std::string name; int v, x;
            in >> name >> v >> x;
            (name == "up" ? cur.up : name == "c0" ? cur.c0 : name == "c1" ? cur.c1 : cur.lower).at(v) = x;
        } else if (cmd == "rules") {
            size_t k;
            in >> k;
            ops.rules.assign(k, Rule());
            for (Rule &r : ops.rules) in >> r.udMask >> r.zeroOnly >> r.halves >> r.mod >> r.rem;
        } else if (cmd == "blen") {
            size_t k;
            in >> k;
            ops.blenQueue.clear();
            ops.blenAt = 0;
            for (size_t i = 0; i < k; i++) { std::string t; int f; in >> t >> f; ops.blenQueue.emplace_back(strtod(t.c_str(), nullptr), f); }
        } else if (cmd == "repair") {
            size_t k;
            in >> k;
            std::vector<int32_t> changed(k);
            for (auto &v : changed) in >> v;
            Error E;
            int32_t nReplaced = -1;
            ops.log.clear();
            const Tree T = cur.view();
            const int rc = repair_drive(T, scratch, ops, (int32_t)k, changed.data(), false, E, &nReplaced);
            printResult(rc, E, nReplaced);
            printState(cur, ops);
            printf("L%s\n", ops.log.c_str());
            printf("B");
            for (int v : scratch.replacedNodes) printf(" %d", v);
            printf(" |");
            for (int v : scratch.visitedNodes) printf(" %d", v);
            bool zero = scratch.touched.empty();
            for (const std::vector<uint8_t> *f : {&scratch.dLow, &scratch.dUp, &scratch.dDist, &scratch.dCh0, &scratch.dCh1, &scratch.inFrontier, &scratch.inTodo})
                for (uint8_t x : *f) zero = zero && !x;
            printf(" | %d |", zero ? 1 : 0);
#define PRINT_STAT(name) printf(" " #name "=%lld", (long long)scratch.stats.name);
            UPDATE_PLAN_STATS(PRINT_STAT)
#undef PRINT_STAT
            printf("\n");
        } else if (cmd == "keepright") {                              // Scratch::keepRootRight for the repairs that follow
            int on = 0;
            in >> on;
            scratch.keepRootRight = on != 0;
        } else if (cmd == "check") {
            State again = cur;
            for (size_t v = 0; v < (size_t)cur.n; v++) if (cur.c0[v] >= 0) again.lower[v] = -1;
            Error E;
            ToyOps &o = ops;
            const std::string keep = o.log;
            o.rulesOn = false;
            const Tree T = again.view();
            const int rc = rebuild_drive(T, o, 0.0, 0, nullptr, nullptr, E);
            o.rulesOn = true;
            o.log = keep;
            printf("same %d\n", !rc && sameContents(cur, again, o) ? 1 : 0);
        } else if (!cmd.empty()) {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
        if (!in && cmd != "save" && cmd != "reset" && cmd != "check") { fprintf(stderr, "short command: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
