// tests/sweep_plan_main.cpp -- maple_amd/csrc/sweep_plan.h on the CPU, compiled on its own (tests/test_sweep_plan.py).
// One command per line on stdin, one answer per line on stdout (doubles as C hex floats, so nothing is rounded on the way):
//   V cur t isFalse                                 -> "V update best"                           blen_verdict
//   O n root c0[n] c1[n]                            -> "O ok order..."                           sweep_order
//   N cur used broke                                -> "N next"                                  next_chunk
//   D n root seed chunk sweeps up[n] c0[n] c1[n] dirty[n]
//       -> per sweep "S updates computed used repairs launches | order... | dist[n]... | dirty[n]..."
//      the sweep on a toy model; chunk -1 = the reference's own loop (one node at a time, written out below without
//      sweep_drive), 0 = the adaptive policy, k > 0 = fixed.
// The toy model: a list is a version number.  estimate = a hash of (node, version of its upper list, version of its lower list)
// mapped to a length or to False; repair(v) bumps versions in a pseudo-random neighbourhood of v chosen from (seed, v, length of
// v) -- its children, its sibling, some ancestors and their other children -- and reports those nodes as visited.
#include "../maple_amd/csrc/sweep_plan.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

using namespace sweep_plan;

static uint64_t mix(uint64_t x)
{
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
static uint64_t mix3(uint64_t a, uint64_t b, uint64_t c) { return mix(mix(mix(a) ^ b) ^ c); }

struct Toy {
    int32_t n, root;
    uint64_t seed;
    std::vector<int32_t> up, c0, c1, mut, lower, upRight, upLeft;
    std::vector<uint8_t> tip, dirty;
    std::vector<double> dist;
    int32_t nextId = 1;

    int upListOf(int v) const { const int p = up[v]; return c0[p] == v ? upRight[p] : upLeft[p]; }
    // a length of a few values, so that the 1 % rule both fires and does not; one estimate in 16 is False, one in 16 is 0.0
    void estimate1(int v, int upl, int low, double *t, uint8_t *isFalse) const
    {
        const uint64_t h = mix3(seed ^ (uint64_t)v, (uint64_t)upl, (uint64_t)low);
        *isFalse = (h & 15) == 0;
        if ((h & 15) == 1) { *t = 0.0; return; }
        const double base = 1e-4 * (double)(1 + ((h >> 8) & 3));
        *t = base * (1.0 + 0.004 * (double)((h >> 16) & 7));               // within 2.8 % of base: some moves are under 1 %
    }
    void bumpUpOf(int w) { const int p = up[w]; (c0[p] == w ? upRight : upLeft)[p] = nextId++; }
    int repair(int v, std::vector<int32_t> &visited)
    {
        uint64_t bits;
        memcpy(&bits, &dist[v], 8);
        uint64_t h = mix3(seed, (uint64_t)v, bits);
        auto coin = [&]() { h = mix(h); return (h >> 20) & 1; };
        visited.push_back(v);
        if (c0[v] >= 0)
            for (int ch : {c0[v], c1[v]})
                if (coin()) { visited.push_back(ch); if (coin()) bumpUpOf(ch); }
        int p = up[v], below = v;
        h = mix(h);
        int climbs = 1 + (int)((h >> 24) % 4);
        while (p >= 0 && climbs-- > 0) {
            visited.push_back(p);
            const int other = c0[p] == below ? c1[p] : c0[p];
            if (coin()) { visited.push_back(other); if (coin()) bumpUpOf(other); }
            if (coin()) lower[p] = nextId++;
            below = p;
            p = up[p];
        }
        return 0;
    }
};

static double hexd(const std::string &s) { return strtod(s.c_str(), nullptr); }

static void naive_sweep(Toy &T, int32_t *updates, std::vector<int32_t> &updated, SweepStats &st)
{
    if (T.c0[T.root] < 0) return;
    std::vector<int32_t> stack, visited;
    for (int ch : {T.c0[T.root], T.c1[T.root]})
        if (T.c0[ch] >= 0) { stack.push_back(T.c0[ch]); stack.push_back(T.c1[ch]); }
    while (!stack.empty()) {
        const int v = stack.back();
        stack.pop_back();
        if (T.dirty[v]) {
            double t, best;
            uint8_t f;
            T.estimate1(v, T.upListOf(v), T.lower[v], &t, &f);
            st.launches++; st.computed++; st.used++;
            if (blen_verdict(T.dist[v], t, f != 0, &best)) {
                T.dist[v] = best;
                (*updates)++;
                updated.push_back(v);
                visited.clear();
                T.repair(v, visited);
                st.repairs++;
                for (int w : visited) T.dirty[w] = 1;
            } else T.dirty[v] = 0;
        }
        if (T.c0[v] >= 0) { stack.push_back(T.c0[v]); stack.push_back(T.c1[v]); }
    }
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        if (kind == "V") {
            std::string a, b;
            int f;
            in >> a >> b >> f;
            double best;
            const bool u = blen_verdict(hexd(a), hexd(b), f != 0, &best);
            printf("V %d %a\n", u ? 1 : 0, best);
        } else if (kind == "N") {
            int cur, used, broke;
            in >> cur >> used >> broke;
            printf("N %d\n", next_chunk(cur, used, broke != 0));
        } else if (kind == "O") {
            int32_t n, root;
            in >> n >> root;
            std::vector<int32_t> c0((size_t)n), c1((size_t)n), order, pos;
            for (auto &x : c0) in >> x;
            for (auto &x : c1) in >> x;
            const bool ok = sweep_order(n, root, c0.data(), c1.data(), order, pos);
            for (size_t i = 0; ok && i < order.size(); i++)
                if (pos[order[i]] != (int32_t)i) { fprintf(stderr, "pos is not the inverse of order\n"); return 2; }
            printf("O %d", ok ? 1 : 0);
            for (int v : order) printf(" %d", v);
            printf("\n");
        } else if (kind == "D") {
            Toy T;
            int chunk, sweeps;
            in >> T.n >> T.root >> T.seed >> chunk >> sweeps;
            const size_t n = (size_t)T.n;
            T.up.resize(n); T.c0.resize(n); T.c1.resize(n); T.dirty.resize(n);
            for (auto &x : T.up) in >> x;
            for (auto &x : T.c0) in >> x;
            for (auto &x : T.c1) in >> x;
            for (auto &x : T.dirty) { int d; in >> d; x = (uint8_t)d; }
            if (!in) { fprintf(stderr, "short D line\n"); return 2; }
            T.mut.assign(n, -1); T.tip.resize(n); T.dist.resize(n); T.lower.resize(n); T.upRight.resize(n); T.upLeft.resize(n);
            for (size_t v = 0; v < n; v++) {
                T.tip[v] = T.c0[v] < 0;
                T.lower[v] = T.nextId++; T.upRight[v] = T.nextId++; T.upLeft[v] = T.nextId++;
                const uint64_t h = mix3(T.seed, 77, v);
                T.dist[v] = (h & 7) == 0 ? 0.0 : 1e-4 * (double)(1 + ((h >> 8) & 3));
            }
            std::vector<int32_t> order, pos;
            if (!sweep_order(T.n, T.root, T.c0.data(), T.c1.data(), order, pos)) { fprintf(stderr, "not a tree\n"); return 2; }
            for (int s = 0; s < sweeps; s++) {
                int32_t updates = 0;
                std::vector<int32_t> updated;
                SweepStats st;
                if (chunk < 0) naive_sweep(T, &updates, updated, st);
                else {
                    const SweepTree V{T.n, T.up.data(), T.c0.data(), T.mut.data(), T.tip.data(), T.dist.data(), T.lower.data(),
                                      T.upRight.data(), T.upLeft.data(), T.dirty.data()};
                    const int rc = sweep_drive(
                        V, order, pos, false, chunk,
                        [&](const std::vector<SweepItem> &items, std::vector<double> &t, std::vector<uint8_t> &isFalse) {
                            if (chunk > 0 && (int)items.size() > chunk) return 3;
                            for (size_t i = 0; i < items.size(); i++)
                                T.estimate1(items[i].node, items[i].upList, items[i].lowList, &t[i], &isFalse[i]);
                            return 0;
                        },
                        [&](int v, std::vector<int32_t> &visited) { return T.repair(v, visited); }, &updates, updated, st);
                    if (rc) { fprintf(stderr, "sweep_drive returned %d\n", rc); return 2; }
                }
                printf("S %d %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " |", updates, st.computed, st.used, st.repairs, st.launches);
                for (int v : updated) printf(" %d", v);
                printf(" |");
                for (double d : T.dist) printf(" %a", d);
                printf(" |");
                for (uint8_t d : T.dirty) printf(" %d", d);
                printf("\n");
            }
        } else if (!kind.empty()) {
            fprintf(stderr, "unknown command %s\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
