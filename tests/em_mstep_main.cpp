// tests/em_mstep_main.cpp -- maple_amd/csrc/em_mstep.h on its own (no HIP): reads the sufficient statistics of EM steps from
// standard input, prints what the maximisation makes of them.  tests/test_em_mstep.py compiles it with the host sanitizers.
//
// One case is a stream of numbers:
//   lRef model useRateVariation usingErrorRate errorRateSiteSpecific numTips observedTotNucsSites errorCount totTreeLength
//   refIdx[lRef]  rootFreqs[4]  counts[16]  waitingTimes[4]
//   under rate variation: waitingTimesSites[lRef*4] countsSites[lRef] trackingNs[lRef+1]
//   with site-specific errors: observedNucsSites[lRef+1] errorCountSites[lRef]
// and prints one line: rc, Q[16], then (n, values) for siteRates, (0 | 1, value) for the error rate, (n, values) for siteErrRates.
#include "../maple_amd/csrc/em_mstep.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static bool read_f(double *v) { return scanf("%lf", v) == 1; }
static bool read_vec(std::vector<double> &v, size_t n)
{
    v.resize(n);
    for (size_t i = 0; i < n; i++) if (!read_f(&v[i])) return false;
    return true;
}

int main()
{
    for (;;) {
        long long lRef, model, rv, u, ss, numTips, observedTot;
        if (scanf("%lld", &lRef) != 1) return 0;
        if (scanf("%lld %lld %lld %lld %lld %lld", &model, &rv, &u, &ss, &numTips, &observedTot) != 6 || lRef <= 0) return 2;
        maple_em::MStepStats s{};
        s.lRef = (int32_t)lRef;
        s.useRateVariation = rv != 0; s.usingErrorRate = u != 0; s.errorRateSiteSpecific = ss != 0;
        s.numTips = numTips; s.observedTotNucsSites = observedTot;
        if (!read_f(&s.errorCount) || !read_f(&s.totTreeLength)) return 2;
        std::vector<uint8_t> refIdx((size_t)lRef);
        for (auto &r : refIdx) { int x; if (scanf("%d", &x) != 1 || x < 0 || x > 3) return 2; r = (uint8_t)x; }
        std::vector<double> rf, counts, wt, wts, cs, tn, on, ecs;
        if (!read_vec(rf, 4) || !read_vec(counts, 16) || !read_vec(wt, 4)) return 2;
        for (int i = 0; i < 16; i++) s.counts[i] = counts[i];
        for (int i = 0; i < 4; i++) s.waitingTimes[i] = wt[i];
        if (rv && (!read_vec(wts, (size_t)lRef * 4) || !read_vec(cs, (size_t)lRef) || !read_vec(tn, (size_t)lRef + 1))) return 2;
        if (ss && (!read_vec(on, (size_t)lRef + 1) || !read_vec(ecs, (size_t)lRef))) return 2;
        s.refIdx = refIdx.data(); s.rootFreqs = rf.data();
        s.waitingTimesSites = wts.data(); s.countsSites = cs.data(); s.trackingNs = tn.data();
        s.observedNucsSites = on.data(); s.errorCountSites = ecs.data();
        double Q[16], err = 0.0;
        std::vector<double> siteRates(rv ? (size_t)lRef : 0), siteErr(ss ? (size_t)lRef : 0);
        const int rc = maple_em::em_mstep(s, (int)model, Q, rv ? siteRates.data() : nullptr, &err, ss ? siteErr.data() : nullptr);
        printf("%d", rc);
        for (int i = 0; i < 16; i++) printf(" %.17g", Q[i]);
        printf(" %zu", siteRates.size());
        for (double x : siteRates) printf(" %.17g", x);
        printf(" %d", u ? 1 : 0);
        if (u) printf(" %.17g", err);
        printf(" %zu", siteErr.size());
        for (double x : siteErr) printf(" %.17g", x);
        printf("\n");
    }
}
