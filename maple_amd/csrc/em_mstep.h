// maple_amd/csrc/em_mstep.h -- the maximisation part of the EM step (expectationMaximizationCalculationRates, M:10852-10947): from
// the sufficient statistics the walk over the branches leaves (em.hip) to the new rate matrix, site rates, error rate and site
// error rates.  Pure host code in the reference's association order, no HIP headers: maple_em_rates calls it, and
// tests/em_mstep_main.cpp feeds it the statistics recorded from the reference (compile with -ffp-contract=off).
#pragma once
#include <cstddef>
#include <cstdint>

namespace maple_em {

enum { EM_UNREST = 0, EM_GTR = 1 };
constexpr double EM_MIN_ERROR_PRB = 0.0000000001;   // minErrorPrb, M:10088

struct MStepStats {                    // what M:10113-10136 accumulates, as it stands at M:10852
    int32_t lRef;
    const uint8_t *refIdx;             // refIndeces [lRef]
    const double *rootFreqs;           // [4]
    bool useRateVariation, usingErrorRate, errorRateSiteSpecific;
    double counts[16], waitingTimes[4], errorCount, totTreeLength;
    int64_t observedTotNucsSites, numTips;
    double *waitingTimesSites;         // [lRef * 4]; M:10913 adds the running tree length in place
    const double *countsSites;         // [lRef]
    const double *trackingNs;          // [lRef + 1]
    const double *observedNucsSites;   // [lRef + 1]
    const double *errorCountSites;     // [lRef]
};

// Returns 0, or -1 where the reference raises (M:10877-10879: a model other than UNREST / GTR without an error model).
// Q16 always; siteRates [lRef] under rate variation; *errorRate under an error model; siteErrRates [lRef] when site-specific.
static inline int em_mstep(MStepStats &s, int model, double *Q16, double *siteRates, double *errorRate, double *siteErrRates)
{
    const int lRef = s.lRef;
    double counts[4][4];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) counts[i][j] = s.counts[i * 4 + j];
    int64_t observedTot = s.observedTotNucsSites;
    if (s.usingErrorRate) observedTot += (int64_t)lRef * s.numTips;                  // M:10853
    if (model == EM_UNREST) {                                                        // M:10855-10864
        for (int i = 0; i < 4; i++) {
            if (s.waitingTimes[i] == 0.0) { for (int j = 0; j < 4; j++) counts[i][j] = 0.0; }
            else {
                for (int j = 0; j < 4; j++) if (i != j) counts[i][j] /= s.waitingTimes[i];
                double sum = 0.0;
                for (int j = 0; j < 4; j++) sum += counts[i][j];
                counts[i][i] = -sum;
            }
        }
    } else if (model == EM_GTR) {                                                    // M:10865-10876
        double nr[4][4] = {};
        for (int i = 0; i < 4; i++) {
            if (s.waitingTimes[i] == 0.0) { for (int j = 0; j < 4; j++) nr[i][j] = 0.0; }
            else {
                for (int j = 0; j < 4; j++) if (i != j) nr[i][j] = (counts[i][j] + counts[j][i]) / s.waitingTimes[i];
                double sum = 0.0;
                for (int j = 0; j < 4; j++) sum += nr[i][j];
                nr[i][i] = -sum;
            }
        }
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) counts[i][j] = nr[i][j];
    } else if (!s.usingErrorRate) return -1;                                         // M:10877-10879
    const double *rf = s.rootFreqs;
    double totRate = -(rf[0] * counts[0][0] + rf[1] * counts[1][1] + rf[2] * counts[2][2] + rf[3] * counts[3][3]);
    if (totRate != 0.0)
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) counts[i][j] = counts[i][j] / totRate;
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) Q16[i * 4 + j] = counts[i][j];

    if (s.usingErrorRate) {                                                          // M:10886-10898
        if (errorRate) *errorRate = s.errorCount / (double)observedTot;
        if (s.errorRateSiteSpecific && siteErrRates) {
            double observedNuc = (double)s.numTips;
            for (int i = 0; i < lRef; i++) {
                observedNuc += s.observedNucsSites[i];
                if (observedNuc > 0) {
                    const double e = s.errorCountSites[i] / observedNuc;
                    siteErrRates[i] = e > EM_MIN_ERROR_PRB ? e : EM_MIN_ERROR_PRB;
                } else siteErrRates[i] = EM_MIN_ERROR_PRB;
            }
        }
    }
    if (s.useRateVariation && siteRates) {                                           // M:10907-10938
        double totTreeLength = s.totTreeLength, normalization = 0.0;
        totRate = 0.0;
        for (int i = 0; i < lRef; i++) {
            double *w = s.waitingTimesSites + (size_t)i * 4;
            totTreeLength += s.trackingNs[i];
            w[s.refIdx[i]] += totTreeLength;
            double totExpected = 0.0;
            for (int j = 0; j < 4; j++) totExpected -= w[j] * counts[j][j];
            if (totExpected == 0.0) siteRates[i] = 1.0;
            else siteRates[i] = (s.countsSites[i] + 1) / (totExpected + 1);
            for (int j = 0; j < 4; j++) totRate -= w[j] * counts[j][j] * siteRates[i];
            double sum = 0.0;
            for (int j = 0; j < 4; j++) sum += w[j];
            normalization += sum;
        }
        totRate = totRate / normalization;
        const double maxRateAllowed = 0.005 * lRef;
        for (int i = 0; i < lRef; i++) {
            const double x = siteRates[i] / totRate;
            const double lo = x > 0.001 ? x : 0.001;                                 // max(0.001, x)
            siteRates[i] = lo < maxRateAllowed ? lo : maxRateAllowed;                // min(maxRateAllowed, .)
        }
    }
    return 0;
}

} // namespace maple_em
