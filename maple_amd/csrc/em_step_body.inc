// maple_amd/csrc/em_step_body.inc -- one step of the EM walk over a (parent upper list, child lower list) pair: the body of the
// reference's inner loop (expectationMaximizationCalculationRates, M:10166-10790), arm for arm and in its association order.
// Included by k_em_walk (em.hip) inside the loop over the two cursors; in scope:
//   e1 / e2 (Ent of the parent / child side), pos (positions consumed so far = the 0-based site), dist, leaf, nMinor,
//   fm / nFm / iFm (the frame's accumulated (position, nucleotide) list, M:10107-10109 + passMutationListThroughBranch), refIdx,
//   lRef, c (Ctx), rf, cb (cumulativeBases) and the accumulation macros:
//   WT(i, x) waitingTimes[i] += x; CNT(i, j, x) counts[i][j] += x; ERRC(x) errorCount += x          (this lane's own sums)
//   WTS(i, x) waitingTimesSites[pos][i] += x; WTS_AT(p, i, x); CS(x) countsSites[pos] += x; TN(p, x) trackingNs[p] += x;
//   ECS(x) errorCountSites[pos] += x; OBS(p, k) observedNucsSites[p] += k; OBSTOT(k) observedTotNucsSites += k
//   NEG(x) the reference's "if x < 0.0: raise" under rate variation.
// and the hooks at the places where the reference, under trackMutations, appends a record (empty in k_em_walk; the sink of
// k_mat_walk, mat_events.hip):
//   MUT(i, j, x) mutationsInf[node].append((i, pos+1, j, x)) if x > minMutProb; MUT_SURE(i, j) the unconditional one of M:10760;
//   ERRREC(i, j, x) errors[node].append((i, pos+1, j, x)) if x > minMutProb; NS_RUN(last) M:10180-10182; NS_SITE() M:10256 / 10432.
// The per-site macros do nothing where the model has no such table.
{
    while (iFm < nFm && fm[iFm].x < pos) iFm++;                          // M:10166-10167
    if (e2.type == 5) {                                                  // M:10168-10187
        const int end = min(e1.pos, e2.pos);                             // (an entry's pos is its LAST position: pos + 1 for a single site)
        if (U && leaf) {
            if (SS) OBS(pos, -(long long)(1 + nMinor));
            else OBSTOT(-(long long)(end - pos) * (1 + nMinor));
        }
        TN(pos, -dist);
        NS_RUN(e2.pos);
        pos = end;
        TN(pos, dist);
        if (U && SS && leaf) OBS(pos, (long long)(1 + nMinor));
    } else if (e1.type == 5) {                                           // M:10189-10206
        const int end = min(e1.pos, e2.pos);
        TN(pos, -dist);
        pos = end;
        TN(pos, dist);
    } else {
        double totLen1 = dist;                                           // M:10208-10225
        if (e1.type < 5) { if (e1.hasD0 && !e1.hasD1) totLen1 += e1.d0; else if (e1.hasD1) totLen1 += e1.d1; }
        else if (e1.hasD0) totLen1 += e1.d0;
        double totLen2 = 0.0;
        if (e2.hasD0) totLen2 += e2.d0;
        if (e1.type == 4 && e2.type == 4) {                              // M:10227-10243
            const int end = min(e1.pos, e2.pos);
            if (totLen2 == 0.0 && dist != 0.0) {
                for (int i = 0; i < 4; i++) WT(i, totLen1 * (double)(cb[end * 4 + i] - cb[pos * 4 + i]));
                while (iFm < nFm && fm[iFm].x < end) {                   // the MAT frame's own differences from the reference
                    const int altNuc = fm[iFm].y, altPos = fm[iFm].x;
                    const int refNuc = refIdx[altPos];                   // (sic: M:10236 indexes by the 1-based position)
                    WT(refNuc, -totLen1);
                    WT(altNuc, totLen1);
                    iFm++;
                    WTS_AT(altPos - 1, altNuc, totLen1);
                    WTS_AT(altPos - 1, refNuc, -totLen1);
                }
            }
            pos = end;
        } else {
            const double r = c.rate(pos);
            auto q = [&](int i, int j) { return c.q(r, i, j); };         // mutMatrix[i][j] (mutMatrices[pos] under rate variation)
            const int refN = refIdx[pos];
            const double *v1 = e1.vec, *v2 = e2.vec;
            if (e1.type == 6) {                                          // M:10247-10422
                if (totLen2 == 0.0) {
                    double normalization = 0.0;
                    WTS(refN, -totLen1);
                    if (e2.type == 6) {
                        if (leaf) NS_SITE();                             // M:10255-10256
                        if (leaf && U) {                                 // M:10257-10293
                            const double errorRate = c.err(pos);
                            double noMutProb = 0.0, mutProb = 0.0, errorProb = 0.0;
                            for (int j = 0; j < 4; j++)
                                if (v2[j] > 0.1) {
                                    noMutProb += v1[j];
                                    errorProb += (1.0 - v1[j]) * errorRate * 0.33333;
                                    for (int i = 0; i < 4; i++) if (j != i) mutProb += v1[i] * q(i, j) * totLen1;
                                }
                            normalization = errorProb + noMutProb + mutProb;
                            errorProb = errorProb / normalization;
                            ERRC(errorProb);
                            ECS(errorProb);
                            for (int j = 0; j < 4; j++)
                                if (v2[j] > 0.1) {
                                    WT(j, totLen1 * v1[j] / normalization);
                                    WTS(j, totLen1 * v1[j] / normalization);
                                    for (int i = 0; i < 4; i++)
                                        if (j != i) {
                                            const double mutProbij = v1[i] * q(i, j) * totLen1 / normalization;
                                            WT(j, totLen1 * mutProbij / 2);
                                            WT(i, totLen1 * mutProbij / 2);
                                            CNT(i, j, mutProbij);
                                            WTS(j, totLen1 * mutProbij / 2);
                                            WTS(i, totLen1 * mutProbij / 2);
                                            CS(mutProbij);
                                            NEG(mutProbij);
                                        }
                                }
                        } else {                                         // M:10296-10336
                            unsigned approxFailed = 0;
                            for (int i = 0; i < 4; i++) {
                                const double stayProb = 1.0 + q(i, i) * totLen1;
                                if (stayProb < 0) {
                                    for (int j = 0; j < 4; j++) normalization += v1[i] * 0.25 * v2[j];
                                    approxFailed |= 1u << i;
                                } else {
                                    for (int j = 0; j < 4; j++) {
                                        if (i == j) normalization += v1[i] * stayProb * v2[j];
                                        else normalization += v1[i] * q(i, j) * totLen1 * v2[j];
                                    }
                                }
                            }
                            for (int i = 0; i < 4; i++)
                                for (int j = 0; j < 4; j++) {
                                    const bool af = (approxFailed >> i) & 1u;
                                    if (i == j) {
                                        const double prob = af ? v1[i] * 0.25 * v2[j] / normalization
                                                               : v1[i] * (1.0 + q(i, i) * totLen1) * v2[j] / normalization;
                                        WT(i, totLen1 * prob);
                                        WTS(i, totLen1 * prob);
                                    } else {
                                        const double prob = af ? v1[i] * 0.25 * v2[j] / normalization
                                                               : v1[i] * q(i, j) * totLen1 * v2[j] / normalization;
                                        WT(i, (totLen1 / 2) * prob);
                                        WT(j, (totLen1 / 2) * prob);
                                        CNT(i, j, prob);
                                        MUT(i, j, prob);
                                        WTS(i, (totLen1 / 2) * prob);
                                        WTS(j, (totLen1 / 2) * prob);
                                        CS(prob);
                                        NEG(prob);
                                    }
                                }
                        }
                    } else {                                             // O over a nucleotide, M:10338-10422
                        const int i2 = (e2.type == 4) ? e1.ref : e2.type;
                        if (leaf && U && nMinor == 0) {                  // M:10343-10380
                            const double errorRate = c.err(pos);
                            double errorProb = (1.0 - v1[i2]) * errorRate * 0.33333;
                            double noMutProb = v1[i2];
                            double mutProb = 0.0;
                            for (int i = 0; i < 4; i++) if (i != i2) mutProb += v1[i] * q(i, i2) * totLen1;
                            normalization = errorProb + noMutProb + mutProb;
                            errorProb = errorProb / normalization;
                            noMutProb = noMutProb / normalization;
                            mutProb = mutProb / normalization;
                            ERRC(errorProb);
                            ERRREC(4, i2, errorProb);
                            ECS(errorProb);
                            WT(i2, totLen1 * noMutProb);
                            WT(i2, (totLen1 / 2) * mutProb);
                            WTS(i2, totLen1 * noMutProb);
                            WTS(i2, totLen1 * mutProb / 2);
                            CS(mutProb);
                            NEG(mutProb);
                            for (int i = 0; i < 4; i++)
                                if (i != i2) {
                                    const double prob = v1[i] * q(i, i2) * totLen1 / normalization;
                                    const double probErr = v1[i] * errorRate * 0.33333 / normalization;
                                    WT(i, totLen1 * (probErr + prob / 2));
                                    CNT(i, i2, prob);
                                    MUT(i, i2, prob);
                                    WTS(i, totLen1 * (probErr + prob / 2));
                                }
                        } else {                                         // M:10382-10422
                            const double stayProb = 1.0 + q(i2, i2) * totLen1;
                            bool approxFailed;
                            if (stayProb < 0) { normalization = 0.25; approxFailed = true; }
                            else {
                                approxFailed = false;
                                for (int i = 0; i < 4; i++) {
                                    if (i == i2) normalization += v1[i] * stayProb;
                                    else normalization += v1[i] * q(i, i2) * totLen1;
                                }
                            }
                            for (int i = 0; i < 4; i++) {
                                if (i == i2) {
                                    const double prob = approxFailed ? v1[i] : v1[i] * (1.0 + q(i, i) * totLen1) / normalization;
                                    WT(i, totLen1 * prob);
                                    WTS(i, totLen1 * prob);
                                } else {
                                    const double prob = approxFailed ? v1[i] : v1[i] * q(i, i2) * totLen1 / normalization;
                                    WT(i, (totLen1 / 2) * prob);
                                    WT(i2, (totLen1 / 2) * prob);
                                    CNT(i, i2, prob);
                                    MUT(i, i2, prob);
                                    WTS(i, (totLen1 / 2) * prob);
                                    WTS(i2, (totLen1 / 2) * prob);
                                    CS(prob);
                                    NEG(prob);
                                }
                            }
                        }
                    }
                }
            } else {                                                     // the parent side shows a nucleotide, M:10424-10788
                const int i1 = (e1.type == 4) ? e2.ref : e1.type;
                if (e2.type == 6) {                                      // ... the child an O vector, M:10430-10676
                    if (leaf) NS_SITE();                                 // M:10431-10432
                    if (v2[i1] > 0.1) {                                  // the parent's nucleotide is possible: nothing happened
                        WT(i1, totLen1);
                        WTS(refN, -totLen1);
                        WTS(i1, totLen1);
                    } else if (leaf && U) {                              // M:10438-10555
                        const double errorRate = c.err(pos);
                        int numAltNucs = 0;
                        for (int i = 0; i < 4; i++) if (v2[i] > 0.1) numAltNucs++;
                        if (e1.hasD1) {                                  // across the root, M:10447-10516
                            double stayProb1 = 1.0 + q(i1, i1) * totLen1;
                            if (stayProb1 < 0) stayProb1 = 0.25;
                            double stayProb2 = 1.0 + q(i1, i1) * e1.d0;
                            bool approxFailed2 = false;
                            if (stayProb2 < 0) { approxFailed2 = true; stayProb2 = 0.25; }
                            double errProb = rf[i1] * stayProb1 * stayProb2 * errorRate * 0.33333 * numAltNucs;
                            double mutProb = 0.0;
                            const double i1rootProb = rf[i1] * stayProb2;
                            for (int i = 0; i < 4; i++)
                                if (v2[i] > 0.1) {
                                    stayProb1 = 1.0 + q(i, i) * totLen1;
                                    bool approxFailed1 = false;
                                    if (stayProb1 < 0) { approxFailed1 = true; stayProb1 = 0.25; }
                                    if (approxFailed1) mutProb += i1rootProb * 0.25;
                                    else mutProb += i1rootProb * q(i1, i) * totLen1;
                                    if (approxFailed2) mutProb += rf[i] * stayProb1 * 0.25;
                                    else mutProb += rf[i] * stayProb1 * q(i, i1) * e1.d0;
                                }
                            const double normalization = errProb + mutProb;
                            errProb = errProb / normalization;
                            WTS(refN, -totLen1);
                            WTS(i1, totLen1 * errProb);
                            WT(i1, totLen1 * errProb);
                            ERRC(errProb);
                            ECS(errProb);
                            for (int i = 0; i < 4; i++)                  // i is the root nucleotide
                                if (v2[i] > 0.1) {
                                    stayProb1 = 1.0 + q(i, i) * totLen1;
                                    bool approxFailed1 = false;
                                    if (stayProb1 < 0) { approxFailed1 = true; stayProb1 = 0.25; }
                                    const double prob1 = approxFailed1 ? i1rootProb * 0.25 / normalization
                                                                       : i1rootProb * q(i1, i) * totLen1 / normalization;
                                    const double probi = approxFailed2 ? rf[i] * stayProb1 * 0.25 / normalization
                                                                       : rf[i] * stayProb1 * q(i, i1) * e1.d0 / normalization;
                                    WT(i, totLen1 * (probi + prob1 / 2));
                                    WT(i1, totLen1 * prob1 / 2);
                                    CNT(i1, i, prob1);
                                    WTS(i, totLen1 * (probi + prob1 / 2));
                                    WTS(i1, totLen1 * prob1 / 2);
                                    CS(prob1);
                                    NEG(prob1);
                                }
                        } else {                                         // M:10518-10555
                            double stayProb = 1.0 + q(i1, i1) * totLen1;
                            bool approxFailed = false;
                            if (stayProb < 0) { approxFailed = true; stayProb = 0.25; }
                            double errProb = stayProb * errorRate * 0.33333 * numAltNucs;
                            double mutProb = 0.0;
                            for (int i = 0; i < 4; i++)
                                if (v2[i] > 0.1) {
                                    if (approxFailed) mutProb += 0.25;
                                    else mutProb += q(i1, i) * totLen1;
                                }
                            const double normalization = errProb + mutProb;
                            errProb = errProb / normalization;
                            WTS(refN, -totLen1);
                            WTS(i1, totLen1 * errProb);
                            WT(i1, totLen1 * errProb);
                            ERRC(errProb);
                            ECS(errProb);
                            for (int i = 0; i < 4; i++)
                                if (v2[i] > 0.1) {
                                    const double prob = q(i1, i) * totLen1 / normalization;
                                    WT(i1, (totLen1 / 2) * prob);
                                    WT(i, (totLen1 / 2) * prob);
                                    CNT(i1, i, prob);
                                    WTS(i1, (totLen1 / 2) * prob);
                                    WTS(i, (totLen1 / 2) * prob);
                                    CS(prob);
                                    NEG(prob);
                                }
                        }
                    } else if (totLen2 == 0.0) {                         // M:10557-10676
                        double normalization = 0.0;
                        if (e1.hasD1) {                                  // across the root, M:10561-10635
                            WTS(refN, -totLen1);
                            double stayProb1 = 1.0 + q(i1, i1) * e1.d0;
                            bool approxFailed1 = false;
                            if (stayProb1 < 0) { approxFailed1 = true; stayProb1 = 0.25; }
                            for (int i = 0; i < 4; i++) {
                                double stayProb2 = 1.0 + q(i, i) * totLen1;
                                bool approxFailed2 = false;
                                if (stayProb2 < 0) { approxFailed2 = true; stayProb2 = 0.25; }
                                if (i1 == i) {
                                    const double prob = rf[i] * stayProb1;
                                    double tot3;
                                    if (approxFailed2) tot3 = 0.25;
                                    else {
                                        tot3 = 0.0;
                                        for (int j = 0; j < 4; j++) tot3 += q(i, j) * v2[j];
                                        tot3 *= totLen1;
                                        tot3 += v2[i];
                                    }
                                    normalization += prob * tot3;
                                } else {
                                    const double prob = approxFailed1 ? rf[i] * 0.25 * stayProb2 * v2[i]
                                                                      : rf[i] * q(i, i1) * e1.d0 * stayProb2 * v2[i];
                                    normalization += prob;
                                }
                            }
                            for (int i = 0; i < 4; i++) {
                                double stayProb2 = 1.0 + q(i, i) * totLen1;
                                bool approxFailed2 = false;
                                if (stayProb2 < 0) { approxFailed2 = true; stayProb2 = 0.25; }
                                if (i1 == i) {
                                    const double prob = rf[i] * stayProb1;
                                    for (int j = 0; j < 4; j++) {
                                        if (j == i) {
                                            const double tot3 = prob * stayProb2 * v2[j] / normalization;
                                            WT(i, totLen1 * tot3);
                                            WTS(i, totLen1 * tot3);
                                        } else {
                                            const double tot3 = approxFailed2 ? prob * 0.25 * v2[j] / normalization
                                                                              : prob * q(i, j) * totLen1 * v2[j] / normalization;
                                            WT(i, (totLen1 / 2) * tot3);
                                            WT(j, (totLen1 / 2) * tot3);
                                            CNT(i, j, tot3);
                                            if (!leaf) MUT(i1, j, tot3); // (sic: i1 == i here, M:10619-10620)
                                            WTS(i, (totLen1 / 2) * tot3);
                                            WTS(j, (totLen1 / 2) * tot3);
                                            CS(tot3);
                                            NEG(tot3);
                                        }
                                    }
                                } else {
                                    const double prob = approxFailed1 ? rf[i] * 0.25 * stayProb2 * v2[i] / normalization
                                                                      : rf[i] * q(i, i1) * e1.d0 * stayProb2 * v2[i] / normalization;
                                    WT(i, totLen1 * prob);
                                    WTS(i, totLen1 * prob);
                                }
                            }
                        } else {                                         // M:10637-10676
                            WTS(refN, -totLen1);
                            const double stayProb = 1.0 + q(i1, i1) * totLen1;
                            bool approxFailed;
                            if (stayProb < 0) { normalization = 0.25; approxFailed = true; }
                            else {
                                approxFailed = false;
                                for (int i = 0; i < 4; i++) {
                                    if (i1 == i) normalization += stayProb * v2[i];
                                    else normalization += q(i1, i) * totLen1 * v2[i];
                                }
                            }
                            for (int i = 0; i < 4; i++) {
                                if (i1 == i) {
                                    const double prob = approxFailed ? v2[i] : (1.0 + q(i, i) * totLen1) * v2[i] / normalization;
                                    WT(i, totLen1 * prob);
                                    WTS(i, totLen1 * prob);
                                } else {
                                    const double prob = approxFailed ? v2[i] : q(i1, i) * totLen1 * v2[i] / normalization;
                                    WT(i1, (totLen1 / 2) * prob);
                                    WT(i, (totLen1 / 2) * prob);
                                    CNT(i1, i, prob);
                                    if (!leaf) MUT(i1, i, prob);         // M:10669-10670
                                    WTS(i1, (totLen1 / 2) * prob);
                                    WTS(i, (totLen1 / 2) * prob);
                                    CS(prob);
                                    NEG(prob);
                                }
                            }
                        }
                    }
                } else {                                                 // two nucleotides, M:10678-10788
                    const int i2 = (e2.type < 4) ? e2.type : e1.ref;
                    if (i2 == i1) {
                        if (totLen2 == 0.0) {
                            WT(i1, totLen1);
                            WTS(i1, totLen1);
                            WTS(refN, -totLen1);
                        }
                    } else if (leaf && U && nMinor == 0) {               // M:10695-10747
                        const double errorRate = c.err(pos);
                        if (!e1.hasD1) {
                            double errorProb = errorRate * 0.33333;
                            double mutProb = q(i1, i2) * totLen1;
                            const double normalization = errorProb + mutProb;
                            errorProb = errorProb / normalization;
                            mutProb = mutProb / normalization;
                            WTS(refN, -totLen1);
                            WTS(i1, totLen1 * (mutProb / 2));
                            WTS(i2, totLen1 * (errorProb + mutProb / 2));
                            CS(mutProb);
                            NEG(mutProb);
                            WT(i1, totLen1 * (errorProb + mutProb / 2));
                            WT(i2, (totLen1 * mutProb / 2));
                            CNT(i1, i2, mutProb);
                            MUT(i1, i2, mutProb);
                            ERRREC(i1, i2, errorProb);
                            ERRC(errorProb);
                            ECS(errorProb);
                        } else {                                         // across the root, M:10722-10747
                            double mutprob1 = rf[i1] * q(i1, i2) * totLen1;
                            double mutprob2 = rf[i2] * q(i2, i1) * e1.d0;
                            double errorProb = rf[i1] * errorRate * 0.33333;
                            const double normalization = mutprob1 + mutprob2 + errorProb;
                            mutprob1 = mutprob1 / normalization;
                            mutprob2 = mutprob2 / normalization;
                            errorProb = errorProb / normalization;
                            WT(i1, totLen1 * (mutprob1 / 2 + errorProb));
                            WT(i2, totLen1 * (mutprob2 + mutprob1 / 2));
                            CNT(i1, i2, mutprob1);
                            MUT(i1, i2, mutprob1);
                            ERRREC(i1, i2, errorProb);
                            ERRC(errorProb);
                            ECS(errorProb);
                            WTS(refN, -totLen1);
                            WTS(i1, (totLen1) * (mutprob1 / 2 + errorProb));
                            WTS(i2, (totLen1) * (mutprob2 + mutprob1 / 2));
                            CS(mutprob1);
                            NEG(mutprob1);
                        }
                    } else if (totLen2 == 0.0) {                         // M:10749-10788
                        if (!e1.hasD1) {
                            WTS(refN, -totLen1);
                            WTS(i1, totLen1 / 2);
                            WTS(i2, totLen1 / 2);
                            CS(1.0);
                            WT(i1, (totLen1 / 2));
                            WT(i2, (totLen1 / 2));
                            CNT(i1, i2, 1.0);
                            MUT_SURE(i1, i2);
                        } else {                                         // across the root
                            double noMutProb1 = 1.0 + q(i1, i1) * e1.d0;
                            if (noMutProb1 < 0) noMutProb1 = 0.25;
                            double noMutProb2 = 1.0 + q(i2, i2) * totLen1;
                            if (noMutProb2 < 0) noMutProb2 = 0.25;
                            double prob1 = rf[i1] * q(i1, i2) * totLen1 * noMutProb1;
                            double prob2 = rf[i2] * q(i2, i1) * e1.d0 * noMutProb2;
                            const double normalization = prob1 + prob2;
                            prob1 = prob1 / normalization;
                            prob2 = prob2 / normalization;
                            WT(i1, (totLen1 / 2) * prob1);
                            WT(i2, (totLen1 / 2) * prob1);
                            CNT(i1, i2, prob1);
                            MUT(i1, i2, prob1);
                            WT(i2, totLen1 * prob2);
                            WTS(refN, -totLen1);
                            WTS(i1, (totLen1 / 2) * prob1);
                            WTS(i2, (totLen1 / 2) * prob1);
                            WTS(i2, totLen1 * prob2);
                            CS(prob1);
                            NEG(prob1);
                        }
                    }
                }
            }
            pos += 1;
        }
    }
}
