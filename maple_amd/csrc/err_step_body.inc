// maple_amd/csrc/err_step_body.inc -- one step of the error-report walk over a (parent upper list, leaf lower list) pair: the body
// of the reference's inner loop (calculateErrorProbabilities, M:9820-9988), arm for arm and in its association order.
// Included by k_err_walk (error_probs.hip) inside the loop over the two cursors; in scope:
//   e1 / e2 (Ent of the parent / leaf side), pos (positions consumed so far = the 0-based site), dist, c (Ctx), rf,
//   minErrorProb and two macros:
//   REC(allele, x)   the reference's file.write(str(pos+1) + "\t" + allele + "\t" + str(x)): allele 0-3 = allelesList, 4 = "X"
//   DEN(x)           a denominator: x == 0.0 is the reference's ZeroDivisionError -- the walk notes the site and ends
//                    (a `break` of the walk's loop: DEN stands outside every inner loop)
// The reference's tuple-length tests read the entry's flags: len(entry1) == 3 + usingErrorRate is hasD0 && !hasD1,
// == 4 + usingErrorRate is hasD1, < 4 + usingErrorRate is !hasD1, len(entry1) > 3 of an O entry is hasD0.
// mutMatrices[pos] and errorRates[pos] are read with the 0-based pos, before pos += 1 (c.rate(pos), c.err(pos)).
{
    if (e2.type == 5) {                                                  // M:9821-9825
        if (e1.type == 4 || e1.type == 5) pos = min(e1.pos, e2.pos);
        else pos += 1;
    } else if (e1.type == 5) {                                           // M:9826-9830
        if (e2.type == 4) pos = min(e1.pos, e2.pos);
        else pos += 1;
    } else {
        double totLen1 = dist;                                           // M:9832-9840
        if (e1.type < 5) {
            if (e1.hasD0 && !e1.hasD1) totLen1 += e1.d0;
            else if (e1.hasD1) totLen1 += e1.d1;
        } else {
            if (e1.hasD0) totLen1 += e1.d0;
        }
        if (e1.type == 4 && e2.type == 4) {                              // M:9843-9844
            pos = min(e1.pos, e2.pos);
        } else {
            const double r = c.rate(pos);
            auto q = [&](int i, int j) { return c.q(r, i, j); };         // mutMatrix[i][j] (mutMatrices[pos] under rate variation)
            const double *v1 = e1.vec, *v2 = e2.vec;
            if (e1.type == 4) {                                          // the parent shows the reference
                if (e2.type == 6) {                                      // M:9846-9874
                    const int i1 = e2.ref;
                    if (v2[i1] < 0.1) {
                        const double errorRate = c.err(pos);
                        int numAltNucs = 0;
                        for (int i = 0; i < 4; i++) if (v2[i] > 0.1) numAltNucs++;
                        double errProb, mutProb;
                        if (e1.hasD1) {                                  // across the root, M:9856-9864
                            errProb = rf[i1] * (1.0 + q(i1, i1) * (totLen1 + e1.d0)) * errorRate * 0.33333 * numAltNucs;
                            mutProb = 0.0;
                            const double i1rootProb = rf[i1] * (1.0 + q(i1, i1) * e1.d0);
                            for (int i = 0; i < 4; i++)
                                if (v2[i] > 0.1) {
                                    mutProb += i1rootProb * q(i1, i) * totLen1;
                                    mutProb += rf[i] * (1.0 + q(i, i) * totLen1) * q(i, i1) * e1.d0;
                                }
                        } else {                                         // M:9865-9871
                            errProb = (1.0 + q(i1, i1) * totLen1) * errorRate * 0.33333 * numAltNucs;
                            mutProb = 0.0;
                            for (int i = 0; i < 4; i++) if (v2[i] > 0.1) mutProb += q(i1, i) * totLen1;
                        }
                        DEN(errProb + mutProb);
                        errProb = errProb / (errProb + mutProb);
                        if (errProb >= minErrorProb) REC(4, errProb);
                    }
                } else {                                                 // a single other nucleotide, M:9876-9894
                    const int i1 = e2.ref, i2 = e2.type;
                    const double errorRate = c.err(pos);
                    double errorProb;
                    if (!e1.hasD1) {
                        errorProb = errorRate * 0.33333;
                        const double mutProb = q(i1, i2) * totLen1;
                        DEN(errorProb + mutProb);
                        errorProb = errorProb / (errorProb + mutProb);
                    } else {                                             // across the root
                        const double mutprob1 = rf[i1] * q(i1, i2) * totLen1;
                        const double mutprob2 = rf[i2] * q(i2, i1) * e1.d0;
                        errorProb = rf[i1] * errorRate * 0.33333;
                        const double normalization = mutprob1 + mutprob2 + errorProb;
                        DEN(normalization);
                        errorProb = errorProb / normalization;
                    }
                    if (errorProb >= minErrorProb) REC(i2, errorProb);
                }
            } else if (e1.type == 6) {                                   // the parent shows an O vector, M:9897-9933
                double normalization = 0.0;
                if (e2.type == 6) {                                      // M:9901-9916
                    const double errorRate = c.err(pos);
                    double noMutProb = 0.0, mutProb = 0.0, errorProb = 0.0;
                    for (int j = 0; j < 4; j++)
                        if (v2[j] > 0.1) {
                            noMutProb += v1[j];
                            errorProb += (1.0 - v1[j]) * errorRate * 0.33333;
                            for (int i = 0; i < 4; i++) if (j != i) mutProb += v1[i] * q(i, j) * totLen1;
                        }
                    normalization = errorProb + noMutProb + mutProb;
                    DEN(normalization);
                    errorProb = errorProb / normalization;
                    if (errorProb >= minErrorProb) REC(4, errorProb);
                } else {                                                 // M:9917-9932
                    const int i2 = (e2.type == 4) ? e1.ref : e2.type;
                    const double errorRate = c.err(pos);
                    double errorProb = (1.0 - v1[i2]) * errorRate * 0.33333;
                    const double noMutProb = v1[i2];
                    double mutProb = 0.0;
                    for (int i = 0; i < 4; i++) if (i != i2) mutProb += v1[i] * q(i, i2) * totLen1;
                    normalization = errorProb + noMutProb + mutProb;
                    DEN(normalization);
                    errorProb = errorProb / normalization;
                    if (errorProb >= minErrorProb) REC(i2, errorProb);
                }
            } else {                                                     // the parent shows another nucleotide, M:9935-9986
                const int i1 = e1.type;
                if (e2.type != i1) {
                    if (e2.type == 6) {                                  // M:9940-9966
                        if (v2[i1] < 0.1) {                              // (where the parent's nucleotide is possible nothing is reported)
                            const double errorRate = c.err(pos);
                            int numAltNucs = 0;
                            for (int i = 0; i < 4; i++) if (v2[i] > 0.1) numAltNucs++;
                            double errProb, mutProb;
                            if (e1.hasD1) {                              // across the root, M:9948-9956
                                errProb = rf[i1] * (1.0 + q(i1, i1) * (totLen1 + e1.d0)) * errorRate * 0.33333 * numAltNucs;
                                mutProb = 0.0;
                                const double i1rootProb = rf[i1] * (1.0 + q(i1, i1) * e1.d0);
                                for (int i = 0; i < 4; i++)
                                    if (v2[i] > 0.1) {
                                        mutProb += i1rootProb * q(i1, i) * totLen1;
                                        mutProb += rf[i] * (1.0 + q(i, i) * totLen1) * q(i, i1) * e1.d0;
                                    }
                            } else {                                     // M:9958-9964
                                errProb = (1.0 + q(i1, i1) * totLen1) * errorRate * 0.33333 * numAltNucs;
                                mutProb = 0.0;
                                for (int i = 0; i < 4; i++) if (v2[i] > 0.1) mutProb += q(i1, i) * totLen1;
                            }
                            DEN(errProb + mutProb);
                            errProb = errProb / (errProb + mutProb);
                            if (errProb >= minErrorProb) REC(4, errProb);
                        }
                    } else {                                             // two different nucleotides, M:9969-9986
                        const int i2 = (e2.type == 4) ? e1.ref : e2.type;
                        const double errorRate = c.err(pos);
                        double errorProb;
                        if (!e1.hasD1) {
                            errorProb = errorRate * 0.33333;
                            const double mutProb = q(i1, i2) * totLen1;
                            DEN(errorProb + mutProb);
                            errorProb = errorProb / (errorProb + mutProb);
                        } else {                                         // across the root
                            const double mutprob1 = rf[i1] * q(i1, i2) * totLen1;
                            const double mutprob2 = rf[i2] * q(i2, i1) * e1.d0;
                            errorProb = rf[i1] * errorRate * 0.33333;
                            const double normalization = mutprob1 + mutprob2 + errorProb;
                            DEN(normalization);
                            errorProb = errorProb / normalization;
                        }
                        if (errorProb >= minErrorProb) REC(i2, errorProb);
                    }
                }
            }
            pos += 1;
        }
    }
}
