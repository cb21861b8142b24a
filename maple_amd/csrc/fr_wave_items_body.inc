// maple_amd/csrc/fr_wave_items_body.inc -- the body of k_fr_updating_wave_s / k_fr_updating_wave: the level's items of one size
// class, dealt to the wavefronts.  Included as the whole body of a kernel
//     template <bool RV, bool U, bool SS> __global__ __launch_bounds__(64) void k(const DevModel *__restrict__ mp, ArenaViewS av,
//         DevTree T, SearchParams P, FPools fp, int budget, int heavyMin, long long laneBase)
// after `using Class = frt::WaveSmall` or `frt::WaveBig` (as merge_step_body.inc is the body of the walks' steps).  Not a function:
// a body that is optimised on its own before it is inlined into its kernel compiles to other code -- the inliner then sees the
// lambdas' captures resolved and takes other decisions (wave_append's append_walk fallback inlined twice, 11 % more code).
    __shared__ Lds lds;
    __shared__ WaveUpdLds<Class::wuIn> L;
    typedef WaveLds<Class::capW> WaveLdsC;
    const DevModel &m = *mp;
    stage_model(m, lds);
    Ctx<RV, U, SS> c(m, lds);
    const int lane = threadIdx.x;
    WaveLdsC &W = *reinterpret_cast<WaveLdsC *>(L.baux);                   // (appendProbNode's staging: baux is free by then)
    static_assert(sizeof(WaveLdsC) <= sizeof(L.baux), "LDS alias");
    const long long lo = (long long)fp.ctr->loU;
    // the level's items that go a wavefront each, listed by k_fr_sort_level (Class::perm, in any order): dealt to the wavefronts one at
    // a time
    const long long nHeavy = (long long)(fp.ctr->*Class::count);
    (void)heavyMin;
    // (what the launch did, for the roofline of the bench line -- the same account as k_fr_updating's: the two lists every
    // mergeVectors reads and the one it writes; kept by lane 0, one atomic per wavefront at the end)
    unsigned long long nU = 0, bU = 0;
    for (;;) {
        // (by ticket, not by stride: a wavefront on a slow item -- long lists next to the root -- holds nothing back but that item.
        // Lane 0 takes the ticket, one atomic per item; nobody waits for anybody.  k_fr_snap_u resets the counter with the list.)
        unsigned long long tk = 0;
        if (lane == 0) tk = atomicAdd(&fp.ctr->ticket[Class::profCls], 1ull);
        const long long kk = (long long)(((unsigned long long)(uint32_t)__shfl((int)(tk >> 32), 0, 64) << 32) | (uint32_t)__shfl((int)tk, 0, 64));
        if (kk >= nHeavy) break;
        nU++;
#ifdef MAPLE_SPR_PROFILE
        const long long tItem0 = wall_clock64();
        int profCls = Class::profCls;
        struct ProfEnd {                                                    // (booked on every way out of the item's block)
            const FPools &fp; const long long t0; int &cls; const int level;
            __device__ ~ProfEnd() {
                if ((threadIdx.x & 63) == 0) {
                    const unsigned long long dt = (unsigned long long)(wall_clock64() - t0);
                    atomicAdd(&fp.ctr->dbgWCnt[cls], 1ull); atomicAdd(&fp.ctr->dbgWT[cls], dt); atomicMax(&fp.ctr->dbgWMax[cls], dt);
                    atomicMax(&fp.ctr->dbgLvlW[level], (dt << 4) | (unsigned long long)cls);
                }
            }
        } profEnd{fp, tItem0, profCls, min(max(fp.ctr->nLevels - 1, 0), FR_PROF_LEVELS - 1)};
#endif
        {
            const long long i = lo + (fp.*Class::perm)[kk];
            FItem &it = fp.U[i];
            FSearch &S = fp.S[it.q];
            if (!fs_live(S.state)) { if (lane == 0) it.flags |= FI_DEAD; continue; }
            const int q = it.q, t1 = it.t1, dir = it.dir;
            const NodeRec r1 = T.nd[t1];
            const int hPassed = it.hPassed, hRpr = it.hRpr;
            const double distance = it.distance, lastLK = it.lastLK;
            const bool rt = S.isRemovedTip != 0;
            const double rbl = S.removedBLen;
            const int other = dir == 0 ? -1 : (dir == 1 ? r1.c1 : r1.c0);
            const int upT = r1.up;
            // every list the item touches must fit the staging areas; else lane 0 walks the item alone
            const FList lp = fvalid(hPassed) ? flist(av, fp, hPassed) : FList{nullptr, nullptr, 0, 0};
            const FList lr = flist(av, fp, hRpr);
            const bool fits = fr_wave_fits(av, T, fp, it, Class::wuIn, Class::capW);
            if (!fits) {
#ifdef MAPLE_SPR_PROFILE
                profCls += 2;
#endif
                if (lane == 0) { atomicAdd(&fp.ctr->wavePath[FR_WP_LANE0_FIT], 1ull); fr_upd_item_lane_call(c, av, T, P, fp, budget, laneBase + blockIdx.x, i, &bU); }
                wave_sync();
                continue;
            }
            bool upd = true;
            double midProb = lastLK;
            int flagsAdd = 0;
            int nM = 0, naM = 0;
            // mergeVectors into L.m / L.maux: 0 ok, -1 None, -2 fatal
            auto merge = [&](const FList &l1, double b1, bool tp1, const FList &l2, double b2, bool tp2, bool upDown) -> int {
                if (l1.n > L.wuIn || l2.n > L.wuIn) return -2;               // (a list that grew beyond the staging on its way through a reference branch)
                wave_sync();
                const int r = wave_merge(c, fref(l1), l1.n, b1, tp1, fref(l2), l2.n, b2, tp2, upDown, L, naM);
                bU += 8ull * (unsigned long long)(l1.n + l1.na + l2.n + l2.na + (r > 0 ? r + naM : 0));
                if (r < 0) return r == -1 ? -1 : -2;
                nM = r;
                return 0;
            };
            auto differs = [&](int listId) -> bool {                        // areVectorsDifferent(L.m, tree list)
                const FList tu = flist(av, fp, ftree(listId));
                const unsigned long long *tw = (const unsigned long long *)tu.w;
                for (int k = lane; k < tu.n; k += 64) L.old[k] = tw[k];
                wave_sync();
                return wave_differ(c, L.m, L.maux, nM, L.old, tu.aux, tu.n);
            };
            auto score = [&]() -> double {                                  // appendProbNode(L.m, removed list)
                wave_sync();
                return wave_append(c, ListRef{(const uint2 *)L.m, L.maux}, nM, fref(lr), lr.n, rt, rbl, W);
            };
            auto push1 = [&](bool u, int node, int d, int h, double dst, double mp, int fails, double pb, int hr, bool needPass) -> int {
                int ref = FR_NONE;
                if (lane == 0) ref = fpush(fp, budget, q, u, node, d, h, dst, mp, fails, hr, pb, needPass);
                return __shfl(ref, 0, 64);
            };
            // trees with MAT local references: a stored list through the branch above a node (passGenomeListThroughBranch,
            // M:3749-3877), the removed list likewise -- what fr_upd_item_lane does for an item next to a reference branch, in
            // the same places.  Every lane gets the handle (-2: no room).
            const bool matAdj = fp.mat && (r1.c0Frame != r1.frameOf || r1.c1Frame != r1.frameOf || r1.upFrame != r1.frameOf);
            auto passW = [&](int h, int mutId, bool up, bool removed) -> int {
                if (!matAdj) return h;
                return wave_pass(c, fp, av, h, mutId, up, removed);          // (the whole wavefront: frontier_dev.h)
            };
            bool dead = false, fallback = false;
            int child0 = FR_NONE, child1 = FR_NONE, hA = -1, hB = -1, hMid = -1;
            double recDist = 0.0;
            if (dir == 0) {
                const bool scored = !(upT == S.parent || upT < 0) && (r1.dist > P.effNon0 || r1.upIsRoot);
                if (scored) {
                    const FList ll = flist(av, fp, ftree(r1.lower));
                    if (merge(lp, distance / 2, false, ll, distance / 2, r1.isTip != 0, true) != 0) dead = true;
                    else {
                        if (r1.totUp >= 0 && !differs(r1.totUp)) upd = false;
                        midProb = score();
                        flagsAdd |= FI_SCORED;
                        if (upd && midProb >= it.pathBest - P.thrOptTopo) {
                            wave_sync();
                            hMid = fstore_wave(fp, L.m, L.maux, nM, naM);
                            if (hMid < 0) { fallback = true; dead = true; }
                            else { hA = hPassed; hB = ftree(r1.lower); recDist = distance; flagsAdd |= FI_REC_UPD; }
                        }
                    }
                }
                if (!dead) {
                    const PRule pr = p_rule(P, scored, midProb, lastLK, it.failsP, it.pathBest);
                    if (pr.go && r1.c0 >= 0) {
                        for (int k = 0; k < 2 && !fallback; k++) {
                            const int ch = k == 0 ? r1.c0 : r1.c1, oth = k == 0 ? r1.c1 : r1.c0;
                            int ref = FR_NONE;
                            const bool cross = matAdj && (k == 0 ? r1.c0Frame : r1.c1Frame) != r1.frameOf;
                            if (upd) {
                                const NodeRec ro = T.nd[oth];
                                const int hOther = passW(ftree(ro.lower), ro.mutId, true, false);   // (the other child's list in t1's frame, M:7107-7109)
                                const FList lo2 = fvalid(hOther) ? flist(av, fp, hOther) : FList{nullptr, nullptr, 0, 0};
                                const int r = fvalid(hOther) ? merge(lp, distance, false, lo2, ro.dist, ro.isTip != 0, true) : -2;
                                if (r == -2) { fallback = true; break; }
                                if (r == 0) {
                                    wave_sync();
                                    int hv = fstore_wave(fp, L.m, L.maux, nM, naM), hr = hRpr;
                                    if (hv >= 0 && cross) {                 // into the child's frame, M:7111-7121
                                        const int mId = T.nd[ch].mutId;
                                        hv = passW(hv, mId, false, false); hr = passW(hRpr, mId, false, true);
                                    }
                                    if (hv < 0 || !fvalid(hr)) { fallback = true; break; }
                                    ref = push1(true, ch, 0, hv, T.nd[ch].dist, midProb, pr.fails, pr.pathBest, hr, false);
                                }
                            } else if ((k == 0 ? r1.upRight : r1.upLeft) >= 0)
                                ref = push1(false, ch, 0, -1, 0.0, midProb, pr.fails, pr.pathBest, hRpr, cross);
                            if (k == 0) child0 = ref; else child1 = ref;
                        }
                    }
                }
            } else {
                const NodeRec ro = T.nd[other];
                // (the parent's upper list and the other child's lower list in t1's frame, M:7186 / 7196)
                const int vectUp = upT >= 0 ? passW(ftree(r1.whichChild ? T.nd[upT].upLeft : T.nd[upT].upRight), r1.mutId, false, false) : -1;
                const int hOther = passW(ftree(ro.lower), ro.mutId, true, false);
                const bool crossO = matAdj && ((dir == 1) ? r1.c1Frame : r1.c0Frame) != r1.frameOf, crossU = matAdj && r1.upFrame != r1.frameOf;
                const bool scored = upT >= 0 && (r1.dist > P.effNon0 || r1.upIsRoot);
                int hBottom = -1;
                if (vectUp == -2 || hOther == -2 || !fvalid(hOther)) {      // (no room for a re-expressed list: the search goes to the one-lane kernel)
                    if (lane == 0) { S.state = FS_FALLBACK; it.flags |= FI_DEAD; }
                    wave_sync();
                    continue;
                }
                const FList lo2 = flist(av, fp, hOther);
                const FList lvu = fvalid(vectUp) ? flist(av, fp, vectUp) : FList{nullptr, nullptr, 0, 0};
                if (scored) {
                    if (!fvalid(vectUp) || r1.totUp < 0) {
                        // The on-the-spot probVectTotUp of M:7198-7200 (and a parent without an upper list for this side): one lane.
                        // Left as it is: the headline tree has NO such item (FCtr::wavePath, profiles/late_levels_before.txt: 0 of a
                        // round's 72 000 wavefront-wide items) -- every branch next to its root is long enough to carry a
                        // probVectTotUp.  Small trees with a zero-length branch at the root do meet it.
#ifdef MAPLE_SPR_PROFILE
                        profCls += 4;
#endif
                        if (lane == 0) { atomicAdd(&fp.ctr->wavePath[FR_WP_LANE0_SPOT], 1ull); fr_upd_item_lane_call(c, av, T, P, fp, budget, laneBase + blockIdx.x, i, &bU); }
                        wave_sync();
                        continue;
                    }
                    int r = merge(lp, distance, false, lo2, ro.dist, ro.isTip != 0, false);
                    if (r == -2) { fallback = true; dead = true; }
                    else if (r != 0) dead = true;
                    else {
                        wave_sync();
                        hBottom = fstore_wave(fp, L.m, L.maux, nM, naM);
                        if (hBottom < 0) { fallback = true; dead = true; }
                        else {
                            const FList lb = flist(av, fp, hBottom);            // (written by this wavefront, fenced in fstore_wave)
                            r = merge(lvu, r1.dist / 2, false, lb, r1.dist / 2, false, true);
                            if (r == -2) { fallback = true; dead = true; }
                            else if (r != 0) dead = true;
                            else {
                                if (!differs(r1.totUp)) upd = false;
                                midProb = score();
                                flagsAdd |= FI_SCORED;
                                if (upd && midProb >= it.pathBest - P.thrOptTopo) {
                                    wave_sync();
                                    hMid = fstore_wave(fp, L.m, L.maux, nM, naM);
                                    if (hMid < 0) { fallback = true; dead = true; }
                                    else { hA = vectUp; hB = hBottom; recDist = r1.dist; flagsAdd |= FI_REC_UPD; }
                                }
                            }
                        }
                    }
                }
                if (!dead) {
                    const PRule pr = p_rule(P, scored, midProb, lastLK, it.failsP, it.pathBest);
                    if (pr.go) {
                        if (upT >= 0) {
                            int hUp = -1;
                            bool stop = false;
                            if (upd) {
                                const int r = fvalid(vectUp) ? merge(lvu, r1.dist, false, lp, distance, false, true) : -2;
                                if (r == -2) { fallback = true; stop = true; }
                                else if (r == 0) { wave_sync(); hUp = fstore_wave(fp, L.m, L.maux, nM, naM); if (hUp < 0) { fallback = true; stop = true; } }
                            } else hUp = ftree(dir == 1 ? r1.upLeft : r1.upRight);
                            int hrO = hRpr, hrU = hRpr;
                            if (upd && crossO && !stop && hUp >= 0) {       // into the other child's frame, M:7342-7352
                                hUp = passW(hUp, ro.mutId, false, false); hrO = passW(hRpr, ro.mutId, false, true);
                                if (hUp == -2 || !fvalid(hrO)) { fallback = true; stop = true; }
                            }
                            if (!stop && fvalid(hUp)) {
                                child0 = upd ? push1(true, other, 0, hUp, ro.dist, midProb, pr.fails, pr.pathBest, hrO, false)
                                             : push1(false, other, 0, -1, 0.0, midProb, pr.fails, pr.pathBest, hRpr, crossO);
                                if (upd && hBottom < 0) {                   // M:7376-7384
                                    const int r = merge(lp, distance, false, lo2, ro.dist, ro.isTip != 0, false);
                                    if (r == 0) { wave_sync(); hBottom = fstore_wave(fp, L.m, L.maux, nM, naM); if (hBottom < 0) fallback = true; }
                                    else { stop = true; if (r == -2) fallback = true; }
                                }
                                if (upd && crossU && !stop && !fallback) {  // out of t1's frame, M:7388-7395
                                    hBottom = passW(hBottom, r1.mutId, true, false); hrU = passW(hRpr, r1.mutId, true, true);
                                    if (hBottom == -2 || !fvalid(hrU)) fallback = true;
                                }
                                if (!stop && !fallback)
                                    child1 = upd ? push1(true, upT, (int)r1.whichChild + 1, hBottom, r1.dist, midProb, pr.fails, pr.pathBest, hrU, false)
                                                 : push1(false, upT, (int)r1.whichChild + 1, -1, 0.0, midProb, pr.fails, pr.pathBest, hRpr, crossU);
                            }
                        } else if (upd) {                                   // t1 is the root and the item still updates: rootVector, one lane
                            // (nothing was pushed or stored yet that the one-lane walk would not redo.  Left as it is for the same
                            // reason: the headline tree's rounds hold no such item among the wavefront-wide ones)
#ifdef MAPLE_SPR_PROFILE
                            profCls += 6;
#endif
                            if (lane == 0) { atomicAdd(&fp.ctr->wavePath[FR_WP_LANE0_ROOT], 1ull); fr_upd_item_lane_call(c, av, T, P, fp, budget, laneBase + blockIdx.x, i, &bU); }
                            wave_sync();
                            continue;
                        } else
                            child0 = push1(false, other, 0, -1, 0.0, midProb, pr.fails, pr.pathBest, hRpr, crossO);
                    }
                }
            }
            if (lane == 0) {
                if (fallback) S.state = FS_FALLBACK;
                it.midProb = midProb; it.recDist = recDist; it.child0 = child0; it.child1 = child1; it.hA = hA; it.hB = hB; it.hMid = hMid;
                it.flags |= (uint8_t)(flagsAdd | (upd ? FI_UPD_OUT : 0) | (dead ? FI_DEAD : 0));
            }
            wave_sync();
        }
    }
    if (lane == 0 && nU) { atomicAdd(&fp.ctr->itemsU, nU); atomicAdd(&fp.ctr->bytesU, bU); }
