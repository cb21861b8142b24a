// maple_amd/csrc/frontier_upd_lane.h -- one list-updating item of the frontier tier by ONE lane (included by the translation
// units that hold a k_fr_updating* kernel: a device function cannot be called across translation units)
#pragma once
#include "frontier_dev.h"

namespace frt {

// ---- items that arrived with needsUpdating == True (M:6982-7091, 7182-7304): lists merged along the path ----------------
// (dir 3: the seeding of a search whose pruned node hangs off the root, M:6916-6960 -- two rootVector calls)
// one such item by one lane (the one-lane list walks of genome_dev.h)
// MAT: the tree has MAT local references -- every list that leaves a frame goes through the branch between the frames
// (passGenomeListThroughBranch; a template switch: the plain tree's kernel carries none of it)
template <bool RV, bool U, bool SS, bool MAT>
__device__ __forceinline__ void fr_upd_item_lane(const Ctx<RV, U, SS> &c, const ArenaViewS &av, const DevTree &T, const SearchParams &P, const FPools &fp,
                                 const int budget, const long long laneId, const long long i, unsigned long long *algBytes = nullptr)
{
        FItem &it = fp.U[i];
        FSearch &S = fp.S[it.q];
        if (!fs_live(S.state)) { it.flags |= FI_DEAD; return; }
        const int q = it.q, t1 = it.t1;
        const NodeRec r1 = T.nd[t1];
        const int hPassed = it.hPassed, hRpr = it.hRpr;
        const double distance = it.distance, lastLK = it.lastLK;
        const bool rt = S.isRemovedTip != 0;
        const double rbl = S.removedBLen;
        bool upd = true;
        double midProb = lastLK;
        Writer wr;
        FScr scr{nullptr, nullptr};
        // merge two lists into scratch (wr / scr); 0 ok, -1 None, -2 fatal / no room (then the search is handed back)
        auto merge = [&](int h1, double b1, bool tp1, int h2, double b2, bool tp2, bool upDown) -> int {
            if (!fvalid(h1) || !fvalid(h2)) return -2;
            const FList l1 = flist(av, fp, h1), l2 = flist(av, fp, h2);
            if (!fscratch(fp, laneId, l1.n + l2.n, scr)) { S.state = FS_FALLBACK; return -2; }
            wr.init(scr.w, scr.a);
            const int r = merge_walk(c, fref(l1), b1, tp1, fref(l2), b2, tp2, upDown, false, 0, 0, wr, nullptr);
            // (the item's algorithmic bytes: the two lists a mergeVectors reads and the one it writes; the lists of the item's
            // areVectorsDifferent and appendProbNode are among them or of the same size)
            if (algBytes) *algBytes += 8ull * (unsigned long long)(l1.n + l1.na + l2.n + l2.na + (r > 0 ? wr.n + wr.na : 0));
            return r == -1 ? -1 : (r < 0 ? -2 : 0);
        };
        // rootVector(list, bLen, isFromTip) without local references (M:4916-4996): the walk, then shorten; a stored handle,
        // -2 when out of room
        auto rootVector = [&](int h, double bLen, bool fromTip) -> int {
            if (!fvalid(h)) return -2;
            const FList l = flist(av, fp, h);
            if (!fscratch(fp, laneId, l.n, scr)) return -2;
            wr.init(scr.w, scr.a);
            root_walk(c, fref(l), bLen, fromTip, wr);
            const int hr = fstore(fp, wr);
            if (hr < 0) return -2;
            const FList lr = flist(av, fp, hr);
            wr.init(scr.w, scr.a);
            shorten_walk(c, fref(lr), lr.n, wr);
            if (wr.n == lr.n) return hr;                                   // nothing merged: the list as it is
            return fstore(fp, wr);
        };
        // a stored list through the branch above a node (-2: no room); the removed list likewise
        auto passL = [&](int h, int mutId, bool up) -> int { return MAT ? fpass_store(fp, av, c.m.lRef, laneId, h, mutId, up) : h; };
        auto passR = [&](int h, int mutId, bool up) -> int { return MAT ? fpass_removed(c, fp, av, laneId, h, mutId, up) : h; };
        if (it.dir == 3) {                                                  // the pruned node's parent is the root; t1 = its sibling
            it.midProb = lastLK;
            it.flags |= FI_UPD_OUT;
            if (r1.c0 >= 0) {
                const int ch1 = r1.c0, ch2 = r1.c1;
                const NodeRec rc1 = T.nd[ch1], rc2 = T.nd[ch2];
                int v1 = rootVector(passL(ftree(rc2.lower), rc2.mutId, true), rc2.dist, rc2.isTip != 0);
                int v2 = v1 < 0 ? -2 : rootVector(passL(ftree(rc1.lower), rc1.mutId, true), rc1.dist, rc1.isTip != 0);
                int rp1 = hRpr, rp2 = hRpr;
                if (MAT && v1 >= 0 && v2 >= 0) {                             // M:6926-6948
                    if (rc1.mutId >= 0) { rp1 = passR(hRpr, rc1.mutId, false); v1 = passL(v1, rc1.mutId, false); }
                    if (rc2.mutId >= 0) { rp2 = passR(hRpr, rc2.mutId, false); v2 = passL(v2, rc2.mutId, false); }
                }
                if (v1 < 0 || v2 < 0 || !fvalid(rp1) || !fvalid(rp2)) { S.state = FS_FALLBACK; return; }
                it.child0 = fpush(fp, budget, q, true, ch1, 0, v1, rc1.dist, lastLK, 0, rp1, it.pathBest);
                it.child1 = fpush(fp, budget, q, true, ch2, 0, v2, rc2.dist, lastLK, 0, rp2, it.pathBest);
            }
            return;
        }
        if (it.dir == 0) {                                                  // moving from a parent to its child, M:6982-7160
            const int upT = r1.up;
            const bool scored = !(upT == S.parent || upT < 0) && (r1.dist > P.effNon0 || r1.upIsRoot);
            if (scored) {
                if (merge(hPassed, distance / 2, false, ftree(r1.lower), distance / 2, r1.isTip != 0, true) != 0) { it.flags |= FI_DEAD; return; }
                const ListRef mid{scr.w, scr.a};
                if (r1.totUp >= 0) { const FList tu = flist(av, fp, ftree(r1.totUp)); if (!differ_walk(c, mid, fref(tu))) upd = false; }
                const FList lr = flist(av, fp, hRpr);
                midProb = append_walk(c, mid, fref(lr), rt, rbl);
                it.flags |= FI_SCORED;
                if (upd && midProb >= it.pathBest - P.thrOptTopo) {          // may be short-listed (M:7071): keep the record's lists
                    const int hm = fstore(fp, wr);
                    if (hm < 0) { S.state = FS_FALLBACK; it.flags |= FI_DEAD; return; }
                    it.hA = hPassed; it.hB = ftree(r1.lower); it.hMid = hm; it.recDist = distance; it.flags |= FI_REC_UPD;
                }
            }
            it.midProb = midProb;
            if (upd) it.flags |= FI_UPD_OUT;
            const PRule pr = p_rule(P, scored, midProb, lastLK, it.failsP, it.pathBest);
            if (pr.go && r1.c0 >= 0) {
                for (int k = 0; k < 2; k++) {                               // child 0 uses vectUpRight, child 1 vectUpLeft
                    const int ch = k == 0 ? r1.c0 : r1.c1, other = k == 0 ? r1.c1 : r1.c0;
                    int ref = FR_NONE;
                    const bool cross = MAT && (k == 0 ? r1.c0Frame : r1.c1Frame) != r1.frameOf;
                    if (upd) {
                        const NodeRec ro = T.nd[other];
                        const int hOther = passL(ftree(ro.lower), ro.mutId, true);   // (the other child's list in t1's frame, M:7107-7109)
                        const int r = hOther == -2 ? -2 : merge(hPassed, distance, false, hOther, ro.dist, ro.isTip != 0, true);
                        if (r == -2) { S.state = FS_FALLBACK; break; }
                        if (r == 0) {
                            int hv = fstore(fp, wr), hr = hRpr;
                            if (hv >= 0 && cross) {                         // into the child's frame, M:7111-7121
                                const int mId = T.nd[ch].mutId;
                                hv = passL(hv, mId, false); hr = passR(hRpr, mId, false);
                            }
                            if (hv < 0 || !fvalid(hr)) { S.state = FS_FALLBACK; break; }
                            ref = fpush(fp, budget, q, true, ch, 0, hv, T.nd[ch].dist, midProb, pr.fails, hr, pr.pathBest);
                        }
                    } else if ((k == 0 ? r1.upRight : r1.upLeft) >= 0)
                        ref = fpush(fp, budget, q, false, ch, 0, -1, 0.0, midProb, pr.fails, hRpr, pr.pathBest, cross);
                    if (k == 0) it.child0 = ref; else it.child1 = ref;
                }
            }
        } else {                                                             // crawling up from a child to its parent t1, M:7162-7434
            const int other = (it.dir == 1) ? r1.c1 : r1.c0;
            const int upT = r1.up;
            const NodeRec ro = T.nd[other];
            int hBottom = -1;
            // (the parent's upper list and the other child's lower list in t1's frame, M:7186 / 7196)
            const int vectUp = upT >= 0 ? passL(ftree(r1.whichChild ? T.nd[upT].upLeft : T.nd[upT].upRight), r1.mutId, false) : -1;
            const int hOther = passL(ftree(ro.lower), ro.mutId, true);
            if (MAT && (vectUp == -2 || hOther == -2)) { S.state = FS_FALLBACK; return; }
            const bool crossO = MAT && ((it.dir == 1) ? r1.c1Frame : r1.c0Frame) != r1.frameOf, crossU = MAT && r1.upFrame != r1.frameOf;
            const bool scored = upT >= 0 && (r1.dist > P.effNon0 || r1.upIsRoot);
            if (scored) {
                int r = merge(hPassed, distance, false, hOther, ro.dist, ro.isTip != 0, false);
                if (r != 0) { it.flags |= FI_DEAD; return; }
                hBottom = fstore(fp, wr);
                if (hBottom < 0) { S.state = FS_FALLBACK; it.flags |= FI_DEAD; return; }
                r = merge(vectUp, r1.dist / 2, false, hBottom, r1.dist / 2, false, true);
                if (r != 0) { it.flags |= FI_DEAD; return; }
                int hm = -1;
                if (r1.totUp >= 0) {
                    const ListRef mid{scr.w, scr.a};
                    const FList tu = flist(av, fp, ftree(r1.totUp));
                    if (!differ_walk(c, mid, fref(tu))) upd = false;
                } else {
                    // "Node has no probVectTotUp ... calculating new one", M:7198-7200: midTot is compared with a list merged on
                    // the spot (midTot moves to the arena first: the scratch is needed for that merge)
                    hm = fstore(fp, wr);
                    if (hm < 0) { S.state = FS_FALLBACK; it.flags |= FI_DEAD; return; }
                    const int rc = merge(vectUp, r1.dist / 2, false, ftree(r1.lower), r1.dist / 2, false, true);
                    if (rc == 0) { const FList lm = flist(av, fp, hm); if (!differ_walk(c, fref(lm), ListRef{scr.w, scr.a})) upd = false; }
                    else if (S.state == FS_FALLBACK) { it.flags |= FI_DEAD; return; }
                }
                const FList lr = flist(av, fp, hRpr);
                if (hm >= 0) { const FList lm = flist(av, fp, hm); midProb = append_walk(c, fref(lm), fref(lr), rt, rbl); }
                else midProb = append_walk(c, ListRef{scr.w, scr.a}, fref(lr), rt, rbl);
                it.flags |= FI_SCORED;
                if (upd && midProb >= it.pathBest - P.thrOptTopo) {          // M:7293
                    if (hm < 0) hm = fstore(fp, wr);
                    if (hm < 0) { S.state = FS_FALLBACK; it.flags |= FI_DEAD; return; }
                    it.hA = vectUp; it.hB = hBottom; it.hMid = hm; it.recDist = r1.dist; it.flags |= FI_REC_UPD;
                }
            }
            it.midProb = midProb;
            if (upd) it.flags |= FI_UPD_OUT;
            const PRule pr = p_rule(P, scored, midProb, lastLK, it.failsP, it.pathBest);
            if (!pr.go) return;
            if (upT >= 0) {
                int hUp = -1;
                int hrO = hRpr, hrU = hRpr;
                if (upd) {
                    const int r = merge(vectUp, r1.dist, false, hPassed, distance, false, true);
                    if (r == -2) { S.state = FS_FALLBACK; return; }
                    if (r == 0) { hUp = fstore(fp, wr); if (hUp < 0) { S.state = FS_FALLBACK; return; } }
                    if (crossO && hUp >= 0) {                                // into the other child's frame, M:7342-7352
                        hUp = passL(hUp, ro.mutId, false); hrO = passR(hRpr, ro.mutId, false);
                        if (hUp == -2 || !fvalid(hrO)) { S.state = FS_FALLBACK; return; }
                    }
                } else hUp = ftree(it.dir == 1 ? r1.upLeft : r1.upRight);
                if (!fvalid(hUp)) return;
                it.child0 = upd ? fpush(fp, budget, q, true, other, 0, hUp, ro.dist, midProb, pr.fails, hrO, pr.pathBest)
                                : fpush(fp, budget, q, false, other, 0, -1, 0.0, midProb, pr.fails, hRpr, pr.pathBest, crossO);
                if (upd && hBottom < 0) {                                    // M:7376-7384
                    const int r = merge(hPassed, distance, false, hOther, ro.dist, ro.isTip != 0, false);
                    if (r != 0) return;
                    hBottom = fstore(fp, wr);
                    if (hBottom < 0) { S.state = FS_FALLBACK; return; }
                }
                if (upd && crossU) {                                         // out of t1's frame, M:7388-7395
                    hBottom = passL(hBottom, r1.mutId, true); hrU = passR(hRpr, r1.mutId, true);
                    if (hBottom == -2 || !fvalid(hrU)) { S.state = FS_FALLBACK; return; }
                }
                it.child1 = upd ? fpush(fp, budget, q, true, upT, (int)r1.whichChild + 1, hBottom, r1.dist, midProb, pr.fails, hrU, pr.pathBest)
                                : fpush(fp, budget, q, false, upT, (int)r1.whichChild + 1, -1, 0.0, midProb, pr.fails, hRpr, pr.pathBest, crossU);
            } else {                                                         // t1 is the root, M:7406-7432
                if (upd) {
                    int hv = rootVector(hPassed, distance, false), hrO = hRpr;
                    if (hv >= 0 && crossO) { hv = passL(hv, ro.mutId, false); hrO = passR(hRpr, ro.mutId, false); }
                    if (hv < 0 || !fvalid(hrO)) { S.state = FS_FALLBACK; return; }
                    it.child0 = fpush(fp, budget, q, true, other, 0, hv, ro.dist, midProb, pr.fails, hrO, pr.pathBest);
                } else
                    it.child0 = fpush(fp, budget, q, false, other, 0, -1, 0.0, midProb, pr.fails, hRpr, pr.pathBest, crossO);
            }
        }
}

// (a real call: k_fr_updating_wave falls back to it from three places and is bound by its LDS, not its registers)
template <bool RV, bool U, bool SS, bool MAT>
__device__ __noinline__ void fr_upd_item_lane_call2(const Ctx<RV, U, SS> &c, const ArenaViewS &av, const DevTree &T, const SearchParams &P,
                                                    const FPools &fp, const int budget, const long long laneId, const long long i,
                                                    unsigned long long *algBytes)
{
    fr_upd_item_lane<RV, U, SS, MAT>(c, av, T, P, fp, budget, laneId, i, algBytes);
}
template <bool RV, bool U, bool SS>
__device__ __forceinline__ void fr_upd_item_lane_call(const Ctx<RV, U, SS> &c, const ArenaViewS &av, const DevTree &T, const SearchParams &P,
                                                      const FPools &fp, const int budget, const long long laneId, const long long i,
                                                      unsigned long long *algBytes = nullptr)
{
    if (fp.mat) fr_upd_item_lane_call2<RV, U, SS, true>(c, av, T, P, fp, budget, laneId, i, algBytes);
    else fr_upd_item_lane_call2<RV, U, SS, false>(c, av, T, P, fp, budget, laneId, i, algBytes);
}

}  // namespace frt
