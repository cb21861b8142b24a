// maple_amd/csrc/frontier_upd_wave.h -- what the two kernels that walk a list-updating item of the frontier tier by a whole
// WAVEFRONT share (k_fr_updating_wave_s in frontier_updw128.hip, k_fr_updating_wave in frontier_upd.hip: one size class of lists
// each, frt::WaveSmall / frt::WaveBig of frontier_dev.h).  The kernels' common text is fr_wave_items_body.inc.
#pragma once
#include "frontier_upd_lane.h"
#include "wave_dev.h"
#include "wave_update.h"

namespace frt {

// ---- the same items by a whole wavefront: the few whose lists are long -------------------------------------------------------
// mergeVectors, areVectorsDifferent and appendProbNode cut along the merge path of the two lists (wave_update.h, wave_dev.h:
// lane d does step d of the walk; bit for bit the one-lane walks), every list of the item in LDS.  An item with a list beyond
// the staging limit is walked by lane 0 alone.
__device__ inline int fstore_wave(const FPools &fp, const unsigned long long *w, const double *a, int n, int na)
{
    const int lane = threadIdx.x & 63;
    unsigned long long id = 0, ow = 0, oa = 0;
    if (lane == 0) {
        id = atomicAdd(&fp.ctr->nLists, 1ull);
        ow = atomicAdd(&fp.ctr->usedW, (unsigned long long)n);
        oa = atomicAdd(&fp.ctr->usedA, (unsigned long long)na);
    }
    auto bc = [](unsigned long long x) {
        return ((unsigned long long)(uint32_t)__shfl((int)(x >> 32), 0, 64) << 32) | (uint32_t)__shfl((int)x, 0, 64);
    };
    id = bc(id); ow = bc(ow); oa = bc(oa);
    if ((long long)id >= fp.capL || (long long)(ow + n) > fp.capW || (long long)(oa + na) > fp.capA) {
        if (lane == 0) fp.ctr->overflow = 1;
        return -2;
    }
    unsigned long long *dw = (unsigned long long *)(fp.tw + ow);
    double *da = fp.ta + oa;
    for (int k = lane; k < n; k += 64) dw[k] = w[k];
    for (int k = lane; k < na; k += 64) da[k] = a[k];
    if (lane == 0) { fp.trec[id] = lrec_make((long long)ow, n, (long long)oa, na); fp.tflag[id] = 0; }
    __threadfence();
    wave_sync();
    return (int)id;
}

// (the LDS figures in the comments of frontier.hip, frontier_dev.h and the two units)
static_assert(sizeof(WaveUpdLds<WaveSmall::wuIn>) == 27680 && sizeof(WaveUpdLds<WaveBig::wuIn>) == 110720 && sizeof(Lds) == 160, "LDS per wavefront");

}  // namespace frt
