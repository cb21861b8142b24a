// maple_amd/csrc/frontier_updw128.hip -- frontier tier of the SPR search: the list-updating items of a level that are walked a
// WAVEFRONT each, small size class (every list the item touches has at most 128 entries: most items of every level but the
// ones next to the root).  27 KB of LDS per wavefront -- five wavefronts per compute unit, 1 280 items at a time -- against
// 108 KB and one per compute unit for the 512-entry class in frontier_upd.hip.  Same code (fr_wave_items_body.inc), other sizes.
#include "frontier_upd_wave.h"

using namespace frt;

namespace {

template <bool RV, bool U, bool SS>
__global__ __launch_bounds__(64) void k_fr_updating_wave_s(const DevModel *__restrict__ mp, ArenaViewS av, DevTree T, SearchParams P, FPools fp,
                                                           int budget, int heavyMin, long long laneBase)
{
    using Class = WaveSmall;
#include "fr_wave_items_body.inc"
}
}  // namespace

int fr_launch_updating_wave_small(maple_ctx *c, hipStream_t s, int grid, const ArenaViewS &av, const DevTree &T, const SearchParams &P,
                                  const FPools &fp, int budget, int heavyMin, long long laneBase)
{
    DISPATCH3(c, k_fr_updating_wave_s, <<<grid, 64, 0, s>>>(c->d_model, av, T, P, fp, budget, heavyMin, laneBase));
    HIPCK(c, hipGetLastError());
    return MAPLE_OK;
}
