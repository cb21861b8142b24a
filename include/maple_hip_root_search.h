/*
 * include/maple_hip_root_search.h -- the parameter struct of maple_tree_find_best_root (declared in include/maple_hip.h, which
 * includes this file; do not include it on its own).  It has a header of its own so that include/maple_hip.h keeps the six structs
 * its binding table (maple_amd/abi.py: STRUCTS) restates; this one is restated by abi.MapleRootSearchParams and checked against
 * this file, fields and compiler layout, by tests/test_abi_root_search_params.py.
 */
#ifndef MAPLE_HIP_ROOT_SEARCH_H
#define MAPLE_HIP_ROOT_SEARCH_H
#include <stdint.h>

typedef struct {
    uint32_t structSize;                        /* as maple_tuning.structSize: 0 is an error, a shorter struct is read for what it has */
    int32_t  strictTopologyStopRules;           /* M:7832 */
    int32_t  allowedFailsTopology;
    double   thresholdLogLKtopology;            /* already x log(lRef) */
    double   thresholdLogLKoptimizationTopology;
    double   thresholdLogLKconsecutivePlacement;
} maple_root_search_params;

#endif
