/*
 * include/maple_hip_mat.h -- the two record structs of maple_tree_mutation_events (declared in include/maple_hip.h, which includes
 * this file; do not include it on its own).  They have a header of their own so that include/maple_hip.h keeps the six structs its
 * binding table (maple_amd/abi.py: STRUCTS) restates; these are restated by abi.MapleMutEvent / abi.MapleNRun and checked against
 * this file, fields and compiler layout, by tests/test_mat_fixtures.py.
 */
#ifndef MAPLE_HIP_MAT_H
#define MAPLE_HIP_MAT_H
#include <stdint.h>

typedef struct { int32_t pos; uint8_t from, to; uint16_t zero; double prob; } maple_mut_event;   /* 16 bytes, one store */
typedef struct { int32_t first, last; } maple_n_run;   /* last == 0: the reference's bare int `first` */

#endif
