"""What the binding knows of the C side (include/maple_hip.h, include/maple_hip_debug.h), stated once: the ABI version, the
error codes, the six structs of maple_hip.h and the one of maple_hip_root_search.h, and the signature of every entry point.  maple_amd/runtime.py calls through what bind() declares;
tests/test_abi_signatures.py compares all of it with the two headers, so a change of either side that the other misses fails there.
"""
import ctypes as C

ABI_VERSION = 4          # MAPLE_ABI_VERSION


class MapleError(RuntimeError):
    """An error status of libmaple_hip.so; ``code`` is the MAPLE_ERR_* value (include/maple_hip.h)."""
    ERR_ARG, ERR_HIP, ERR_NOMEM, ERR_STATE, ERR_FATAL = -1, -2, -3, -4, -5

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


class MapleParams(C.Structure):
    _fields_ = [("thresholdProb", C.c_double), ("minBLenSensitivity", C.c_double),
                ("thresholdDiffForUpdate", C.c_double), ("thresholdFoldChangeUpdate", C.c_double),
                ("defaultBLen", C.c_double)]


class MapleSearchParams(C.Structure):
    _fields_ = [("strictTopologyStopRules", C.c_int32), ("allowedFailsTopology", C.c_int32),
                ("thresholdLogLKtopology", C.c_double), ("thresholdTopologyPlacement", C.c_double),
                ("thresholdLogLKoptimizationTopology", C.c_double), ("thresholdLogLKconsecutivePlacement", C.c_double),
                ("effectivelyNon0BLen", C.c_double), ("wideSearchBudget", C.c_int32), ("searchTier", C.c_int32)]


class MapleTuning(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("wavePerItemMax", C.c_int32), ("placementChunkMax", C.c_int32), ("noCladeScan", C.c_int32), ("verbose", C.c_int32),
                ("wideOutsideFrontier", C.c_int32), ("denseWideScoring", C.c_int32), ("waveAllBelow", C.c_int32), ("noOverHint", C.c_int32), ("noAheadExpansion", C.c_int32), ("noAheadSpeculation", C.c_int32)]


class MaplePlacementParams(C.Structure):
    _fields_ = [("oneMutBLen", C.c_double), ("effectivelyNon0BLen", C.c_double), ("thresholdLogLK", C.c_double),
                ("thresholdLogLKoptimization", C.c_double), ("thresholdLogLKconsecutivePlacement", C.c_double),
                ("allowedFails", C.c_int32), ("strictStopRules", C.c_int32), ("onlyFindIdentical", C.c_int32)]


class MapleBlenSweepParams(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("effectivelyNon0BLen", C.c_double), ("fastPass", C.c_int32), ("chunk", C.c_int32)]


class MapleEmTotals(C.Structure):
    _fields_ = [("counts", C.c_double * 16), ("waitingTimes", C.c_double * 4), ("errorCount", C.c_double), ("totTreeLength", C.c_double),
                ("observedTotNucsSites", C.c_int64), ("numTips", C.c_int64)]


class MapleRootSearchParams(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("strictTopologyStopRules", C.c_int32), ("allowedFailsTopology", C.c_int32),
                ("thresholdLogLKtopology", C.c_double), ("thresholdLogLKoptimizationTopology", C.c_double),
                ("thresholdLogLKconsecutivePlacement", C.c_double)]


class MapleMutEvent(C.Structure):
    _fields_ = [("pos", C.c_int32), ("from", C.c_uint8), ("to", C.c_uint8), ("zero", C.c_uint16), ("prob", C.c_double)]


class MapleNRun(C.Structure):
    _fields_ = [("first", C.c_int32), ("last", C.c_int32)]


STRUCTS = {"maple_params": MapleParams, "maple_search_params": MapleSearchParams, "maple_tuning": MapleTuning,
           "maple_placement_params": MaplePlacementParams, "maple_blen_sweep_params": MapleBlenSweepParams, "maple_em_totals": MapleEmTotals}
# include/maple_hip_root_search.h (tests/test_abi_root_search_params.py): passed by reference as a plain pointer
ROOT_SEARCH_STRUCTS = {"maple_root_search_params": MapleRootSearchParams}
# include/maple_hip_mat.h (tests/test_mat_fixtures.py): the records of maple_tree_mutation_events, filled through plain pointers
MAT_STRUCTS = {"maple_mut_event": MapleMutEvent, "maple_n_run": MapleNRun}
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "float": C.c_float, "double": C.c_double}

# name: (return type, parameter types), written as the headers write them and in their order
SIGNATURES = {
    "maple_abi_version": ("int", ()),
    "maple_create": ("int", ("maple_ctx **", "int", "int32_t", "const uint8_t *", "const double *", "const maple_params *", "uint64_t")),
    "maple_destroy": ("int", ("maple_ctx *",)),
    "maple_set_tuning": ("int", ("maple_ctx *", "const maple_tuning *")),
    "maple_last_error": ("const char *", ("maple_ctx *",)),
    "maple_set_model": ("int", ("maple_ctx *", "const double *", "const double *", "int", "double", "const double *")),
    "maple_get_model": ("int", ("maple_ctx *", "double *", "double *", "double *")),
    "maple_lists_update": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const int64_t *", "const int32_t *", "const uint32_t *",
        "const int64_t *", "const double *")),
    "maple_lists_upload": ("int", ("maple_ctx *", "int32_t", "const int64_t *", "const int32_t *", "const uint32_t *", "const int64_t *",
        "const double *", "int32_t *")),
    "maple_lists_sizes": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "int32_t *", "int32_t *")),
    "maple_lists_download": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const int64_t *", "int32_t *", "uint32_t *", "const int64_t *",
        "double *")),
    "maple_arena_mark": ("int", ("maple_ctx *", "int64_t *")),
    "maple_arena_release": ("int", ("maple_ctx *", "int64_t")),
    "maple_arena_stats": ("int", ("maple_ctx *", "int64_t *", "int64_t *", "int64_t *", "int64_t *")),
    "maple_arena_compact": ("int", ("maple_ctx *", "int64_t", "const int32_t *", "int32_t *")),
    "maple_mutations_upload": ("int", ("maple_ctx *", "int32_t", "const int64_t *", "const int32_t *", "int32_t *")),
    "maple_set_fatal_policy": ("int", ("maple_ctx *", "int")),
    "maple_append_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const int32_t *", "const uint8_t *", "const double *", "double *")),
    "maple_merge_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const double *", "const uint8_t *", "const int32_t *",
        "const double *", "const uint8_t *", "const uint8_t *", "const int32_t *", "const int32_t *", "int32_t *", "double *")),
    "maple_blen_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const int32_t *", "const uint8_t *", "double *", "uint8_t *")),
    "maple_differ_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const int32_t *", "uint8_t *")),
    "maple_candset_create": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const int32_t *", "int32_t", "int32_t *")),
    "maple_candset_destroy": ("int", ("maple_ctx *", "int32_t")),
    "maple_append_candset": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "int", "double", "double *")),
    "maple_minor_candset": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "int", "uint8_t *")),
    "maple_root_prob_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "double *")),
    "maple_minor_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const int32_t *", "int", "uint8_t *")),
    "maple_pass_branch_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const int32_t *", "const uint8_t *", "int32_t *")),
    "maple_shorten_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "int32_t *")),
    "maple_root_vector_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const double *", "const uint8_t *", "const int64_t *",
        "const int32_t *", "int32_t *")),
    "maple_update_partials": ("int", ("maple_ctx *", "int32_t", "int32_t", "const int32_t *", "const int32_t *", "const int32_t *",
        "const uint8_t *", "const int32_t *", "const int32_t *", "double *", "int32_t *", "int32_t *", "int32_t *", "int32_t *", "int32_t",
        "const int32_t *", "int32_t *")),
    "maple_update_partials_touched": ("int", ("maple_ctx *", "int32_t", "int32_t *", "int32_t *")),
    "maple_tree_optimize_blens": ("int", ("maple_ctx *", "int32_t", "int32_t", "const int32_t *", "const int32_t *", "const int32_t *",
        "const uint8_t *", "const int32_t *", "const int32_t *", "double *", "int32_t *", "int32_t *", "int32_t *", "int32_t *", "uint8_t *",
        "const maple_blen_sweep_params *", "int32_t *", "int32_t", "int32_t *", "int32_t *")),
    "maple_tree_optimize_blens_stats": ("int", ("maple_ctx *", "int64_t *")),
    "maple_tree_rebuild_lists": ("int", ("maple_ctx *", "int32_t", "int32_t", "const int32_t *", "const int32_t *", "const int32_t *",
        "const uint8_t *", "const int32_t *", "double *", "int32_t *", "int32_t *", "int32_t *", "int32_t *", "double", "int32_t", "int32_t *",
        "int32_t *")),
    "maple_evaluate_placement_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const int32_t *", "const int32_t *", "const double *",
        "const int32_t *", "const uint8_t *", "const uint8_t *", "double *")),
    "maple_tree_upload": ("int", ("maple_ctx *", "int32_t", "int32_t", "const int32_t *", "const int32_t *", "const int32_t *", "const double *",
        "const uint8_t *", "const int32_t *", "const int32_t *", "const int32_t *", "const int32_t *", "const int32_t *")),
    "maple_tree_patch": ("int", ("maple_ctx *", "int32_t", "int32_t", "const int32_t *", "const int32_t *", "const int32_t *", "const int32_t *",
        "const double *", "const uint8_t *", "const int32_t *", "const int32_t *", "const int32_t *", "const int32_t *")),
    "maple_spr_search_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const maple_search_params *", "int32_t", "int32_t *",
        "double *", "double *", "int32_t *", "double *", "double *", "int32_t *", "int32_t *", "int32_t *")),
    "maple_spr_search_visited": ("int", ("maple_ctx *", "int64_t", "int32_t *", "int32_t *", "int64_t *")),
    "maple_placement_prepare": ("int", ("maple_ctx *", "const maple_placement_params *")),
    "maple_placement_ahead": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const maple_placement_params *", "int32_t *")),
    "maple_placement_ahead_stats": ("int", ("maple_ctx *", "int64_t *")),
    "maple_placement_search_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const maple_placement_params *", "int32_t *", "double *",
        "double *", "int32_t *", "int32_t *", "int32_t *")),
    "maple_placement_supports_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const maple_placement_params *", "double", "double",
        "int64_t", "int64_t *", "int32_t *", "double *", "double *", "int32_t *", "int32_t *")),
    "maple_em_expectation": ("int", ("maple_ctx *", "const int32_t *", "maple_em_totals *", "double *", "double *", "double *", "double *",
        "double *")),
    "maple_em_rates": ("int", ("maple_ctx *", "const int32_t *", "int", "double *", "double *", "double *", "double *")),
    "maple_tree_log_lk": ("int", ("maple_ctx *", "const int32_t *", "double *", "double *", "double *")),
    "maple_tree_error_probs": ("int", ("maple_ctx *", "const int32_t *", "double", "int32_t", "int32_t *", "int64_t *", "int32_t *",
        "int64_t", "int32_t *", "uint8_t *", "double *", "int64_t *")),
    "maple_tree_mutation_events": ("int", ("maple_ctx *", "const int32_t *", "double", "int64_t *", "int64_t *", "int64_t *", "int64_t",
        "maple_mut_event *", "int64_t", "maple_n_run *", "int64_t", "maple_mut_event *", "int64_t *")),
    "maple_tree_find_best_root": ("int", ("maple_ctx *", "const int32_t *", "const maple_root_search_params *", "int32_t *", "double *",
        "int32_t *", "double *", "int32_t", "int32_t *", "double *", "int32_t *")),
    "maple_append_batch_dev": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const int32_t *", "const uint8_t *", "const double *",
        "double *", "void *")),
    "maple_append_queries_dev": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "int32_t", "const int32_t *", "int", "double", "double *",
        "void *")),
    "maple_append_queries_argmax_dev": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "int32_t", "const int32_t *", "const int32_t *", "int",
        "double", "double *", "int32_t *", "void *")),
    "maple_comm_unique_id": ("int", ("maple_ctx *", "uint8_t *")),
    "maple_comm_init": ("int", ("maple_ctx *", "int32_t", "int32_t", "const uint8_t *")),
    "maple_argmax_allreduce_dev": ("int", ("maple_ctx *", "int32_t", "double *", "int32_t *", "void *")),
    "maple_timing_reset": ("int", ("maple_ctx *",)),
    "maple_timing_read": ("int", ("maple_ctx *", "int32_t *", "double *")),
    "maple_timing_read_each": ("int", ("maple_ctx *", "int32_t", "float *", "int32_t *")),
    "maple_timing_read_kind": ("int", ("maple_ctx *", "int32_t", "int32_t *", "double *", "double *", "double *")),
    "maple_append_algorithmic_bytes": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const int32_t *", "int", "uint64_t *")),
}

# include/maple_hip_debug.h: measurement aids and test hooks, exported by libmaple_hip_debug.so only (Device(..., debug=True))
DEBUG_SIGNATURES = {
    "maple_debug_frontier_levels": ("int", ("maple_ctx *", "int32_t", "int64_t *", "int64_t *", "float *", "float *", "int32_t *", "int64_t *",
        "int64_t *")),
    "maple_debug_frontier_handbacks": ("int", ("maple_ctx *", "int64_t *", "int64_t *")),
    "maple_debug_frontier_wave_paths": ("int", ("maple_ctx *", "int64_t *", "int32_t", "float *", "int32_t *", "double *", "int32_t *")),
    "maple_debug_wave_append_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const int32_t *", "const uint8_t *", "const double *",
        "double *", "float *")),
    "maple_debug_trace_query": ("int", ("maple_ctx *", "int32_t")),
    "maple_debug_calib_walk": ("int", ("maple_ctx *", "uint64_t", "int32_t", "float *")),
    "maple_debug_calib_write": ("int", ("maple_ctx *", "uint64_t", "int32_t", "int32_t", "float *")),
    "maple_debug_trace_read": ("int", ("maple_ctx *", "int32_t *", "int32_t *", "double *")),
    "maple_debug_live_resources": ("int", ("int64_t *", "int64_t *", "int64_t *")),
    "maple_debug_gpv_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const double *", "const double *", "const double *",
        "const double *", "const uint8_t *", "const uint8_t *", "double *")),
    "maple_debug_simplify_batch": ("int", ("maple_ctx *", "int32_t", "const double *", "const int32_t *", "int32_t *")),
    "maple_debug_frontier_pass_batch": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const int32_t *", "const uint8_t *", "int32_t",
        "int32_t *", "uint8_t *", "uint8_t *")),
    "maple_debug_score_rows": ("int", ("maple_ctx *", "int32_t", "int32_t", "const int32_t *", "const uint8_t *", "const double *", "int32_t",
        "const int32_t *", "const int32_t *", "int64_t", "double", "double *", "uint64_t *", "int32_t *", "int64_t *")),
    "maple_debug_update_items": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const double *", "const uint8_t *", "const int32_t *",
        "const double *", "const uint8_t *", "const uint8_t *", "const uint8_t *", "const int32_t *", "int32_t *", "uint8_t *", "uint8_t *")),
    "maple_debug_sweep_estimate": ("int", ("maple_ctx *", "int32_t", "const int32_t *", "const int32_t *", "const int32_t *", "const uint8_t *",
        "double *", "uint8_t *")),
    "maple_debug_update_partials_stats": ("int", ("maple_ctx *", "int64_t *", "int32_t", "int32_t *")),
    "maple_debug_update_partials_stat_names": ("const char *", ()),
    "maple_debug_update_partials_visited": ("int", ("maple_ctx *", "int32_t", "int32_t *", "int32_t *")),
}


def ctype(c):
    """The ctypes type of a C type of the table: a scalar by its width, a pointer to one of the structs as POINTER(its class) (byref
    of another struct is refused), every other pointer as c_void_p (numpy data pointers, byref(...), None, and the integer device
    pointers and stream handles of the _dev entry points all pass)."""
    if c == "const char *":
        return C.c_char_p
    if c.endswith("*"):
        pointee = c[:-1].replace("const ", "").strip()
        return C.POINTER(STRUCTS[pointee]) if pointee in STRUCTS else C.c_void_p
    return SCALARS[c]


def bind(lib, debug=False, require_all=True):
    """Declare restype / argtypes on every entry point of the table that ``lib`` exports (debug: those of maple_hip_debug.h too),
    then check that the library has this binding's ABI version.  require_all: a symbol the library does not export is an error
    (without it: a library with a subset of the ABI, such as the CPU twin of the tests).  Binding a library again changes nothing."""
    for header, table in (("maple_hip.h", SIGNATURES), ("maple_hip_debug.h", DEBUG_SIGNATURES if debug else {})):
        for name, (ret, params) in table.items():
            if not hasattr(lib, name):
                if require_all or name == "maple_abi_version":       # fail early if a declared symbol is not exported
                    raise MapleError(f"{lib._name} does not export {name} (include/{header}): rebuild it with __graft_entry__.build()")
                continue
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = ctype(ret), [ctype(p) for p in params]
    version = lib.maple_abi_version()
    if version != ABI_VERSION:
        raise MapleError(f"{lib._name} has ABI version {version}, this binding is written for version {ABI_VERSION} "
                         "(MAPLE_ABI_VERSION, include/maple_hip.h): rebuild it with __graft_entry__.build()")
    return lib
