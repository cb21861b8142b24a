"""ctypes binding of libmaple_hip.so (the C ABI in include/maple_hip.h).

This is the only way the host reaches the GPU kernels.  There is no CPU
fallback: if the shared library is missing or no MI355X is visible,
construction raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .abi import (DEBUG_SIGNATURES, SIGNATURES, MapleBlenSweepParams, MapleEmTotals, MapleError, MapleParams,  # noqa: F401
                  MaplePlacementParams, MapleRootSearchParams, MapleSearchParams, MapleTuning, bind)
from .genome_list import PackedLists, pack_lists, pack_mutations, unpack_list

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmaple_hip.so")

# the C side as the binding declares it: maple_amd/abi.py (the structs and MapleError are re-exported: callers import them from here)
EXPORTS, DEBUG_EXPORTS = list(SIGNATURES), list(DEBUG_SIGNATURES)
LIB_PATH_DEBUG = os.path.join(HERE, "libmaple_hip_debug.so")

EM_MODELS = {"UNREST": 0, "GTR": 1}
# the records of maple_tree_mutation_events as numpy sees them: maple_mut_event / maple_n_run of include/maple_hip_mat.h
MUT_EVENT_DTYPE = np.dtype([("pos", "<i4"), ("from", "u1"), ("to", "u1"), ("zero", "<u2"), ("prob", "<f8")], align=True)
N_RUN_DTYPE = np.dtype([("first", "<i4"), ("last", "<i4")], align=True)

_lib = None
_lib_debug = None


def load_library(debug=False):
    """Load libmaple_hip.so (``debug``: libmaple_hip_debug.so, the same library with the entry points of
    include/maple_hip_debug.h); raises if it has not been built (see __graft_entry__.build)."""
    global _lib, _lib_debug
    if (_lib_debug if debug else _lib) is None:
        default = LIB_PATH_DEBUG if debug else LIB_PATH
        # (kernel-variant experiments: another build of the library.  MAPLE_HIP_LIB names a product build and never the debug
        # one -- a product variant has no maple_debug_* symbols, a debug build behind the product handle would carry the debug ABI;
        # MAPLE_HIP_LIB_DEBUG names a debug variant)
        lib_path = os.environ.get("MAPLE_HIP_LIB_DEBUG" if debug else "MAPLE_HIP_LIB", default)
        if not os.path.exists(lib_path):
            raise MapleError(f"{lib_path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`; "
                             "there is no CPU fallback for the placement path")
        # PyTorch-ROCm ships its own HIP runtime; whichever copy of libamdhip64 is loaded first serves the whole
        # process, and torch cannot see the GPU if the system copy got there before it.  Load torch's first.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = bind(C.CDLL(lib_path), debug)      # fails early if a declared symbol is not exported or the ABI version is another
        if debug:
            _lib_debug = lib
        else:
            _lib = lib
    return _lib_debug if debug else _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _i32(x):
    return np.ascontiguousarray(x, dtype=np.int32)


def _u8(x):
    return np.ascontiguousarray(x, dtype=np.uint8)


def _f64(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def debug_live_resources():
    """(allocations, bytes, handles) the library holds at this moment in this process, over all contexts: device and page-locked
    allocations with their bytes, streams and events (maple_debug_live_resources, debug library).  Compare differences."""
    a, b, h = C.c_int64(), C.c_int64(), C.c_int64()
    rc = load_library(debug=True).maple_debug_live_resources(C.byref(a), C.byref(b), C.byref(h))
    if rc != 0:
        raise MapleError(f"maple_debug_live_resources failed ({rc})", rc)
    return a.value, b.value, h.value


class Device:
    """One GPU context: model tables, the genome-list arena and the batched operators."""

    def __init__(self, ref_idx, root_freqs, *, device=0, thresholdProb=1e-8, minBLenSensitivity=None,
                 thresholdDiffForUpdate=1e-5, thresholdFoldChangeUpdate=1.01, defaultBLen=0.000033,
                 arena_bytes=0, lib=None, debug=False):
        # (lib: another library with the same C ABI, handed in explicitly -- the tests diff libmaple_hip.so against its CPU twin
        # this way; nothing in the package ever passes one)
        # (debug: libmaple_hip_debug.so -- the same library plus the measurement aids and test hooks of include/maple_hip_debug.h)
        self.lib = bind(lib, debug, require_all=False) if lib is not None else load_library(debug)
        self.ref_idx = _u8(ref_idx)
        self.lRef = int(len(self.ref_idx))
        if minBLenSensitivity is None:
            minBLenSensitivity = 0.001 / self.lRef
        p = MapleParams(thresholdProb, minBLenSensitivity, thresholdDiffForUpdate, thresholdFoldChangeUpdate, defaultBLen)
        rf = _f64(root_freqs)
        h = C.c_void_p()
        rc = self.lib.maple_create(C.byref(h), int(device), self.lRef, _ptr(self.ref_idx), _ptr(rf), C.byref(p), arena_bytes)
        if rc != 0:
            raise MapleError(f"maple_create failed ({rc}): no usable MI355X / HIP runtime; the placement path has no "
                             "CPU fallback")
        self.h = h
        self.device = int(device)
        self.u = False

    # -- plumbing --------------------------------------------------------------------------
    def _ck(self, rc):
        if rc != 0:
            msg = self.lib.maple_last_error(self.h)
            raise MapleError(f"libmaple_hip error {rc}: {msg.decode() if msg else ''}", rc)

    def close(self):
        if getattr(self, "h", None):
            self.lib.maple_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- model -------------------------------------------------------------------------------
    def set_tuning(self, *, wave_per_item_max=0, placement_chunk_max=0, no_clade_scan=False, verbose=0, wide_outside_frontier=False,
                   dense_wide_scoring=False, wave_all_below=0, no_over_hint=False, no_ahead_expansion=False, no_ahead_speculation=False):
        """How the library schedules its work (never what it computes): see maple_tuning in include/maple_hip.h."""
        t = MapleTuning(C.sizeof(MapleTuning), int(wave_per_item_max), int(placement_chunk_max), int(bool(no_clade_scan)), int(verbose),
                        int(bool(wide_outside_frontier)), int(bool(dense_wide_scoring)), int(wave_all_below), int(bool(no_over_hint)),
                        int(no_ahead_expansion), int(bool(no_ahead_speculation)))
        self._ck(self.lib.maple_set_tuning(self.h, C.byref(t)))

    def set_model(self, Q, siteRates=None, usingErrorRate=False, errorRateGlobal=0.0, errorRates=None):
        Qf = _f64(np.asarray(Q, dtype=np.float64).reshape(16))
        sr = None if siteRates is None else _f64(siteRates)
        er = None if (errorRates is None or not usingErrorRate) else _f64(errorRates)
        self._ck(self.lib.maple_set_model(self.h, _ptr(Qf), _ptr(sr), bool(usingErrorRate), errorRateGlobal or 0.0, _ptr(er)))
        self.u = bool(usingErrorRate)
        self.rv, self.ss = sr is not None, er is not None

    def get_model(self):
        cr = np.zeros(self.lRef + 1)
        ce = np.zeros(self.lRef + 1)
        te = C.c_double()
        self._ck(self.lib.maple_get_model(self.h, _ptr(cr), _ptr(ce), C.byref(te)))
        return cr, ce, te.value

    # -- lists -------------------------------------------------------------------------------
    def upload_packed(self, pl: PackedLists):
        first = C.c_int32()
        self._ck(self.lib.maple_lists_upload(self.h, len(pl), _ptr(pl.ent_off), _ptr(pl.pos), _ptr(pl.meta),
                                             _ptr(pl.aux_off), _ptr(pl.aux), C.byref(first)))
        return np.arange(first.value, first.value + len(pl), dtype=np.int32)

    def update_lists(self, ids, lists):
        """maple_lists_update: new contents (reference tuple form) for the existing list ids; the ids stay valid."""
        pl = pack_lists(lists, self.u)
        ids = _i32(ids)
        assert len(ids) == len(pl)
        self._ck(self.lib.maple_lists_update(self.h, len(pl), _ptr(ids), _ptr(pl.ent_off), _ptr(pl.pos), _ptr(pl.meta),
                                             _ptr(pl.aux_off), _ptr(pl.aux)))

    def upload(self, lists):
        """Upload genome lists given in the reference's tuple form; returns their ids."""
        return self.upload_packed(pack_lists(lists, self.u))

    def sizes(self, ids):
        ids = _i32(ids)
        ne = np.zeros(len(ids), dtype=np.int32)
        na = np.zeros(len(ids), dtype=np.int32)
        self._ck(self.lib.maple_lists_sizes(self.h, len(ids), _ptr(ids), _ptr(ne), _ptr(na)))
        return ne, na

    def download_packed(self, ids) -> PackedLists:
        """Download lists (all ids >= 0) in the packed CSR form."""
        good = _i32(ids)
        ne, na = self.sizes(good)
        eo = np.zeros(len(good) + 1, dtype=np.int64)
        ao = np.zeros(len(good) + 1, dtype=np.int64)
        np.cumsum(ne, out=eo[1:])
        np.cumsum(na, out=ao[1:])
        pos = np.zeros(max(1, eo[-1]), dtype=np.int32)
        meta = np.zeros(max(1, eo[-1]), dtype=np.uint32)
        aux = np.zeros(max(1, ao[-1]), dtype=np.float64)
        if len(good):
            self._ck(self.lib.maple_lists_download(self.h, len(good), _ptr(good), _ptr(eo), _ptr(pos), _ptr(meta),
                                                   _ptr(ao), _ptr(aux)))
        return PackedLists(eo, pos, meta, ao, aux)

    def download(self, ids):
        """Download lists by id into the reference's tuple form (None for id -1)."""
        ids = _i32(ids)
        good = ids[ids >= 0]
        pk = self.download_packed(good)
        eo, ao, pos, meta, aux = pk.ent_off, pk.aux_off, pk.pos, pk.meta, pk.aux
        out, k = [], 0
        for i in ids:
            if i < 0:
                out.append(None)
            else:
                out.append(unpack_list(pos[eo[k]:eo[k + 1]], meta[eo[k]:eo[k + 1]], aux[ao[k]:ao[k + 1]], self.u))
                k += 1
        return out

    def set_fatal_policy(self, tolerate: bool):
        """tolerate=True: an item that hits a state the reference raises on gets list id -2 instead of failing its batch."""
        self._ck(self.lib.maple_set_fatal_policy(self.h, bool(tolerate)))

    def mark(self):
        m = C.c_int64()
        self._ck(self.lib.maple_arena_mark(self.h, C.byref(m)))
        return m.value

    def release(self, mark):
        self._ck(self.lib.maple_arena_release(self.h, mark))

    def stats(self):
        a, b, c_, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._ck(self.lib.maple_arena_stats(self.h, C.byref(a), C.byref(b), C.byref(c_), C.byref(d)))
        return dict(n_lists=a.value, n_entries=b.value, n_aux=c_.value, cap_entries=d.value)

    def arena_compact(self, live):
        """Keep only the lists `live` (-1 entries stay -1): returns their new ids.  Every other id, mark, candidate set and the
        uploaded tree are gone afterwards (maple_arena_compact)."""
        live = _i32(live)
        new = np.zeros(len(live), np.int32)
        self._ck(self.lib.maple_arena_compact(self.h, len(live), _ptr(live), _ptr(new)))
        return new

    def upload_mutations(self, mut_lists):
        off, mut3 = pack_mutations(mut_lists)
        first = C.c_int32()
        self._ck(self.lib.maple_mutations_upload(self.h, len(off) - 1, _ptr(off), _ptr(mut3), C.byref(first)))
        return np.arange(first.value, first.value + len(off) - 1, dtype=np.int32)

    # -- batched operators ----------------------------------------------------------------------
    def append_batch(self, parent, child, isTipC, bLen):
        parent, child = _i32(parent), _i32(child)
        n = len(parent)
        tip = _u8(np.broadcast_to(isTipC, n))
        bl = _f64(np.broadcast_to(bLen, n))
        out = np.zeros(n)
        self._ck(self.lib.maple_append_batch(self.h, n, _ptr(parent), _ptr(child), _ptr(tip), _ptr(bl), _ptr(out)))
        return out

    def merge_batch(self, l1, b1, tip1, l2, b2, tip2, isUpDown, returnLK=False, numMinor1=None, numMinor2=None):
        l1, l2 = _i32(l1), _i32(l2)
        n = len(l1)
        b1, b2 = _f64(np.broadcast_to(b1, n)), _f64(np.broadcast_to(b2, n))
        t1, t2 = _u8(np.broadcast_to(tip1, n)), _u8(np.broadcast_to(tip2, n))
        ud = _u8(np.broadcast_to(isUpDown, n))
        nm1 = None if numMinor1 is None else _i32(np.broadcast_to(numMinor1, n))
        nm2 = None if numMinor2 is None else _i32(np.broadcast_to(numMinor2, n))
        out = np.zeros(n, dtype=np.int32)
        lk = np.zeros(n) if returnLK else None
        self._ck(self.lib.maple_merge_batch(self.h, n, _ptr(l1), _ptr(b1), _ptr(t1), _ptr(l2), _ptr(b2), _ptr(t2),
                                            _ptr(ud), _ptr(nm1), _ptr(nm2), _ptr(out), _ptr(lk)))
        return (out, lk) if returnLK else out

    def blen_batch(self, parent, child, fromTipC):
        parent, child = _i32(parent), _i32(child)
        n = len(parent)
        tip = _u8(np.broadcast_to(fromTipC, n))
        t = np.zeros(n)
        f = np.zeros(n, dtype=np.uint8)
        self._ck(self.lib.maple_blen_batch(self.h, n, _ptr(parent), _ptr(child), _ptr(tip), _ptr(t), _ptr(f)))
        return t, f.astype(bool)

    def differ_batch(self, l1, l2):
        l1, l2 = _i32(l1), _i32(l2)
        out = np.zeros(len(l1), dtype=np.uint8)
        self._ck(self.lib.maple_differ_batch(self.h, len(l1), _ptr(l1), _ptr(l2), _ptr(out)))
        return out.astype(bool)

    def candset_create(self, lists, frame_idx, n_frames):
        lists, frame_idx = _i32(lists), _i32(frame_idx)
        sid = C.c_int32()
        self._ck(self.lib.maple_candset_create(self.h, len(lists), _ptr(lists), _ptr(frame_idx), n_frames, C.byref(sid)))
        return sid.value, len(lists)

    def candset_destroy(self, cset):
        self._ck(self.lib.maple_candset_destroy(self.h, cset[0]))

    def append_candset(self, cset, frame_lists, isTipC, bLen):
        fl = _i32(frame_lists)
        out = np.zeros(cset[1])
        self._ck(self.lib.maple_append_candset(self.h, cset[0], _ptr(fl), bool(isTipC), bLen, _ptr(out)))
        return out

    def minor_candset(self, cset, frame_lists, onlyFindIdentical=False):
        fl = _i32(frame_lists)
        out = np.zeros(cset[1], dtype=np.uint8)
        self._ck(self.lib.maple_minor_candset(self.h, cset[0], _ptr(fl), bool(onlyFindIdentical), _ptr(out)))
        return out

    def root_prob_batch(self, lists):
        lists = _i32(lists)
        out = np.zeros(len(lists))
        self._ck(self.lib.maple_root_prob_batch(self.h, len(lists), _ptr(lists), _ptr(out)))
        return out

    def minor_batch(self, l1, l2, onlyFindIdentical=False):
        l1, l2 = _i32(l1), _i32(l2)
        out = np.zeros(len(l1), dtype=np.uint8)
        self._ck(self.lib.maple_minor_batch(self.h, len(l1), _ptr(l1), _ptr(l2), bool(onlyFindIdentical), _ptr(out)))
        return out

    def pass_branch_batch(self, lists, mutLists, dirIsUp):
        lists, mutLists = _i32(lists), _i32(mutLists)
        n = len(lists)
        up = _u8(np.broadcast_to(dirIsUp, n))
        out = np.zeros(n, dtype=np.int32)
        self._ck(self.lib.maple_pass_branch_batch(self.h, n, _ptr(lists), _ptr(mutLists), _ptr(up), _ptr(out)))
        return out

    def shorten_batch(self, lists):
        lists = _i32(lists)
        out = np.zeros(len(lists), dtype=np.int32)
        self._ck(self.lib.maple_shorten_batch(self.h, len(lists), _ptr(lists), _ptr(out)))
        return out

    def root_vector_batch(self, lists, bLen, isFromTip, paths):
        """paths[i] = mutation-list ids on the walk node -> root (node first)."""
        lists = _i32(lists)
        n = len(lists)
        bl = _f64(np.broadcast_to(bLen, n))
        tip = _u8(np.broadcast_to(isFromTip, n))
        off = np.zeros(n + 1, dtype=np.int64)
        flat = []
        for i, p in enumerate(paths):
            flat.extend(int(x) for x in p)
            off[i + 1] = len(flat)
        pm = _i32(flat if flat else [0])
        out = np.zeros(n, dtype=np.int32)
        self._ck(self.lib.maple_root_vector_batch(self.h, n, _ptr(lists), _ptr(bl), _ptr(tip), _ptr(off), _ptr(pm),
                                                  _ptr(out)))
        return out

    def tree_patch(self, n_total, nodes, up, c0, c1, dist, tip, lower, up_right, up_left, tot_up):
        """maple_tree_patch: the records of the touched (and new) nodes; see include/maple_hip.h."""
        nodes = _i32(nodes)
        cols = [_i32(x) for x in (up, c0, c1)] + [_f64(dist), _u8(tip)] + [_i32(x) for x in (lower, up_right, up_left, tot_up)]
        assert all(len(x) == len(nodes) for x in cols)
        self._ck(self.lib.maple_tree_patch(self.h, n_total, len(nodes), _ptr(nodes), *[_ptr(x) for x in cols]))
        self.n_nodes = n_total

    def update_partials(self, root, up, c0, c1, tip, mut, depth, dist, lower, up_right, up_left, tot_up, changed):
        """maple_update_partials: the four list-id columns and ``dist`` are updated IN PLACE (they must be C-contiguous
        int32 / float64 arrays -- nothing is copied); returns the number of lists replaced."""
        for name, arr, dt in (("up", up, np.int32), ("child0", c0, np.int32), ("child1", c1, np.int32), ("isTip", tip, np.uint8),
                              ("mutList", mut, np.int32), ("depth", depth, np.int32), ("dist", dist, np.float64),
                              ("lower", lower, np.int32), ("upRight", up_right, np.int32), ("upLeft", up_left, np.int32),
                              ("totUp", tot_up, np.int32)):
            if not (isinstance(arr, np.ndarray) and arr.dtype == dt and arr.flags.c_contiguous and len(arr) == len(up)):
                raise ValueError(f"update_partials: column {name} must be a C-contiguous {np.dtype(dt).name} array of {len(up)}")
        ch = _i32(changed)
        n_rep = C.c_int32(0)
        self._ck(self.lib.maple_update_partials(self.h, len(up), root, _ptr(up), _ptr(c0), _ptr(c1), _ptr(tip), _ptr(mut),
                                                _ptr(depth), _ptr(dist), _ptr(lower), _ptr(up_right), _ptr(up_left), _ptr(tot_up),
                                                len(ch), _ptr(ch), C.byref(n_rep)))
        return int(n_rep.value)

    def optimize_blens(self, root, up, c0, c1, tip, mut, depth, dist, lower, up_right, up_left, tot_up, dirty, effectivelyNon0BLen,
                       fast_pass=False, chunk=0, cap_order=None):
        """maple_tree_optimize_blens: one call of traverseTreeToOptimizeBranchLengths on the caller's columns.  ``dist``, the four
        list-id columns and ``dirty`` (uint8) are updated IN PLACE (C-contiguous arrays, nothing is copied).  Returns
        (updates, order, nOrder): the reference's return value, the nodes handed to a repair in order (the first ``cap_order``
        of them, default all) and their full count."""
        n = len(up)
        for name, arr, dt in (("up", up, np.int32), ("child0", c0, np.int32), ("child1", c1, np.int32), ("isTip", tip, np.uint8),
                              ("mutList", mut, np.int32), ("depth", depth, np.int32), ("dist", dist, np.float64),
                              ("lower", lower, np.int32), ("upRight", up_right, np.int32), ("upLeft", up_left, np.int32),
                              ("totUp", tot_up, np.int32), ("dirty", dirty, np.uint8)):
            if not (isinstance(arr, np.ndarray) and arr.dtype == dt and arr.flags.c_contiguous and len(arr) == n):
                raise ValueError(f"optimize_blens: column {name} must be a C-contiguous {np.dtype(dt).name} array of {n}")
        cap = n if cap_order is None else int(cap_order)
        order = np.zeros(max(cap, 1), dtype=np.int32)
        p = MapleBlenSweepParams(C.sizeof(MapleBlenSweepParams), float(effectivelyNon0BLen), int(bool(fast_pass)), int(chunk))
        n_upd, n_ord = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.maple_tree_optimize_blens(self.h, n, root, _ptr(up), _ptr(c0), _ptr(c1), _ptr(tip), _ptr(mut), _ptr(depth),
                                                    _ptr(dist), _ptr(lower), _ptr(up_right), _ptr(up_left), _ptr(tot_up), _ptr(dirty),
                                                    C.byref(p), C.byref(n_upd), cap, _ptr(order) if cap else None, C.byref(n_ord)))
        return int(n_upd.value), order[:min(cap, n_ord.value)].copy(), int(n_ord.value)

    def optimize_blens_stats(self):
        """maple_tree_optimize_blens_stats, since the context was created: dict(launches, computed, used, repairs, sweeps)."""
        out = np.zeros(5, dtype=np.int64)
        self._ck(self.lib.maple_tree_optimize_blens_stats(self.h, _ptr(out)))
        return dict(zip(("launches", "computed", "used", "repairs", "sweeps"), (int(x) for x in out)))

    def debug_wave_append_batch(self, pl, cl, isTipC, bLen):
        """appendProbNode with one wavefront per pair (maple_debug_wave_append_batch); returns (values, kernel ms)."""
        pl, cl = _i32(pl), _i32(cl)
        n = len(pl)
        tip = _u8(np.broadcast_to(isTipC, n))
        bl = _f64(np.broadcast_to(bLen, n))
        out = np.zeros(n)
        ms = C.c_float(0.0)
        self._ck(self.lib.maple_debug_wave_append_batch(self.h, n, _ptr(pl), _ptr(cl), _ptr(tip), _ptr(bl), _ptr(out), C.byref(ms)))
        return out, float(ms.value)

    def update_partials_touched(self, cap=65536):
        """Nodes whose lists / branch length the last update_partials replaced (ascending)."""
        out = np.zeros(cap, dtype=np.int32)
        n = C.c_int32(0)
        self._ck(self.lib.maple_update_partials_touched(self.h, cap, _ptr(out), C.byref(n)))
        return out[:n.value].copy()

    def evaluate_placement_batch(self, midTot, down, up, distance, removed, isRemovedTip, fromTip1):
        midTot, down, up, removed = _i32(midTot), _i32(down), _i32(up), _i32(removed)
        n = len(midTot)
        dist = _f64(np.broadcast_to(distance, n))
        rt, ft = _u8(np.broadcast_to(isRemovedTip, n)), _u8(np.broadcast_to(fromTip1, n))
        out = np.zeros((n, 4))
        self._ck(self.lib.maple_evaluate_placement_batch(self.h, n, _ptr(midTot), _ptr(down), _ptr(up), _ptr(dist),
                                                         _ptr(removed), _ptr(rt), _ptr(ft), _ptr(out)))
        return out

    # -- tree mirror + device-resident SPR search ------------------------------------------------------
    def upload_tree(self, root, up, child0, child1, dist, isTip, lower, upRight, upLeft, totUp, mutList):
        n = len(up)
        arrs = [_i32(x) for x in (up, child0, child1)]
        d, tip = _f64(dist), _u8(isTip)
        ls = [_i32(x) for x in (lower, upRight, upLeft, totUp, mutList)]
        self._ck(self.lib.maple_tree_upload(self.h, n, root, _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), _ptr(d),
                                            _ptr(tip), _ptr(ls[0]), _ptr(ls[1]), _ptr(ls[2]), _ptr(ls[3]), _ptr(ls[4])))
        self.n_nodes = n

    def spr_search_batch(self, nodes, *, strict, allowedFails, thresholdLogLKtopology, thresholdTopologyPlacement,
                         thresholdLogLKoptimizationTopology, thresholdLogLKconsecutivePlacement, effectivelyNon0BLen,
                         ws_entries_per_lane=0, want_removed_partials=False, wide_search_budget=0, search_tier=0):
        """startTopologyUpdatesParallel's worker body (M:9615-9711) for `nodes`, searches run on the GPU."""
        nodes = _i32(nodes)
        n = len(nodes)
        sp = MapleSearchParams(int(bool(strict)), int(allowedFails), thresholdLogLKtopology, thresholdTopologyPlacement,
                               thresholdLogLKoptimizationTopology, thresholdLogLKconsecutivePlacement,
                               effectivelyNon0BLen, int(wide_search_budget), int(search_tier))
        out = dict(bestNode=np.zeros(n, np.int32), bestScore=np.zeros(n), blen=np.zeros((n, 3)),
                   placement=np.zeros(n, np.int32), improvement=np.zeros(n), currentLK=np.zeros(n),
                   nAppend=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
        rpr = np.zeros(n, np.int32) if want_removed_partials else None
        self._ck(self.lib.maple_spr_search_batch(self.h, n, _ptr(nodes), C.byref(sp), ws_entries_per_lane,
                                                 _ptr(out["bestNode"]), _ptr(out["bestScore"]), _ptr(out["blen"]),
                                                 _ptr(out["placement"]), _ptr(out["improvement"]),
                                                 _ptr(out["currentLK"]), _ptr(out["nAppend"]), _ptr(out["status"]),
                                                 _ptr(rpr)))
        if want_removed_partials:
            out["removedPartials"] = rpr
        return out

    def spr_search_visited(self, cap=1 << 22):
        """(query index, node) pairs of every branch the searches of the last spr_search_batch may have read (see the header).
        If they do not fit in ``cap`` the call is repeated with the room it asked for."""
        for _ in range(2):
            q = np.zeros(cap, np.int32)
            v = np.zeros(cap, np.int32)
            n = C.c_int64()
            rc = self.lib.maple_spr_search_visited(self.h, cap, _ptr(q), _ptr(v), C.byref(n))
            if rc == MapleError.ERR_ARG and n.value > cap:
                cap = int(n.value)
                continue
            self._ck(rc)
            return q[: n.value], v[: n.value]
        self._ck(rc)

    def placement_prepare(self, *, oneMutBLen, effectivelyNon0BLen, thresholdLogLK, thresholdLogLKoptimization,
                          thresholdLogLKconsecutivePlacement, allowedFails=5, strictStopRules=True, onlyFindIdentical=False):
        """Per-tree tables + root vector of the placement search, created outside any arena mark of the caller."""
        pp = MaplePlacementParams(oneMutBLen, effectivelyNon0BLen, thresholdLogLK, thresholdLogLKoptimization,
                                  thresholdLogLKconsecutivePlacement, int(allowedFails), int(bool(strictStopRules)),
                                  int(bool(onlyFindIdentical)))
        self._ck(self.lib.maple_placement_prepare(self.h, C.byref(pp)))

    def placement_ahead(self, q_lists, *, oneMutBLen, effectivelyNon0BLen, thresholdLogLK, thresholdLogLKoptimization,
                        thresholdLogLKconsecutivePlacement, allowedFails=5, strictStopRules=True, onlyFindIdentical=False):
        """Announce the next samples of a serial placement loop (maple_placement_ahead): their score rows are made in one launch
        and kept current under tree_patch; single-sample placement_search_batch calls for them, in this order and with these
        parameters, then skip the scoring.  Returns how many of the leading samples got rows (0: nothing changes)."""
        q = _i32(q_lists)
        pp = MaplePlacementParams(oneMutBLen, effectivelyNon0BLen, thresholdLogLK, thresholdLogLKoptimization,
                                  thresholdLogLKconsecutivePlacement, int(allowedFails), int(bool(strictStopRules)),
                                  int(bool(onlyFindIdentical)))
        taken = C.c_int32(0)
        self._ck(self.lib.maple_placement_ahead(self.h, len(q), _ptr(q), C.byref(pp), C.byref(taken)))
        return taken.value

    def placement_ahead_stats(self):
        out = np.zeros(5, dtype=np.int64)
        self._ck(self.lib.maple_placement_ahead_stats(self.h, _ptr(out)))
        return dict(zip(("searches", "fallbacks", "expanded_items", "traversals_ahead_used", "traversals_ahead_dropped"), (int(x) for x in out)))

    def placement_search_batch(self, q_lists, *, oneMutBLen, effectivelyNon0BLen, thresholdLogLK,
                               thresholdLogLKoptimization, thresholdLogLKconsecutivePlacement, allowedFails=5,
                               strictStopRules=True, onlyFindIdentical=False):
        """findBestParentForNewSample (M:7912-8292) for many query lists against the uploaded (frozen) tree."""
        q = _i32(q_lists)
        n = len(q)
        pp = MaplePlacementParams(oneMutBLen, effectivelyNon0BLen, thresholdLogLK, thresholdLogLKoptimization,
                                  thresholdLogLKconsecutivePlacement, int(allowedFails), int(bool(strictStopRules)),
                                  int(bool(onlyFindIdentical)))
        out = dict(bestNode=np.zeros(n, np.int32), bestScore=np.zeros(n), blen=np.zeros((n, 3)),
                   bestDiffs=np.zeros(n, np.int32), nAppend=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
        self._ck(self.lib.maple_placement_search_batch(self.h, n, _ptr(q), C.byref(pp), _ptr(out["bestNode"]),
                                                       _ptr(out["bestScore"]), _ptr(out["blen"]), _ptr(out["bestDiffs"]),
                                                       _ptr(out["nAppend"]), _ptr(out["status"])))
        return out

    def placement_supports_batch(self, q_lists, *, oneMutBLen, effectivelyNon0BLen, thresholdLogLK,
                                 thresholdLogLKoptimization, thresholdLogLKconsecutivePlacement,
                                 thresholdLogLKoptimizationTopology, minBranchSupport=0.01, allowedFails=5,
                                 strictStopRules=True, onlyFindIdentical=False):
        """findBestParentForNewSample(..., computePlacementSupportOnly=True) (M:8101-8290) for many query lists: per query
        (possiblePlacements = [(node, support, (top, bottom, appending)), ...], list id of bestPlacementTotalLh or -1)."""
        q = _i32(q_lists)
        n = len(q)
        pp = MaplePlacementParams(oneMutBLen, effectivelyNon0BLen, thresholdLogLK, thresholdLogLKoptimization,
                                  thresholdLogLKconsecutivePlacement, int(allowedFails), int(bool(strictStopRules)),
                                  int(bool(onlyFindIdentical)))
        cap = 128 * max(1, n)
        off = np.zeros(n + 1, np.int64)
        node, supp, bl = np.zeros(cap, np.int32), np.zeros(cap), np.zeros((cap, 3))
        best, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._ck(self.lib.maple_placement_supports_batch(self.h, n, _ptr(q), C.byref(pp), thresholdLogLKoptimizationTopology,
                                                         minBranchSupport, cap, _ptr(off), _ptr(node), _ptr(supp), _ptr(bl),
                                                         _ptr(best), _ptr(status)))
        out = []
        for g in range(n):
            a, b = off[g], off[g + 1]
            out.append(([(int(node[i]), float(supp[i]), tuple(float(x) for x in bl[i])) for i in range(a, b)], int(best[g])))
        return out, status

    def debug_gpv_batch(self, i12, totLen, mutMatrix, errorRate, vect, upNode, flag):
        """getPartialVec (M:4073-4141) for n calls, each with its own 4x4 matrix; vect rows are read where i12 == 6."""
        i12 = _i32(i12)
        n = len(i12)
        M = _f64(np.asarray(mutMatrix, dtype=np.float64).reshape(n, 16))
        v = _f64(np.asarray(vect, dtype=np.float64).reshape(n, 4))
        out = np.zeros((n, 4))
        self._ck(self.lib.maple_debug_gpv_batch(self.h, n, _ptr(i12), _ptr(_f64(totLen)), _ptr(M), _ptr(_f64(errorRate)), _ptr(v),
                                                _ptr(_u8(upNode)), _ptr(_u8(flag)), _ptr(out)))
        return out

    def debug_simplify_batch(self, vec, refA):
        v = _f64(np.asarray(vec, dtype=np.float64).reshape(-1, 4))
        out = np.zeros(len(v), dtype=np.int32)
        self._ck(self.lib.maple_debug_simplify_batch(self.h, len(v), _ptr(v), _ptr(_i32(refA)), _ptr(out)))
        return out

    def debug_frontier_pass_batch(self, lists, mutLists, dirIsUp, wave_form=False):
        """passGenomeListThroughBranch of removed lists as the frontier tier of the SPR search runs it
        (maple_debug_frontier_pass_batch): one lane per item, or one wavefront per item with wave_form.  Returns (list ids --
        the input id where the tier handed its handle back --, grades 0 / 1 / 2, same-handle flags)."""
        lists, mutLists = _i32(lists), _i32(mutLists)
        n = len(lists)
        up = _u8(np.broadcast_to(dirIsUp, n))
        out = np.zeros(n, dtype=np.int32)
        grade, same = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self._ck(self.lib.maple_debug_frontier_pass_batch(self.h, n, _ptr(lists), _ptr(mutLists), _ptr(up), bool(wave_form),
                                                          _ptr(out), _ptr(grade), _ptr(same)))
        return out, grade, same.astype(bool)

    def debug_score_rows(self, form, q_lists, qTip, qBLen, cands, out_col=None, ld_out=None, fill=float("nan")):
        """Rows of the whole-tree searches' score table from explicit lists (maple_debug_score_rows): form 0 the dense kernel with
        bitmap, form 1 the witness filter.  Returns (out [nQ, ld_out] -- `fill` where no finite score was written --, finMask
        uint64 [nQ, nWords], prefix int32 [nQ, nWords + 1], pairs walked or -1)."""
        q_lists, cands = _i32(q_lists), _i32(cands)
        nQ, nC = len(q_lists), len(cands)
        ld = nC if ld_out is None else int(ld_out)
        nW = (nC + 63) // 64
        tip, bl = _u8(np.broadcast_to(qTip, nQ)), _f64(np.broadcast_to(qBLen, nQ))
        col = None if out_col is None else _i32(out_col)
        assert col is None or len(col) == nC
        out = np.zeros((nQ, max(ld, 1)))
        mask = np.zeros((nQ, nW), dtype=np.uint64)
        prefix = np.zeros((nQ, nW + 1), dtype=np.int32)
        pairs = C.c_int64(-1)
        self._ck(self.lib.maple_debug_score_rows(self.h, form, nQ, _ptr(q_lists), _ptr(tip), _ptr(bl), nC, _ptr(cands), _ptr(col),
                                                 ld, fill, _ptr(out), _ptr(mask), _ptr(prefix), C.byref(pairs)))
        return out, mask, prefix, pairs.value

    def debug_update_items(self, l1, b1, tip1, l2, b2, tip2, upDown, mode, old):
        """One level's items of the repair by the library's own fused kernels (maple_debug_update_items): mergeVectors, then
        shorten / areVectorsDifferent as mode 0 / 1 / 2 says, against old (-1: none).  Returns (list ids, -1 where the merge is None
        or mode 2 found no difference; None flags; verdicts)."""
        l1, l2, old = _i32(l1), _i32(l2), _i32(old)
        n = len(l1)
        b1, b2 = _f64(np.broadcast_to(b1, n)), _f64(np.broadcast_to(b2, n))
        t1, t2, ud, md = (_u8(np.broadcast_to(x, n)) for x in (tip1, tip2, upDown, mode))
        out = np.full(n, -1, dtype=np.int32)
        none, diff = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self._ck(self.lib.maple_debug_update_items(self.h, n, _ptr(l1), _ptr(b1), _ptr(t1), _ptr(l2), _ptr(b2), _ptr(t2), _ptr(ud), _ptr(md),
                                                   _ptr(old), _ptr(out), _ptr(none), _ptr(diff)))
        return out, none.astype(bool), diff.astype(bool)

    def debug_sweep_estimate(self, up_lists, mut_lists, low_lists, tip):
        """One chunk's estimates of the branch-length sweep by the library's own fused kernels (maple_debug_sweep_estimate): the upper
        list passed downwards through the mutation list (-1: none) against the lower list.  Returns (lengths, False flags)."""
        up_lists, mut_lists, low_lists = _i32(up_lists), _i32(mut_lists), _i32(low_lists)
        n = len(up_lists)
        assert len(mut_lists) == n and len(low_lists) == n
        tp = _u8(np.broadcast_to(tip, n))
        t = np.zeros(n)
        f = np.zeros(n, dtype=np.uint8)
        self._ck(self.lib.maple_debug_sweep_estimate(self.h, n, _ptr(up_lists), _ptr(mut_lists), _ptr(low_lists), _ptr(tp), _ptr(t), _ptr(f)))
        return t, f.astype(bool)

    def debug_update_partials_stats(self):
        """The arms the last update_partials took (maple_debug_update_partials_stats): {counter name: count}, the names as the
        library gives them (update_plan.h, UPDATE_PLAN_STATS)."""
        names = self.lib.maple_debug_update_partials_stat_names().decode().split()
        counts = np.zeros(len(names), dtype=np.int64)
        n = C.c_int32()
        self._ck(self.lib.maple_debug_update_partials_stats(self.h, _ptr(counts), len(counts), C.byref(n)))
        assert n.value == len(names), (n.value, names)
        return dict(zip(names, (int(x) for x in counts)))

    def debug_update_partials_visited(self, cap=65536):
        """The nodes the last update_partials visited, with repeats, in order (maple_debug_update_partials_visited)."""
        nodes = np.zeros(cap, dtype=np.int32)
        n = C.c_int32()
        self._ck(self.lib.maple_debug_update_partials_visited(self.h, cap, _ptr(nodes), C.byref(n)))
        return nodes[: n.value].copy()

    def debug_calib_walk(self, nbytes, repeats=1):
        ms = C.c_float()
        self._ck(self.lib.maple_debug_calib_walk(self.h, nbytes, repeats, C.byref(ms)))
        return ms.value

    def debug_calib_write(self, nbytes, mode, repeats=1):
        ms = C.c_float()
        self._ck(self.lib.maple_debug_calib_write(self.h, nbytes, mode, repeats, C.byref(ms)))
        return ms.value

    def debug_trace_query(self, q):
        self._ck(self.lib.maple_debug_trace_query(self.h, q))

    def debug_trace_read(self):
        n = C.c_int32()
        it = np.zeros(4 * 4096, dtype=np.int32)
        va = np.zeros(2 * 4096, dtype=np.float64)
        self._ck(self.lib.maple_debug_trace_read(self.h, C.byref(n), _ptr(it), _ptr(va)))
        k = min(n.value, 4096)
        return it[: 4 * k].reshape(k, 4), va[: 2 * k].reshape(k, 2)

    # -- device-resident forms (pointers into HBM, e.g. torch tensors' data_ptr()) ------------------
    def append_batch_dev(self, n, parent_ptr, child_ptr, tip_ptr, blen_ptr, out_ptr, stream=0):
        self._ck(self.lib.maple_append_batch_dev(self.h, n, parent_ptr, child_ptr, tip_ptr, blen_ptr, out_ptr, stream))

    def append_queries_dev(self, nQ, qlist_ptr, nC, cand_ptr, isTipC, bLen, out_ptr, stream=0):
        self._ck(self.lib.maple_append_queries_dev(self.h, nQ, qlist_ptr, nC, cand_ptr, bool(isTipC), bLen, out_ptr, stream))

    def append_queries_argmax_dev(self, nQ, qlist_ptr, nC, cand_ptr, rank_ptr, isTipC, bLen, best_score_ptr, best_idx_ptr, stream=0):
        self._ck(self.lib.maple_append_queries_argmax_dev(self.h, nQ, qlist_ptr, nC, cand_ptr, rank_ptr, bool(isTipC), bLen,
                                                          best_score_ptr, best_idx_ptr, stream))

    def comm_unique_id(self):
        buf = np.zeros(128, dtype=np.uint8)
        self._ck(self.lib.maple_comm_unique_id(self.h, _ptr(buf)))
        return buf

    def comm_init(self, world, rank, unique_id):
        self._ck(self.lib.maple_comm_init(self.h, world, rank, _ptr(_u8(unique_id))))

    def argmax_allreduce_dev(self, n, score_ptr, idx_ptr, stream=0):
        self._ck(self.lib.maple_argmax_allreduce_dev(self.h, n, score_ptr, idx_ptr, stream))

    def timing_reset(self):
        self._ck(self.lib.maple_timing_reset(self.h))

    def timing_read_each(self, cap=256):
        ms = np.zeros(cap, dtype=np.float32)
        n = C.c_int32()
        self._ck(self.lib.maple_timing_read_each(self.h, cap, _ptr(ms), C.byref(n)))
        return ms[: n.value].tolist()

    def frontier_levels(self, cap=4096):
        """Per level of the last frontier-tier pass: (updating items, cached items, ms of k_fr_updating, ms of k_fr_cached)."""
        iu, ic = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        ws, wb = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        mu, mc = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
        n = C.c_int32()
        self._ck(self.lib.maple_debug_frontier_levels(self.h, cap, _ptr(iu), _ptr(ic), _ptr(mu), _ptr(mc), C.byref(n), _ptr(ws), _ptr(wb)))
        k = min(cap, n.value)
        self.last_wave_items = (ws[:k], wb[:k])      # (of the updating items: walked a wavefront each, small / 512-entry class)
        return iu[:k], ic[:k], mu[:k], mc[:k]

    WAVE_PATHS = ("lane0_no_fit", "lane0_spot_tot_up", "lane0_root")
    WAVE_SLOTS = ("small class", "512 class", "small class, lane 0 (a list does not fit)", "512 class, lane 0 (a list does not fit)",
                  "small class, lane 0 (on-the-spot probVectTotUp)", "512 class, lane 0 (on-the-spot probVectTotUp)",
                  "small class, lane 0 (root item)", "512 class, lane 0 (root item)")

    def frontier_wave_paths(self, cap=64):
        """Of the last frontier-tier pass (maple_debug_frontier_wave_paths): a dict of the items the wavefront-wide kernels handed to
        lane 0, by WAVE_PATHS, and -- from a library built with MAPLE_SPR_PROFILE, else None -- per WAVE_SLOTS (count, total ms, slowest ms) and
        per level (slowest wavefront-wide item's ms, its slot)."""
        counts, slots = np.zeros(3, np.int64), np.zeros(24, np.float64)
        ms, slot = np.zeros(cap, np.float32), np.zeros(cap, np.int32)
        prof = C.c_int32()
        self._ck(self.lib.maple_debug_frontier_wave_paths(self.h, _ptr(counts), cap, _ptr(ms), _ptr(slot), _ptr(slots), C.byref(prof)))
        paths = dict(zip(self.WAVE_PATHS, counts.tolist()))
        if not prof.value:
            return paths, None, None
        return paths, slots.reshape(3, 8).T.copy(), (ms, slot)

    HANDBACK_REASONS = ("other", "merge_within_tolerance", "passed_from_shortened", "fifth_shortened_list", "own_list_shortened",
                        "marked_without_layout", "wide_short_list_or_slots", "wide_scanned_list_shortened")

    def frontier_handbacks(self):
        """Of the last frontier-tier pass (maple_debug_frontier_handbacks): (the searches it handed to the one-lane kernel, a dict
        of those that were given a reason, by HANDBACK_REASONS)."""
        reasons = np.zeros(8, np.int64)
        n = C.c_int64()
        self._ck(self.lib.maple_debug_frontier_handbacks(self.h, _ptr(reasons), C.byref(n)))
        return int(n.value), dict(zip(self.HANDBACK_REASONS, reasons.tolist()))

    def tree_rebuild_lists(self, root, up, c0, c1, tip, mut, dist, lower, bump_len=0.0):
        """reCalculateAllGenomeLists (M:6013-6347) with the level loop inside the library (maple_tree_rebuild_lists): returns
        (lower, upRight, upLeft, totUp, bad) -- new id columns, ``dist`` (float64, contiguous) updated in place when bump_len > 0,
        ``bad`` = nodes whose branches are still inconsistent (empty when the build went through)."""
        n = len(up)
        up, c0, c1 = _i32(up), _i32(c0), _i32(c1)
        tip = np.ascontiguousarray(np.asarray(tip, np.uint8))
        mutp = None if mut is None else _i32(mut)
        assert dist.dtype == np.float64 and dist.flags.c_contiguous
        lower = _i32(lower).copy()
        ur, ul, tu = (np.full(n, -1, np.int32) for _ in range(3))
        bad = np.zeros(max(64, n), np.int32)                  # (every node can be named: nothing is dropped)
        nbad = C.c_int32()
        self._ck(self.lib.maple_tree_rebuild_lists(self.h, n, root, _ptr(up), _ptr(c0), _ptr(c1), _ptr(tip), _ptr(mutp), _ptr(dist),
                                                   _ptr(lower), _ptr(ur), _ptr(ul), _ptr(tu), bump_len, len(bad), _ptr(bad),
                                                   C.byref(nbad)))
        return lower, ur, ul, tu, np.unique(bad[: min(nbad.value, len(bad))])

    def em_expectation(self, n_minor=None):
        """The expectation part of one EM step on the uploaded tree (maple_em_expectation; the statistics of M:10113-10136 as
        they stand at M:10852): a dict with counts [4][4], waitingTimes [4], errorCount, totTreeLength, observedTotNucsSites, numTips
        and the per-site tables waitingTimesSites [lRef][4], countsSites, trackingNs, observedNucsSites, errorCountSites (zeros
        where the current model has none).  n_minor[v] = len(minorSequences[v]), None = all 0."""
        L = self.lRef
        nm = None if n_minor is None else _i32(n_minor)
        tot = MapleEmTotals()
        wts, cs, tn, on, ecs = np.zeros(4 * L), np.zeros(L), np.zeros(L + 1), np.zeros(L + 1), np.zeros(L)
        self._ck(self.lib.maple_em_expectation(self.h, _ptr(nm), C.byref(tot), _ptr(wts), _ptr(cs), _ptr(tn), _ptr(on), _ptr(ecs)))
        return dict(counts=np.array(tot.counts).reshape(4, 4), waitingTimes=np.array(tot.waitingTimes), errorCount=tot.errorCount,
                    totTreeLength=tot.totTreeLength, observedTotNucsSites=int(tot.observedTotNucsSites), numTips=int(tot.numTips),
                    waitingTimesSites=wts.reshape(L, 4), countsSites=cs, trackingNs=tn, observedNucsSites=on, errorCountSites=ecs)

    def em_rates(self, n_minor=None, model="UNREST"):
        """One whole EM step on the uploaded tree (maple_em_rates, M:10077-10947): (Q [4][4], siteRates or None, errorRate or None,
        siteErrRates or None) for the model of the last set_model.  model: "UNREST" / "GTR" (another name is an error unless the
        current model has error rates, as at M:10877)."""
        L = self.lRef
        nm = None if n_minor is None else _i32(n_minor)
        code = model if isinstance(model, int) else EM_MODELS.get(model, 2)
        Q = np.zeros(16)
        sr = np.zeros(L) if getattr(self, "rv", False) else None
        se = np.zeros(L) if getattr(self, "ss", False) else None
        er = C.c_double()
        self._ck(self.lib.maple_em_rates(self.h, _ptr(nm), code, _ptr(Q), _ptr(sr), C.byref(er), _ptr(se)))
        return Q.reshape(4, 4), sr, (er.value if self.u else None), se

    def tree_log_lk(self, n_minor=None, per_node=False):
        """calculateTreeLikelihood (M:9721-9779) on the uploaded tree inside the library (maple_tree_log_lk): (totalLK, rootLK), with
        per_node also the contribution of every internal node (float64 [n]; 0.0 for leaves and unreachable slots).
        n_minor[v] = len(minorSequences[v]), None = all 0."""
        nm = None if n_minor is None else _i32(n_minor)
        n = getattr(self, "n_nodes", 0)                      # (0: no tree yet, the library says so)
        if nm is not None and n and len(nm) != n:
            raise MapleError(f"n_minor has {len(nm)} entries, the uploaded tree {n} nodes", MapleError.ERR_ARG)
        total, root = C.c_double(), C.c_double()
        node = np.zeros(n) if per_node and n else None
        self._ck(self.lib.maple_tree_log_lk(self.h, _ptr(nm), C.byref(total), C.byref(root), _ptr(node)))
        return (total.value, root.value, node) if per_node else (total.value, root.value)

    def tree_error_probs(self, n_minor, min_error_prob, cap_leaves, cap):
        """One maple_tree_error_probs call with the capacities as given (cap = 0: counted only): (status, leaf_nodes int32
        [cap_leaves], off int64 [cap_leaves + 1], nLeaves, pos int32 [cap], allele uint8 [cap], prob float64 [cap], nRecords).  Nothing
        is raised: the status is the library's, the message Device.last_error()."""
        nm = None if n_minor is None else _i32(n_minor)
        n = getattr(self, "n_nodes", 0)
        if nm is not None and n and len(nm) != n:
            raise MapleError(f"n_minor has {len(nm)} entries, the uploaded tree {n} nodes", MapleError.ERR_ARG)
        leaf, off = np.full(cap_leaves, -1, np.int32), np.zeros(cap_leaves + 1, np.int64)
        pos, al, pr = ((np.zeros(cap, np.int32), np.zeros(cap, np.uint8), np.zeros(cap)) if cap > 0 else (None, None, None))
        n_leaves, n_rec = C.c_int32(), C.c_int64()
        rc = self.lib.maple_tree_error_probs(self.h, _ptr(nm), float(min_error_prob), int(cap_leaves), _ptr(leaf), _ptr(off),
                                             C.byref(n_leaves), int(cap), _ptr(pos), _ptr(al), _ptr(pr), C.byref(n_rec))
        return rc, leaf, off, n_leaves.value, pos, al, pr, n_rec.value

    def last_error(self):
        msg = self.lib.maple_last_error(self.h)
        return msg.decode() if msg else ""

    def error_probabilities(self, n_minor=None, min_error_prob=0.01):
        """calculateErrorProbabilities (M:9783-10020) on the uploaded tree inside the library (maple_tree_error_probs), as arrays:
        (leaf_nodes int32 [nLeaves] in the reference's order, off int64 [nLeaves + 1], pos int32, allele uint8, prob float64) --
        the records of leaf k are [off[k], off[k + 1]): the 1-based position, the index into allelesList or 4 for "X", and the
        posterior probability of a sequencing error, kept where it is >= min_error_prob.  A counting call, then the full one.
        n_minor[v] = len(minorSequences[v]), None = all 0."""
        n = getattr(self, "n_nodes", 0)                      # (0: no tree yet, the library says so)
        rc, _, _, n_leaves, _, _, _, n_rec = self.tree_error_probs(n_minor, min_error_prob, n, 0)
        self._ck(rc)
        rc, leaf, off, n_leaves, pos, al, pr, n_rec = self.tree_error_probs(n_minor, min_error_prob, n_leaves, n_rec)
        self._ck(rc)
        empty = (np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0))
        return (leaf, off) + (empty if pos is None else (pos, al, pr))

    def tree_mutation_events(self, n_minor, min_mut_prob, cap_mut, cap_ns, cap_err):
        """One maple_tree_mutation_events call with the capacities as given (all 0: counted only): (status, mutOff, nsOff, errOff
        int64 [n + 1], mut MUT_EVENT_DTYPE [cap_mut], ns N_RUN_DTYPE [cap_ns], err MUT_EVENT_DTYPE [cap_err], nRecords int64 [3]);
        an array of capacity 0 is None.  Nothing is raised: the status is the library's, the message Device.last_error()."""
        nm = None if n_minor is None else _i32(n_minor)
        n = getattr(self, "n_nodes", 0)
        if nm is not None and n and len(nm) != n:
            raise MapleError(f"n_minor has {len(nm)} entries, the uploaded tree {n} nodes", MapleError.ERR_ARG)
        offs = [np.zeros(n + 1, np.int64) for _ in range(3)]
        mut = np.zeros(cap_mut, MUT_EVENT_DTYPE) if cap_mut > 0 else None
        ns = np.zeros(cap_ns, N_RUN_DTYPE) if cap_ns > 0 else None
        err = np.zeros(cap_err, MUT_EVENT_DTYPE) if cap_err > 0 else None
        n_rec = np.zeros(3, np.int64)
        rc = self.lib.maple_tree_mutation_events(self.h, _ptr(nm), float(min_mut_prob), _ptr(offs[0]), _ptr(offs[1]), _ptr(offs[2]),
                                                 int(cap_mut), _ptr(mut), int(cap_ns), _ptr(ns), int(cap_err), _ptr(err), _ptr(n_rec))
        return rc, offs[0], offs[1], offs[2], mut, ns, err, n_rec

    def mutation_events(self, n_minor=None, min_mut_prob=0.01):
        """The records expectationMaximizationCalculationRates(tree, root, trackMutations=True) leaves on the nodes (M:10077-10850,
        --estimateMAT) for the uploaded tree, inside the library (maple_tree_mutation_events), as arrays: (mutOff, nsOff, errOff,
        mut, ns, err) -- node v's records are [off[v], off[v + 1]) of its stream; mut / err: MUT_EVENT_DTYPE (pos 1-based, from / to
        indices into allelesListExt, prob kept where > min_mut_prob), ns: N_RUN_DTYPE (last == 0: the reference's bare int).  A
        counting call, then the full one.  n_minor[v] = len(minorSequences[v]), None = all 0."""
        rc, _, _, _, _, _, _, n_rec = self.tree_mutation_events(n_minor, min_mut_prob, 0, 0, 0)
        self._ck(rc)
        rc, mo, no, eo, mut, ns, err, _ = self.tree_mutation_events(n_minor, min_mut_prob, *(int(x) for x in n_rec))
        self._ck(rc)
        return (mo, no, eo, np.zeros(0, MUT_EVENT_DTYPE) if mut is None else mut, np.zeros(0, N_RUN_DTYPE) if ns is None else ns,
                np.zeros(0, MUT_EVENT_DTYPE) if err is None else err)

    def tree_find_best_root(self, n_minor=None, *, strictTopologyStopRules, allowedFailsTopology, thresholdLogLKtopology,
                            thresholdLogLKoptimizationTopology, thresholdLogLKconsecutivePlacement, cap_best=None, struct_size=None):
        """The search of findBestRoot (M:7730-7848) on the uploaded tree inside the library (maple_tree_find_best_root):
        (bestNode, bestLKdiff, nodesVisited, branchScore [n] float64 with NaN where no rooting was scored, bestNodes int32 [k],
        bestScores float64 [k], nBest) -- the reference's bestNodes dict in insertion order, k = min(nBest, cap_best);
        cap_best None = room for every node.  n_minor[v] = len(minorSequences[v]), None = all 0.  struct_size: what the params
        struct claims as its size (None: its real size)."""
        nm = None if n_minor is None else _i32(n_minor)
        n = getattr(self, "n_nodes", 0)                      # (0: no tree yet, the library says so)
        if nm is not None and n and len(nm) != n:
            raise MapleError(f"n_minor has {len(nm)} entries, the uploaded tree {n} nodes", MapleError.ERR_ARG)
        p = MapleRootSearchParams(C.sizeof(MapleRootSearchParams) if struct_size is None else struct_size, int(bool(strictTopologyStopRules)),
                                  int(min(max(allowedFailsTopology, -(1 << 31)), (1 << 31) - 1)), thresholdLogLKtopology,
                                  thresholdLogLKoptimizationTopology, thresholdLogLKconsecutivePlacement)
        cap = n if cap_best is None else int(cap_best)
        best, visited, n_best, diff = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
        score = np.full(n, np.nan) if n else None
        nodes = np.zeros(cap, np.int32) if cap > 0 else None
        scores = np.zeros(cap) if cap > 0 else None
        self._ck(self.lib.maple_tree_find_best_root(self.h, _ptr(nm), C.byref(p), C.byref(best), C.byref(diff), C.byref(visited),
                                                    _ptr(score), cap, _ptr(nodes), _ptr(scores), C.byref(n_best)))
        k = min(cap, n_best.value)
        return (best.value, diff.value, visited.value, score, np.zeros(0, np.int32) if nodes is None else nodes[:k],
                np.zeros(0) if scores is None else scores[:k], n_best.value)

    def timing_read(self):
        """(number of timed *_dev launches since the last reset, their summed HIP-event time in ms)."""
        n, ms = C.c_int32(), C.c_double()
        self._ck(self.lib.maple_timing_read(self.h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    KIND_SPR_SCORE, KIND_SPR_SEARCH, KIND_SPR_REPLAY, KIND_APPEND_QUERIES, KIND_APPEND_PAIRS, KIND_PLACE_SCORE = 1, 2, 3, 4, 5, 6
    KIND_FR_UPDATING, KIND_FR_CACHED, KIND_FR_REPLAY, KIND_FR_WIDE = 7, 8, 9, 10

    def timing_read_kind(self, kind):
        """(launches, summed HIP-event ms, units of work, algorithmic bytes) of one kind of timed launch since the reset."""
        n, ms, u, b = C.c_int32(), C.c_double(), C.c_double(), C.c_double()
        self._ck(self.lib.maple_timing_read_kind(self.h, kind, C.byref(n), C.byref(ms), C.byref(u), C.byref(b)))
        return n.value, ms.value, u.value, b.value

    def append_algorithmic_bytes(self, parent, child=None, child_once=False):
        parent = _i32(parent)
        ch = None if child is None else _i32(child)
        b = C.c_uint64()
        self._ck(self.lib.maple_append_algorithmic_bytes(self.h, len(parent), _ptr(parent), _ptr(ch),
                                                         bool(child_once), C.byref(b)))
        return b.value
