"""Host-side mirror of the reference's operator interface for the placement path.

Same names, argument meaning and return conventions as the top-level functions
of MAPLEv0.7.5.4.py that the search loops call:
``None`` for an impossible merge (M:4758), ``-inf`` for an impossible
attachment (M:6663), ``False`` for a zero branch length (M:5301).  Every call
goes through the C ABI into the HIP kernels; the ``*_many`` forms are the
batched shape the searches actually use (thousands of candidates per launch).
"""
from __future__ import annotations

import numpy as np

from .runtime import Device


class GenomeOps:
    def __init__(self, dev: Device):
        self.dev = dev

    # ---- scoring --------------------------------------------------------------------------
    def appendProbNode(self, probVectP, probVectC, isTipC, bLen):
        """M:6505-6785."""
        return self.appendProbNode_many([probVectP], [probVectC], [isTipC], [bLen])[0]

    def appendProbNode_many(self, parents, children, isTipC, bLen):
        d = self.dev
        mark = d.mark()
        try:
            ids = d.upload(list(parents) + list(children))
            n = len(parents)
            out = d.append_batch(ids[:n], ids[n:], np.asarray(isTipC, dtype=bool), np.asarray(bLen, dtype=float))
        finally:
            d.release(mark)
        return [float(x) for x in out]

    # ---- merging ----------------------------------------------------------------------------
    def mergeVectors(self, probVect1, bLen1, fromTip1, probVect2, bLen2, fromTip2, returnLK=False, isUpDown=False,
                     numMinor1=0, numMinor2=0):
        """M:4446-4859 (isUpDown=True is the up-down merge)."""
        d = self.dev
        mark = d.mark()
        try:
            ids = d.upload([probVect1, probVect2])
            res = d.merge_batch(ids[:1], [bLen1 or 0.0], [fromTip1], ids[1:], [bLen2 or 0.0], [fromTip2], [isUpDown],
                                returnLK=returnLK, numMinor1=[numMinor1], numMinor2=[numMinor2])
            if returnLK:
                out, lk = res
                return d.download(out)[0], float(lk[0])
            return d.download(res)[0]
        finally:
            d.release(mark)

    def estimateBranchLengthWithDerivative(self, probVectP, probVectC, fromTipC=False):
        """M:5040-5358."""
        d = self.dev
        mark = d.mark()
        try:
            ids = d.upload([probVectP, probVectC])
            t, f = d.blen_batch(ids[:1], ids[1:], [fromTipC])
        finally:
            d.release(mark)
        return False if f[0] else float(t[0])

    def areVectorsDifferent(self, probVect1, probVect2):
        """M:5419-5472."""
        if probVect2 is None:
            return True
        d = self.dev
        mark = d.mark()
        try:
            ids = d.upload([probVect1, probVect2])
            return bool(d.differ_batch(ids[:1], ids[1:])[0])
        finally:
            d.release(mark)

    def passGenomeListThroughBranch(self, probVect, mutations, dirIsUp=False):
        """M:3749-3877."""
        d = self.dev
        mark = d.mark()
        try:
            ids = d.upload([probVect])
            mids = d.upload_mutations([mutations])
            return d.download(d.pass_branch_batch(ids, mids, [dirIsUp]))[0]
        finally:
            d.release(mark)

    def shorten(self, vec):
        """M:3721-3745.  Returns the shortened list (the reference edits in place)."""
        d = self.dev
        mark = d.mark()
        try:
            return d.download(d.shorten_batch(d.upload([vec])))[0]
        finally:
            d.release(mark)

    def rootVector(self, probVect, bLen, isFromTip, pathMutations):
        """M:4916-4996; ``pathMutations`` = tree.mutations[] on the walk node -> root (node first)."""
        d = self.dev
        mark = d.mark()
        try:
            ids = d.upload([probVect])
            mids = d.upload_mutations(pathMutations)
            return d.download(d.root_vector_batch(ids, [bLen or 0.0], [isFromTip], [mids]))[0]
        finally:
            d.release(mark)

    def evaluatePlacement(self, midTot, downVect, upVect, distance, removedPartials, isRemovedTip, fromTip1):
        """M:6790-6806 -> (appendingCost, bestBottomLength, bestTopLength, bestAppendingLength)."""
        d = self.dev
        mark = d.mark()
        try:
            ids = d.upload([midTot, downVect, upVect, removedPartials])
            out = d.evaluate_placement_batch(ids[0:1], ids[1:2], ids[2:3], [distance], ids[3:4], [isRemovedTip],
                                             [fromTip1])
        finally:
            d.release(mark)
        return tuple(float(x) for x in out[0])


ERROR_REPORT_ALLELES = ("A", "C", "G", "T", "X")                         # allelesList, then the reference's "X" (code 4)


def format_error_report(leaf_nodes, off, pos, allele, prob, minor_ids, node_name, names_in_tree):
    """The text calculateErrorProbabilities writes (M:9804-9807, 9873 and its kin) for the arrays of
    Device.error_probabilities: per leaf ``>name``; for a leaf with minor sequences their ``>name`` lines (minor_ids[v] = the ids
    of minorSequences[v]); otherwise one ``pos\\tallele\\tprob`` line per record, prob as Python's str(float).  node_name[v] =
    name[v], the index of v's own name in names_in_tree."""
    off = np.asarray(off).tolist()
    pos, allele, prob = np.asarray(pos).tolist(), np.asarray(allele).tolist(), np.asarray(prob, dtype=np.float64).tolist()
    out = []
    for k, v in enumerate(np.asarray(leaf_nodes).tolist()):
        out.append(">" + names_in_tree[node_name[v]] + "\n")
        if len(minor_ids[v]) > 0:
            out.extend(">" + names_in_tree[i] + "\n" for i in minor_ids[v])
        else:
            out.extend(str(pos[i]) + "\t" + ERROR_REPORT_ALLELES[allele[i]] + "\t" + str(prob[i]) + "\n" for i in range(off[k], off[k + 1]))
    return "".join(out)


MAT_ALLELES = ("A", "C", "G", "T", "?")                                    # allelesListExt (M:3661)


def format_root_state(root_vect, min_mut_prob):
    """The root's ``rootState={...}`` of stringForNode (M:2750-2781) from rootVector(probVect[root], False, isTip, ...) as a list
    of the reference's tuples (GenomeOps.rootVector / Device.download): an N run as ``N<first>-<last>``, a nucleotide as
    ``<allele><pos>:1.0``, an O entry as its alleles with a value above min_mut_prob, values as Python's str(float)."""
    out, pos, first = "rootState={", 0, True
    for e in root_vect:
        if e[0] != 4:
            if not first:
                out += ","
            first = False
        if e[0] == 5:
            out += "N" + str(pos + 1) + "-" + str(e[1])
            pos = e[1]
        elif e[0] == 6:
            out += ",".join(MAT_ALLELES[i] + str(pos + 1) + ":" + str(float(e[-1][i])) for i in range(4) if e[-1][i] > min_mut_prob)
            pos += 1
        elif e[0] < 4:
            out += MAT_ALLELES[e[0]] + str(pos + 1) + ":1.0"
            pos += 1
        else:
            pos = e[1]
    return out + "}"


def format_mat_annotation(mut_off, ns_off, err_off, mut, ns, err, *, root, up, children, dist, errors_on, effectivelyNon0BLen,
                          supportFor0Branches=False, root_state=None):
    """Per node, what the reference's stringForNode(tree, v, "", dist[v], estimateMAT=True, networkOutput=False,
    aBayesPlusOn=False) returns (M:2673-2809) for the arrays of Device.mutation_events: the
    ``[&mutationsInf={A123C:0.98,...},Ns={5,10-20},errors={...}]`` block under the conditions of M:2706 and M:2719 (a non-root node
    whose dist is above effectivelyNon0BLen, or supportFor0Branches, or an error model -- errors_on; then dist non-zero, or an error
    model, or a leaf), the root's ``[&rootState={...}]`` (root_state: format_root_state's text, None: left out), the empty string
    where the reference writes nothing and for slots the root does not reach.  Probabilities go through Python's str(float)."""
    mut_off, ns_off, err_off = (np.asarray(x).tolist() for x in (mut_off, ns_off, err_off))

    def events(a, lo, hi):
        pos, fr, to, pr = a["pos"][lo:hi].tolist(), a["from"][lo:hi].tolist(), a["to"][lo:hi].tolist(), a["prob"][lo:hi].tolist()
        return ",".join(MAT_ALLELES[f] + str(p) + MAT_ALLELES[t] + ":" + str(x) for p, f, t, x in zip(pos, fr, to, pr))

    out = []
    for v in range(len(up)):
        strings = []
        d = dist[v] or 0.0
        if up[v] is not None and up[v] >= 0:
            if (d > effectivelyNon0BLen or supportFor0Branches or errors_on) and (d or errors_on or not len(children[v])):
                if mut_off[v + 1] > mut_off[v]:
                    strings.append("mutationsInf={" + events(mut, mut_off[v], mut_off[v + 1]) + "}")
                if ns_off[v + 1] > ns_off[v]:
                    first, last = ns["first"][ns_off[v]:ns_off[v + 1]].tolist(), ns["last"][ns_off[v]:ns_off[v + 1]].tolist()
                    strings.append("Ns={" + ",".join(str(a) if b == 0 else str(a) + "-" + str(b) for a, b in zip(first, last)) + "}")
                if errors_on and not len(children[v]) and err_off[v + 1] > err_off[v]:
                    strings.append("errors={" + events(err, err_off[v], err_off[v + 1]) + "}")
        elif v == root and root_state is not None:               # (another slot without a parent is one the root does not reach)
            strings.append(root_state)
        out.append("[&" + ",".join(strings) + "]" if strings else "")
    return out


class TreeOps:
    """The tree-level functions of the path under the reference's own names, on a ``HostTree`` whose lists live in the
    device arena (``tree.upload(dev)`` or ``HostTree.from_mirror``).  Thin delegation: the work is in
    ``maple_spr_search_batch`` / ``maple_placement_search_batch`` and the level-synchronous batches of ``tree_host``."""

    def __init__(self, dev: Device, tree):
        self.dev, self.tree = dev, tree
        self._searcher = None
        self._searcher_key = None

    def upload_topology(self):
        """(Re)send the topology and list ids after the host changed the tree (maple_tree_upload)."""
        self.tree.upload_topology(self.dev)
        self._searcher = None

    # M:7912 -- returns (bestNode, bestScore, bestBranchLengths, bestDiffs) like the reference; with
    # computePlacementSupportOnly=True (possiblePlacements, bestPlacementTotalLh), M:8264-8290
    def findBestParentForNewSample(self, diffs, *, oneMutBLen, effectivelyNon0BLen, thresholdLogLK, thresholdLogLKoptimization,
                                   thresholdLogLKconsecutivePlacement, allowedFails=5, strictStopRules=True,
                                   onlyFindIdentical=False, computePlacementSupportOnly=False,
                                   thresholdLogLKoptimizationTopology=None, minBranchSupport=0.01):
        from .search import PlacementParams, PlacementSearcher
        key = (oneMutBLen, effectivelyNon0BLen, thresholdLogLK, thresholdLogLKoptimization,
               thresholdLogLKconsecutivePlacement, allowedFails, strictStopRules, onlyFindIdentical)
        if self._searcher is None or self._searcher_key != key:
            self._searcher = PlacementSearcher(self.dev, self.tree, PlacementParams(
                oneMutBLen=oneMutBLen, effectivelyNon0BLen=effectivelyNon0BLen, thresholdLogLK=thresholdLogLK,
                thresholdLogLKoptimization=thresholdLogLKoptimization,
                thresholdLogLKconsecutivePlacement=thresholdLogLKconsecutivePlacement, allowedFails=allowedFails,
                strictStopRules=strictStopRules, onlyFindIdentical=onlyFindIdentical))
            self._searcher_key = key
        if computePlacementSupportOnly:
            thr = thresholdLogLKoptimization if thresholdLogLKoptimizationTopology is None else thresholdLogLKoptimizationTopology
            return self._searcher.find_placement_supports([diffs], thr, minBranchSupport)[0]
        return self._searcher.find_best_parent_for_new_sample(diffs)[:4]

    # M:9580 -- the worker body for `nodes`; returns the list of (node, placement, improvement) the reference's worker returns
    def startTopologyUpdatesParallel(self, nodes, *, strictTopologyStopRules, allowedFailsTopology, thresholdLogLKtopology,
                                     thresholdTopologyPlacement, thresholdLogLKoptimizationTopology,
                                     thresholdLogLKconsecutivePlacement, effectivelyNon0BLen):
        res = self.dev.spr_search_batch(nodes, strict=strictTopologyStopRules, allowedFails=allowedFailsTopology,
                                        thresholdLogLKtopology=thresholdLogLKtopology,
                                        thresholdTopologyPlacement=thresholdTopologyPlacement,
                                        thresholdLogLKoptimizationTopology=thresholdLogLKoptimizationTopology,
                                        thresholdLogLKconsecutivePlacement=thresholdLogLKconsecutivePlacement,
                                        effectivelyNon0BLen=effectivelyNon0BLen)
        bad = res["status"][res["status"] < -1]
        if len(bad):      # -1 is the reference's swallowed exception (M:9703); anything below is a capacity problem, not "no move"
            raise RuntimeError(f"SPR search could not finish some queries (status {sorted(set(bad.tolist()))}: workspace, "
                               "removed-partials pool or short-list capacity)")
        return [(int(n), int(p), float(i)) for n, p, i in zip(nodes, res["placement"], res["improvement"]) if p >= 0]

    def reCalculateAllGenomeLists(self):                                   # M:6013
        from .tree_host import rebuild_genome_lists
        t = self.tree
        t.id_lower, t.id_upRight, t.id_upLeft, t.id_totUp = rebuild_genome_lists(self.dev, t)

    def sync(self):
        """After a LOCAL change (one placed sample + updatePartials): only the touched nodes go to the library
        (maple_tree_patch); falls back to upload_topology when that is not possible.  Returns the number of patched nodes."""
        n = self.tree.sync(self.dev)
        if self._searcher is not None:
            if n == -1 or self._searcher.world != 1:
                self._searcher = None                                  # (its candidate shards describe the old tree)
            else:
                self._searcher._prepared = False                       # the root vector may have changed: prepare again
        return n

    def updatePartials(self, changed_nodes):                               # M:5479 (level-synchronous, any number of changes)
        from .tree_host import update_genome_lists
        return update_genome_lists(self.dev, self.tree, list(changed_nodes))

    def calculateTreeLikelihood(self):                                     # M:9721
        from .tree_host import tree_log_likelihood
        return tree_log_likelihood(self.dev, self.tree)[0]

    def expectationMaximizationCalculationRates(self, model="UNREST"):     # M:10077 (trackMutations=False)
        from .tree_host import estimate_rates
        return estimate_rates(self.dev, self.tree, model)

    # M:9783 -- the reference's (tree, root, file, minErrorProb, namesInTree) with tree and root this object's; the names the
    # reference reads off its tree are arguments here (HostTree keeps counts, not names): name[v] (None: v itself) and
    # minorSequences[v], the ids of v's minor sequences (None: allowed when no leaf has any)
    def calculateErrorProbabilities(self, file, minErrorProb, namesInTree, name=None, minorSequences=None):
        t = self.tree
        if minorSequences is None:
            if any(t.n_minor):
                raise ValueError("the tree has minor sequences: calculateErrorProbabilities needs their ids (minorSequences)")
            minorSequences = [()] * t.n
        if any(len(m) != k for m, k in zip(minorSequences, t.n_minor)):
            raise ValueError("minorSequences does not have the tree's n_minor entries per node")
        res = self.dev.error_probabilities(t.n_minor if any(t.n_minor) else None, minErrorProb)
        file.write(format_error_report(*res, minorSequences, range(t.n) if name is None else name, namesInTree))

    # --estimateMAT (M:12529-12532, 12601-12606): expectationMaximizationCalculationRates(tree, root, trackMutations=True) and then,
    # per node, the annotation stringForNode writes into the Nexus tree; minMutProb is the reference's global of that name
    def estimateMAT(self, minMutProb, effectivelyNon0BLen, supportFor0Branches=False):
        t, d = self.tree, self.dev
        res = d.mutation_events(t.n_minor if any(t.n_minor) else None, minMutProb)
        root = t.root
        mark = d.mark()
        try:                                                             # rootVector(probVect[root], False, isTip, tree, root), M:2754
            is_tip = len(t.children[root]) == 0 and t.n_minor[root] == 0
            path = [int(t.id_mut[root])] if t.id_mut[root] >= 0 else []
            root_vect = d.download(d.root_vector_batch([int(t.id_lower[root])], [0.0], [is_tip], [path]))[0]
        finally:
            d.release(mark)
        return format_mat_annotation(*res, root=root, up=t.up, children=t.children, dist=t.dist, errors_on=bool(d.u),
                                     effectivelyNon0BLen=effectivelyNon0BLen, supportFor0Branches=supportFor0Branches,
                                     root_state=format_root_state(root_vect, minMutProb))

    def traverseTreeToOptimizeBranchLengths(self, effectivelyNon0BLen, fastPass=False):  # M:8727 (default: the Gauss-Seidel sweep)
        from .tree_host import optimize_branch_lengths, optimize_branch_lengths_fast_pass
        if fastPass:
            return optimize_branch_lengths_fast_pass(self.dev, self.tree, effectivelyNon0BLen)[0]
        return optimize_branch_lengths(self.dev, self.tree, effectivelyNon0BLen)[0]

    def findBestRoot(self, **kw):                                          # M:7730 (the search; re-rooting stays with the caller)
        from .tree_host import find_best_root
        return find_best_root(self.dev, self.tree, **kw)
