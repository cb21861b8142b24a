"""The wavefront-wide kernels of the frontier tier's updating levels (k_fr_updating_wave_s / k_fr_updating_wave,
maple_amd/csrc/fr_wave_items_body.inc): items are dealt to the wavefronts by ticket, and the three kinds of item a wavefront still
hands whole to its lane 0 are counted per call (maple_debug_frontier_wave_paths).

The 400-tip divergent tree of test_hip_scale.test_frontier_wavefront_size_classes_are_both_used_and_equal_the_lane_forms, every
level by wavefronts (wave_all_below = 1 << 30), against a lane per item (wave_all_below = -1) and against the one-lane-per-search
kernels (search_tier = 1): the same searches field by field.  The two references are computed once per model and tree form.

The on-the-spot probVectTotUp items and the root items stay one-lane paths (the headline tree has none of either among its
wavefront-wide items: profiles/late_levels_before.txt), so what is asserted about them is that they OCCUR on these trees and are
counted, and that the searches are the same with them."""
import numpy as np
import pytest

from test_hip_scale import world_model_kwargs

pytestmark = pytest.mark.gpu

FIELDS = ("status", "bestNode", "placement", "nAppend", "bestScore", "currentLK", "improvement", "blen")
WAVES_SMALL, WAVES_BIG = 1280, 256       # wavefronts of the two kernels (search_plan.h: gridWaveSmall, gridWave)


class World:
    """The tree on a device in its two forms, with the lane-form references of every (form, batch) asked for, made once."""

    def __init__(self, mode, zero_root_child=False):
        import bench
        from maple_amd.host import reference_tables, tip_genome_list
        from maple_amd.runtime import Device
        from maple_amd.synth import make_dataset
        from maple_amd.tree_host import HostTree
        from maple_amd.tree_mirror import TreeMirror
        data = make_dataset(n_samples=400, l_ref=29903, seed=9, mean_diffs=60.0, frac_with_n=0.1, frac_ambig=0.05)
        ref_idx, rf = reference_tables(data.ref)
        self.mode = mode
        mkw = world_model_kwargs(mode, len(ref_idx), 9)
        self.dev = dev = Device(ref_idx, rf, arena_bytes=1 << 30, debug=True)
        dev.set_model(**mkw)
        tip_kw = dict(error_rates=mkw["errorRates"]) if mode == "siteerr" else {}
        tips = {int(v): tip_genome_list(dl, ref_idx, **tip_kw) for v, dl in zip(data.tip_node, data.diffs)}
        blen = np.array(data.blen, dtype=np.float64)
        self.zeroed = -1
        if zero_root_child:
            # a child of the root on a zero-length branch has no probVectTotUp: an item that crawls up to it merges one on the spot
            parent = np.asarray(data.parent)
            root = int(np.flatnonzero(parent < 0)[0])
            inner = [int(v) for v in np.flatnonzero(parent == root) if int(v) not in tips]
            assert inner
            self.zeroed = inner[0]
            blen[self.zeroed] = 0.0
        self.m = m = TreeMirror(dev, data.parent, blen, tips).build()
        if zero_root_child:
            assert m.tot_up[self.zeroed] == -1 and m.parent[self.zeroed] == m.root
        self.kw = bench.search_kwargs(dev.lRef)
        self.nodes = bench.preorder_nodes(m)
        self.ht = HostTree.from_mirror(m)
        self.form, self.with_refs = None, False
        self.refs = {}

    def upload(self, form):
        from maple_amd.mat import add_local_references
        m, ht, dev = self.m, self.ht, self.dev
        if form == self.form:
            return
        if form == "plain":                                         # (its lists stay in the arena: it can come back)
            dev.upload_tree(m.root, m.parent, m.children[:, 0], m.children[:, 1], m.dist, m.is_tip, m.lower, m.up_right, m.up_left, m.tot_up,
                            -np.ones(m.n_nodes, dtype=np.int32))
        else:
            if not self.with_refs:                                  # (the references are added to the host tree once)
                assert add_local_references(dev, ht, 40) > 0
                self.with_refs = True
            dist = np.asarray([float(x or 0.0) for x in ht.dist])
            dev.upload_tree(ht.root, m.parent, m.children[:, 0], m.children[:, 1], dist, m.is_tip, ht.id_lower, ht.id_upRight, ht.id_upLeft,
                            ht.id_totUp, ht.id_mut)
        self.form = form

    def search(self, nodes, wave_all_below=0, **kw):
        self.dev.set_tuning(wave_all_below=wave_all_below)
        try:
            return self.dev.spr_search_batch(np.asarray(nodes, dtype=np.int32), wide_search_budget=-1, **dict(self.kw, **kw))
        finally:
            self.dev.set_tuning()

    def references(self, form):
        """(a lane per item, the one-lane-per-search kernels) for every node of the pre-order on the tree in this form"""
        self.upload(form)
        if form not in self.refs:
            self.refs[form] = (self.search(self.nodes, wave_all_below=-1), self.search(self.nodes, search_tier=1))
        return self.refs[form]

    def close(self):
        self.dev.close()


@pytest.fixture(scope="module", params=["ratevar", "siteerr"])
def world(request):
    w = World(request.param)
    yield w
    w.close()


def same(got, want, what):
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]), (what, k, int((np.asarray(got[k]) != np.asarray(want[k])).sum()))


def check_every_node(w, form):
    by_lane_items, by_lane_searches = w.references(form)
    got = w.search(w.nodes, wave_all_below=1 << 30)
    paths, _, _ = w.dev.frontier_wave_paths()
    same(got, by_lane_items, (form, "a lane per item"))
    same(got, by_lane_searches, (form, "one lane per search"))
    assert (got["status"] == 0).any()
    return paths


def test_every_level_by_wavefronts_equals_the_lane_forms_and_counts_its_one_lane_items(world):
    spot = root = 0
    for form in ("plain", "local references"):
        paths = check_every_node(world, form)
        print(f"{form}: items handed to lane 0 by the wavefront-wide kernels: {paths}")
        assert set(paths) == {"lane0_no_fit", "lane0_spot_tot_up", "lane0_root"} and min(paths.values()) >= 0
        spot += paths["lane0_spot_tot_up"]
        root += paths["lane0_root"]
    assert root > 0, "no root item among the wavefront-wide items"
    if spot == 0:
        # the tree as made has a probVectTotUp on every branch next to the root: the same tree with one root child on a
        # zero-length branch (the CPU mirror says tot_up = -1 there)
        z = World(world.mode, zero_root_child=True)
        try:
            for form in ("plain", "local references"):
                paths = check_every_node(z, form)
                print(f"{form}, zero-length branch above node {z.zeroed}: {paths}")
                spot += paths["lane0_spot_tot_up"]
        finally:
            z.close()
    assert spot > 0, "no on-the-spot probVectTotUp item among the wavefront-wide items"


def test_a_handful_of_searches_next_to_the_root(world):
    """m <= 64: heavyMin = 1, every item goes by wavefronts (search_plan.h), and the searches start where the lists are longest."""
    m = world.m
    near = {int(c) for c in m.children[m.root] if c >= 0}
    near |= {int(g) for c in list(near) for g in m.children[c] if g >= 0}
    batch = [int(v) for v in world.nodes if int(m.parent[v]) in near][:8]
    assert len(batch) == 8
    for form in ("plain", "local references"):
        world.upload(form)
        got = world.search(batch)
        same(got, world.search(batch, search_tier=1), (form, "8 searches"))
        iu, _, _, _ = world.dev.frontier_levels()
        ws, wb = world.dev.last_wave_items
        # (seeds of a search whose parent is the root are dir-3 items, which no wavefront takes)
        assert iu.sum() > 0 and int(ws.sum() + wb.sum()) > 0


def test_items_are_dealt_once_each_whatever_the_level_holds(world):
    """A level with fewer wavefront-wide items of a class than the class's kernel has wavefronts, and one with more than four times
    as many: the ticket counter hands every item of the list to exactly one wavefront -- the call walks as many items as its levels
    hold, and the searches are those of the lane forms.  (Four copies of the round in one batch: the tree alone has no level of
    more than 4 x 1 280 items.  The static dealing this replaces gave the lane forms' searches bit for bit at the commit before:
    test_hip_scale's comparisons; the lane forms are what is compared with here.)"""
    copies = 4
    by_lane_items, _ = world.references("plain")
    nodes = np.tile(world.nodes, copies)
    world.dev.timing_reset()
    got = world.search(nodes, wave_all_below=1 << 30)
    launches, ms, units, nbytes = world.dev.timing_read_kind(type(world.dev).KIND_FR_UPDATING)
    iu, _, _, _ = world.dev.frontier_levels()
    ws, wb = world.dev.last_wave_items
    print("levels' wavefront-wide items (small class, 512 class):", list(zip(ws.tolist(), wb.tolist())))
    assert ((ws > 0) & (ws < WAVES_SMALL)).any() or ((wb > 0) & (wb < WAVES_BIG)).any()
    assert (ws > 4 * WAVES_SMALL).any() or (wb > 4 * WAVES_BIG).any()
    assert int(units) == int(iu.sum()) and int(iu.sum()) > 0
    for k in FIELDS:
        assert np.array_equal(got[k], np.concatenate([by_lane_items[k]] * copies)), k
