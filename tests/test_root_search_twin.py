"""The hand-made tree of tests/test_hip_root_search.py::test_an_abandoned_rooting on the CPU twin (oracle/libmaple_cpu.so behind the
same C ABI): tree_host.find_best_root -- the Python path the native call is held to -- really abandons both sides of one node on
it and still scores the two branches elsewhere, so the GPU test cannot pass vacuously.  No GPU is needed."""
import ctypes as C
import os
import subprocess

from test_hip_root_search import EVERY, Q_SMOKE, abandoned_tree, below_roots_children

ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")


def test_the_python_path_abandons_a_rooting_on_the_hand_made_tree():
    from maple_amd.host import reference_tables
    from maple_amd.runtime import Device
    from maple_amd.tree_host import find_best_root
    subprocess.check_call(["make", "-C", ORACLE, "-s"])
    lib = C.CDLL(os.path.join(ORACLE, "libmaple_cpu.so"))
    lib.maple_last_error.restype = C.c_char_p
    ref_idx, root_freqs = reference_tables("acgtacgtacgtacgtacgt")
    dev = Device(ref_idx, root_freqs, lib=lib)
    dev.set_model(Q_SMOKE)
    tree = abandoned_tree(dev, ref_idx)
    before = dev.stats()
    node, best, best_nodes, visited = find_best_root(dev, tree, **EVERY)
    assert dev.stats() == before
    assert below_roots_children(tree) == [0, 1, 2, 3, 5, 6]
    assert list(best_nodes) == [8, 6, 5] or list(best_nodes) == [8, 5, 6]
    assert (node, best, visited) == (8, 0.0, 3) and best_nodes[5] < 0.0 and best_nodes[6] < 0.0
    dev.close()
