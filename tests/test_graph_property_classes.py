"""GPU (-m gpu): the three instantiations of the graph-property label kernel template (csrc/graph_labels.hip: a wavefront per
graph with one word per row, a block per graph with one word, a block per graph with two words) against each other and
against the bits recorded from the three hand-written kernels the template replaced (tests/golden/graph_labels_bits.npz,
golden/make_graph_labels_bits.py).  Raw launches through ops.graph_labels_launch into NaN-poisoned outputs, status preset
to -7; every comparison is of int32 bit patterns."""
import functools

import numpy as np
import pytest

import graph_labels_classes as GB
import graph_property_cases as GC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _run(cls):
    from kp_gnn_amd import ops
    return GB.run_class(ops, cls)


def test_the_three_classes_agree_bit_for_bit():
    """The header's claim that the bits of a graph do not depend on the team's width, nor on the row's: the edge-size cases
    (n in 1, 2, 3, 31, 32, 33, 63, 64) and every second served fixture graph through the wavefront class (n <= 32 only), the
    block class, and the two-word class sized for 64 and for 128 - status 0 and equal bits wherever a graph was launched."""
    from kp_gnn_amd import ops
    cases = GB.small_cases()
    names = [k for k in cases if k.startswith("edge/")] + [k for k in cases if k.startswith("fixture/")][::2]
    assert len(names) == 3 * len(GC.EDGE_SIZES) + 27
    runs = {"wave": _run("wave"), "block": _run("block")}
    for cap in (64, 128):
        nptr, node, graph, st = GB.launch(ops, [cases[k] for k in names], np.arange(len(names)), cap, GB.LARGE)
        runs[f"large sized for {cap}"] = {k: (node[nptr[i]:nptr[i + 1]], graph[i], int(st[i])) for i, k in enumerate(names)}
    assert {cases[k][0] <= GB.WAVE_NODES for k in names} == {False, True}
    for k in names:
        node0, graph0, st0 = runs["block"][k]
        assert st0 == 0, k
        for which, run in runs.items():
            if which == "wave" and cases[k][0] > GB.WAVE_NODES:
                assert k not in run
                continue
            node, graph, st = run[k]
            assert st == 0, (k, which, st)
            assert np.array_equal(node, node0) and np.array_equal(graph, graph0), (k, which)


@pytest.mark.parametrize("cls", list(GB.CLASSES))
def test_the_bits_of_the_kernels_the_template_replaced(cls):
    """Each instantiation on its recorded cases: the inputs are regenerated and their checksums compared first, so a failure
    here says whether the inputs changed or the kernel did; then every status and every bit of node_out and graph_out."""
    z = np.load(GB.GOLDEN)
    cases = GB.cases_of(cls)
    assert list(cases) == z[f"{cls}/names"].tolist()
    assert [int(GB.checksum(v)) for v in cases.values()] == z[f"{cls}/crc"].tolist(), "the inputs are not the recorded ones"
    got = _run(cls)
    want_node, want_graph, want_status = z[f"{cls}/node"], z[f"{cls}/graph"], z[f"{cls}/status"]
    assert want_node.dtype == np.int32 and want_graph.dtype == np.int32 and want_node.shape == (sum(v[0] for v in cases.values()), 3)
    row = 0
    for i, (k, (n, _, _, _)) in enumerate(cases.items()):
        node, graph, st = got[k]
        assert st == int(want_status[i]) == 0, (k, st)
        assert np.array_equal(graph, want_graph[i]), (k, graph.view(np.float32), want_graph[i].view(np.float32))
        assert np.array_equal(node, want_node[row:row + n]), k
        row += n
