"""GPU (-m gpu): the device K-hop pre-transform through its C ABI (kpgnn_khop_dev_count / _fill via _lib.launch,
csrc/khop_transform.hip).  Integer outputs, compared bit for bit: with the reference's own goldens
(tests/golden/khop_preprocess.npz) and with the host library.  `status` is asserted exactly for every graph, so no fallback
can hide a wrong kernel: nothing here has a fallback at all."""
import functools
import os

import networkx as nx
import numpy as np
import pytest

from khop_device_cases import SENTINEL, batch_of, cabi_run, check_against_host, from_nx, host_per_graph, size_class_graphs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP, WAVE = 64, 32
OK, TOO_LARGE, RANGE, ENDPOINT, TYPE, SHAPE = 0, 1, 2, 3, 4, 5


def _caps():
    from kp_gnn_amd import _lib
    assert (_lib.KHOP_MAX_NODES, _lib.KHOP_WAVE_NODES) == (CAP, WAVE)


def _by_class(nptr):
    n = np.diff(nptr)
    small, large = np.flatnonzero(n <= WAVE), np.flatnonzero(n > WAVE)
    return [(ids.tolist(), max(1, min(CAP, int(n[ids].max())))) for ids in (small, large) if ids.size]


def _mixed(nptr):
    return [(list(range(len(nptr) - 1)), CAP)]


def test_reference_goldens_bit_for_bit():
    _caps()
    z = np.load(os.path.join(ROOT, "tests", "golden", "khop_preprocess.npz"))
    cases = sorted({k.split("/in/")[0] for k in z.files if "/in/" in k})
    served = 0
    for c in cases:
        a = z["args/" + c.split("/")[0]]
        args = tuple(int(v) for v in a[:6]) + (str(a[6]),)
        n = int(z[c + "/in/num_nodes"])
        ei = np.asarray(z[c + "/in/edge_index"], dtype=np.int64).reshape(2, -1)
        ea = np.asarray(z[c + "/in/edge_attr"], dtype=np.int64) if c + "/in/edge_attr" in z.files else None
        nptr, eptr = np.array([0, n]), np.array([0, ei.shape[1]])
        outs, status, _, deg, E_out = cabi_run(nptr, eptr, ei, ea, args, [([0], min(n, CAP))])
        if n > CAP:                                     # decided from the input, not from the status
            assert status.tolist() == [TOO_LARGE] and E_out == 0, c
            for k, v in outs.items():
                assert v is None or bool((v == SENTINEL).all()), (c, k)
            continue
        served += 1
        assert status.tolist() == [OK], c
        if ei.shape[1] == 0:                            # the reference's early return (Q8): no edges, zero statistics
            assert E_out == 0 and not outs["peripheral_edge_attr"].any() and not outs["peripheral_configuration_attr"].any(), c
            assert not z[c + "/out/peripheral_edge_attr"].any()
            continue
        want = sorted(k.split("/out/")[1] for k in z.files if k.startswith(c + "/out/"))
        got = sorted(k for k in ("edge_index", "edge_attr", "pe_attr", "peripheral_edge_attr", "peripheral_configuration_attr")
                     if outs[k] is not None)
        assert want == got, (c, want, got)
        for k in want:
            g = z[c + "/out/" + k]
            assert g.shape == outs[k].shape and np.array_equal(g, outs[k]), (c, k)
        assert not outs["batch"].any()
    assert served >= 25


ARGS = ((4, 5, 3, 2, 4, 6, "spd"), (4, 5, 3, 2, 4, 6, "gd"), (8, 50, 6, 3, 50, 50, "spd"))


@functools.lru_cache(maxsize=None)
def _sizes_batch():
    graphs = size_class_graphs([1, 2, 31, 32, 33, 63, 64]) + [from_nx(nx.path_graph(CAP + 1))]
    return batch_of(graphs)


@functools.lru_cache(maxsize=None)
def _sizes_want(args):
    nptr, eptr, ei, ea = _sizes_batch()
    G = len(nptr) - 1
    return host_per_graph(nptr, eptr, ei, ea, args, [g for g in range(G) if nptr[g + 1] - nptr[g] <= CAP])


@pytest.mark.parametrize("args", ARGS, ids=lambda a: "k%d_%s" % (a[0], a[6]))
@pytest.mark.parametrize("how", ["per_class", "mixed"])
def test_size_classes_match_the_host_route(args, how):
    _caps()
    nptr, eptr, ei, ea = _sizes_batch()
    n = np.diff(nptr)
    assert {1, 2, 31, 32, 33, 63, 64, 65} <= set(n.tolist()) and eptr[2] == eptr[3] and eptr[1] < eptr[2] and eptr[3] < eptr[4]
    status = [OK if v <= CAP else TOO_LARGE for v in n]         # every graph at or below the cap is served by the kernel
    run = cabi_run(nptr, eptr, ei, ea, args, _by_class(nptr) if how == "per_class" else _mixed(nptr))
    check_against_host(run, nptr, _sizes_want(args), status)


def test_no_graphs_is_ok_without_a_launch():
    _caps()
    outs, status, _, _, E_out = cabi_run(np.array([0]), np.array([0]), np.zeros((2, 0), np.int64), None, ARGS[0], [([], 1)])
    assert status.size == 0 and E_out == 0                      # G == 0
    nptr, eptr, ei, ea = batch_of([from_nx(nx.path_graph(4))])
    run = cabi_run(nptr, eptr, ei, ea, ARGS[0], [([], 8), ([0], 8), ([], 40)])         # n_ids == 0 either side of a launch
    check_against_host(run, nptr, host_per_graph(nptr, eptr, ei, ea, ARGS[0], [0]), [OK])
    assert run[4] == 12


def _codes_batch(bad):
    graphs = [from_nx(nx.path_graph(5)), bad, from_nx(nx.cycle_graph(6)), from_nx(nx.random_regular_graph(3, 40, seed=1))]
    return batch_of(graphs)


@pytest.mark.parametrize("how", ["per_class", "mixed"])
def test_status_codes_leave_the_other_graphs_served(how):
    _caps()
    k8 = from_nx(nx.complete_graph(8), typed=False)
    n, ei, ea = from_nx(nx.cycle_graph(7))
    past = ei.copy()
    past[1, 3] = 7                                              # one past the graph's last node
    big_type = ea.copy()
    big_type[2] = 64                                            # above the histogram's 63
    dup = np.concatenate([ei, ei[:, :1]], axis=1)               # a duplicate whose summed type is 40 + 40
    dup_t = np.concatenate([ea, [40]])
    dup_t[0] = 40
    for bad, args, code in ((k8, (16, 50, 1, 1, 1, 1, "gd"), RANGE), ((n, past, ea), ARGS[0], ENDPOINT),
                            ((n, ei, big_type), ARGS[0], TYPE), ((n, dup, dup_t), ARGS[1], TYPE)):
        nptr, eptr, bei, bea = _codes_batch(bad)
        run = cabi_run(nptr, eptr, bei, bea, args, _by_class(nptr) if how == "per_class" else _mixed(nptr))
        check_against_host(run, nptr, host_per_graph(nptr, eptr, bei, bea, args, [0, 2, 3]), [OK, code, OK, OK])
    # a shape the kernel is not instantiated for refuses every graph of the launch and writes nothing
    nptr, eptr, bei, bea = _codes_batch(from_nx(nx.path_graph(3)))
    for args in ((17, 50, 1, 1, 1, 1, "spd"), (4, 5, 9, 2, 4, 6, "spd"), (4, 5, 3, 9, 4, 6, "gd")):
        run = cabi_run(nptr, eptr, bei, bea, args, _by_class(nptr) if how == "per_class" else _mixed(nptr))
        check_against_host(run, nptr, {}, [SHAPE] * 4)
    # ... and the largest covered shape is served
    args = (16, 50, 8, 8, 50, 50, "spd")
    run = cabi_run(nptr, eptr, bei, bea, args, _mixed(nptr))
    check_against_host(run, nptr, host_per_graph(nptr, eptr, bei, bea, args, range(4)), [OK] * 4)


def test_two_runs_and_a_permutation_of_the_edges_give_identical_bits():
    _caps()
    nptr, eptr, ei, ea = _sizes_batch()
    args = ARGS[2]
    first = cabi_run(nptr, eptr, ei, ea, args, _by_class(nptr))
    again = cabi_run(nptr, eptr, ei, ea, args, _by_class(nptr))
    rng = np.random.default_rng(5)
    perm = np.concatenate([eptr[g] + rng.permutation(int(eptr[g + 1] - eptr[g])) for g in range(len(nptr) - 1)]).astype(np.int64)
    assert not np.array_equal(perm, np.arange(perm.size))
    shuffled = cabi_run(nptr, eptr, np.ascontiguousarray(ei[:, perm]), ea[perm], args, _by_class(nptr))
    for other in (again, shuffled):
        assert np.array_equal(first[1], other[1]) and np.array_equal(first[2], other[2]) and first[4] == other[4]
        for k, v in first[0].items():
            assert np.array_equal(v, other[0][k]), k
