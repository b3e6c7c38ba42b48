"""GPU (-m gpu): the K-hop pre-transform for graphs above 64 nodes through its C ABI (kpgnn_khop_large_count / _fill via
_lib.launch, csrc/khop_large.hip).  Integer outputs, compared bit for bit with the host library (khop_batch per graph on one
thread).  Every output is pre-filled with a sentinel and `status` is asserted exactly from the inputs, so the kernel cannot
pass by deferring to the host: nothing here has a fallback at all."""
import functools

import networkx as nx
import numpy as np
import pytest

from khop_device_cases import batch_of, check_against_host, from_nx, host_per_graph
from khop_large_cases import edgeless, kinds, large_run, one_way

pytestmark = pytest.mark.gpu

OK, TOO_LARGE, RANGE, ENDPOINT, TYPE, SHAPE = 0, 1, 2, 3, 4, 5
CAP = 2048


def _caps():
    from kp_gnn_amd import _lib
    assert (_lib.KHOP_MAX_NODES, _lib.KHOP_LARGE_MAX_NODES) == (64, CAP)


def _args(kernel, periph, K=4, max_attr=5, H=2, T=2, max_ec=4, max_dc=6):
    return (K, max_attr, H if periph else 0, T if periph else 0, max_ec, max_dc, kernel)


def _word_boundaries():
    graphs = [g for n in (65, 127, 128, 129, 192, 193) for g in kinds(n)]
    graphs.insert(2, edgeless(70))                              # an edgeless graph between two that have edges
    return graphs, {}, [OK] * len(graphs)


def _small():
    graphs = [g for n in (1, 2, 33, 64) for g in kinds(n)]
    return graphs, {}, [OK] * len(graphs)


def _directed():
    return [one_way(from_nx(nx.random_regular_graph(3, 100, seed=100)))], {}, [OK]


def _duplicates():
    n, ei, ea = from_nx(nx.random_regular_graph(3, 90, seed=90))
    twice = (n, np.concatenate([ei, ei], axis=1), np.concatenate([ea, ea]))
    t3 = np.concatenate([ea, [22, 22]])                         # three copies of edge 0, 22 each: 66 is above the histogram's 63
    t3[0] = 22
    thrice = (n, np.concatenate([ei, ei[:, :1], ei[:, :1]], axis=1), t3)
    return [twice, thrice], {}, [OK, TYPE]


def _self_loops():
    n, ei, ea = from_nx(nx.random_regular_graph(3, 90, seed=91))
    loops = np.arange(0, 90, 9, dtype=np.int64)
    assert loops.size == 10
    return [(n, np.concatenate([ei, np.stack([loops, loops])], axis=1), np.concatenate([ea, np.full(10, 3)]))], {}, [OK]


def _clamps():
    return [from_nx(nx.random_regular_graph(4, 100, seed=4))], dict(max_attr=2, max_ec=3, max_dc=4), [OK]


def _hist32():
    # every edge has type 2, so ONE bin of the peripheral histogram of a node's 259 neighbours counts 259 * 258 = 66,822 edges
    return [from_nx(nx.complete_graph(260), typed=False)], dict(K=1, T=2, H=1, max_ec=100000), [OK]


def _range():
    graphs = [from_nx(nx.path_graph(80)), from_nx(nx.complete_graph(70), typed=False), from_nx(nx.path_graph(75))]
    return graphs, dict(K=8), [OK, RANGE, OK]


def _cap():
    return [from_nx(nx.path_graph(CAP)), from_nx(nx.path_graph(CAP + 1))], dict(K=2), [OK, TOO_LARGE]


def _simulation():
    return [from_nx(nx.random_regular_graph(3, 1280, seed=1280), typed=False)], dict(K=3), [OK]


CASES = {"word_boundaries": _word_boundaries, "small": _small, "directed": _directed, "duplicates": _duplicates,
         "self_loops": _self_loops, "clamps": _clamps, "hist32": _hist32, "range": _range, "cap": _cap, "simulation": _simulation}


@functools.lru_cache(maxsize=None)
def _case(name):
    graphs, over, status = CASES[name]()
    return batch_of(graphs), over, status


@functools.lru_cache(maxsize=None)
def _host(name, args):
    (nptr, eptr, ei, ea), _, status = _case(name)
    return host_per_graph(nptr, eptr, ei, ea, args, [g for g, st in enumerate(status) if st == OK])


def _want(name, kernel, periph):
    args = _args(kernel, periph, **_case(name)[1])
    if args[0] == 1:
        args = args[:6] + ("spd",)      # one hop: the kernel argument only enters at k > 0, so both share one host run
    return _host(name, args)


@pytest.mark.parametrize("periph", [True, False], ids=["periph", "plain"])
@pytest.mark.parametrize("kernel", ["spd", "gd"])
@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_the_host_route(name, kernel, periph):
    _caps()
    (nptr, eptr, ei, ea), over, status = _case(name)
    n = np.diff(nptr)
    args = _args(kernel, periph, **over)
    if name == "range":                 # the host refuses exactly that graph (walk counts pass 2^31 by hop 7) and serves the paths
        from kp_gnn_amd import KpgnnError
        with pytest.raises(KpgnnError, match="2\\^31"):
            host_per_graph(nptr, eptr, ei, ea, args, [1])
    want = _want(name, kernel, periph)
    if name == "hist32" and periph:
        assert int(want[0]["peripheral_edge_attr"][..., 1].max()) == 259 * 258 > 65535
    if name == "clamps":
        w = want[0]
        assert int(w["edge_attr"][:, 1:].max()) == 2 + 1
        assert not periph or (int(w["peripheral_edge_attr"][..., 1].max()) == 3 and int(w["peripheral_configuration_attr"].max()) == 4)
    cap = min(CAP, max(100, int(n.max())))
    run = large_run(nptr, eptr, ei, ea, args, [(list(range(len(n))), cap)])
    check_against_host(run, nptr, want, status)


def _codes_batch(bad):
    graphs = [from_nx(nx.path_graph(70)), bad, from_nx(nx.cycle_graph(66)), from_nx(nx.random_regular_graph(3, 140, seed=1)),
              from_nx(nx.path_graph(5))]
    return batch_of(graphs)


@pytest.mark.parametrize("how", ["one_launch", "two_launches"])
def test_status_codes_leave_the_other_graphs_served(how):
    _caps()
    k70 = from_nx(nx.complete_graph(70), typed=False)
    n, ei, ea = from_nx(nx.cycle_graph(97))
    past = ei.copy()
    past[1, 3] = 97                                             # one past the graph's last node
    big_type = ea.copy()
    big_type[2] = 64                                            # above the histogram's 63
    dup = np.concatenate([ei, ei[:, :1]], axis=1)               # a duplicate whose summed type is 40 + 40
    dup_t = np.concatenate([ea, [40]])
    dup_t[0] = 40
    split = (lambda G: [(list(range(G)), 140)]) if how == "one_launch" else (lambda G: [([0, 1], 140), (list(range(2, G)), 140)])
    a_spd, a_gd = _args("spd", True, H=3), _args("gd", True, H=3)
    for bad, args, code in ((k70, (16, 50, 1, 1, 1, 1, "gd"), RANGE), ((n, past, ea), a_spd, ENDPOINT),
                            ((n, ei, big_type), a_spd, TYPE), ((n, dup, dup_t), a_gd, TYPE)):
        nptr, eptr, bei, bea = _codes_batch(bad)
        run = large_run(nptr, eptr, bei, bea, args, split(5))
        check_against_host(run, nptr, host_per_graph(nptr, eptr, bei, bea, args, [0, 2, 3, 4]), [OK, code, OK, OK, OK])
    # a shape the kernel is not instantiated for refuses every graph of the launch and writes nothing
    nptr, eptr, bei, bea = _codes_batch(from_nx(nx.path_graph(83)))
    for args in ((17, 50, 1, 1, 1, 1, "spd"), (4, 5, 9, 2, 4, 6, "spd"), (4, 5, 3, 9, 4, 6, "gd")):
        check_against_host(large_run(nptr, eptr, bei, bea, args, split(5)), nptr, {}, [SHAPE] * 5)
    # a graph above THIS launch's max_nodes is TOO_LARGE although the cap would cover it
    args = _args("spd", True)
    run = large_run(nptr, eptr, bei, bea, args, [(list(range(5)), 83)])
    check_against_host(run, nptr, host_per_graph(nptr, eptr, bei, bea, args, [0, 1, 2, 4]), [OK, OK, OK, TOO_LARGE, OK])
    # ... and the largest covered shape is served
    args = (16, 50, 8, 8, 50, 50, "spd")
    run = large_run(nptr, eptr, bei, bea, args, split(5))
    check_against_host(run, nptr, host_per_graph(nptr, eptr, bei, bea, args, range(5)), [OK] * 5)


def test_ids_outside_the_call_are_skipped_and_unnamed_graphs_are_not_written():
    _caps()
    nptr, eptr, ei, ea = _codes_batch(from_nx(nx.path_graph(83)))
    args = _args("gd", True)
    outs, status, _, deg, E_out = run = large_run(nptr, eptr, ei, ea, args, [([-1, 3, 5, 1, 1 << 20], 140)])
    assert status.tolist() == [-1, OK, -1, OK, -1]              # graphs 0, 2 and 4 are in no launch: not even a status
    want = host_per_graph(nptr, eptr, ei, ea, args, [1, 3])
    assert E_out == sum(w["edge_index"].shape[1] for w in want.values())
    status[[0, 2, 4]] = TOO_LARGE                               # (any status but 0: check_against_host then wants them untouched)
    check_against_host((outs, status) + run[2:], nptr, want, status.tolist())


def test_two_runs_and_a_permutation_of_the_edges_give_identical_bits():
    _caps()
    graphs = kinds(193) + [from_nx(nx.random_regular_graph(4, 193 - 1, seed=7))]
    nptr, eptr, ei, ea = batch_of(graphs)
    args = (8, 50, 6, 3, 50, 50, "spd")
    launches = [(list(range(len(graphs))), 193)]
    first = large_run(nptr, eptr, ei, ea, args, launches)
    again = large_run(nptr, eptr, ei, ea, args, launches)
    rng = np.random.default_rng(5)
    perm = np.concatenate([eptr[g] + rng.permutation(int(eptr[g + 1] - eptr[g])) for g in range(len(nptr) - 1)]).astype(np.int64)
    assert not np.array_equal(perm, np.arange(perm.size))
    shuffled = large_run(nptr, eptr, np.ascontiguousarray(ei[:, perm]), ea[perm], args, launches)
    assert first[1].tolist() == [OK] * len(graphs) and first[4] > 0
    for other in (again, shuffled):
        assert np.array_equal(first[1], other[1]) and first[2].tobytes() == other[2].tobytes() and first[4] == other[4]
        assert first[3].tobytes() == other[3].tobytes()        # the workspace degrees
        for k, v in first[0].items():
            assert v.tobytes() == other[0][k].tobytes(), k
