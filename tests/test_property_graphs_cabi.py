"""kpgnn_property_graphs_generate / _fill through ctypes (csrc/property_graphs.hip): the refusals, which need no device, and on
the GPU (-m gpu) the bits of the host route - rows, features, the five columns per graph and the filled edge_index - for every
type at the sizes on both sides of every bound the kernel has (tests/property_graph_cases.py DEVICE_SIZES), with and without
the relabelling and `randomize`, through the block class where the wavefront class would serve, in a call that mixes the
classes, and with exhausted graphs, whose rows must stay as they were."""
import ctypes

import numpy as np
import pytest
import torch

import property_graph_cases as PC

ROW_SENTINEL, FEATURE_SENTINEL, SENTINEL = 0x5A5A5A5A5A5A5A5A, -3.0, -7
NO_SHUFFLE, NO_RANDOMIZE = 1, 2
G8 = 8


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _call(nodes, graph_type, seed=0, first_graph=0, flags=0, max_attempts=4096, force_block=0, classes=None):
    """_generate, the cumulative sum of the edge counts, _fill - over pattern-filled buffers.  classes: [(ids, max_nodes)], one
    launch of each entry per item; None is one launch over all graphs sized for the largest.  Host arrays
    (rc of every call, rows [N,2] uint64, features, info [5,G], edge_ptr, edge_index)."""
    from kp_gnn_amd import _lib
    dev, lib = _dev(), _lib.load()
    nodes = np.asarray(nodes, dtype=np.int32)
    G, node_ptr = nodes.size, np.concatenate([[0], np.cumsum(nodes)]).astype(np.int64)
    N = int(node_ptr[-1])
    rows = torch.full((N, 2), ROW_SENTINEL, dtype=torch.int64, device=dev)
    feat = torch.full((N,), FEATURE_SENTINEL, dtype=torch.float32, device=dev)
    info = torch.full((5, G), SENTINEL, dtype=torch.int32, device=dev)
    nptr = torch.from_numpy(node_ptr).to(dev)
    d = _lib.PgDesc()
    d.G, d.nodes, d.node_ptr = G, nodes.ctypes.data, nptr.data_ptr()
    d.graph_type, d.flags, d.max_attempts, d.force_block = PC.TYPES[graph_type], flags, max_attempts, force_block
    d.seed, d.first_graph = seed, first_graph
    d.rows, d.features, d.info = rows.data_ptr(), feat.data_ptr(), info.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ids = [(None if c is None else torch.tensor(c[0], dtype=torch.int32, device=dev), G if c is None else len(c[0]),
            int(nodes.max()) if c is None else c[1]) for c in (classes or [None])]
    rcs = []

    def run(fn):
        for ids_d, n_ids, cap in ids:
            d.graph_ids, d.n_ids, d.max_nodes = (None if ids_d is None else ids_d.data_ptr()), n_ids, cap
            rcs.append(fn(ctypes.byref(d), stream))

    run(lib.kpgnn_property_graphs_generate)
    torch.cuda.synchronize(dev)
    info_h = info.cpu().numpy()
    counts = np.where(info_h[0] == SENTINEL, 0, info_h[0])
    edge_ptr = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)
    E = int(edge_ptr[-1])
    ei = torch.full((2, max(E, 1)), SENTINEL, dtype=torch.int64, device=dev)
    eptr = torch.from_numpy(edge_ptr).to(dev)
    d.edge_ptr, d.edge_index, d.E = eptr.data_ptr(), ei.data_ptr(), E
    run(lib.kpgnn_property_graphs_fill)
    torch.cuda.synchronize(dev)
    return rcs, rows.cpu().numpy().view(np.uint64), feat.cpu().numpy(), info_h, edge_ptr, ei.cpu().numpy()[:, :E]


def _check(got, want, served=None):
    """The device's answer against the host route's tuple; `served`: the graphs a launch covered (all by default)."""
    rcs, rows, feat, info, edge_ptr, ei = got
    node_ptr, w_eptr, w_ei, w_feat, w_source, w_types, w_attempts, w_status = want
    assert all(rc == 0 for rc in rcs), rcs
    G = len(node_ptr) - 1
    served = np.arange(G) if served is None else np.asarray(served)
    assert np.array_equal(info[4, served], w_status[served]) and np.array_equal(info[3, served], w_attempts[served])
    assert np.array_equal(info[2, served], w_types[served]) and np.array_equal(info[1, served], w_source[served])
    assert np.array_equal(info[0, served], np.diff(w_eptr)[served])
    w_rows = PC.rows_of(node_ptr, w_eptr, w_ei)
    for g in served:
        n0, n1 = node_ptr[g], node_ptr[g + 1]
        if w_status[g] == 0:
            assert np.array_equal(rows[n0:n1], w_rows[n0:n1]), g
            assert np.array_equal(feat[n0:n1].view(np.uint32), w_feat[n0:n1].view(np.uint32)), g
            assert np.array_equal(ei[:, edge_ptr[g]:edge_ptr[g + 1]], w_ei[:, w_eptr[g]:w_eptr[g + 1]]), g
        else:                                                       # untouched
            assert (rows[n0:n1] == np.uint64(ROW_SENTINEL)).all() and (feat[n0:n1] == FEATURE_SENTINEL).all(), g


@pytest.mark.gpu
@pytest.mark.parametrize("flags", (0, NO_SHUFFLE | NO_RANDOMIZE))
@pytest.mark.parametrize("t", tuple(PC.TYPES))
def test_bits_of_the_host_route(t, flags):
    """G = 8 graphs of each size, which leaves a wavefront-class block's four teams busy twice; graph ids above 2^32 and a
    negative seed, so both halves of each reach the counter."""
    seed, first = -11, 2 ** 33 + 3
    for n in PC.DEVICE_SIZES:
        want = PC.host((n,) * G8, seed, t, first, 4096, not flags & NO_RANDOMIZE, not flags & NO_SHUFFLE)
        assert (want[7] == 0).all()
        got = _call([n] * G8, t, seed, first, flags)
        _check(got, want)
        if flags and t in PC.FIXED:                                 # the canonical adjacency itself
            A = np.zeros((n, n), dtype=bool)
            for i, j in PC.canonical(n, t, 0, 0, 0):
                A[i, j] = A[j, i] = True
            e = got[4][1]
            assert np.array_equal(PC.adjacency(n, got[5][:, :e]), A) and (got[3][3] == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", (33, 64))
def test_the_block_class_gives_the_wavefront_class_its_bits(n):
    for t in ("RANDOM", "BARABASI_ALBERT", "TREE", "ERDOS_RENYI", "CAVEMAN"):
        want = PC.host((n,) * G8, 5, t)
        _check(_call([n] * G8, t, 5, force_block=1), want)
        _check(_call([n] * G8, t, 5, classes=[(list(range(G8)), 128)]), want)


@pytest.mark.gpu
def test_a_call_that_mixes_the_classes():
    nodes = (15, 100, 64, 65, 3, 128, 2, 33, 24)
    want = PC.host(nodes, 9)
    wave = [g for g, n in enumerate(nodes) if n <= 64]
    block = [g for g, n in enumerate(nodes) if n > 64]
    _check(_call(nodes, "RANDOM", 9, classes=[(wave, 64), (block, 128)]), want)
    _check(_call(nodes, "RANDOM", 9, classes=[(block[:1], 100), (wave[:2], 64)]), want, served=block[:1] + wave[:2])
    got = _call(nodes, "RANDOM", 9)                                 # one launch, the block class for all
    _check(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("n,G", ((4, 64), (70, 24)))
def test_exhausted_graphs_keep_their_rows(n, G):
    """max_attempts = 1 in either class: status 1, attempts 1 and the edge count 0 where the first attempt leaves a node alone,
    their rows and features still the pattern, nothing of them in edge_index; the others are the host route's."""
    want = PC.host((n,) * G, 0, "ERDOS_RENYI", max_attempts=1)
    assert set(want[7].tolist()) == {0, 1}
    got = _call([n] * G, "ERDOS_RENYI", max_attempts=1)
    _check(got, want)
    assert (got[3][3] == 1).all() and got[5].shape[1] == want[2].shape[1] and (got[5] != SENTINEL).all()


@pytest.mark.gpu
def test_a_graph_beyond_its_launch_class_is_left_alone():
    """A plan that puts a 100-node graph into a launch sized for 64: that graph gets status 1 with attempts 0 and nothing
    else; its neighbours in the launch are served."""
    nodes = (20, 100, 30)
    want = PC.host(nodes, 2)
    rcs, rows, feat, info, edge_ptr, ei = got = _call(nodes, "RANDOM", 2, classes=[([0, 1, 2], 64)])
    _check(got, want, served=[0, 2])
    assert info[:, 1].tolist() == [0, 0, int(want[5][1]), 0, 1]
    assert (rows[20:120] == np.uint64(ROW_SENTINEL)).all() and (feat[20:120] == FEATURE_SENTINEL).all()


def test_refusals_come_before_any_device_call():
    """No stream, no device memory: nothing may be launched."""
    from kp_gnn_amd import _lib
    lib = _lib.load()
    a = 0x10000                                       # dummy, non-NULL: never dereferenced
    sizes = np.array([15, 20], dtype=np.int32)

    def rc(fn=lib.kpgnn_property_graphs_generate, nodes=sizes, G=2, n_ids=2, graph_type=0, flags=0, max_attempts=4096, first_graph=0,
           max_nodes=64, **null):
        d = _lib.PgDesc()
        d.G, d.n_ids, d.nodes = G, n_ids, None if nodes is None else nodes.ctypes.data
        d.graph_type, d.flags, d.max_attempts, d.first_graph, d.max_nodes = graph_type, flags, max_attempts, first_graph, max_nodes
        for k in ("node_ptr", "rows", "features", "info", "edge_ptr", "edge_index"):
            setattr(d, k, null.get(k, a))
        d.E = null.get("E", 4)
        return fn(ctypes.byref(d), None)

    for fn in (lib.kpgnn_property_graphs_generate, lib.kpgnn_property_graphs_fill):
        assert fn(None, None) == -1
        assert rc(fn, max_attempts=0) == -1 and rc(fn, first_graph=-1) == -1 and rc(fn, G=-1) == -1 and rc(fn, n_ids=3) == -1
        assert rc(fn, graph_type=4) == -1 and rc(fn, graph_type=12) == -1 and rc(fn, graph_type=-1) == -1
        assert b"graph_type" in lib.kpgnn_last_error()
        assert rc(fn, flags=4) == -1 and b"flags" in lib.kpgnn_last_error()
        assert rc(fn, max_nodes=0) == -1 and rc(fn, max_nodes=129) == -1
        assert rc(fn, nodes=None) == -1 and rc(fn, node_ptr=None) == -1 and rc(fn, rows=None) == -1 and rc(fn, info=None) == -1
        assert b"NULL" in lib.kpgnn_last_error()
        for bad in (1, 129, 0, -2):
            assert rc(fn, nodes=np.array([15, bad], dtype=np.int32)) == -3 and b"outside [2, 128]" in lib.kpgnn_last_error()
        assert rc(fn, G=0, n_ids=0, nodes=None, node_ptr=None, rows=None, features=None, info=None, edge_ptr=None, edge_index=None) == 0
        assert rc(fn, n_ids=0) == 0
    assert rc(features=None) == -1
    assert rc(lib.kpgnn_property_graphs_fill, edge_ptr=None) == -1 and rc(lib.kpgnn_property_graphs_fill, edge_index=None) == -1
    assert rc(lib.kpgnn_property_graphs_fill, E=-1) == -1 and rc(lib.kpgnn_property_graphs_fill, E=0, edge_index=None) == 0
