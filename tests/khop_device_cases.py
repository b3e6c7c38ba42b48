"""Shared by tests/test_khop_device_cabi.py and tests/test_khop_device.py: small graph batches, the host route as the
yardstick (khop_transform.khop_batch, itself pinned to the reference's goldens and to the numpy oracle by
tests/test_khop_host.py), and the two-pass C-ABI call of the device K-hop pre-transform (kpgnn_khop_dev_count, a scan,
kpgnn_khop_dev_fill) with every output pre-filled with a sentinel."""
import ctypes

import networkx as nx
import numpy as np
import torch

SENTINEL = -7
OUT_KEYS = ("edge_index", "edge_attr", "pe_attr", "peripheral_edge_attr", "peripheral_configuration_attr", "batch")


def dev():
    return torch.device("cuda:0")


def from_nx(G, typed=True):
    """(n, edge_index [2,E] local ids, edge_attr [E]) of an undirected networkx graph: both directions, types 2..4 by endpoints."""
    n = G.number_of_nodes()
    ei = np.array(sorted(G.to_directed().edges), dtype=np.int64).reshape(-1, 2).T
    ea = 2 + (ei[0] + ei[1]) % 3 if typed else np.full(ei.shape[1], 2, dtype=np.int64)
    return n, np.ascontiguousarray(ei), ea.astype(np.int64)


def batch_of(graphs):
    """Concatenate [(n, ei, ea), ...] into (node_ptr, edge_ptr, edge_index local ids, edge_attr)."""
    nptr = np.cumsum([0] + [g[0] for g in graphs]).astype(np.int64)
    eptr = np.cumsum([0] + [g[1].shape[1] for g in graphs]).astype(np.int64)
    ei = np.concatenate([g[1].reshape(2, -1) for g in graphs], axis=1) if graphs else np.zeros((2, 0), np.int64)
    ea = np.concatenate([g[2] for g in graphs]) if graphs else np.zeros(0, np.int64)
    return nptr, eptr, np.ascontiguousarray(ei.astype(np.int64)), ea.astype(np.int64)


def size_class_graphs(sizes):
    """Paths, cycles, a star and a 3-regular graph (even n) of each size; an edgeless graph between two that have edges."""
    out = []
    for n in sizes:
        if n == 1:
            out.append((1, np.zeros((2, 0), np.int64), np.zeros(0, np.int64)))
            continue
        out.append(from_nx(nx.path_graph(n)))
        if n >= 3:
            out.append(from_nx(nx.cycle_graph(n)))
            out.append(from_nx(nx.star_graph(n - 1)))
        if n >= 4 and n % 2 == 0:
            out.append(from_nx(nx.random_regular_graph(3, n, seed=n)))
    out.insert(2, (5, np.zeros((2, 0), np.int64), np.zeros(0, np.int64)))
    return out


def host_per_graph(nptr, eptr, ei, ea, args, which):
    """khop_batch of each graph of `which` on its own: {g: dict of numpy arrays with LOCAL node ids}."""
    from kp_gnn_amd import khop_transform as KT
    out = {}
    for g in which:
        sl = slice(int(eptr[g]), int(eptr[g + 1]))
        r = KT.khop_batch([0, int(nptr[g + 1] - nptr[g])], [0, sl.stop - sl.start], ei[:, sl], None if ea is None else ea[sl],
                          *args, num_threads=1)
        out[g] = {k: None if r[k] is None else r[k].numpy() for k in OUT_KEYS}
    return out


def cabi_run(nptr, eptr, ei, ea, args, launches):
    """Count pass, scan, fill pass through _lib.launch.  `launches`: [(graph ids, max_nodes), ...], each one call per pass.
    Returns (outputs as numpy arrays - every tensor pre-filled with SENTINEL -, status [G] (pre-filled with -1), node_off [N],
    degrees [N], E_out)."""
    from kp_gnn_amd import _lib
    K, max_attr, H, T, max_ec, max_dc, kernel = args
    G, N, E = len(nptr) - 1, int(nptr[-1]), int(eptr[-1])
    d_ = dev()
    i64 = dict(dtype=torch.int64, device=d_)
    t_nptr, t_eptr = torch.from_numpy(np.asarray(nptr, np.int64)).to(d_), torch.from_numpy(np.asarray(eptr, np.int64)).to(d_)
    t_ei = torch.from_numpy(np.ascontiguousarray(ei)).to(d_)
    t_ea = None if ea is None else torch.from_numpy(np.ascontiguousarray(ea)).to(d_)
    st = torch.full((max(G, 1),), -1, dtype=torch.int32, device=d_)
    ws = torch.full((max(2 * N, 1),), SENTINEL, **i64)
    d = _lib.KhopDevDesc()
    d.G, d.N, d.E_in = G, N, E
    d.node_ptr, d.edge_ptr, d.edge_index = t_nptr.data_ptr(), t_eptr.data_ptr(), t_ei.data_ptr()
    d.edge_attr = None if t_ea is None else t_ea.data_ptr()
    d.K, d.max_edge_attr_num, d.max_hop_num, d.max_edge_type, d.max_edge_count, d.max_distance_count = K, max_attr, H, T, max_ec, max_dc
    d.kernel = 0 if kernel == "spd" else 1
    d.workspace, d.workspace_bytes, d.status = ws.data_ptr(), ws.numel() * 8, st.data_ptr()
    ids_d = [(torch.tensor(list(ids), dtype=torch.int32, device=d_), len(ids), cap) for ids, cap in launches]

    def run(name):
        for t, n_ids, cap in ids_d:
            d.graph_ids, d.n_ids, d.max_nodes = (t.data_ptr() if n_ids else None), n_ids, cap
            _lib.launch(name, d_, ctypes.byref(d))

    run("kpgnn_khop_dev_count")
    deg = ws[N:2 * N]
    assert N == 0 or int(deg.min()) >= 0, "a degree was left unwritten"
    node_off = deg.cumsum(0) - deg
    E_out = int(deg.sum()) if N else 0
    want_p = H > 0 and T > 0
    outs = {"edge_index": torch.full((2, E_out), SENTINEL, **i64), "edge_attr": torch.full((E_out, K), SENTINEL, **i64),
            "pe_attr": torch.full((N, K - 1), SENTINEL, **i64) if K > 1 else None,
            "peripheral_edge_attr": torch.full((N, K, T, 2), SENTINEL, **i64) if want_p else None,
            "peripheral_configuration_attr": torch.full((N, K, H + 1), SENTINEL, **i64) if want_p else None,
            "batch": torch.full((N,), SENTINEL, **i64)}
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    d.node_off, d.E_out = ptr(node_off), E_out
    d.out_edge_index, d.out_edge_attr, d.out_pe_attr = ptr(outs["edge_index"]), ptr(outs["edge_attr"]), ptr(outs["pe_attr"])
    d.out_pea, d.out_pca, d.out_batch = ptr(outs["peripheral_edge_attr"]), ptr(outs["peripheral_configuration_attr"]), ptr(outs["batch"])
    run("kpgnn_khop_dev_fill")
    torch.cuda.synchronize()
    return ({k: None if v is None else v.cpu().numpy() for k, v in outs.items()}, st[:G].cpu().numpy(), node_off.cpu().numpy(),
            deg.cpu().numpy(), E_out)


def check_against_host(run, nptr, want, want_status):
    """`run` = cabi_run's result; `want` = host_per_graph of the graphs expected to be served; `want_status` [G].  Served
    graphs equal the host route bit for bit, the slices of the others still hold the sentinel, no edge row is left unwritten."""
    outs, status, node_off, deg, E_out = run
    assert status.tolist() == list(want_status)
    covered = 0
    for g, st in enumerate(want_status):
        n0, n1 = int(nptr[g]), int(nptr[g + 1])
        if st != 0:
            assert not deg[n0:n1].any(), g
            for k in ("pe_attr", "peripheral_edge_attr", "peripheral_configuration_attr", "batch"):
                assert outs[k] is None or bool((outs[k][n0:n1] == SENTINEL).all()), (g, k)
            continue
        w = want[g]
        E_g = w["edge_index"].shape[1]
        e0 = int(node_off[n0]) if n1 > n0 else 0
        assert int(deg[n0:n1].sum()) == E_g, g
        assert np.array_equal(outs["edge_index"][:, e0:e0 + E_g], w["edge_index"] + n0), g
        assert np.array_equal(outs["edge_attr"][e0:e0 + E_g], w["edge_attr"]), g
        for k in ("pe_attr", "peripheral_edge_attr", "peripheral_configuration_attr"):
            assert (outs[k] is None) == (w[k] is None), (g, k)
            if w[k] is not None:
                assert outs[k][n0:n1].shape == w[k].shape and np.array_equal(outs[k][n0:n1], w[k]), (g, k)
        assert bool((outs["batch"][n0:n1] == g).all()), g
        covered += E_g
    assert covered == E_out
