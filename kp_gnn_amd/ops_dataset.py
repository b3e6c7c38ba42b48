"""The dataset ops over raw graphs (node_ptr, edge_ptr, edge_index): resistance_distance, graph_property_labels, count_labels,
khop_transform, and random_regular_graphs and property_graphs, which make such graphs; ops.py re-exports them.  One host program: RawGraphs validates, upload() moves the index arrays, a host-only
*_plan function of the graph sizes lists (entry point, ids, max_nodes, workspace_bytes) in launch order, run_plan() issues it,
reads the status once, raises the op's refusals and returns the graphs left to the host route.  The descriptor, the status
preset, the refusal texts and the fill stay with each op."""
import collections
import ctypes

import numpy as np
import torch

from . import _lib, graph_count as GCN, graph_property as GP, khop_transform as KT, property_graphs as PG, regular_graphs as RG
from .raw_graphs import RawGraphs


# ------------------------------------------------------------------------------------------------ the shared pieces
def upload(g, dev):
    """(node_ptr, edge_ptr, edge_index [2,E] int64) of the call `g` on `dev`."""
    return (torch.from_numpy(g.node_ptr).to(dev), torch.from_numpy(g.edge_ptr).to(dev),
            g.edge_index.to(device=dev, dtype=torch.int64).contiguous())


def largest_member(limit):
    """The cap rule "the class's largest graph, at most `limit` (a larger one gets its status from the kernel), at least 1"."""
    return lambda sizes, bound: max(1, min(limit, int(sizes.max())))


def size_classes(entry, nodes, bounds, cap, skip=None, workspace_bytes=0):
    """One launch of `entry` per non-empty size class, [(entry, ids, max_nodes, workspace_bytes)]: class i holds the graphs with
    bounds[i-1] < n <= bounds[i] in call order, the last one every larger graph too, and the graphs of the mask `skip` are in
    none.  max_nodes = cap(sizes of the members, bounds[i]): the cap rule picks the kernel's instantiation, so it is the op's."""
    cls = sum((nodes > bound).astype(np.int8) for bound in bounds[:-1])
    if skip is not None:
        cls[skip] = -1
    classes = [(np.flatnonzero(cls == i), bound) for i, bound in enumerate(bounds)]
    return [(entry, ids, cap(nodes[ids], bound), workspace_bytes) for ids, bound in classes if ids.size]


def workspace_runs(ids, nodes, slab_bytes, workspace_bytes):
    """`ids` (graphs a kernel serves on a slab of a device workspace each, in call order) cut into runs whose slabs - each
    sized for the run's largest graph - fit `workspace_bytes`; a graph that does not fit alone is a run of its own.
    [(ids, max_nodes, bytes)]."""
    out, i = [], 0
    while i < ids.size:
        j, cap = i + 1, int(nodes[ids[i]])
        while j < ids.size:
            c = max(cap, int(nodes[ids[j]]))
            if (j + 1 - i) * slab_bytes(c) > workspace_bytes:
                break
            j, cap = j + 1, c
        out.append((ids[i:j], cap, (j - i) * slab_bytes(cap)))
        i = j
    return out


def refusals(status, refused):
    """Raise for the first refusal in the host array `status`, else return the graphs a host route has to fill (status != 0).
    `refused`: [(codes, exception(graph, code))] in the op's order of precedence - the first entry with a hit raises, naming
    the first graph that has one of its codes."""
    todo = np.flatnonzero(status != 0)
    for codes, exception in refused if todo.size else ():
        hit = todo[np.isin(status[todo], codes)]
        if hit.size:
            raise exception(int(hit[0]), int(status[hit[0]]))
    return todo


def run_plan(plan, dev, launch, st, refused):
    """Walk `plan` in order - launch(entry, ids on the device as int32, max_nodes, workspace, workspace_bytes) - then read the
    device status `st`, the one read of the call: (status on the host, refusals() of it).  The entries that ask for workspace
    bytes come last and share ONE uint8 allocation sized for the largest; a plan that is a generator is advanced to them only
    after the entries before them are launched, so the host cuts its runs while the device works."""
    keep, plan = [], iter(plan)
    for first in plan:
        runs = [first] + (list(plan) if first[3] else [])
        ws = torch.empty(max(nbytes for *_, nbytes in runs), dtype=torch.uint8, device=dev) if first[3] else None
        for entry, ids, cap, nbytes in runs:
            keep.append(torch.from_numpy(ids.astype(np.int32)).to(dev))
            launch(entry, keep[-1], cap, ws, nbytes)
    status = st.cpu()
    return status, refusals(status.numpy(), refused)


# ------------------------------------------------------------------------------------------------ resistance distance
def resistance_plan(nodes, large="host", slab_bytes=None, workspace_bytes=1 << 30):
    """The launches of resistance_distance, one by one: the wavefront class, the block class (with every graph no class serves:
    status 2 from the kernel) and, for large="device", the runs of the graphs of 129 .. RD_LARGE_MAX_NODES nodes on
    slab_bytes(max_nodes) of workspace a graph."""
    big = (nodes > _lib.RD_MAX_NODES) & (nodes <= _lib.RD_LARGE_MAX_NODES) & (large == "device")
    yield from size_classes("kpgnn_resistance_distance", nodes, (_lib.RD_WAVE_NODES, _lib.RD_MAX_NODES), largest_member(_lib.RD_MAX_NODES), big)
    for run in workspace_runs(np.flatnonzero(big), nodes, slab_bytes, int(workspace_bytes)):
        yield ("kpgnn_resistance_distance_large",) + run


def resistance_distance(node_ptr, edge_ptr, edge_index, device, large="host", workspace_bytes=1 << 30):
    """The reference's `rd` node feature (data_utils.py:280-303) of G graphs at once: (rd [N,1] float32 on `device`, status
    [G] int32 on the host).  node_ptr / edge_ptr [G+1]: host offsets of each graph's nodes and edges; edge_index [2,E] int64
    (host or device): ids global within the call, edges grouped by graph.  The graphs are bucketed by size on the host, one
    kpgnn_resistance_distance launch per class (n <= 32: a wavefront per graph; n <= 128: a block per graph), and `status` is
    read back once.  It tells which graphs the kernel served (0); those it did not - a directed list (1), more nodes than the
    kernels serve (2), a failed pivot (3) - are filled from khop_transform.resistance_distance_host, and an edge endpoint
    outside its graph (4) raises IndexError before anything else is launched or filled.
    large: who serves a graph of more than 128 nodes.  "host": nobody on the device - it gets status 2 from the block-class
    launch and the float64 host route fills it.  "device": a third class, 128 < n <= 2048, goes to
    kpgnn_resistance_distance_large (csrc/resistance_large.hip: the matrix in a device workspace, blocked Gauss-Jordan), in
    runs of graphs whose slabs fit `workspace_bytes` (one graph always runs, whatever it needs), one launch per run on one
    workspace allocated once per call; status 2 is then n > 2048.  The two are different float64 computations: their float32
    roundings may differ in the last bit."""
    if large not in ("host", "device"):
        raise ValueError(f"unknown large {large!r}")
    g = RawGraphs(node_ptr, edge_ptr, edge_index)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.KpgnnError("ops.resistance_distance is the device route: khop_transform.resistance_distance_host is the host one")
    out = torch.zeros((g.N, 1), dtype=torch.float32, device=dev)
    if g.G == 0:
        return out, torch.from_numpy(np.zeros(0, dtype=np.int32))
    nptr, eptr, ei = upload(g, dev)
    st = torch.empty(g.G, dtype=torch.int32, device=dev)

    def launch(entry, ids, max_nodes, ws, nbytes):
        d = _lib.RdDesc() if ws is None else _lib.RdLargeDesc()
        d.G, d.n_ids, d.E, d.max_nodes = g.G, ids.numel(), g.E, max_nodes
        d.node_ptr, d.edge_ptr, d.edge_index, d.graph_ids = nptr.data_ptr(), eptr.data_ptr(), ei.data_ptr(), ids.data_ptr()
        d.out, d.status = out.data_ptr(), st.data_ptr()
        if ws is not None:
            d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
        _lib.launch(entry, dev, ctypes.byref(d))

    slab = lambda cap: int(_lib.load().kpgnn_rd_large_workspace_bytes(cap, 1))  # noqa: E731
    status, todo = run_plan(resistance_plan(g.nodes, large, slab, workspace_bytes), dev, launch, st, [
        ((_lib.RD_RANGE,), lambda i, code: IndexError(f"graph {i}: an edge endpoint lies outside its nodes [{g.node_ptr[i]}, {g.node_ptr[i + 1]})"))])
    if todo.size:
        ei_h = g.edge_index_host()
        rows, vals = [], []
        for i in todo:
            n0, n1, e0, e1 = g.node_ptr[i], g.node_ptr[i + 1], g.edge_ptr[i], g.edge_ptr[i + 1]
            rows.append(np.arange(n0, n1))
            vals.append(KT.resistance_distance_host(n1 - n0, ei_h[:, e0:e1] - n0).astype(np.float32))
        out[torch.from_numpy(np.concatenate(rows)).to(dev), 0] = torch.from_numpy(np.concatenate(vals)).to(dev)
    return out, status


# ------------------------------------------------------------------------------------------------ graph-property labels
GRAPH_LABELS_AUTO = "device"     # graph_property_labels(route="auto"): DESIGN.md 5.24 has the measurement behind it


def graph_labels_plan(nodes, large="host"):
    """The launches of graph_property_labels: the wavefront class, then the block class with every graph no class serves
    (status 2) and, for large="device", the graphs of 65 .. GL_LARGE_MAX_NODES nodes as one kpgnn_graph_labels_large launch
    sized for its largest member."""
    big = (nodes > _lib.GL_MAX_NODES) & (nodes <= _lib.GL_LARGE_MAX_NODES) & (large == "device")
    plan = size_classes("kpgnn_graph_labels", nodes, (_lib.GL_WAVE_NODES, _lib.GL_MAX_NODES), largest_member(_lib.GL_MAX_NODES), big)
    if big.any():
        plan.append(("kpgnn_graph_labels_large", np.flatnonzero(big), int(nodes[big].max()), 0))
    return plan


def graph_labels_launch(G, nptr, eptr, ei, E, feat, src, ids, max_nodes, node_out, graph_out, status, entry="kpgnn_graph_labels"):
    """One launch of `entry` (kpgnn_graph_labels or kpgnn_graph_labels_large: one descriptor) over device tensors: the graphs
    `ids` (int32) of a call of G graphs, sized for max_nodes."""
    d = _lib.GraphLabelsDesc()
    d.G, d.n_ids, d.E, d.max_nodes = G, ids.numel(), E, max_nodes
    d.node_ptr, d.edge_ptr, d.edge_index, d.graph_ids = nptr.data_ptr(), eptr.data_ptr(), ei.data_ptr(), ids.data_ptr()
    d.features, d.source = feat.data_ptr(), src.data_ptr()
    d.node_out, d.graph_out, d.status = node_out.data_ptr(), graph_out.data_ptr(), status.data_ptr()
    _lib.launch(entry, node_out.device, ctypes.byref(d))


def graph_property_labels(node_ptr, edge_ptr, edge_index, features, source, device, route="auto", large="host"):
    """The labels of the reference's graph- and node-property dataset (datasets/GraphPropertyDataset.py genereate_dataset) of G
    raw graphs at once: (node_labels [N,3] float32: sssp | eccentricity | laplacian features, graph_labels [G,3] float32:
    is_connected | diameter | spectral_radius), both on `device`.  node_ptr / edge_ptr [G+1]: host offsets; edge_index [2,E]
    int64 LOCAL ids, edges grouped by graph (host or device); features [N] float32 or float64 (widened to double, which is
    exact); source [G] the local id of each graph's source node.
    route "device": the graphs are bucketed by size on the host, one kpgnn_graph_labels launch per class (n <= 32: a
    wavefront per graph; n <= 64: a block per graph), and `status` is read back once.  Graphs the kernel did not serve - a
    directed list (1), more than 64 nodes (2) - are filled from graph_property.labels_host_f64 inside the same call; an edge
    endpoint outside its graph (3), a self loop (4) and a source outside its graph (5) raise ValueError naming the first such
    graph.  route "host": graph_property.graph_property_labels_host, moved to the device.  "auto" is GRAPH_LABELS_AUTO.  The
    integer labels are the same whichever route served a graph; the two float64 computations of the spectral radius and of
    the laplacian column may differ in the last float32 bit.
    large (route "device" only): who serves a graph of 65 to 128 nodes.  "host", the default: nobody on the device - it gets
    status 2 from the block-class launch and labels_host_f64 fills it.  "device": a third class, 64 < n <= GL_LARGE_MAX_NODES,
    goes to kpgnn_graph_labels_large (csrc/graph_labels.hip, W = 2: two words per row, the double matrix in LDS, a block per
    graph) in one more launch sized for its largest member; status 2 is then n > 128, and the status is still read once."""
    if route not in ("auto", "device", "host"):
        raise ValueError(f"unknown route {route!r}")
    if large not in ("host", "device"):
        raise ValueError(f"unknown large {large!r}: 'host' or 'device'")
    route = GRAPH_LABELS_AUTO if route == "auto" else route
    dev = torch.device(device)
    if route == "host":
        return GP.graph_property_labels_host(node_ptr, edge_ptr, edge_index, features, source, dev)
    if dev.type != "cuda":
        raise _lib.KpgnnError("ops.graph_property_labels(route='device') needs a GPU device: graph_property_labels_host is the host route")
    g = RawGraphs(node_ptr, edge_ptr, edge_index, source=source)
    if not torch.is_tensor(features):
        features = torch.from_numpy(np.ascontiguousarray(features))
    if features.dtype not in (torch.float32, torch.float64) or features.numel() != g.N:
        raise ValueError("features must be [N] float32 or float64")
    node_out = torch.zeros((g.N, 3), dtype=torch.float32, device=dev)
    graph_out = torch.zeros((g.G, 3), dtype=torch.float32, device=dev)
    if g.G == 0:
        return node_out, graph_out
    nptr, eptr, ei = upload(g, dev)
    feat = features.reshape(-1).to(device=dev, dtype=torch.float64).contiguous()
    src = torch.from_numpy(np.clip(g.source, -1, 1 << 30).astype(np.int32)).to(dev)     # (any value outside [0, n) is status 5)
    st = torch.empty(g.G, dtype=torch.int32, device=dev)
    launch = lambda entry, ids, max_nodes, ws, nbytes: graph_labels_launch(  # noqa: E731
        g.G, nptr, eptr, ei, g.E, feat, src, ids, max_nodes, node_out, graph_out, st, entry=entry)
    what = {_lib.GL_ENDPOINT: lambda i: f"an edge endpoint lies outside its nodes [0, {int(g.nodes[i])})",
            _lib.GL_SELF_LOOP: lambda i: "a self loop (the labels are defined for graphs without one)",
            _lib.GL_SOURCE: lambda i: f"source {int(g.source[i])} lies outside its nodes [0, {int(g.nodes[i])})"}
    _, todo = run_plan(graph_labels_plan(g.nodes, large), dev, launch, st, [(tuple(what), lambda i, code: ValueError(f"graph {i}: {what[code](i)}"))])
    if todo.size:
        node_h, graph_h = GP.labels_host_f64(g.node_ptr, g.edge_ptr, g.edge_index, features, g.source, graphs=todo)
        rows = torch.from_numpy(np.concatenate([np.arange(g.node_ptr[i], g.node_ptr[i + 1]) for i in todo])).to(dev)
        node_out[rows] = torch.from_numpy(node_h[rows.cpu().numpy()].astype(np.float32)).to(dev)
        gi = torch.from_numpy(todo).to(dev)
        graph_out[gi] = torch.from_numpy(graph_h[todo].astype(np.float32)).to(dev)
    return node_out, graph_out


# ------------------------------------------------------------------------------------------------ substructure-count labels
COUNT_LABELS_AUTO = "device"      # count_labels(route="auto"): DESIGN.md 5.25 has the measurement behind it


def count_labels_plan(nodes, slab_bytes, workspace_bytes=1 << 28):
    """The launches of count_labels, one by one: the wavefront class and the word class, each sized for its BOUND whatever its members,
    then the runs of the graphs of 65 .. CL_MAX_NODES nodes on slab_bytes(max_nodes) of workspace a graph.  A graph above
    CL_MAX_NODES is in no launch: count_labels presets its status."""
    word = (_lib.CL_WAVE_NODES, _lib.CL_WORD_NODES)
    yield from size_classes("kpgnn_count_labels", nodes, word, lambda sizes, bound: bound, nodes > _lib.CL_WORD_NODES)
    big = np.flatnonzero((nodes > _lib.CL_WORD_NODES) & (nodes <= _lib.CL_MAX_NODES))
    for run in workspace_runs(big, nodes, slab_bytes, int(workspace_bytes)):
        yield ("kpgnn_count_labels",) + run


def count_labels_launch(G, nptr, eptr, ei, E, ids, max_nodes, out, status, workspace=None, workspace_bytes=0):
    """One kpgnn_count_labels launch over device tensors: the graphs `ids` (int32) of a call of G graphs, sized for max_nodes
    (which picks the size class); `workspace` (uint8) holds a slab per id when max_nodes > CL_WORD_NODES."""
    d = _lib.CountLabelsDesc()
    d.G, d.n_ids, d.E, d.max_nodes = G, ids.numel(), E, max_nodes
    d.node_ptr, d.edge_ptr, d.edge_index, d.graph_ids = nptr.data_ptr(), eptr.data_ptr(), ei.data_ptr(), ids.data_ptr()
    d.out, d.status = out.data_ptr(), status.data_ptr()
    d.workspace, d.workspace_bytes = (workspace.data_ptr() if workspace is not None else None), int(workspace_bytes)
    _lib.launch("kpgnn_count_labels", out.device, ctypes.byref(d))


def count_labels(node_ptr, edge_ptr, edge_index, device, route="auto", workspace_bytes=1 << 28):
    """The labels of the reference's substructure-counting dataset (datasets/GraphCountDataset.py process) of G raw graphs at
    once: y [G,5] float64 on `device`, tri | tailed | star | cyc4 | cus.  node_ptr / edge_ptr [G+1]: host offsets; edge_index
    [2,E] int64 LOCAL ids, edges grouped by graph (host or device).
    route "device": the graphs are bucketed by size on the host, one kpgnn_count_labels launch per class (n <= 32: a wavefront
    per graph; n <= 64: a block per graph; n <= 2048: a block per graph on a slab of a device workspace, in runs of graphs
    whose slabs fit `workspace_bytes` - one graph always runs - on one workspace allocated once per call), and `status` is
    read back once.  Graphs the kernel did not serve - a directed list (1), a self loop (2), more than 2048 nodes (3) - are
    filled from graph_count.count_labels_host_f64 inside the same call; an edge endpoint outside its graph (4) raises
    ValueError naming the first such graph.  route "host": graph_count.count_labels_host, moved to the device.  "auto" is
    COUNT_LABELS_AUTO.  The four integer labels are the same whichever route served a graph; the two float64 sums of cus may
    differ in their last bits."""
    if route not in ("auto", "device", "host"):
        raise ValueError(f"unknown route {route!r}")
    route = COUNT_LABELS_AUTO if route == "auto" else route
    dev = torch.device(device)
    if route == "host":
        return GCN.count_labels_host(node_ptr, edge_ptr, edge_index, dev)
    if dev.type != "cuda":
        raise _lib.KpgnnError("ops.count_labels(route='device') needs a GPU device: graph_count.count_labels_host is the host route")
    g = RawGraphs(node_ptr, edge_ptr, edge_index)
    out = torch.zeros((g.G, 5), dtype=torch.float64, device=dev)
    if g.G == 0:
        return out
    nptr, eptr, ei = upload(g, dev)
    # (no launch for a graph above the cap: its status is set here; -1 marks a graph no launch wrote, which is an error below)
    st = torch.from_numpy(np.where(g.nodes > _lib.CL_MAX_NODES, _lib.CL_TOO_LARGE, -1).astype(np.int32)).to(dev)
    slab = lambda cap: int(_lib.load().kpgnn_count_labels_workspace_bytes(cap))  # noqa: E731
    launch = lambda entry, ids, max_nodes, ws, nbytes: count_labels_launch(g.G, nptr, eptr, ei, g.E, ids, max_nodes, out, st, ws, nbytes)  # noqa: E731
    _, todo = run_plan(count_labels_plan(g.nodes, slab, workspace_bytes), dev, launch, st, [
        ((_lib.CL_ENDPOINT,), lambda i, code: ValueError(f"graph {i}: an edge endpoint lies outside its nodes [0, {int(g.nodes[i])})")),
        ((-1,), lambda i, code: _lib.KpgnnError(f"kpgnn_count_labels left graph {i} without a status"))])
    if todo.size:
        y = GCN.count_labels_host_f64(g.node_ptr, g.edge_ptr, g.edge_index, graphs=todo)
        out[torch.from_numpy(todo).to(dev)] = torch.from_numpy(y[todo]).to(dev)
    return out


# ------------------------------------------------------------------------------------------------ the K-hop pre-transform
def khop_plan(nodes, large="host", slab_bytes=None):
    """The launches of khop_transform, the _count pass over every class and then the _fill pass over every class: the
    wavefront class and the block class of kpgnn_khop_dev on 8 * max(2N, 1) bytes - the block class with every larger graph
    (status 1) unless large="device" - and then, for large="device", every graph above KHOP_MAX_NODES nodes as one class of
    kpgnn_khop_large, sized for its largest member of at most KHOP_LARGE_MAX_NODES nodes, on slab_bytes(max_nodes) bytes
    rounded down to whole int64."""
    big = (nodes > _lib.KHOP_MAX_NODES) & (large == "device")
    classes = size_classes("kpgnn_khop_dev", nodes, (_lib.KHOP_WAVE_NODES, _lib.KHOP_MAX_NODES), largest_member(_lib.KHOP_MAX_NODES),
                           big, 8 * max(2 * int(nodes.sum()), 1))
    if big.any():
        cap = int(nodes[big & (nodes <= _lib.KHOP_LARGE_MAX_NODES)].max(initial=_lib.KHOP_MAX_NODES + 1))
        classes.append(("kpgnn_khop_large", np.flatnonzero(big), cap, slab_bytes(cap) // 8 * 8))
    return [(pair + pass_, ids, cap, nbytes) for pass_ in ("_count", "_fill") for pair, ids, cap, nbytes in classes]


def khop_transform(node_ptr, edge_ptr, edge_index, edge_attr, K, max_edge_attr_num, max_hop_num, max_edge_type,
                   max_edge_count, max_distance_count, kernel, device, large="host"):
    """khop_transform.khop_batch on the device: (the same dict of collated int64 tensors, on `device`; status [G] int32 on the
    host).  node_ptr / edge_ptr [G+1]: host offsets; edge_index [2,E] LOCAL ids and edge_attr [E] or None, host or device.
    The graphs are bucketed by size (n <= 32: a wavefront per graph; n <= 64: a block per graph), kpgnn_khop_dev_count runs per
    class, the per-graph edge counts and `status` come back in ONE read, the degrees are scanned with cumsum, and
    kpgnn_khop_dev_fill writes the tensors.  Graphs the kernel did not serve - more than 64 nodes (1), a summed edge type above
    63 (4), K / max_edge_type / max_hop_num beyond 16 / 8 / 8 (5) - go through khop_batch on the host: their edge counts join
    the scan and their slices are copied in, so the result is the same whichever route served a graph.  A walk count >= 2^31
    (2) raises what khop_batch raises for that graph (KpgnnError), an edge endpoint outside its graph (3) ValueError.
    large="device": the graphs of more than 64 and at most KHOP_LARGE_MAX_NODES nodes are a third class, served inside the same
    call by kpgnn_khop_large_count / _fill (a wavefront per source row, csrc/khop_large.hip): their degrees join the same scan
    and the same read, their status is 0, and only graphs above that cap, 4 and 5 go to the host.  "host", the default, leaves
    every graph above 64 nodes to khop_batch.  The tensors are the same bits either way."""
    if large not in ("host", "device"):
        raise ValueError(f"unknown large {large!r}: 'host' or 'device'")
    g = RawGraphs(node_ptr, edge_ptr, edge_index)
    G, N, E, nodes, node_ptr, edge_ptr, edge_index = g.G, g.N, g.E, g.nodes, g.node_ptr, g.edge_ptr, g.edge_index
    if edge_attr is not None:
        if not torch.is_tensor(edge_attr):
            edge_attr = torch.from_numpy(np.ascontiguousarray(np.asarray(edge_attr, dtype=np.int64)))
        edge_attr = edge_attr.reshape(-1)
        if edge_attr.shape[0] != E:
            raise ValueError("edge_attr does not match edge_ptr")
    if kernel not in ("spd", "gd"):
        raise ValueError(f"unknown kernel {kernel!r}")
    if K < 1 or min(max_edge_attr_num, max_hop_num, max_edge_type, max_edge_count, max_distance_count) < 0:
        raise ValueError("bad K-hop arguments")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.KpgnnError("ops.khop_transform is the device route: khop_transform.khop_batch is the host one")
    args = (K, max_edge_attr_num, max_hop_num, max_edge_type, max_edge_count, max_distance_count, kernel)
    want_p = max_hop_num > 0 and max_edge_type > 0
    i64 = dict(dtype=torch.int64, device=dev)
    nptr, eptr, ei = upload(g, dev)
    ea = None if edge_attr is None else edge_attr.to(**i64).contiguous()
    st = torch.zeros(G, dtype=torch.int32, device=dev)
    d = _lib.KhopDevDesc()
    d.G, d.N, d.E_in = G, N, E
    d.node_ptr, d.edge_ptr, d.edge_index = nptr.data_ptr(), eptr.data_ptr(), ei.data_ptr()
    d.edge_attr = None if ea is None else ea.data_ptr()
    d.K, d.max_edge_attr_num, d.max_hop_num, d.max_edge_type, d.max_edge_count, d.max_distance_count = args[:6]
    d.kernel = 0 if kernel == "spd" else 1
    d.status = st.data_ptr()
    ws = torch.zeros(max(2 * N, 1), **i64)                  # [0, N) any-hop masks, [N, 2N) K-hop out-degrees
    plan = khop_plan(nodes, large, lambda cap: int(_lib.load().kpgnn_khop_large_workspace_bytes(N, E, cap)))
    count, fill = plan[:len(plan) // 2], plan[len(plan) // 2:]
    # the third class: its own pair, its own workspace, degrees in front
    ws_l = next((torch.zeros(nbytes // 8, **i64) for entry, _, _, nbytes in count if entry == "kpgnn_khop_large_count"), None)
    ids_d = [torch.from_numpy(ids.astype(np.int32)).to(dev) for _, ids, _, _ in count]

    def run(pass_):
        for (entry, ids, cap, nbytes), i_d in zip(pass_, ids_d):
            w = ws_l if entry.startswith("kpgnn_khop_large") else ws
            d.graph_ids, d.n_ids, d.max_nodes = i_d.data_ptr(), ids.size, cap
            d.workspace, d.workspace_bytes = w.data_ptr(), nbytes
            _lib.launch(entry, dev, ctypes.byref(d), timed=("khop_dev", lambda: 0))

    run(count)
    deg = ws[N:2 * N]
    if ws_l is not None:
        deg += ws_l[:N]                                     # (0 wherever the large pair did not serve)
    run_sum = torch.cat([deg.new_zeros(1), deg.cumsum(0)])
    back = torch.cat([st.long(), run_sum[nptr[1:]] - run_sum[nptr[:-1]]]).cpu().numpy()         # the one read
    status, g_edges = back[:G].astype(np.int32), back[G:].copy()

    def walk_count(i, code):
        sl = slice(int(edge_ptr[i]), int(edge_ptr[i + 1]))
        KT.khop_batch([0, int(nodes[i])], [0, sl.stop - sl.start], edge_index[:, sl].cpu().numpy(),
                      None if edge_attr is None else edge_attr[sl].cpu().numpy(), *args, num_threads=1)     # raises
        return _lib.KpgnnError(f"graph {i}: a walk count >= 2^31 within {K} hops")

    todo = refusals(status, [
        ((_lib.KHOP_ENDPOINT,), lambda i, code: ValueError(f"graph {i}: an edge endpoint lies outside its {int(nodes[i])} nodes")),
        ((_lib.KHOP_RANGE,), walk_count)])
    host = None
    if todo.size:                                           # the host route for what the kernel did not serve
        ei_h = edge_index.cpu().numpy()
        ea_h = None if edge_attr is None else edge_attr.cpu().numpy()
        esl = [np.arange(edge_ptr[i], edge_ptr[i + 1]) for i in todo]
        ecat = np.concatenate(esl)
        h_nptr = np.concatenate([[0], np.cumsum(nodes[todo])])
        h_eptr = np.concatenate([[0], np.cumsum([a.size for a in esl])])
        host = KT.khop_batch(h_nptr, h_eptr, ei_h[:, ecat], None if ea_h is None else ea_h[ecat], *args)
        g_edges[todo] = np.diff(host["edge_ptr"].numpy())
        deg[torch.from_numpy(node_ptr[todo]).to(dev)] = torch.from_numpy(g_edges[todo]).to(dev)   # on the graph's first node
    out_eptr = np.concatenate([[0], np.cumsum(g_edges)]).astype(np.int64)
    E_out = int(out_eptr[-1])
    node_off = deg.cumsum(0) - deg
    out = {"edge_index": torch.empty((2, E_out), **i64), "edge_attr": torch.empty((E_out, K), **i64),
           "pe_attr": torch.zeros((N, K - 1), **i64) if K > 1 else None,
           "peripheral_edge_attr": torch.zeros((N, K, max_edge_type, 2), **i64) if want_p else None,
           "peripheral_configuration_attr": torch.zeros((N, K, max_hop_num + 1), **i64) if want_p else None,
           "batch": torch.empty(N, **i64), "edge_ptr": torch.from_numpy(out_eptr).to(dev), "node_ptr": nptr}
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    d.node_off, d.E_out = ptr(node_off), E_out
    d.out_edge_index, d.out_edge_attr, d.out_pe_attr = ptr(out["edge_index"]), ptr(out["edge_attr"]), ptr(out["pe_attr"])
    d.out_pea, d.out_pca = ptr(out["peripheral_edge_attr"]), ptr(out["peripheral_configuration_attr"])
    d.out_batch = ptr(out["batch"])
    run(fill)
    if host is not None:
        h_off = host["edge_ptr"].numpy()
        e_dst = np.concatenate([np.arange(out_eptr[i], out_eptr[i + 1]) for i in todo])
        n_dst = np.concatenate([np.arange(node_ptr[i], node_ptr[i + 1]) for i in todo])
        shift = np.repeat(node_ptr[todo] - h_nptr[:-1], np.diff(h_off))            # host ids -> ids of this call
        e_dst, n_dst = torch.from_numpy(e_dst).to(dev), torch.from_numpy(n_dst).to(dev)
        out["edge_index"][:, e_dst] = (host["edge_index"] + torch.from_numpy(shift)).to(dev)
        out["edge_attr"][e_dst] = host["edge_attr"].to(dev)
        out["batch"][n_dst] = torch.from_numpy(np.repeat(todo, nodes[todo])).to(dev)
        for k in ("pe_attr", "peripheral_edge_attr", "peripheral_configuration_attr"):
            if out[k] is not None:
                out[k][n_dst] = host[k].to(dev)
    return out, torch.from_numpy(status)


# ------------------------------------------------------------------------------------------------ random regular graphs
RegularGraphs = collections.namedtuple("RegularGraphs", "node_ptr edge_ptr edge_index attempts exhausted route")
RegularGraphs.__doc__ = """What random_regular_graphs returns: node_ptr / edge_ptr [G+1] host int64 arrays, edge_index [2, G n d]
int64 on the call's device (LOCAL ids, (src, dst)-sorted per graph) - the triple ops.khop_transform and RawGraphs accept -
attempts [G] host int32 (pairings drawn per graph; None on the networkx route), exhausted: the graphs (host int64 array) that
used up max_attempts and were filled from networkx, and the route that served the call."""


def regular_graphs_route(n, d, dev, route="auto"):
    """The route random_regular_graphs takes: "auto" is the pairing model inside its limits - on the device where there is one,
    else on the host, the same bits - and networkx beyond them (d >= 5, n > 2048, n * d > 8192)."""
    if route not in ("auto", "device", "host", "networkx"):
        raise ValueError(f"unknown route {route!r}")
    if route != "auto":
        return route
    return "networkx" if not RG.within_limits(n, d) else "device" if dev.type == "cuda" else "host"


def random_regular_graphs(G, n, d, seed, device, first_graph=0, route="auto", max_attempts=4096):
    """G uniform random simple d-regular graphs on n nodes as raw graphs, a RegularGraphs record.  Graph g is a function of
    (seed, first_graph + g, n, d) alone: the pairing model with rejection of include/kpgnn.h (kpgnn_random_regular_graphs).
    route "device": one kpgnn_random_regular_graphs launch (csrc/regular_graphs.hip), then ONE read of attempts and status;
    edge_index never leaves the device.  Beyond the kernel's limits it raises KpgnnError.  route "host":
    regular_graphs.random_regular_graphs_host, the same bits from numpy, moved to `device` (which may be the CPU).  On both, a
    graph that used up max_attempts pairings is filled from nx.random_regular_graph(d, n, seed + first_graph + g) inside the
    same call and named in `exhausted` (at the default cap this has a probability below e^-55 for every served shape).
    route "networkx": batch.regular_graphs(G, seed + first_graph, n, d) - another draw, networkx's Steger-Wormald procedure
    on Python's Mersenne Twister, uniform only asymptotically.  "auto": regular_graphs_route.  An odd n * d or d >= n raises
    ValueError on every route."""
    G, n, d, seed, first_graph, max_attempts = int(G), int(n), int(d), int(seed), int(first_graph), int(max_attempts)
    dev = torch.device(device)
    route = regular_graphs_route(n, d, dev, route)
    RG.check_arguments(G, n, d, max_attempts, first_graph)
    m = n * d
    if route == "networkx":
        from .batch import regular_graphs
        if G == 0:
            node_ptr, edge_ptr, ei = np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros((2, 0), np.int64)
        else:
            node_ptr, edge_ptr, ei = regular_graphs(G, seed + first_graph, n=n, degree=d)
        return RegularGraphs(node_ptr, edge_ptr, torch.from_numpy(ei).to(dev), None, np.zeros(0, np.int64), route)
    if route == "host":
        node_ptr, edge_ptr, ei, attempts, status = RG.random_regular_graphs_host(G, n, d, seed, first_graph, max_attempts)
        ei = torch.from_numpy(ei).to(dev)
    else:
        if dev.type != "cuda":
            raise _lib.KpgnnError("ops.random_regular_graphs(route='device') needs a GPU device: route='host' gives the same graphs")
        ptr = np.arange(G + 1, dtype=np.int64)
        node_ptr, edge_ptr = ptr * n, ptr * m
        ei = torch.empty((2, G * m), dtype=torch.int64, device=dev)
        back = torch.empty((2, G), dtype=torch.int32, device=dev)
        desc = _lib.RrgDesc()
        desc.G, desc.n, desc.d, desc.max_attempts, desc.seed, desc.first_graph = G, n, d, max_attempts, seed, first_graph
        desc.edge_index, desc.attempts, desc.status = ei.data_ptr(), back[0].data_ptr(), back[1].data_ptr()
        _lib.launch("kpgnn_random_regular_graphs", dev, ctypes.byref(desc))
        attempts, status = back.cpu().numpy()                       # the one read
    todo = np.flatnonzero(status != _lib.RRG_OK)
    if todo.size:
        from .batch import regular_graphs
        cols = torch.from_numpy(np.concatenate([np.arange(g * m, (g + 1) * m) for g in todo])).to(dev)
        fill = np.concatenate([regular_graphs(1, seed + first_graph + int(g), n=n, degree=d)[2] for g in todo], axis=1)
        ei[:, cols] = torch.from_numpy(fill).to(dev)
    return RegularGraphs(node_ptr, edge_ptr, ei, attempts, todo.astype(np.int64), route)


# ------------------------------------------------------------------------------------------------ graph-property graphs
PROPERTY_GRAPHS_AUTO = "device"   # property_graphs(route="auto") where there is a device: DESIGN.md 5.32 has the measurement behind it

PropertyGraphs = collections.namedtuple("PropertyGraphs", "node_ptr edge_ptr edge_index features source types attempts exhausted route")
PropertyGraphs.__doc__ = """What property_graphs returns: node_ptr / edge_ptr [G+1] host int64 arrays, edge_index [2, E] int64 (LOCAL
ids, (src, dst)-sorted per graph) and features [N] float32 on the call's device - with source [G] (host int32) what
ops.graph_property_labels takes, and the triple what ops.khop_transform and RawGraphs accept - types [G] and attempts [G]
host int32, exhausted: the graphs (host int64 array) that used up max_attempts and have no edges, and the route that served
the call."""


def property_graphs_plan(nodes):
    """The launches of property_graphs: the wavefront class (n <= PG_WAVE_NODES) and the block class, each sized for its
    largest member."""
    return size_classes("kpgnn_property_graphs", nodes, (_lib.PG_WAVE_NODES, _lib.PG_MAX_NODES), largest_member(_lib.PG_MAX_NODES))


def property_graphs(nodes, seed, device, graph_type="RANDOM", first_graph=0, route="auto", max_attempts=4096, randomize=True, shuffle=True):
    """The random graphs of the reference's graph- and node-property dataset (datasets/graph_generation.py generate_graph) as
    raw graphs with their node features and source nodes, a PropertyGraphs record.  nodes: an int or a length-G sequence of
    node counts in [2, 128] (ValueError beyond, whatever the route); graph_type: a name of _lib.PG_TYPES or its id.  Graph g
    is a function of (seed, first_graph + g, nodes[g], graph_type, randomize, shuffle) alone: the definition of
    include/kpgnn.h (kpgnn_property_graphs_generate), the reference's laws on a Philox stream - another draw than the
    reference's.
    route "device": the graphs are bucketed by size on the host, one kpgnn_property_graphs_generate launch per class (n <= 64:
    a wavefront per graph; n <= 128: a block per graph), ONE read of the [5, G] block of edge counts, sources, types, attempts
    and statuses, the cumulative sum on the host, and one kpgnn_property_graphs_fill launch per class; edge_index and features
    never leave the device.  route "host": property_graphs.property_graphs_host, the same bits from numpy, moved to `device`
    (which may be the CPU).  "auto": PROPERTY_GRAPHS_AUTO on a GPU device, else the host.  A graph that used up max_attempts
    is named in `exhausted` and has no edges (STAR at 128 nodes, the slowest case, keeps all its leaves attached with
    probability 0.98^127: once in 13 attempts; 4096 rejections in a row have a probability below e^-300)."""
    if route not in ("auto", "device", "host"):
        raise ValueError(f"unknown route {route!r}")
    nodes = PG.check_nodes(nodes)
    t = PG.type_id(graph_type)
    seed, first_graph, max_attempts = int(seed), int(first_graph), int(max_attempts)
    if max_attempts < 1 or max_attempts > 1 << 27 or first_graph < 0:
        raise ValueError(f"bad max_attempts={max_attempts} first_graph={first_graph}")
    dev = torch.device(device)
    if route == "auto":
        route = PROPERTY_GRAPHS_AUTO if dev.type == "cuda" else "host"
    G = nodes.shape[0]
    if route == "host":
        node_ptr, edge_ptr, ei, feat, source, types, attempts, status = PG.property_graphs_host(
            nodes, seed, t, first_graph, max_attempts, randomize, shuffle)
        return PropertyGraphs(node_ptr, edge_ptr, torch.from_numpy(ei).to(dev), torch.from_numpy(feat).to(dev), source, types,
                              attempts, np.flatnonzero(status != _lib.PG_OK).astype(np.int64), route)
    if dev.type != "cuda":
        raise _lib.KpgnnError("ops.property_graphs(route='device') needs a GPU device: route='host' gives the same graphs")
    node_ptr = np.concatenate([[0], np.cumsum(nodes)]).astype(np.int64)
    N = int(node_ptr[-1])
    feat = torch.zeros(N, dtype=torch.float32, device=dev)
    if G == 0:
        z = np.zeros(0, dtype=np.int32)
        return PropertyGraphs(node_ptr, np.zeros(1, np.int64), torch.zeros((2, 0), dtype=torch.int64, device=dev), feat, z, z, z,
                              np.zeros(0, np.int64), route)
    nodes32 = np.ascontiguousarray(nodes.astype(np.int32))
    nptr = torch.from_numpy(node_ptr).to(dev)
    rows = torch.empty((N, 2), dtype=torch.int64, device=dev)
    info = torch.empty((5, G), dtype=torch.int32, device=dev)
    d = _lib.PgDesc()
    d.G, d.nodes, d.node_ptr = G, nodes32.ctypes.data, nptr.data_ptr()
    d.graph_type, d.max_attempts, d.seed, d.first_graph = t, max_attempts, seed, first_graph
    d.flags = (0 if shuffle else _lib.PG_NO_SHUFFLE) | (0 if randomize else _lib.PG_NO_RANDOMIZE)
    d.rows, d.features, d.info = rows.data_ptr(), feat.data_ptr(), info.data_ptr()
    plan = [(ids, cap, torch.from_numpy(ids.astype(np.int32)).to(dev)) for _, ids, cap, _ in property_graphs_plan(nodes)]

    def run(entry):
        for ids, cap, ids_d in plan:
            d.graph_ids, d.n_ids, d.max_nodes = ids_d.data_ptr(), ids.size, cap
            _lib.launch(entry, dev, ctypes.byref(d))

    run("kpgnn_property_graphs_generate")
    counts, source, types, attempts, status = info.cpu().numpy()        # the one read
    edge_ptr = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)
    E = int(edge_ptr[-1])
    ei = torch.empty((2, E), dtype=torch.int64, device=dev)
    eptr = torch.from_numpy(edge_ptr).to(dev)
    d.edge_ptr, d.edge_index, d.E = eptr.data_ptr(), ei.data_ptr() if E else None, E
    run("kpgnn_property_graphs_fill")
    return PropertyGraphs(node_ptr, edge_ptr, ei, feat, source.copy(), types.copy(), attempts.copy(),
                          np.flatnonzero(status != _lib.PG_OK).astype(np.int64), route)
