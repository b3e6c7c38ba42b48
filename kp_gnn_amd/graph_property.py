"""The synthetic graph- and node-property task (the reference's datasets/GraphPropertyDataset.py, which feeds
train_graph_property.py and train_node_property.py): the labels of raw graphs, their normalisation and the input features.

    node labels  [N,3]  sssp | eccentricity | graph_laplacian_features      (the order of genereate_dataset: the sssp row first)
    graph labels [G,3]  is_connected | diameter | spectral_radius

graph_property_labels_host is the float64 numpy route and the specification of ops.graph_property_labels (the device route,
csrc/graph_labels.hip).  It restates datasets/graph_algorithms.py without its triple loop: all-pairs shortest paths by a
vectorised BFS over boolean matrices (the reference runs Floyd-Warshall three times per graph), the spectral radius by
eigvalsh, and is_connected LITERALLY - m = 1 + ceil(log2 n) float64 squarings and min > 0 - so that a graph of more than 64
nodes keeps the reference's answer, overflow included (an overflowed product makes inf * 0 = nan, and nan > 0 is False).  The
rule is "every ordered pair has a walk of length exactly 2^m", not connectivity: a connected bipartite graph answers False.
An asymmetric (directed) list takes max(axis=0) over the directed distances and np.linalg.eig, as the reference does.
"""
import collections
import math

import numpy as np
import torch

from .raw_graphs import RawGraphs, i64

NODE_LABELS = ("sssp", "eccentricity", "graph_laplacian_features")
GRAPH_LABELS = ("is_connected", "diameter", "spectral_radius")


def check_graph(g, n, ei, s):
    """The refusals both routes share (kpgnn.h KPGNN_GL_ENDPOINT / _SELF_LOOP / _SOURCE, in that order): ValueError naming graph g."""
    if ei.size and (int(ei.min()) < 0 or int(ei.max()) >= n):
        raise ValueError(f"graph {g}: an edge endpoint lies outside its nodes [0, {n})")
    if bool((ei[0] == ei[1]).any()):
        raise ValueError(f"graph {g}: a self loop (the labels are defined for graphs without one)")
    if n > 0 and not 0 <= s < n:
        raise ValueError(f"graph {g}: source {s} lies outside its nodes [0, {n})")


def distances(A):
    """dist[i, j]: the length of the shortest directed path i -> j over the boolean adjacency A, -1 where there is none; all
    sources advance together, one boolean matrix product per level."""
    n = A.shape[0]
    dist = np.full((n, n), -1, dtype=np.int64)
    seen = np.eye(n, dtype=bool)
    dist[seen] = 0
    front, Ai, level = seen.astype(np.float32), A.astype(np.float32), 0
    while True:
        nxt = (front @ Ai > 0) & ~seen
        if not nxt.any():
            return dist
        level += 1
        dist[nxt] = level
        seen |= nxt
        front = nxt.astype(np.float32)


def labels_one(n, ei, F, s):
    """One graph, float64: (node labels [n,3], graph labels [3]).  ei [2,e] local ids, F [n], s the source node."""
    node, graph = np.zeros((n, 3)), np.zeros(3)
    if n == 0:
        return node, graph
    A = np.zeros((n, n), dtype=bool)
    A[ei[0], ei[1]] = True
    Af = A.astype(np.float64)
    dist = distances(A)
    node[:, 0] = np.maximum(dist[s], 0)                        # all_pairs_shortest_paths(adj, 0)[source]: unreachable -> 0
    node[:, 1] = dist.max(axis=0)                              # unreachable pairs are -1, the diagonal is 0
    node[:, 2] = Af.sum(axis=0) * F - Af @ F                   # graph_laplacian(A) @ F
    B = Af
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(int(1 + math.ceil(math.log2(n)))):
            B = np.dot(B, B)
        graph[0] = float(np.min(B) > 0)
    graph[1] = dist.max()
    if not A.any():
        graph[2] = 0.0
    elif (A == A.T).all():
        graph[2] = np.abs(np.linalg.eigvalsh(Af)).max()
    else:
        W = np.linalg.eig(Af)[0]
        graph[2] = np.abs(W[np.argmax(np.absolute(W))].real)
    return node, graph


def _split(node_ptr, edge_ptr, edge_index, features, source):
    g = RawGraphs(node_ptr, edge_ptr, edge_index, source=source)
    F = np.asarray(features.cpu() if torch.is_tensor(features) else features)
    if F.dtype not in (np.float32, np.float64):
        raise ValueError("features must be float32 or float64")
    F = F.astype(np.float64).reshape(-1)
    if F.shape[0] != g.N:
        raise ValueError("features does not match node_ptr")
    return g.node_ptr, g.edge_ptr, g.edge_index_host(), F, g.source


def labels_host_f64(node_ptr, edge_ptr, edge_index, features, source, graphs=None):
    """The float64 labels of the graphs `graphs` (all when None): (node [N,3], graph [G,3]) float64 arrays, rows of other
    graphs zero."""
    node_ptr, edge_ptr, ei, F, source = _split(node_ptr, edge_ptr, edge_index, features, source)
    G = node_ptr.shape[0] - 1
    node, graph = np.zeros((int(node_ptr[-1]), 3)), np.zeros((G, 3))
    for g in (range(G) if graphs is None else graphs):
        n0, n1, e0, e1 = int(node_ptr[g]), int(node_ptr[g + 1]), int(edge_ptr[g]), int(edge_ptr[g + 1])
        check_graph(g, n1 - n0, ei[:, e0:e1], int(source[g]))
        node[n0:n1], graph[g] = labels_one(n1 - n0, ei[:, e0:e1], F[n0:n1], int(source[g]))
    return node, graph


def graph_property_labels_host(node_ptr, edge_ptr, edge_index, features, source, device="cpu", route="host"):
    """The labels of G raw graphs by the float64 host route: (node_labels [N,3] float32, graph_labels [G,3] float32) on
    `device`, each value rounded to float once.  node_ptr / edge_ptr [G+1] offsets, edge_index [2,E] LOCAL ids grouped by
    graph, features [N] float32 or float64, source [G] the local id of each graph's source node.  An edge endpoint outside its
    graph, a self loop or a source outside its graph raise ValueError naming the first such graph."""
    if route != "host":
        raise ValueError(f"graph_property_labels_host is the host route, got route {route!r}")
    node, graph = labels_host_f64(node_ptr, edge_ptr, edge_index, features, source)
    dev = torch.device(device)
    return torch.from_numpy(node.astype(np.float32)).to(dev), torch.from_numpy(graph.astype(np.float32)).to(dev)


def normalize_labels(node_labels, graph_labels, node_ptr, train_ids):
    """GraphPropertyDataset.process: every label column divided by its maximum over the TRAINING graphs `train_ids` (node
    columns: over their nodes).  Plain torch division, so a column whose training maximum is 0 gives 0 / 0 = nan as there."""
    ptr = torch.as_tensor(i64(node_ptr))
    ids = torch.as_tensor(i64(train_ids))
    rows = torch.cat([torch.arange(int(ptr[g]), int(ptr[g + 1])) for g in ids.tolist()]) if ids.numel() else ids
    max_node = node_labels[rows.to(node_labels.device)].max(0)[0]
    max_graph = graph_labels[ids.to(graph_labels.device)].max(0)[0]
    return node_labels / max_node, graph_labels / max_graph


GraphPropertySplit = collections.namedtuple("GraphPropertySplit", "node_ptr edge_ptr edge_index x pos y")


def generate_split(nodes, seed, device, graph_type="RANDOM", first_graph=0, route="auto", large="device"):
    """One split of the dataset from its seed (the reference's GenerateGraphPropertyDataset for one list of node counts): the
    graphs of ops.property_graphs(nodes, seed, device, graph_type, first_graph, route), their labels by
    ops.graph_property_labels on the same tensors (route and `large` passed on) and their inputs, as (node_ptr, edge_ptr: host
    int64; edge_index [2,E] int64, x [N,2] float32 = source_features, pos [N,3] float32 node labels, y [G,3] float32 graph
    labels: on `device`) - what normalize_labels and KHopDataset.from_graphs(pos=) take.  KpgnnError if a graph used up its
    attempts.  On a GPU device no graph exists on the host at any point."""
    from . import _lib, ops_dataset
    g = ops_dataset.property_graphs(nodes, seed, device, graph_type=graph_type, first_graph=first_graph, route=route)
    if g.exhausted.size:
        raise _lib.KpgnnError(f"graph {int(g.exhausted[0])} (and {g.exhausted.size - 1} more) found no graph without an isolated node")
    pos, y = ops_dataset.graph_property_labels(g.node_ptr, g.edge_ptr, g.edge_index, g.features, g.source, device,
                                               route=g.route, large=large)
    return GraphPropertySplit(g.node_ptr, g.edge_ptr, g.edge_index, source_features(g.features, g.source, g.node_ptr), pos, y)


def reference_splits(extrapolation=False):
    """The node counts of the reference's splits (GraphPropertyDataset.py genereate_dataset), a dict of int64 arrays in the
    reference's order - the sizes of a split in turn, all graphs of a size together.  "train": 512 graphs of each size
    15 .. 24.  "val" and "test": 128 and 256 graphs of each size 15 .. 19 - the reference pairs its FIVE counts with the first
    five sizes of range(15, 25).  With extrapolation, instead of "test", the nine splits "test-(20,25)", "test-(25,30)",
    "test-(30,35)", "test-(35,40)", "test-(40,45)", "test-(45,50)", "test-(60,65)", "test-(75,80)" and "test-(95,100)" of
    256 graphs of each of their five sizes."""
    def counts(per, sizes):
        return np.repeat(np.asarray(sizes, dtype=np.int64), per)

    out = {"train": counts(512, range(15, 25)), "val": counts(128, range(15, 20))}
    if not extrapolation:
        out["test"] = counts(256, range(15, 20))
        return out
    for lo in (20, 25, 30, 35, 40, 45, 60, 75, 95):
        out[f"test-({lo},{lo + 5})"] = counts(256, range(lo, lo + 5))
    return out


def source_features(x_feature, source, node_ptr):
    """The reference's node input [one-hot(source), feature] as float32 [N,2] (GenerateGraphPropertyDataset: to_categorical of
    the source node stacked with the random feature), on x_feature's device."""
    ptr, source = i64(node_ptr), i64(source)
    x_feature = torch.as_tensor(x_feature)
    out = torch.zeros((int(ptr[-1]), 2), dtype=torch.float32, device=x_feature.device)
    if bool(((source < 0) | (source >= np.diff(ptr))).any()):
        raise ValueError("source outside its graph")
    out[torch.as_tensor(ptr[:-1] + source, device=out.device), 0] = 1.0
    out[:, 1] = x_feature.reshape(-1).to(torch.float32)
    return out
