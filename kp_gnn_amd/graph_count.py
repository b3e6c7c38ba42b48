"""The synthetic substructure-counting task (the reference's datasets/GraphCountDataset.py process, which feeds
train_structure_counting.py): the five labels of raw graphs, their normalisation and the training target.

    y [G,5] float64   tri | tailed | star | cyc4 | cus         (the reference's order; its y is float64 too)

count_labels_host_f64 is the float64 numpy route and the specification of ops.count_labels (the device route,
csrc/count_labels.hip).  It writes the reference's five expressions LITERALLY, as float64 matrix expressions on the dense 0/1
matrix of each graph - not in the reduced integer form the kernel uses - so that a directed list and a list with self loops
keep the reference's answer.  The reading of the .mat file, the index vectors and the graph generators are not part of it.
"""
import numpy as np
import torch

from .raw_graphs import RawGraphs

COUNT_LABELS = ("tri", "tailed", "star", "cyc4", "cus")


def check_graph(g, n, ei):
    """The one refusal both routes share (kpgnn.h KPGNN_CL_ENDPOINT): ValueError naming graph g."""
    if ei.size and (int(ei.min()) < 0 or int(ei.max()) >= n):
        raise ValueError(f"graph {g}: an edge endpoint lies outside its nodes [0, {n})")


def labels_one(n, ei):
    """One graph, float64 [5]: GraphCountDataset.process on the dense matrix a of the edge list ei [2,e] (local ids)."""
    if n == 0:
        return np.zeros(5)
    a = np.zeros((n, n))
    a[ei[0], ei[1]] = 1.0
    A2 = a.dot(a)
    A3 = A2.dot(a)
    deg = a.sum(0)
    tri = np.trace(A3) / 6
    tailed = ((np.diag(A3) / 2) * (deg - 2)).sum()
    cyc4 = 1 / 8 * (np.trace(A3.dot(a)) + np.trace(A2) - 2 * A2.sum())
    cus = (a * np.exp(-A2.sum(1))[None, :]).dot(a).sum()           # a . diag(w) . a: a . diag(w) scales the columns of a
    d = deg.astype(np.int64)
    star = float((d * (d - 1) * (d - 2) // 6).sum())                # sum of comb(deg, 3), exact
    return np.asarray([tri, tailed, star, cyc4, cus], dtype=np.float64)


def _split(node_ptr, edge_ptr, edge_index):
    g = RawGraphs(node_ptr, edge_ptr, edge_index)
    return g.node_ptr, g.edge_ptr, g.edge_index_host()


def count_labels_host_f64(node_ptr, edge_ptr, edge_index, graphs=None):
    """The float64 labels [G,5] of the graphs `graphs` (all when None), rows of other graphs zero.  node_ptr / edge_ptr [G+1]
    offsets, edge_index [2,E] LOCAL ids grouped by graph.  An edge endpoint outside its graph raises ValueError naming the
    graph."""
    node_ptr, edge_ptr, ei = _split(node_ptr, edge_ptr, edge_index)
    G = node_ptr.shape[0] - 1
    y = np.zeros((G, 5))
    for g in (range(G) if graphs is None else graphs):
        n, e0, e1 = int(node_ptr[g + 1] - node_ptr[g]), int(edge_ptr[g]), int(edge_ptr[g + 1])
        check_graph(int(g), n, ei[:, e0:e1])
        y[g] = labels_one(n, ei[:, e0:e1])
    return y


def count_labels_host(node_ptr, edge_ptr, edge_index, device="cpu"):
    """count_labels_host_f64 as a float64 tensor [G,5] on `device`."""
    return torch.from_numpy(count_labels_host_f64(node_ptr, edge_ptr, edge_index)).to(torch.device(device))


def normalize_count_labels(y):
    """train_structure_counting.py: every column divided by its standard deviation over the WHOLE dataset (torch's default,
    unbiased).  Plain torch division, so a column of zero deviation gives inf / nan as there."""
    return y / y.std(0)


def count_targets(y, task):
    """Column `task` (an index, or a name of COUNT_LABELS) of the labels as float32 [G]: the target of
    regression_loss(score, target, "l1"), the reference's |score - y[:, task]|.mean()."""
    if isinstance(task, str):
        task = COUNT_LABELS.index(task)
    if not 0 <= int(task) < len(COUNT_LABELS):
        raise ValueError(f"task {task} is not one of the {len(COUNT_LABELS)} label columns")
    return y[:, int(task)].to(torch.float32).contiguous()
