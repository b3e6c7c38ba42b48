"""The validated view of a call over raw graphs (node_ptr, edge_ptr, edge_index), shared by the device front end
(ops_dataset.py) and the float64 host routes (graph_property.py, graph_count.py).  Host only: numpy and torch, never the HIP
library.  khop_transform.khop_batch checks less than this and keeps its own lines."""
import numpy as np
import torch


def i64(a):
    """`a` (a tensor on any device, an array, a list) as a flat contiguous int64 array on the host."""
    return np.ascontiguousarray(np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.int64)).reshape(-1)


class RawGraphs:
    """G graphs: node_ptr / edge_ptr [G+1] contiguous int64 host arrays, nodes = diff(node_ptr), N nodes and E edges in all,
    edge_index [2,E] - a tensor left on the device it came on (an array or a list becomes an int64 host tensor) - and, where
    the op takes one, source [G] as int64.  Anything else raises ValueError: the counts, then the offsets, then edge_index."""

    def __init__(self, node_ptr, edge_ptr, edge_index, source=None):
        self.node_ptr, self.edge_ptr = i64(node_ptr), i64(edge_ptr)
        self.source = None if source is None else i64(source)
        self.G = G = self.node_ptr.shape[0] - 1
        if G < 0 or self.edge_ptr.shape[0] != G + 1 or (source is not None and self.source.shape[0] != G):
            raise ValueError("node_ptr and edge_ptr must both have G + 1 entries" if source is None else
                             "node_ptr and edge_ptr must have G + 1 entries and source G")
        self.nodes = np.diff(self.node_ptr)
        if self.node_ptr[0] != 0 or self.edge_ptr[0] != 0 or bool((self.nodes < 0).any()) or bool((np.diff(self.edge_ptr) < 0).any()):
            raise ValueError("node_ptr / edge_ptr must start at 0 and not decrease")
        self.N, self.E = int(self.node_ptr[-1]), int(self.edge_ptr[-1])
        if not torch.is_tensor(edge_index):
            edge_index = torch.from_numpy(np.ascontiguousarray(np.asarray(edge_index, dtype=np.int64)))
        if edge_index.numel() != 2 * self.E:
            raise ValueError("edge_index does not match edge_ptr")
        self.edge_index = edge_index.reshape(2, self.E)

    def edge_index_host(self):
        """edge_index as an int64 array on the host."""
        return np.asarray(self.edge_index.cpu(), dtype=np.int64)
