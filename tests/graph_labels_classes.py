"""What test_graph_property_classes.py and golden/make_graph_labels_bits.py share: the cases whose bits are recorded, their input
checksums, and raw launches of one instantiation of the label kernel template (csrc/graph_labels.hip) into poisoned outputs."""
import os
import zlib

import numpy as np

import graph_property_cases as GC
import graph_property_large_cases as GL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_labels_bits.npz")
SMALL, LARGE = "kpgnn_graph_labels", "kpgnn_graph_labels_large"
WAVE_NODES = 32
# instantiation -> (entry, max_nodes of the launch, the largest graph it is given)
CLASSES = {"wave": (SMALL, 32, 32), "block": (SMALL, 64, 64), "large": (LARGE, 128, 128)}


def _fixture(path, names_key):
    z = np.load(path)
    return {k: (int(z[f"{k}/n"]), z[f"{k}/ei"].astype(np.int64), z[f"{k}/F"], int(z[f"{k}/source"])) for k in z[names_key].tolist()}


def small_cases():
    """name -> (n, edge_index, F, source): the 53 served graphs of golden/graph_property.npz and the 24 edge-size cases."""
    c = {f"fixture/{k}": v for k, v in _fixture(GC.GOLDEN, "served/names").items()}
    c.update({f"edge/{k}": v for k, v in GC.inputs(GC.edge_size_cases(), seed=5).items()})
    assert len(c) == 53 + 3 * len(GC.EDGE_SIZES)
    return c


def large_cases():
    """name -> (n, edge_index, F, source): the 17 graphs of golden/graph_property_large.npz and the 41 boundary cases."""
    c = {f"fixture/{k}": v for k, v in _fixture(GL.GOLDEN, "names").items()}
    c.update({f"boundary/{k}": v for k, v in GC.inputs(GL.boundary_cases(), seed=7).items()})
    assert len(c) == 17 + 5 * len(GL.BOUNDARY_SIZES) + 1
    return c


def cases_of(cls):
    """The cases recorded through the instantiation `cls`, in launch order."""
    c = large_cases() if cls == "large" else small_cases()
    return {k: v for k, v in c.items() if v[0] <= CLASSES[cls][2]}


def checksum(item):
    """zlib.crc32 of a case's inputs as the kernel reads them: n and source, edge_index as int64, F as float64."""
    n, ei, F, s = item
    raw = np.asarray([n, s], dtype=np.int64).tobytes() + np.ascontiguousarray(ei, dtype=np.int64).tobytes() + np.ascontiguousarray(F, dtype=np.float64).tobytes()
    return np.uint32(zlib.crc32(raw))


def launch(ops, items, ids, max_nodes, entry):
    """The graphs `ids` of the call `items` in ONE launch of `entry` sized for max_nodes, into NaN-poisoned outputs with status
    preset to -7: (node_ptr, node_out bits [N,3] int32, graph_out bits [G,3] int32, status [G] int32) as numpy arrays."""
    import torch
    dev = torch.device("cuda:0")
    nptr, eptr, ei, F, src = GC.pack(items)
    G, N, E = len(items), int(nptr[-1]), int(eptr[-1])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)  # noqa: E731
    node = torch.full((N, 3), float("nan"), dtype=torch.float32, device=dev)
    graph = torch.full((G, 3), float("nan"), dtype=torch.float32, device=dev)
    st = torch.full((G,), -7, dtype=torch.int32, device=dev)
    ops.graph_labels_launch(G, t(nptr, torch.int64), t(eptr, torch.int64), t(ei, torch.int64), E, t(F, torch.float64), t(src, torch.int32),
                            t(np.asarray(ids, dtype=np.int64), torch.int32), max_nodes, node, graph, st, entry=entry)
    torch.cuda.synchronize()
    bits = lambda x: x.cpu().contiguous().view(torch.int32).numpy()  # noqa: E731
    return nptr, bits(node), bits(graph), st.cpu().numpy()


def run_class(ops, cls):
    """name -> (node bits [n,3], graph bits [3], status) of cases_of(cls), all in one launch of that instantiation."""
    cases = cases_of(cls)
    entry, max_nodes, _ = CLASSES[cls]
    nptr, node, graph, st = launch(ops, list(cases.values()), np.arange(len(cases)), max_nodes, entry)
    return {k: (node[nptr[i]:nptr[i + 1]], graph[i], int(st[i])) for i, k in enumerate(cases)}
