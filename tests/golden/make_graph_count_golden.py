"""Writes tests/golden/graph_count.npz: the graphs of tests/graph_count_cases.py and, for each, the y row [5] float64 that the
reference's GraphCountDataset.process computes on the CPU.

    python tests/golden/make_graph_count_golden.py --reference /path/to/reference/checkout

The reference's datasets/GraphCountDataset.py is loaded by path, at generation time only.  It imports torch_geometric, which
this project does not need: minimal stand-ins of our own for torch_geometric.data.InMemoryDataset and Data go into
sys.modules first.  The cases' dense float64 adjacencies are written to a temporary randomgraph.mat (an object array under
the key A, a dummy F and index vectors) and process() is called on an instance made with __new__, whose raw_paths,
processed_paths and collate are ours and with torch.save patched out for the call.  Nothing of the reference's text is written
anywhere: the fixture holds edge lists (graphs of at most 64 nodes; larger ones are regenerated from the cases module and
only their node and directed-edge counts are kept) and recorded numbers."""
import argparse
import importlib.util
import os
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import graph_count_cases as GC  # noqa: E402


def _stand_ins():
    class InMemoryDataset:
        pre_filter = None
        pre_transform = None

    class Data:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    tg, data, data_data = types.ModuleType("torch_geometric"), types.ModuleType("torch_geometric.data"), types.ModuleType("torch_geometric.data.data")
    data.InMemoryDataset, data.Data, data_data.Data = InMemoryDataset, Data, Data
    tg.data, data.data = data, data_data
    sys.modules.update({"torch_geometric": tg, "torch_geometric.data": data, "torch_geometric.data.data": data_data})


def reference_rows(reference, graphs):
    """[(n, edge_index)] -> (y [G,5] float64 of the reference's process(), its wall time in seconds)."""
    import scipy.io as sio
    import torch
    _stand_ins()
    spec = importlib.util.spec_from_file_location("ref_graph_count_dataset", os.path.join(reference, "datasets", "GraphCountDataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    A = np.empty((1, len(graphs)), dtype=object)
    for i, (n, ei) in enumerate(graphs):
        a = np.zeros((n, n))
        a[ei[0], ei[1]] = 1.0
        A[0, i] = a
    got = []
    with tempfile.TemporaryDirectory() as tmp:
        mat = os.path.join(tmp, "randomgraph.mat")
        idx = np.arange(len(graphs))[None, :]
        sio.savemat(mat, {"A": A, "F": np.zeros((len(graphs), 1)), "train_idx": idx, "val_idx": idx, "test_idx": idx})
        ds = mod.GraphCountDataset.__new__(mod.GraphCountDataset)
        ds.raw_paths, ds.processed_paths = [mat], [os.path.join(tmp, "data.pt")]
        ds.collate = lambda data_list: (got.extend(data_list), None)
        save, torch.save = torch.save, lambda *a, **k: None
        try:
            t0 = time.perf_counter()
            ds.process()
            seconds = time.perf_counter() - t0
        finally:
            torch.save = save
    assert len(got) == len(graphs)
    for d in got:
        assert d.y.dtype == torch.float64 and tuple(d.y.shape) == (1, 5)
    return np.stack([d.y.numpy()[0] for d in got]), seconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (holds datasets/GraphCountDataset.py)")
    ap.add_argument("--out", default=GC.GOLDEN)
    args = ap.parse_args()
    arrays = {}
    for group, cases in GC.groups():
        names = list(cases)
        y, _ = reference_rows(args.reference, [cases[k] for k in names])
        arrays[group + "/names"] = np.asarray(names)
        for k, row in zip(names, y):
            n, ei = cases[k]
            arrays[f"{k}/n"], arrays[f"{k}/edges"], arrays[f"{k}/y"] = np.int64(n), np.int64(ei.shape[1]), row
            if n <= 64:
                arrays[f"{k}/ei"] = ei.astype(np.int16)
            print(f"{group} {k}: n {n} directed edges {ei.shape[1]} y {row.tolist()}", flush=True)
    np.savez_compressed(args.out, **arrays)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
