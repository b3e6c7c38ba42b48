"""Writes tests/golden/graph_property_large.npz: the 17 graphs of 65 to 128 nodes of tests/graph_property_large_cases.py
(fixture_cases) with their features and source node, and for each what the reference's label functions answer on the CPU, as
float64.

    python tests/golden/make_graph_property_large_golden.py --reference /path/to/reference/checkout

As make_graph_property_golden.py: the reference's datasets/graph_algorithms.py (it imports only math, queue and numpy) is loaded
by path, at generation time only, and called the way genereate_dataset calls it, on the dense float64 0/1 adjacency.  Its
all-pairs shortest paths are a triple Python loop run three times per graph, about two seconds each at 128 nodes: the whole file
takes about a minute.  Nothing of the reference's text is written anywhere: the fixture holds edge lists, features and recorded
numbers."""
import argparse
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import graph_property_cases as GC  # noqa: E402
import graph_property_large_cases as GL  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (holds datasets/graph_algorithms.py)")
    ap.add_argument("--out", default=GL.GOLDEN)
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_graph_algorithms", os.path.join(args.reference, "datasets", "graph_algorithms.py"))
    ga = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ga)
    cases = GL.fixture_cases()
    arrays = {"names": np.asarray(list(cases))}
    for name, (n, ei, F, s) in GC.inputs(cases, seed=29).items():
        adj = np.zeros((n, n))
        adj[ei[0], ei[1]] = 1.0
        assert (adj == adj.T).all() and not adj.diagonal().any()
        with np.errstate(all="ignore"):
            node = np.stack([ga.all_pairs_shortest_paths(adj, 0)[s], ga.eccentricity(adj), ga.graph_laplacian_features(adj, F)], axis=1)
            graph = np.asarray([ga.is_connected(adj), ga.diameter(adj), ga.spectral_radius(adj)], dtype=np.float64)
        # ei as int16 and the integer columns as they are: np.load gives them back, the tests widen
        for k, v in (("n", np.int64(n)), ("ei", ei.astype(np.int16)), ("F", F), ("source", np.int64(s)), ("node", node.astype(np.float64)), ("graph", graph)):
            arrays[f"{name}/{k}"] = v
        print(f"{name}: n {n} edges {ei.shape[1] // 2} source {s} graph labels {graph.tolist()}", flush=True)
    np.savez_compressed(args.out, **arrays)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
