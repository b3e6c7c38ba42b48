"""ops.graph_property_labels on graphs of 65 to 100 nodes - the reference's extrapolation sizes: large="device", the kernel of
csrc/graph_labels.hip (W = 2), against large="host", the default, which leaves every such graph to the float64 numpy route.

    python scripts/graph_labels_large.py --out profiles/graph_labels_large/graph_labels_large.json
    python scripts/graph_labels_large.py --graphs 200 --rounds 1                # a smaller look

The graphs are drawn with plain numpy, seeded, symmetric, without self loops: G(n, p) at p = 0.03, 0.06, 0.12 and 0.3 (a fifth
of the graphs each) and, for the last fifth, random recursive trees, ladders and grids in turn (a ladder of n // 2 rungs and
the most square grid of at most n nodes: a node left over stays isolated).  The reference's own mix of generators needs
networkx and is not reproduced here.  ONE process, the two settings ALTERNATING per round, `--rounds` (3) rounds after one
warm-up call of each; every figure is the wall time of a whole ops.graph_property_labels(route="device") call from host arrays
to labels on the device, ended by a device synchronise: launches, the one status read-back and every host fill included.  The
host fill runs numpy with the BLAS threads the environment sets (`host_threads`).  The two settings' labels are compared: how
many of the integer labels (sssp, eccentricity, is_connected, diameter) and of the float32 spectral radii differ."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSITIES = (0.03, 0.06, 0.12, 0.3)


def pairs_of(kind, n, rng):
    """Undirected pairs (u [e], v [e]) of one graph of n nodes."""
    import numpy as np
    if kind < len(DENSITIES):
        u, v = np.nonzero(np.triu(rng.random((n, n)) < DENSITIES[kind], 1))
        return u, v
    shape = (kind - len(DENSITIES)) % 3
    if shape == 0:                                          # a random recursive tree: node i hangs off a node before it
        v = np.arange(1, n)
        return (rng.random(n - 1) * v).astype(np.int64), v
    if shape == 1:                                          # a ladder
        r = n // 2
        a = np.arange(r - 1)
        return np.concatenate([a, a + r, np.arange(r)]), np.concatenate([a + 1, a + r + 1, np.arange(r) + r])
    rows = int(n ** 0.5)                                    # a grid
    cols = n // rows
    idx = np.arange(rows * cols).reshape(rows, cols)
    return np.concatenate([idx[:, :-1].ravel(), idx[:-1].ravel()]), np.concatenate([idx[:, 1:].ravel(), idx[1:].ravel()])


def draw(G, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    nptr, eptr, eis, src, kinds = [0], [0], [], [], {}
    for g in range(G):
        n = int(rng.integers(65, 101))
        kind = g % 5 if g % 5 < len(DENSITIES) else len(DENSITIES) + (g // 5) % 3
        u, v = pairs_of(kind, n, rng)
        ei = np.stack([np.concatenate([u, v]), np.concatenate([v, u])]).astype(np.int64)
        assert ei.size == 0 or (int(ei.max()) < n and not (ei[0] == ei[1]).any())
        eis.append(ei)
        nptr.append(nptr[-1] + n)
        eptr.append(eptr[-1] + ei.shape[1])
        src.append(int(rng.integers(0, n)))
        name = f"gnp_{DENSITIES[kind]}" if kind < len(DENSITIES) else ("tree", "ladder", "grid")[kind - len(DENSITIES)]
        kinds[name] = kinds.get(name, 0) + 1
    return (np.asarray(nptr, dtype=np.int64), np.asarray(eptr, dtype=np.int64), np.concatenate(eis, axis=1), rng.random(nptr[-1]),
            np.asarray(src, dtype=np.int64)), kinds


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from kp_gnn_amd import ops
    dev = torch.device("cuda:0")
    (nptr, eptr, ei, F, src), kinds = draw(args.graphs, 4321)

    def call(large):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        node, graph = ops.graph_property_labels(nptr, eptr, ei, F, src, dev, route="device", large=large)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, node.cpu(), graph.cpu()

    times, last = {"device": [], "host": []}, {}
    for large in times:                                      # warm-up of each at the timed shape
        call(large)
    for _ in range(args.rounds):
        for large in times:                                  # alternating: a drift of the machine reaches both alike
            ms, node, graph = call(large)
            times[large].append(ms)
            last[large] = (node, graph)
        print("[graph_labels_large] round done", file=sys.stderr, flush=True)
    (node_d, graph_d), (node_h, graph_h) = last["device"], last["host"]
    as_int = lambda t: t.contiguous().view(torch.int32).long()  # noqa: E731
    ulps = (as_int(graph_d[:, 2]) - as_int(graph_h[:, 2])).abs()
    nodes = np.diff(nptr)
    result = {"device": torch.cuda.get_device_name(0), "graphs": args.graphs, "nodes": int(nptr[-1]), "edges": int(eptr[-1]),
              "min_nodes": int(nodes.min()), "max_nodes": int(nodes.max()), "kinds": kinds, "rounds": args.rounds,
              "host_threads": os.environ.get("OMP_NUM_THREADS"), "torch_threads": torch.get_num_threads(),
              "connected_by_the_rule": int(graph_d[:, 0].sum()),
              "integer_node_labels_that_differ": int((node_d[:, :2] != node_h[:, :2]).sum()),
              "integer_graph_labels_that_differ": int((graph_d[:, :2] != graph_h[:, :2]).sum()),
              "spectral_radii_that_differ": int((ulps != 0).sum()), "spectral_radius_max_f32_ulps": int(ulps.max()),
              "laplacian_max_abs_diff": float((node_d[:, 2].double() - node_h[:, 2].double()).abs().max()),
              "large_device_ms": spread(times["device"]), "large_host_ms": spread(times["host"]),
              "host_over_device": statistics.median(times["host"]) / statistics.median(times["device"])}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
