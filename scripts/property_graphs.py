"""ops.property_graphs at the reference's split shapes: the device route against the host route of the same call.

    python scripts/property_graphs.py --out profiles/property_graphs/call.json
    python scripts/property_graphs.py --splits train --reps 3 --no-networkx

Per split (graph_property.reference_splits(extrapolation=True): "train" is 5,120 graphs of 15 .. 24 nodes, "test-(95,100)" 1,280
graphs of 95 .. 99):
  device   the whole call - launches per size class, the one read-back, the cumulative sum, the fill launches - `--reps` times
           after a warm-up, wall clock between two device synchronisations: median, min and max in milliseconds; and the
           generate launches alone between two stream events ("generate_ms").
  host     property_graphs_host through the same front end, once, wall clock.
  The two results are compared field by field before a time is reported.
"networkx": for scale, the time per graph of the plain networkx constructors behind each type (no shuffle, no randomize, no
retry) at the split's smallest and largest size, over `--draws` graphs each.  The reference's own generator is not run here."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def networkx_ms(n, draws):
    """{type: milliseconds per graph} of the networkx constructors at n nodes."""
    import math
    import random

    import networkx as nx
    r = max(i for i in range(1, int(math.isqrt(n)) + 1) if n % i == 0)
    rng = random.Random(0)

    def attach(levels):
        G = nx.empty_graph(n)
        B = rng.randrange(1, n)
        F = rng.randrange(B + 1, n + 1) if levels == 2 else n
        G.add_edges_from((i - 1, i) for i in range(1, B))
        G.add_edges_from((i, rng.randrange(B)) for i in range(B, F))
        G.add_edges_from((i, rng.randrange(B, F)) for i in range(F, n))
        return G

    makers = {
        "ERDOS_RENYI": lambda s: nx.fast_gnp_random_graph(n, rng.random(), s),
        "BARABASI_ALBERT": lambda s: nx.barabasi_albert_graph(n, rng.randrange(1, n), s),
        "GRID": lambda s: nx.grid_2d_graph(r, n // r),
        "CAVEMAN": lambda s: nx.caveman_graph(r, n // r),
        "TREE": lambda s: nx.random_powerlaw_tree(n, seed=s, tries=10000),
        "LADDER": lambda s: nx.ladder_graph(n // 2),
        "LINE": lambda s: nx.path_graph(n),
        "STAR": lambda s: nx.star_graph(n - 1),
        "CATERPILLAR": lambda s: attach(1),
        "LOBSTER": lambda s: attach(2),
    }
    out = {}
    for name, make in makers.items():
        t0, made = time.perf_counter(), 0
        for s in range(draws):
            try:
                nx.to_numpy_array(make(s))
                made += 1
            except nx.NetworkXError:        # a power-law tree sequence that found no tree
                pass
        out[name] = (time.perf_counter() - t0) * 1e3 / max(made, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splits", nargs="*", default=["train", "test-(95,100)"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--draws", type=int, default=50, help="networkx graphs per type and size")
    ap.add_argument("--no-networkx", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from kp_gnn_amd import _lib, graph_property as GP, ops
    dev = torch.device("cuda:0")
    splits = GP.reference_splits(extrapolation=True)
    result = {"device": torch.cuda.get_device_name(0), "seed": args.seed, "reps": args.reps, "splits": {}}
    for name in args.splits:
        nodes = splits[name]
        call = lambda route: ops.property_graphs(nodes, args.seed, dev, route=route)  # noqa: E731
        d = call("device")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = call("host")
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
        same = (np.array_equal(d.edge_ptr, h.edge_ptr) and torch.equal(d.edge_index, h.edge_index) and torch.equal(d.features, h.features)
                and all(np.array_equal(getattr(d, k), getattr(h, k)) for k in ("source", "types", "attempts", "exhausted")))
        if not same:
            raise SystemExit(f"{name}: the device route and the host route differ, no time is reported")
        ms, gen = [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call("device")
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        # the generate launches alone: the call again with events around every launch of that entry
        launch = _lib.launch
        spans = []

        def timed(entry, device, *a, **k):
            if entry != "kpgnn_property_graphs_generate":
                return launch(entry, device, *a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = launch(entry, device, *a, **k)
            e1.record()
            spans.append((e0, e1))
            return rc

        for _ in range(args.reps):
            spans.clear()
            _lib.launch = timed
            try:
                call("device")
            finally:
                _lib.launch = launch
            torch.cuda.synchronize()
            gen.append(sum(e0.elapsed_time(e1) for e0, e1 in spans))
        row = {"graphs": int(nodes.size), "nodes": [int(nodes.min()), int(nodes.max())], "edges": int(d.edge_ptr[-1]),
               "device_ms": {"median": statistics.median(ms), "min": min(ms), "max": max(ms)},
               "generate_ms": {"median": statistics.median(gen), "min": min(gen), "max": max(gen)},
               "host_ms": host_ms, "mean_attempts": float(d.attempts.mean()), "max_attempts": int(d.attempts.max()),
               "exhausted": int(d.exhausted.size), "types": {str(t): int(c) for t, c in zip(*np.unique(d.types, return_counts=True))}}
        if not args.no_networkx:
            row["networkx_ms_per_graph"] = {str(n): networkx_ms(n, args.draws) for n in (int(nodes.min()), int(nodes.max()))}
        result["splits"][name] = row
        print(f"{name}: device {row['device_ms']['median']:.3f} ms (generate {row['generate_ms']['median']:.3f} ms), host {host_ms:.1f} ms, "
              f"{row['mean_attempts']:.2f} attempts a graph", file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
