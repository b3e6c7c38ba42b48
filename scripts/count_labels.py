"""ops.count_labels on three workloads, device route against host route, and the reference's own process() as context.

    python scripts/count_labels.py --out profiles/count_labels/count_labels.json
    python scripts/count_labels.py --scale 0.1 --rounds 2                        # a smaller look
    python scripts/count_labels.py --reference /path/to/reference --out ...      # CPU only: times the reference on workload (a)

  (a) 5,000 graphs of 10 to 30 nodes: half G(n, p), half random 3- or 4-regular (networkx.random_regular_graph, fixed seeds) -
      the two families of the reference's randomgraph.mat, which is not shipped with it
  (b) 2,000 G(n, p) graphs of 20 to 620 nodes, expected degree 8
  (c) 100 random 3-regular graphs of 1,280 nodes
ONE process, per workload:
  device   ops.count_labels(route="device") from host arrays to labels on the device, its one status read-back included, wall
           clock around a device synchronize; the median of `--reps` calls per round, after a warm-up call at the timed shape
  kernels  each size class's kpgnn_count_labels launch alone on resident tensors, between two stream events; median of `--reps`
  host     graph_count.count_labels_host (float64 numpy, one thread of control; numpy's BLAS threads as the environment sets
           them), moved to the device; one call per round
The four integer columns of the two routes must be equal and cus within its bound before any time is reported.  With
--reference (no GPU needed) the reference's GraphCountDataset.process is timed on workload (a) through the stand-ins of
tests/golden/make_graph_count_golden.py and its rows are compared with the host route's."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pack(graphs):
    import numpy as np
    nptr = np.concatenate([[0], np.cumsum([n for n, _ in graphs])]).astype(np.int64)
    eptr = np.concatenate([[0], np.cumsum([ei.shape[1] for _, ei in graphs])]).astype(np.int64)
    return nptr, eptr, np.concatenate([ei for _, ei in graphs], axis=1)


def _gnp(n, p, rng):
    import numpy as np
    upper = np.triu(rng.random((n, n)) < p, 1)
    u, v = np.nonzero(upper | upper.T)
    return n, np.stack([u, v]).astype(np.int64)


def _regular(n, d, seed):
    import networkx as nx
    import numpy as np
    e = np.asarray(list(nx.random_regular_graph(d, n, seed=seed).edges()), dtype=np.int64).reshape(-1, 2).T
    return n, np.concatenate([e, e[::-1]], axis=1)


def workload(name, scale):
    import numpy as np
    rng = np.random.default_rng({"a": 101, "b": 202, "c": 303}[name])
    graphs = []
    if name == "a":
        G = max(2, int(5000 * scale))
        for i in range(G):
            n = int(rng.integers(10, 31))
            if i % 2 == 0:
                graphs.append(_gnp(n, rng.uniform(0.1, 0.5), rng))
            else:
                d = 4 if n % 2 else 3 + int(rng.integers(0, 2))                 # (n d must be even)
                graphs.append(_regular(n, d, seed=1000 + i))
    elif name == "b":
        for _ in range(max(2, int(2000 * scale))):
            n = int(rng.integers(20, 621))
            graphs.append(_gnp(n, min(0.5, 8.0 / n), rng))
    else:
        graphs = [_regular(1280, 3, seed=5000 + i) for i in range(max(2, int(100 * scale)))]
    return graphs


def wall_ms(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return (time.perf_counter() - t0) * 1e3, out


def summary(vals):
    return dict(median=statistics.median(vals), min=min(vals), max=max(vals), rounds=vals)


def check_equal(a, b, nodes, what):
    """a, b [G,5] float64 numpy: integer columns equal, cus within (n + 8) 2^-52 |b| + n 2^-1022."""
    import numpy as np
    if not np.array_equal(a[:, :4], b[:, :4]):
        raise SystemExit(f"{what}: the integer columns differ, no time is reported")
    bound = (nodes + 8) * 2.0 ** -52 * np.abs(b[:, 4]) + nodes * 2.0 ** -1022
    if not (np.abs(a[:, 4] - b[:, 4]) <= bound).all():
        raise SystemExit(f"{what}: cus beyond its bound, no time is reported")
    return float((np.abs(a[:, 4] - b[:, 4]) / np.maximum(bound, 1e-300)).max())


def kernel_ms(nptr, eptr, ei, dev, reps, workspace_bytes):
    """class name -> median milliseconds of its launch(es) alone, on resident tensors."""
    import numpy as np
    import torch
    from kp_gnn_amd import _lib, ops, ops_dataset
    G, E = nptr.shape[0] - 1, int(eptr[-1])
    nodes = np.diff(nptr)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)  # noqa: E731
    nptr_d, eptr_d, ei_d = t(nptr, torch.int64), t(eptr, torch.int64), t(ei, torch.int64)
    out = torch.zeros((G, 5), dtype=torch.float64, device=dev)
    st = torch.zeros(G, dtype=torch.int32, device=dev)
    slab = lambda cap: int(_lib.load().kpgnn_count_labels_workspace_bytes(cap))  # noqa: E731
    res = {}
    for cls, sel in (("wave", nodes <= 32), ("word", (nodes > 32) & (nodes <= 64)), ("large", (nodes > 64) & (nodes <= 2048))):
        ids = np.flatnonzero(sel)
        if ids.size == 0:
            continue
        runs = [(ids, 32 if cls == "wave" else 64, 0)] if cls != "large" else ops_dataset.workspace_runs(ids, nodes, slab, workspace_bytes)
        ws = torch.empty(max(8, max(r[2] for r in runs)), dtype=torch.uint8, device=dev)
        jobs = [(t(r[0], torch.int32), r[1], r[2]) for r in runs]
        go = lambda: [ops.count_labels_launch(G, nptr_d, eptr_d, ei_d, E, i, cap, out, st, ws, nb) for i, cap, nb in jobs]  # noqa: E731
        go()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            go()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        res[cls] = dict(graphs=int(ids.size), launches=len(jobs), median_ms=statistics.median(ms), min_ms=min(ms))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="a,b,c")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each workload's graph count")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="device-route calls per round")
    ap.add_argument("--workspace-bytes", type=int, default=1 << 28)
    ap.add_argument("--reference", default=None, help="a reference checkout: time its process() on workload (a) and stop")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from kp_gnn_amd import graph_count as GCN, ops
    result = {"host_threads": os.environ.get("OMP_NUM_THREADS"), "scale": args.scale}
    if args.reference:
        sys.path.insert(0, os.path.join(HERE, "tests"))
        sys.path.insert(0, os.path.join(HERE, "tests", "golden"))
        sys.dont_write_bytecode = True                 # (no cache next to the fixtures)
        from make_graph_count_golden import reference_rows
        graphs = workload("a", args.scale)
        nptr, eptr, ei = _pack(graphs)
        y_ref, seconds = reference_rows(args.reference, graphs)
        t0 = time.perf_counter()
        y_host = GCN.count_labels_host_f64(nptr, eptr, ei)
        host_s = time.perf_counter() - t0
        worst = check_equal(y_host, y_ref, np.diff(nptr), "host route against the reference")
        result["a"] = {"graphs": len(graphs), "nodes": int(nptr[-1]), "edges": int(eptr[-1]), "reference_process_ms": seconds * 1e3,
                       "host_route_ms_same_machine": host_s * 1e3, "integer_columns_equal": True, "cus_worst_fraction_of_bound": worst}
    else:
        dev = torch.device("cuda:0")
        sync = torch.cuda.synchronize
        result["device"] = torch.cuda.get_device_name(0)
        for name in args.workloads.split(","):
            graphs = workload(name, args.scale)
            nptr, eptr, ei = _pack(graphs)
            nodes = np.diff(nptr)
            device = lambda: ops.count_labels(nptr, eptr, ei, dev, route="device", workspace_bytes=args.workspace_bytes)  # noqa: E731
            host = lambda: GCN.count_labels_host(nptr, eptr, ei, dev)  # noqa: E731
            y_d = device()                                                   # warm-up at the timed shape: code objects, allocator
            device()
            t_dev, t_host = [], []
            for _ in range(args.rounds):                                     # alternating: a drift of the machine reaches both alike
                t_dev.append(statistics.median(wall_ms(device, sync)[0] for _ in range(args.reps)))
                ms, y_h = wall_ms(host, sync)
                t_host.append(ms)
            worst = check_equal(y_d.cpu().numpy(), y_h.cpu().numpy(), nodes, f"workload {name}")
            result[name] = {"graphs": len(graphs), "nodes": int(nptr[-1]), "edges": int(eptr[-1]), "max_nodes": int(nodes.max()),
                            "integer_columns_equal": True, "cus_worst_fraction_of_bound": worst,
                            "device_route_ms": summary(t_dev), "host_route_ms": summary(t_host),
                            "host_over_device": statistics.median(t_host) / statistics.median(t_dev),
                            "kernels": kernel_ms(nptr, eptr, ei, dev, args.reps * args.rounds, args.workspace_bytes)}
            print(f"workload {name}: device {statistics.median(t_dev):.3f} ms, host {statistics.median(t_host):.3f} ms", file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
