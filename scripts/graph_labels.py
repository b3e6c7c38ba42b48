"""ops.graph_property_labels at the shape of the reference's default graph-property dataset: 7,680 graphs of 15 to 24 nodes
(GraphPropertyDataset.py: 5,120 training, 1,280 validation and 1,280 test graphs), kernel route against host route, and the
resident dataset built with and without the node targets.

    python scripts/graph_labels.py --out profiles/graph_labels/graph_labels.json
    python scripts/graph_labels.py --graphs 512 --rounds 2                      # a smaller look

The graphs are G(n, p) draws without singleton nodes (the reference rejects those too), p uniform in [0.1, 0.5]; the reference's
own mix of generators needs networkx and is not reproduced here.  ONE process:
  kernel   ops.graph_property_labels(route="device") from host arrays to labels on the device, its one status read-back
           included, wall clock around a device synchronize; the median of `--reps` calls per round
  host     graph_property.graph_property_labels_host (float64 numpy, one thread of control; numpy's BLAS threads as the
           environment sets them), one call per round
  dataset  KHopDataset.from_graphs(...) without and with pos=labels, one call each per round
The two routes' labels are compared as the tests compare them: integer labels equal, spectral radius within one float32 ulp."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def draw(G, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    nptr, eptr, eis, src = [0], [0], [], []
    while len(src) < G:
        n = int(rng.integers(15, 25))
        upper = np.triu(rng.random((n, n)) < rng.uniform(0.1, 0.5), 1)
        A = upper | upper.T
        if not A.any(axis=0).all():
            continue
        u, v = np.nonzero(A)
        eis.append(np.stack([u, v]).astype(np.int64))
        nptr.append(nptr[-1] + n)
        eptr.append(eptr[-1] + u.size)
        src.append(int(rng.integers(0, n)))
    N = nptr[-1]
    return (np.asarray(nptr, dtype=np.int64), np.asarray(eptr, dtype=np.int64), np.concatenate(eis, axis=1), rng.random(N),
            np.asarray(src, dtype=np.int64))


def wall_ms(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return (time.perf_counter() - t0) * 1e3, out


def summary(vals):
    return dict(median=statistics.median(vals), min=min(vals), max=max(vals), rounds=vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=7680)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="kernel-route calls per round")
    ap.add_argument("--no-dataset", action="store_true", help="skip the KHopDataset builds")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    from kp_gnn_amd import graph_property as GP, ops
    from kp_gnn_amd.dataset import KHopDataset
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    nptr, eptr, ei, F, src = draw(args.graphs, 1234)
    khop_args = (3, 50, 6, 3, 50, 50, "spd")

    kernel = lambda: ops.graph_property_labels(nptr, eptr, ei, F, src, dev, route="device")  # noqa: E731
    host = lambda: GP.graph_property_labels_host(nptr, eptr, ei, F, src, dev)  # noqa: E731
    node_d, graph_d = kernel()                                       # warm-up at the timed shape: code objects, allocator
    kernel()
    x = GP.source_features(torch.from_numpy(F), src, nptr)
    build = lambda pos: KHopDataset.from_graphs(nptr, eptr, ei, None, dev, khop_args, x=x, y=graph_d, pos=pos)  # noqa: E731
    if not args.no_dataset:
        build(None)
    t_kernel, t_host, t_plain, t_pos = [], [], [], []
    for _ in range(args.rounds):                                     # alternating: a drift of the machine reaches all alike
        t_kernel.append(statistics.median(wall_ms(kernel, sync)[0] for _ in range(args.reps)))
        ms, (node_h, graph_h) = wall_ms(host, sync)
        t_host.append(ms)
        if not args.no_dataset:
            t_plain.append(wall_ms(lambda: build(None), sync)[0])
            t_pos.append(wall_ms(lambda: build(kernel()[0]), sync)[0])
    ints_equal = bool(torch.equal(node_d[:, :2], node_h[:, :2]) and torch.equal(graph_d[:, :2], graph_h[:, :2]))
    as_int = lambda t: t.cpu().contiguous().view(torch.int32).long()  # noqa: E731
    ulps = int((as_int(graph_d[:, 2]) - as_int(graph_h[:, 2])).abs().max())
    lap = float((node_d[:, 2].double() - node_h[:, 2].double()).abs().max())
    result = {"device": torch.cuda.get_device_name(0), "graphs": args.graphs, "nodes": int(nptr[-1]), "edges": int(eptr[-1]),
              "host_threads": os.environ.get("OMP_NUM_THREADS"), "connected_by_the_rule": int(graph_d[:, 0].sum()),
              "integer_labels_equal": ints_equal, "spectral_radius_max_f32_ulps": ulps, "laplacian_max_abs_diff": lap,
              "kernel_route_ms": summary(t_kernel), "host_route_ms": summary(t_host),
              "host_over_kernel": statistics.median(t_host) / statistics.median(t_kernel),
              "reference_recipe_s_per_64_graphs_of_24_nodes_on_another_cpu": 2.75}
    if t_plain:
        result["from_graphs_ms"] = summary(t_plain)
        result["from_graphs_with_pos_labels_ms"] = summary(t_pos)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
