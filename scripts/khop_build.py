"""Building a resident dataset from raw graphs, measured on both routes.

    python scripts/khop_build.py --out profiles/khop/khop_build.json
    python scripts/khop_build.py --graphs 2000 --rounds 2

For `--graphs` (10,000) synthetic molecules per workload - ZINC-shaped with the ZINC arguments (8, 50, 6, 3, 50, 50, "spd"), the
same molecules with (16, 50, 6, 3, 50, 50, "gd"), QM9-shaped with (6, 50, 5, 4, 20, 15, "spd") - ONE process times, alternating
per round after one warm-up of each:
    host route    khop_transform.khop_batch on `--threads` threads (default: the CPUs this process may use), then
                  KHopDataset.from_collated on its host tensors (chunked upload, CSR build, dictionary);
    device route  KHopDataset.from_graphs(route="device"): ops.khop_transform per chunk (kpgnn_khop_dev_count, a scan,
                  kpgnn_khop_dev_fill), the CSR build on the tensors where they lie, the dictionary.
Every figure is a host clock around work that ends in a device synchronise; the device route's launches are also bracketed by
HIP events (_lib.LaunchTimer) and their sum is reported as `device_launches_s`.  A round's datasets are compared tensor for
tensor once.  Reported: the median over the rounds and the spread (min .. max) of khop_batch, from_collated, their sum and
from_graphs, and `auto` - "device" when from_graphs' median is below the host route's sum, "host" otherwise.

Two more workloads (`--workloads regular1280,tu_mixed`; `--graphs` does not apply) measure who should serve graphs above 64
nodes INSIDE the device route - from_graphs(route="device", large="host"), where ops.khop_transform hands them to khop_batch
and copies the slices in, against large="device", the kernels of csrc/khop_large.hip:
    regular1280   100 random 3-regular graphs of 1280 nodes with run_simulation.py's arguments (8, 10, 1, 1, 1, 1, "spd"), no
                  edge types;
    tu_mixed      2,000 seeded random graphs of 20 .. 620 nodes, mean degree 4, (3, 50, 3, 1, 50, 50, "gd").
Same process, same alternation, same comparison; `device_wins` is true when the device leg's median is below the host leg's by
more than the host leg's spread between rounds (max - min)."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKLOADS = {"zinc": ("zinc", (8, 50, 6, 3, 50, 50, "spd")), "zinc_gd16": ("zinc", (16, 50, 6, 3, 50, 50, "gd")),
             "qm9": ("qm9", (6, 50, 5, 4, 20, 15, "spd"))}


LARGE_WORKLOADS = {"regular1280": (8, 10, 1, 1, 1, 1, "spd"), "tu_mixed": (3, 50, 3, 1, 50, 50, "gd")}


def large_graphs(name):
    """(node_ptr, edge_ptr, edge_index [2,E] local ids) of a LARGE_WORKLOADS entry; every edge in both directions, no types."""
    import networkx as nx
    import numpy as np
    if name == "regular1280":
        graphs = [nx.random_regular_graph(3, 1280, seed=s) for s in range(100)]
    else:
        sizes = np.random.default_rng(1).integers(20, 621, size=2000)
        graphs = [nx.gnm_random_graph(int(n), 2 * int(n), seed=s) for s, n in enumerate(sizes)]
    eis = [np.array(sorted(g.to_directed().edges), dtype=np.int64).reshape(-1, 2).T for g in graphs]
    node_ptr = np.cumsum([0] + [g.number_of_nodes() for g in graphs]).astype(np.int64)
    edge_ptr = np.cumsum([0] + [e.shape[1] for e in eis]).astype(np.int64)
    return node_ptr, edge_ptr, np.ascontiguousarray(np.concatenate(eis, axis=1))


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)


def same(a, b):
    import torch
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a, b))
    return a == b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    from kp_gnn_amd import _lib
    from kp_gnn_amd import khop_transform as KT
    from kp_gnn_amd._env import usable_cpus
    from kp_gnn_amd.batch import KHopBatch
    from kp_gnn_amd.dataset import KHopDataset
    if not torch.cuda.is_available():
        raise SystemExit("khop_build.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    threads = args.threads or usable_cpus()
    res = dict(graphs=args.graphs, threads=threads, device=torch.cuda.get_device_name(0), workloads={})
    for name in args.workloads.split(","):
        if name in LARGE_WORKLOADS:
            kargs = LARGE_WORKLOADS[name]
            node_ptr, edge_ptr, ei = large_graphs(name)
            xt = torch.ones(int(node_ptr[-1]), 1)

            def leg(large):
                timer = _lib.LaunchTimer()
                _lib.set_launch_timer(timer)
                try:
                    t0 = time.perf_counter()
                    ds = KHopDataset.from_graphs(node_ptr, edge_ptr, ei, None, dev, kargs, x=xt, route="device", large=large)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                finally:
                    _lib.set_launch_timer(None)
                return ds, dt, sum(a.elapsed_time(b) for kind, _, a, b in timer.records if kind == "khop_dev") * 1e-3

            torch.set_num_threads(threads)
            a, b = leg("host")[0], leg("device")[0]                     # warm-up of each leg and the one comparison
            identical = all(same(u, v) for u, v in zip(a.state(), b.state()))
            khop_edges = int(a.h_edges.sum())
            del a, b
            t_host, t_dev, t_launch = [], [], []
            for _ in range(args.rounds):
                t_host.append(leg("host")[1])
                _, td, tl = leg("device")
                t_dev.append(td), t_launch.append(tl)
            n = node_ptr[1:] - node_ptr[:-1]
            entry = dict(args=list(kargs), graphs=int(n.size), nodes=int(node_ptr[-1]), input_edges=int(edge_ptr[-1]),
                         khop_edges=khop_edges, min_nodes=int(n.min()), max_nodes=int(n.max()), graphs_above_64=int((n > 64).sum()),
                         large_host_s=spread(t_host), large_device_s=spread(t_dev), device_launches_s=spread(t_launch),
                         identical=identical)
            h, d = entry["large_host_s"], entry["large_device_s"]
            entry["device_wins"] = bool(h["median"] - d["median"] > h["max"] - h["min"])
            res["workloads"][name] = entry
            print(f"[khop_build] {name}: large=host {h['median']:.3f} s ({h['min']:.3f} .. {h['max']:.3f}), large=device "
                  f"{d['median']:.3f} s ({d['min']:.3f} .. {d['max']:.3f}; launches {entry['device_launches_s']['median']:.4f}), "
                  f"identical={identical}, device_wins={entry['device_wins']}", file=sys.stderr, flush=True)
            continue
        shape, kargs = WORKLOADS[name]
        node_ptr, edge_ptr, ei, ea, x = KT.synth_molecules(args.graphs, 1, shape=KT.qm9_shape() if shape == "qm9" else None)
        xt = torch.from_numpy(x).view(-1, 1)

        def host_route():
            t0 = time.perf_counter()
            out = KT.khop_batch(node_ptr, edge_ptr, ei, ea, *kargs, num_threads=threads)
            t1 = time.perf_counter()
            hb = KHopBatch(x=xt, edge_index=out["edge_index"], edge_attr=out["edge_attr"], pe_attr=out["pe_attr"],
                           peripheral_edge_attr=out["peripheral_edge_attr"],
                           peripheral_configuration_attr=out["peripheral_configuration_attr"], batch=out["batch"],
                           num_graphs=args.graphs)
            hb.edge_ptr = out["edge_ptr"].numpy()
            ds = KHopDataset.from_collated(hb, node_ptr, dev)
            torch.cuda.synchronize()
            return ds, t1 - t0, time.perf_counter() - t1, int(out["edge_index"].shape[1]), sum(
                v.numel() * 8 for v in out.values() if v is not None)

        def device_route():
            timer = _lib.LaunchTimer()
            _lib.set_launch_timer(timer)
            try:
                t0 = time.perf_counter()
                ds = KHopDataset.from_graphs(node_ptr, edge_ptr, ei, ea, dev, kargs, x=xt, route="device")
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            finally:
                _lib.set_launch_timer(None)
            launches = sum(a.elapsed_time(b) for kind, _, a, b in timer.records if kind == "khop_dev") * 1e-3
            return ds, dt, launches

        a, _, _, khop_edges, host_bytes = host_route()              # warm-up of each route (library load, LDS attributes,
        b, _, _ = device_route()                                    # allocator) and the one comparison
        identical = all(same(u, v) for u, v in zip(a.state(), b.state()))
        del a, b
        t_khop, t_coll, t_host, t_dev, t_launch = [], [], [], [], []
        for _ in range(args.rounds):
            ds, tk, tc, _, _ = host_route()
            del ds
            t_khop.append(tk), t_coll.append(tc), t_host.append(tk + tc)
            ds, td, tl = device_route()
            del ds
            t_dev.append(td), t_launch.append(tl)
        entry = dict(args=list(kargs), nodes=int(node_ptr[-1]), input_edges=int(edge_ptr[-1]), khop_edges=khop_edges,
                     host_khop_tensor_bytes=host_bytes, max_nodes=int((node_ptr[1:] - node_ptr[:-1]).max()),
                     khop_batch_s=spread(t_khop), from_collated_s=spread(t_coll), host_route_s=spread(t_host),
                     from_graphs_device_s=spread(t_dev), device_launches_s=spread(t_launch), identical=identical)
        entry["auto"] = "device" if entry["from_graphs_device_s"]["median"] < entry["host_route_s"]["median"] else "host"
        res["workloads"][name] = entry
        print(f"[khop_build] {name}: host {entry['host_route_s']['median']:.3f} s (khop_batch {entry['khop_batch_s']['median']:.3f}"
              f" + from_collated {entry['from_collated_s']['median']:.3f}), device {entry['from_graphs_device_s']['median']:.3f} s"
              f" (launches {entry['device_launches_s']['median']:.4f}), identical={identical}, auto={entry['auto']}",
              file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
