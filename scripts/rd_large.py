"""The resistance-distance column of graphs above 128 nodes: ops.resistance_distance(large="device") - the kernel of
csrc/resistance_large.hip - against large="host", the float64 numpy.linalg.pinv per graph that is the default.

    python scripts/rd_large.py --out profiles/rd_large/rd_large.json
    python scripts/rd_large.py --shapes tu_mixed_hop1 --rounds 1

Every figure is the wall time of a whole ops.resistance_distance call with the edge list already on the device, ended by a
device synchronise: launches, the status read-back and every host fill included.  ONE process, the two settings ALTERNATING
per round, `--rounds` (3) rounds after one warm-up call of each.  Shapes:
    regular1280_hop1    100 random 3-regular graphs of 1280 nodes (batch.regular_graphs), their 1-hop lists;
    regular1280_k3spd   the same graphs, their K = 3 spd lists made by the device pre-transform
                        (ops.khop_transform(large="device"), arguments (3, 10, 1, 1, 1, 1, "spd"));
    tu_mixed_hop1       scripts/khop_build.py's tu_mixed: 2,000 seeded random graphs of 20 .. 620 nodes, mean degree 4;
    single2048          ONE random 3-regular graph of 2048 nodes, alone in its call: what the largest graph costs when nothing
                        runs beside it (one workgroup, one compute unit).
The device setting is timed on the FULL call.  A host round of the full call takes minutes (0.6 s per 1280-node graph), so the
host setting is timed on a SAMPLE: the call that holds every `--every`-th (tenth) graph above 128 nodes of the shape and
nothing else, reported as seconds per graph and scaled to the shape's count of such graphs (`host_full_estimate_s`; graphs of
up to 128 nodes take the same launches under either setting and are left out of it).  The device setting is also timed on that
same sample call, so `sample_ratio_host_over_device` compares like with like.  `max_abs_device_minus_host` is taken over the
sampled graphs, float32 rows against float32 rows; `status_device` counts the kernel's status codes over the full call."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ("regular1280_hop1", "regular1280_k3spd", "tu_mixed_hop1", "single2048")
K3_SPD = (3, 10, 1, 1, 1, 1, "spd")


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)


def raw_graphs(name):
    """(node_ptr, edge_ptr, edge_index [2,E] LOCAL ids) of a shape's raw graphs."""
    from kp_gnn_amd.batch import regular_graphs
    if name.startswith("regular1280"):
        return regular_graphs(100, 0, n=1280, degree=3)
    if name == "single2048":
        return regular_graphs(1, 7, n=2048, degree=3)
    sys.path.insert(0, os.path.join(HERE, "scripts"))
    from khop_build import large_graphs
    return large_graphs("tu_mixed")


def edge_lists(name, dev):
    """(node_ptr, edge_ptr, edge_index with GLOBAL ids on the device) the feature is computed from."""
    import numpy as np
    import torch
    from kp_gnn_amd import ops
    node_ptr, edge_ptr, ei = raw_graphs(name)
    if name.endswith("k3spd"):
        out, status = ops.khop_transform(node_ptr, edge_ptr, torch.from_numpy(ei), None, *K3_SPD, dev, large="device")
        assert not bool(status.any())
        return node_ptr, out["edge_ptr"].cpu().numpy(), out["edge_index"].contiguous()
    glob = ei + np.repeat(node_ptr[:-1], np.diff(edge_ptr))[None, :]
    return node_ptr, edge_ptr, torch.from_numpy(glob).to(dev)


def sub_call(node_ptr, edge_ptr, ei_d, ids):
    """The call that holds the graphs `ids` alone."""
    import numpy as np
    import torch
    n, e = np.diff(node_ptr)[ids], np.diff(edge_ptr)[ids]
    nptr, eptr = np.concatenate([[0], np.cumsum(n)]), np.concatenate([[0], np.cumsum(e)])
    parts = [ei_d[:, int(edge_ptr[g]):int(edge_ptr[g + 1])] - int(node_ptr[g]) + int(nptr[i]) for i, g in enumerate(ids)]
    return nptr.astype(np.int64), eptr.astype(np.int64), torch.cat(parts, dim=1).contiguous()


def measure(name, args, dev):
    import numpy as np
    import torch
    from kp_gnn_amd import ops

    def call(batch, large):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rd, status = ops.resistance_distance(*batch, dev, large=large, workspace_bytes=args.workspace_bytes)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, rd, status

    full = edge_lists(name, dev)
    nodes = np.diff(full[0])
    big = np.flatnonzero(nodes > 128)
    ids = big[::args.every] if big.size > args.every else big
    sample = sub_call(*full, ids)
    legs = (("device_full", full, "device"), ("device_sample", sample, "device"), ("host_sample", sample, "host"))
    times, last = {k: [] for k, _, _ in legs}, {}
    for k, batch, large in legs:                     # warm-up of each
        call(batch, large)
    for _ in range(args.rounds):
        for k, batch, large in legs:                 # alternating: a drift of the machine reaches every setting alike
            t, rd, status = call(batch, large)
            times[k].append(t)
            last[k] = (rd, status)
        print(f"[rd_large] {name}: round done", file=sys.stderr, flush=True)
    a, b = last["device_sample"][0].cpu().reshape(-1).double(), last["host_sample"][0].cpu().reshape(-1).double()
    full_rows = last["device_full"][0].cpu().reshape(-1)
    rows = torch.cat([full_rows[int(full[0][g]):int(full[0][g + 1])] for g in ids])
    st = last["device_full"][1]
    host_per_graph = [t / ids.size for t in times["host_sample"]]
    entry = dict(graphs=int(nodes.size), nodes=int(full[0][-1]), edges=int(full[1][-1]), max_nodes=int(nodes.max()),
                 graphs_above_128=int(big.size), sampled_graphs=int(ids.size), sampled_nodes=int(sample[0][-1]),
                 device_full_s=spread(times["device_full"]), device_sample_s=spread(times["device_sample"]),
                 host_sample_s=spread(times["host_sample"]), host_s_per_graph=spread(host_per_graph),
                 host_full_estimate_s=statistics.median(host_per_graph) * int(big.size),
                 sample_ratio_host_over_device=statistics.median(times["host_sample"]) / statistics.median(times["device_sample"]),
                 status_device={str(s): int((st == s).sum()) for s in range(5)},
                 status_host_sample={str(s): int((last["host_sample"][1] == s).sum()) for s in range(5)},
                 max_abs_device_minus_host=float((a - b).abs().max()),
                 sample_rows_equal_full_rows=bool(torch.equal(rows.view(torch.int32), last["device_sample"][0].cpu().reshape(-1).view(torch.int32))))
    d, h = entry["device_full_s"], entry["host_s_per_graph"]
    print(f"[rd_large] {name}: device, full call {d['median']:.4f} s ({d['min']:.4f} .. {d['max']:.4f}); host {h['median']:.4f} s per "
          f"graph on {ids.size} sampled graphs, {entry['host_full_estimate_s']:.1f} s for all {big.size}; sample: host / device "
          f"{entry['sample_ratio_host_over_device']:.1f}; max |device - host| {entry['max_abs_device_minus_host']:.3e}",
          file=sys.stderr, flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--every", type=int, default=10, help="the host setting is timed on every N-th graph above 128 nodes")
    ap.add_argument("--workspace-bytes", type=int, default=1 << 30)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "every": args.every,
              "workspace_bytes": args.workspace_bytes, "host_threads": torch.get_num_threads(), "shapes": {}}
    for name in args.shapes.split(","):
        result["shapes"][name] = measure(name, args, dev)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
