"""kpgnn_random_regular_graphs alone, between two stream events, and the attempts it takes.

    python scripts/regular_graphs.py --out profiles/regular_graphs/kernel.json
    python scripts/regular_graphs.py --shapes 20,3 1280,3 --graphs 100 10000 --reps 7

Per (n, d) and graph count G: the launch on resident outputs (ops.random_regular_graphs' own launch, without its one read-back),
`--reps` times after a warm-up at the timed shape, each between two events on the stream: median, min and max in milliseconds.
The first `--check` graphs of every shape are compared with the host route bit for bit before a time is reported.  "attempts":
the mean number of pairings per graph over the largest G of each shape, whose reciprocal is the acceptance rate."""
import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["20,3", "1280,3", "20,4", "1280,4"], help="n,d pairs")
    ap.add_argument("--graphs", nargs="*", type=int, default=[100, 10000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check", type=int, default=8, help="graphs per shape compared with the host route")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from kp_gnn_amd import _lib, regular_graphs as RG
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "seed": args.seed, "reps": args.reps, "shapes": {}}
    for shape in args.shapes:
        n, d = (int(v) for v in shape.split(","))
        rows = {}
        for G in sorted(args.graphs):
            ei = torch.empty((2, G * n * d), dtype=torch.int64, device=dev)
            back = torch.empty((2, G), dtype=torch.int32, device=dev)
            desc = _lib.RrgDesc()
            desc.G, desc.n, desc.d, desc.max_attempts, desc.seed, desc.first_graph = G, n, d, 4096, args.seed, 0
            desc.edge_index, desc.attempts, desc.status = ei.data_ptr(), back[0].data_ptr(), back[1].data_ptr()
            go = lambda: _lib.launch("kpgnn_random_regular_graphs", dev, ctypes.byref(desc))  # noqa: E731
            go()
            torch.cuda.synchronize()
            c = min(G, args.check)
            want = RG.random_regular_graphs_host(c, n, d, args.seed)
            if not (np.array_equal(ei.view(2, G, n * d)[:, :c].cpu().numpy().reshape(2, -1), want[2])
                    and np.array_equal(back[0, :c].cpu().numpy(), want[3])):
                raise SystemExit(f"n={n} d={d} G={G}: the kernel and the host route differ, no time is reported")
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                go()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            attempts, status = back.cpu().numpy()
            rows[str(G)] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
                            "mean_attempts": float(attempts.mean()), "max_attempts": int(attempts.max()), "exhausted": int((status != 0).sum())}
            print(f"n={n} d={d} G={G}: {statistics.median(ms):.3f} ms, {attempts.mean():.2f} attempts a graph", file=sys.stderr, flush=True)
        result["shapes"][shape] = rows
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
