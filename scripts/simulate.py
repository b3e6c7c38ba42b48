"""The regular-graph simulation (the reference's run_simulation.py) on the device: collision rates and stage timings.

    python scripts/simulate.py --n 20 40 80 160 320 640 1280 --R 3 --N 100 --K 6
    python scripts/simulate.py --n 1280 --K 8 --out profiles/collisions/simulate_n1280.json
    python scripts/simulate.py --n 20 --N 50 --graph            # whole-graph collision rate

Flags are the reference's (--n, --R, --N, --K, --graph) plus --seed and --generator (networkx | device).  Prints ONE JSON
object: "rates" {"n,k": collision rate} and "seconds" {"n": {stage: seconds}} (generate: networkx on the host, or
ops.random_regular_graphs with --generator device; pre_transform: ops.khop_transform; forward: KGINConv;
count: ops.collision_count and its read-back), each stage fenced by device synchronises and summed over k = 1 .. K.  The first n
of a run also pays for loading the code objects: put a small n in front of the one to be timed.  No plotting."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description="Node configuration simulation experiment")
    ap.add_argument("--R", type=int, default=3, help="node degree (r) of the synthetic r-regular graphs")
    ap.add_argument("--n", nargs="*", type=int, default=[20], help="numbers of nodes of the regular graphs")
    ap.add_argument("--N", type=int, default=100, help="number of graphs in the simulation")
    ap.add_argument("--K", type=int, default=6, help="largest number of hops to consider")
    ap.add_argument("--graph", action="store_true", default=False, help="whole-graph collision rate; otherwise node")
    ap.add_argument("--seed", type=int, default=0, help="seed of the first graph and of the layer's parameters")
    ap.add_argument("--generator", choices=("networkx", "device"), default="networkx",
                    help="who draws the graphs: networkx on the host, or the pairing-model kernel on the device (another draw)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    from kp_gnn_amd import ops, simulation
    dev = torch.device("cuda:0")
    rates, seconds = {}, {}
    for n in args.n:                                     # one call per n, so that the stage times are per n as well
        seconds[str(n)] = {}
        rates.update(simulation.simulate([n], R=args.R, N=args.N, K=args.K, graph=args.graph, seed=args.seed, device=dev,
                                         timings=seconds[str(n)], generator=args.generator))
    result = {"device": torch.cuda.get_device_name(0), "R": args.R, "N": args.N, "K": args.K, "graph": args.graph, "seed": args.seed,
              "generator": args.generator,
              "native_collisions": ops.native_collisions(),
              "rates": {f"{n},{k}": r for (n, k), r in rates.items()}, "seconds": seconds}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
