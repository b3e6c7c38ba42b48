"""ops.collision_count at the simulation's top size, kernel against the blocked framework expression.

    python scripts/collision_count.py --out profiles/collisions/count.json
    python scripts/collision_count.py --rows 20000 --rounds 3                 # a smaller look

The input is `--rows` (128,000 = 1280 nodes x 100 graphs) fp32 rows of `--cols` (16) columns drawn with replacement from a pool
of `--pool` (1,000) distinct random rows, so that collisions are common, as they are among the embeddings of a regular graph.
ONE process, both routes alternating per round after a warm-up of each at the timed shape:
  kernel     kpgnn_collision_count's two launches (workspace and result allocated inside, from the caching allocator),
             bracketed by two HIP events; `--reps` calls per round, the round's figure is their median
  framework  ops.collision_count_reference on the device (blocks of 2048 rows), one call per round between two events
Reported: the median over the rounds and their spread, pairs per second, the share of the fp32 vector peak at 3 flops per
(pair, column) - subtract, multiply, add - against 157.3 TFLOP/s, and the two counts of each route (they must agree)."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_FP32_VECTOR = 157.3e12


def event_ms(fn):
    import torch
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z), out


def summary(vals):
    return dict(median=statistics.median(vals), min=min(vals), max=max(vals), rounds=vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=128000)
    ap.add_argument("--cols", type=int, default=16)
    ap.add_argument("--pool", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="kernel calls per round")
    ap.add_argument("--no-framework", action="store_true", help="time the kernel only")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    from kp_gnn_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    pool = torch.randn(args.pool, args.cols, generator=g)
    pick = torch.randint(0, args.pool, (args.rows,), generator=g)
    o = pool[pick].to(dev)
    eps = 1e-10
    per_row = torch.bincount(pick, minlength=args.pool).double()
    expected = int((per_row * (per_row - 1) / 2).sum().item())      # pairs of copies of one pool row (pool rows are O(1) apart)

    def kernel():
        return ops._collision_count_launch(o, eps)

    def framework():
        return torch.stack(ops.collision_count_reference(o, eps))

    counts = {"kernel": kernel().tolist()}                           # warm-up at the timed shape: code objects, allocator
    kernel()
    if not args.no_framework:
        counts["framework"] = framework().tolist()
    torch.cuda.synchronize()
    t_kernel, t_frame = [], []
    for _ in range(args.rounds):                                     # alternating: a drift of the machine reaches both alike
        t_kernel.append(statistics.median(event_ms(kernel)[0] for _ in range(args.reps)))
        if not args.no_framework:
            t_frame.append(event_ms(framework)[0])
    pairs = args.rows * (args.rows - 1) // 2
    ms = statistics.median(t_kernel)
    result = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "cols": args.cols, "pool": args.pool, "eps": eps,
              "pairs": pairs, "expected_upper": expected, "counts_upper_diag": counts,
              "kernel_ms": summary(t_kernel), "kernel_pairs_per_s": pairs / (ms * 1e-3),
              "kernel_flops_per_pair_column": 3, "kernel_tflops": 3.0 * pairs * args.cols / (ms * 1e-3) / 1e12,
              "kernel_share_of_fp32_vector_peak": 3.0 * pairs * args.cols / (ms * 1e-3) / PEAK_FP32_VECTOR,
              "peak_fp32_vector_tflops": PEAK_FP32_VECTOR / 1e12}
    if t_frame:
        result["framework_ms"] = summary(t_frame)
        result["framework_over_kernel"] = statistics.median(t_frame) / ms
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
