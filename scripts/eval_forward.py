"""Evaluation-mode forward (model.eval() under torch.no_grad(): the reference's val() / test() loops) of bench.py's default
body - KP-GIN+, K = L = 8, h = 104 - at B = 2048 and B = 64 graphs, timed eagerly and as one captured hipGraph:

    python scripts/eval_forward.py [--iters 200] [--warmup 10] [--no-profile]

Prints ONE JSON line.  Times are device events around `iters` back-to-back forwards that end in a synchronise; the kernel list
next to them comes from a run of its own (a fresh child process under `rocprofv3 --kernel-trace --stats`, eager launches), so
tracing never touches a timed window.  The workload and model builders are bench.py's, by import.  The BatchNorms get seeded
running statistics (the values do not change the time, only make the forward a realistic one)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

BATCHES = (2048, 64)


def setup(batch, device):
    wl = bench.WORKLOADS["zinc"]
    args = argparse.Namespace(workload="zinc", model=wl["model"], K=wl["K"], layers=wl["layers"], hidden=wl["hidden"],
                              batch=batch, kernel=wl["kernel"], loss=wl["loss"], combine="geometric")
    model = bench.build_model(args, device).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                C = m.num_features
                m.running_mean.copy_(0.5 * torch.randn(C, generator=g))
                m.running_var.copy_(0.5 + 1.5 * torch.rand(C, generator=g))
                m.weight.copy_(0.5 + torch.rand(C, generator=g))
                m.bias.copy_(0.2 * torch.randn(C, generator=g))
    b = bench.make_batch(args, 0, max(1, min(16, bench.usable_cpus()))).to(device)
    b.build_csr()
    return model, b


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(batch, device, iters, warmup):
    model, b = setup(batch, device)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                score = model(b)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        eager = [timed(lambda: model(b), iters) for _ in range(3)]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = model(b)
        graph.replay()
        torch.cuda.synchronize()
        replay = [timed(graph.replay, iters) for _ in range(3)]
        same = bool(torch.equal(captured, score))
    return {"graphs": batch, "nodes": int(b.num_nodes), "eager_ms": round(min(eager), 4), "graph_ms": round(min(replay), 4),
            "eager_ms_runs": [round(t, 4) for t in eager], "graph_ms_runs": [round(t, 4) for t in replay],
            "graph_equals_eager": same, "score_absmax": float(score.abs().max())}


def worker(batch, device, forwards):
    """The profiled child: `forwards` eager forwards, nothing else."""
    model, b = setup(batch, device)
    with torch.no_grad():
        for _ in range(forwards):
            model(b)
    torch.cuda.synchronize()


def kernel_list(batch, forwards):
    """Kernels of the eager eval forward from a rocprofv3 run of its own: [{name, calls_per_forward, avg_us, us_per_forward}],
    by time.  The first forward's one-time work (index packing, CSR) is in the totals, spread over `forwards`."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--worker", str(batch), "--forwards", str(forwards)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=280)
        if r.returncode != 0:
            raise SystemExit("the profiled run failed:\n" + r.stdout[-2000:])
        f = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not f:
            raise SystemExit("rocprofv3 left no kernel_stats.csv:\n" + r.stdout[-2000:])
        rows = list(csv.DictReader(open(max(f, key=os.path.getmtime))))
    out = []
    for r in rows:
        calls, total = int(r["Calls"]), int(r["TotalDurationNs"])
        out.append({"name": r["Name"][:160], "calls_per_forward": round(calls / forwards, 2), "avg_us": round(total / calls / 1e3, 2),
                    "us_per_forward": round(total / forwards / 1e3, 2)})
    out.sort(key=lambda k: -k["us_per_forward"])
    return out


def verdict(kernels):
    blas = [k["name"] for k in kernels if "Cijk_" in k["name"]]
    native = [k["name"] for k in kernels if "at::native" in k["name"] and k["avg_us"] >= 10.0]
    return {"cijk_kernels": blas, "at_native_10us_or_more": native,
            "kernel_us_per_forward": round(sum(k["us_per_forward"] for k in kernels), 1),
            "launches_per_forward": round(sum(k["calls_per_forward"] for k in kernels), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child runs (times only)")
    ap.add_argument("--worker", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--forwards", type=int, default=12, help="forwards of a profiled child run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_forward.py needs an MI355X (no CPU fallback for the product path)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    if args.worker is not None:
        worker(args.worker, device, args.forwards)
        return
    doc = {"metric": "ms per eval/no-grad forward, KP-GIN+ K=8 L=8 h=104 (bench.py's default body)", "iters": args.iters,
           "device": torch.cuda.get_device_name(device), "csrc_digest": bench.csrc_digest()}
    for batch in BATCHES:
        doc[f"b{batch}"] = measure(batch, device, args.iters, args.warmup)
    if not args.no_profile:
        for batch in BATCHES:
            ks = kernel_list(batch, args.forwards)
            doc[f"b{batch}"]["verdict"] = verdict(ks)
            doc[f"b{batch}"]["kernels"] = ks
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
