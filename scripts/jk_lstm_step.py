"""Training-step time (forward + loss + backward, no optimiser) of KP-GIN+, K = 8, L = 8, h = 104, JK = attention on 2048
synthetic_zinc_batch molecules (scripts/jk_step.py's configuration) with the scoring LSTM on kpgnn_jk_lstm_fwd / _bwd and with
ops.set_native_jk_lstm(False) (nn.LSTM on the stacked states, the route before the native scorer):

    python scripts/jk_lstm_step.py                        # both variants, 3 alternating pairs of fresh processes
    python scripts/jk_lstm_step.py --variant native       # one run of one variant in this process (what the pairs start)
    python scripts/jk_lstm_step.py --variant native --no-graph --steps 10 --warmup 3      # e.g. under a kernel trace

Both variants are timed eagerly; the native one also as ONE captured hipGraph (the framework module is not captured: that is
the state of affairs this script records, not something it tries).  Per run: `--steps` steps after `--warmup`, each bracketed
by two HIP events, the run's figure the median step; torch.cuda.max_memory_allocated over the eager steps; the C-ABI launches
of one eager step; the bytes the scorer needs per direction, counted from the shapes.  Reported per variant: the median over
the runs and their spread (min .. max)."""
import argparse
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import jk_step as J      # noqa: E402  (the configuration, batch, model and timing loop are that script's)


def lstm_bytes(N, H, P, S):
    """Bytes the scorer has to move per direction, from the shapes (csrc/jk_lstm.hip).  fwd: the states once (4 N S H), the
    pre-activations written and read back and the activations written (3 x 4 N S 8P), the cell states (4 N S 2P), the score.
    bwd: activations and cell states read, dgin written and read twice (gx and the parameter gradients), h_prev written and
    read, the states read once and gx written once."""
    gin, cst, x, sc = 4 * N * S * 8 * P, 4 * N * S * 2 * P, 4 * N * S * H, 4 * N * S
    return dict(fwd=x + 3 * gin + cst + sc, bwd=gin + 2 * cst + sc + 3 * gin + 2 * cst + 2 * x)


def one_run(args):
    sys.path.insert(0, HERE)
    import torch
    from kp_gnn_amd import _lib, ops, ops_dense
    ops.set_native_jk_lstm(args.variant == "native")
    dev = torch.device("cuda:0")
    b = J.build_batch(dev)
    model = J.build_model("attention", dev)
    params = [p for p in model.parameters() if p.requires_grad]

    def step():
        score = model(b)
        loss, dscore = ops_dense.regression_loss_and_grad(score, b.y, "l1")
        with ops.deferred_reductions():
            grads = torch.autograd.grad(score, params, grad_outputs=dscore, allow_unused=True)
        return loss, grads

    w = J.CONFIG
    out = dict(device=torch.cuda.get_device_name(0), variant=args.variant, steps=args.steps, warmup=args.warmup, config=w,
               num_nodes=b.num_nodes, native_jk_lstm=ops.native_jk_lstm(), loss=float(step()[0]),
               lstm_bytes=lstm_bytes(b.num_nodes, w["H"], w["L"], w["L"] + 1))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    out["eager_ms"] = J.timed(step, args.steps, args.warmup)
    out["max_memory_allocated"] = torch.cuda.max_memory_allocated(dev)
    if args.variant == "native" and not args.no_graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            keep = step()
        out["graph_ms"] = J.timed(g.replay, args.steps, args.warmup)
        out["graph_loss"] = float(keep[0])
        del g, keep
    names, real = [], _lib.launch

    def spy(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)

    _lib.launch = spy
    try:
        step()
        torch.cuda.synchronize()
    finally:
        _lib.launch = real
    counts = {}
    for n in names:
        counts[n] = counts.get(n, 0) + 1
    out["launches"] = counts
    out["launch_total"] = len(names)
    return out


def compare(args):
    """Fresh processes, alternating: framework, native, framework, native, ...  (this process never opens the device).  Every
    run has a time limit of its own, and the first run that fails or is killed ends the comparison: nothing more is started."""
    variants = ["framework", "native"]
    runs = {v: [] for v in variants}
    limit = ["timeout", "-k", "10", str(args.run_timeout)] if shutil.which("timeout") else []
    for _ in range(args.runs):
        for v in variants:
            cmd = limit + [sys.executable, os.path.abspath(__file__), "--variant", v, "--steps", str(args.steps),
                           "--warmup", str(args.warmup)] + (["--no-graph"] if args.no_graph else [])
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.run_timeout + 30, cwd=HERE)
            if r.returncode != 0:
                print(f"[jk_lstm_step] the {v} run failed with exit status {r.returncode}; stopping", file=sys.stderr)
                sys.exit(1 if r.returncode == 1 else 3)      # (3: not an ordinary failure - the caller should start nothing more)
            runs[v].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(f"[jk_lstm_step] {v} run {len(runs[v])} done", file=sys.stderr, flush=True)
    first = runs["native"][0]
    result = {"device": first["device"], "steps": args.steps, "warmup": args.warmup, "runs": args.runs, "config": J.CONFIG,
              "num_nodes": first["num_nodes"], "lstm_bytes": first["lstm_bytes"], "variants": {}}
    for v in variants:
        ws = runs[v]
        e = dict(eager_ms=J.summary([x["eager_ms"] for x in ws]),
                 max_memory_allocated=J.summary([x["max_memory_allocated"] for x in ws]),
                 loss=ws[0]["loss"], launches=ws[0]["launches"], launch_total=ws[0]["launch_total"])
        if "graph_ms" in ws[0]:
            e["graph_ms"] = J.summary([x["graph_ms"] for x in ws])
            e["graph_loss"] = ws[0]["graph_loss"]
        else:
            e["graph_ms"] = "not captured"
        result["variants"][v] = e
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--variant", choices=("native", "framework"), default=None, help="one run of this variant in this process")
    ap.add_argument("--no-graph", action="store_true", help="eager steps only")
    ap.add_argument("--runs", type=int, default=3, help="pairs of runs")
    ap.add_argument("--run-timeout", type=int, default=240, help="seconds one run may take")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    result = one_run(args) if args.variant else compare(args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
