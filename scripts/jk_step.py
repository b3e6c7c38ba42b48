"""Training-step time (forward + loss + backward, no optimiser) of KP-GIN+, K = 8, L = 8, h = 104 on 2048 synthetic_zinc_batch
molecules with the jumping-knowledge readouts JK = sum / max / attention, with the native reduce (kpgnn_jk_reduce_fwd / _bwd:
the S = 9 states read in place) and with ops.set_native_jk(False) (the torch.stack expressions):

    python scripts/jk_step.py                         # all three JKs, both variants, 3 alternating pairs of fresh processes
    python scripts/jk_step.py --variant native        # one run of one variant in this process (what the pairs start)
    python scripts/jk_step.py --variant native --jk max --no-graph --steps 5      # e.g. under a kernel trace

sum and max are timed eagerly and as one captured hipGraph; attention eagerly only here (scripts/jk_lstm_step.py times its
scoring LSTM, native against the framework module, and captures the native step).  Per run: `--steps` steps after `--warmup`, each bracketed by two HIP
events; the run's figure is the median step.  Also per run: torch.cuda.max_memory_allocated over the eager steps, the C-ABI
launches of one eager step (name: count, in order of first appearance), and the bytes the reduce needs per direction, counted
from the shapes.  Reported per variant: the median over the runs and their spread (min .. max)."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIG = dict(model="KPGINPlus", K=8, L=8, H=104, graphs=2048, drop=0.0)
JKS = ("sum", "max", "attention")
CAPTURED = ("sum", "max")


def build_batch(dev):
    from kp_gnn_amd.batch import synthetic_zinc_batch
    b = synthetic_zinc_batch(CONFIG["graphs"], seed0=1, K=CONFIG["K"], num_threads=min(16, os.cpu_count() or 1)).to(dev)
    b.build_csr()
    return b


def build_model(JK, dev):
    import torch
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    w = CONFIG
    ns = argparse.Namespace(model_name=w["model"], hidden_size=w["H"], K=w["K"], num_layer=w["L"], num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(0)
    gnn = B.make_GNN(ns)(num_layer=w["L"], gnn_layer=make_gnn_layer(ns), JK=JK, norm_type="Batch",
                         init_emb=B.EmbeddingEncoder(21, w["H"]), residual=True, virtual_node=False, use_rd=False,
                         num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=w["drop"])
    return B.GraphRegression(gnn, "sum").to(dev).train()


def reduce_bytes(N, H, S, JK):
    """Bytes the reduce has to move per direction, from the shapes (csrc/jk_reduce.hip): fwd 4 N H (S + 1) (+ N H for arg, + the
    [N,S] score and weights); max bwd 4 N H (S + 1) + N H; softmax bwd 4 N H (2 S + 1) + three [N,S] arrays."""
    fwd = 4 * N * H * (S + 1)
    if JK == "sum":
        return dict(fwd=fwd, bwd=0)
    if JK == "max":
        return dict(fwd=fwd + N * H, bwd=4 * N * H * (S + 1) + N * H)
    return dict(fwd=fwd + 2 * 4 * N * S, bwd=4 * N * H * (2 * S + 1) + 3 * 4 * N * S)


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, z in ev:
        a.record()
        fn()
        z.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(z) for a, z in ev)


def one_jk(JK, b, dev, steps, warmup, graph):
    import torch
    from kp_gnn_amd import _lib, ops, ops_dense
    model = build_model(JK, dev)
    params = [p for p in model.parameters() if p.requires_grad]

    def step():
        score = model(b)
        loss, dscore = ops_dense.regression_loss_and_grad(score, b.y, "l1")
        with ops.deferred_reductions():
            grads = torch.autograd.grad(score, params, grad_outputs=dscore, allow_unused=True)
        return loss, grads

    mode = "softmax" if JK == "attention" else JK
    out = dict(num_nodes=b.num_nodes, native_jk=ops.native_jk(mode), loss=float(step()[0]),
               reduce_bytes=reduce_bytes(b.num_nodes, CONFIG["H"], CONFIG["L"] + 1, JK))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    out["eager_ms"] = timed(step, steps, warmup)
    out["max_memory_allocated"] = torch.cuda.max_memory_allocated(dev)
    if graph and JK in CAPTURED:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            keep = step()
        out["graph_ms"] = timed(g.replay, steps, warmup)
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


def one_run(args):
    sys.path.insert(0, HERE)
    import torch
    from kp_gnn_amd import ops
    ops.set_native_jk(args.variant == "native")
    dev = torch.device("cuda:0")
    b = build_batch(dev)
    jks = JKS if args.jk == "all" else (args.jk,)
    return {"device": torch.cuda.get_device_name(0), "variant": args.variant, "steps": args.steps, "warmup": args.warmup,
            "config": CONFIG, "jk": {JK: one_jk(JK, b, dev, args.steps, args.warmup, not args.no_graph) for JK in jks}}


def summary(vals):
    return dict(median=statistics.median(vals), min=min(vals), max=max(vals), runs=vals)


def compare(args):
    """Fresh processes, alternating: framework, native, framework, native, ...  (this process never opens the device).  Every
    run has a time limit of its own, and the first run that fails or is killed ends the comparison: nothing more is started."""
    variants = ["framework", "native"]
    runs = {v: [] for v in variants}
    limit = ["timeout", "-k", "10", str(args.run_timeout)] if shutil.which("timeout") else []
    for _ in range(args.runs):
        for v in variants:
            cmd = limit + [sys.executable, os.path.abspath(__file__), "--variant", v, "--jk", args.jk,
                           "--steps", str(args.steps), "--warmup", str(args.warmup)] + (["--no-graph"] if args.no_graph else [])
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.run_timeout + 30, cwd=HERE)
            if r.returncode != 0:
                print(f"[jk_step] the {v} run failed with exit status {r.returncode}; stopping", file=sys.stderr)
                sys.exit(1 if r.returncode == 1 else 3)      # (3: not an ordinary failure - the caller should start nothing more)
            runs[v].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(f"[jk_step] {v} run {len(runs[v])} done", file=sys.stderr, flush=True)
    result = {"device": runs["native"][0]["device"], "steps": args.steps, "warmup": args.warmup, "runs": args.runs,
              "config": CONFIG, "jk": {}}
    for JK in runs["native"][0]["jk"]:
        entry = {}
        for v in variants:
            ws = [r["jk"][JK] for r in runs[v]]
            e = dict(eager_ms=summary([x["eager_ms"] for x in ws]),
                     max_memory_allocated=summary([x["max_memory_allocated"] for x in ws]),
                     loss=ws[0]["loss"], launches=ws[0]["launches"], launch_total=ws[0]["launch_total"],
                     num_nodes=ws[0]["num_nodes"], reduce_bytes=ws[0]["reduce_bytes"])
            if "graph_ms" in ws[0]:
                e["graph_ms"] = summary([x["graph_ms"] for x in ws])
            entry[v] = e
        result["jk"][JK] = entry
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jk", choices=JKS + ("all",), default="all")
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
