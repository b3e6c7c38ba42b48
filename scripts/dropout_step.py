"""Training-step time (forward + loss + backward, no optimiser) of two bodies that drop out, with the native dropout
(kpgnn_dropout_fwd / _bwd: counter-based masks, the residual in the same launch) and with ops.set_native_dropout(False)
(nn.Dropout + a framework add), eagerly and as one captured hipGraph, on synthetic_zinc_batch data:

    tu           KP-GIN,  K = 4, L = 4, h = 32, JK = last, residual, drop_prob = 0.5, 2048 graphs, GraphClassification (sum, C = 2)
                 (train_TU.py's --drop_prob 0.5)
    zinc_b2048   KP-GIN+, K = 8, L = 8, h = 104, JK = concat, residual, drop_prob = 0.1, 2048 graphs   (bench.py's default body with
                 the bodies' own constructor default for drop_prob)

    python scripts/dropout_step.py                      # both workloads, both variants, 3 alternating pairs of fresh processes
    python scripts/dropout_step.py --variant native     # one run of one variant in this process (what the pairs start)

Per run: `--steps` steps after `--warmup`, each bracketed by two HIP events; the run's figure is the median step.  Also per run:
torch.cuda.max_memory_allocated over the eager steps and the C-ABI launches of one eager step (name: count, in order of first
appearance).  Reported per variant: the median over the runs and their spread (min .. max)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKLOADS = {
    "tu": dict(model="KPGIN", K=4, L=4, H=32, JK="last", drop=0.5, graphs=2048, head="classification"),
    "zinc_b2048": dict(model="KPGINPlus", K=8, L=8, H=104, JK="concat", drop=0.1, graphs=2048, head="regression"),
}


def build(w, dev):
    import torch
    from kp_gnn_amd import body as B
    from kp_gnn_amd.batch import synthetic_zinc_batch
    from kp_gnn_amd.layers import make_gnn_layer
    ns = argparse.Namespace(model_name=w["model"], hidden_size=w["H"], K=w["K"], num_layer=w["L"], num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(0)
    gnn = B.make_GNN(ns)(num_layer=w["L"], gnn_layer=make_gnn_layer(ns), JK=w["JK"], norm_type="Batch",
                         init_emb=B.EmbeddingEncoder(21, w["H"]), residual=True, virtual_node=False, use_rd=False,
                         num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=w["drop"])
    model = B.GraphClassification(gnn, "sum", 2) if w["head"] == "classification" else B.GraphRegression(gnn, "sum")
    model = model.to(dev).train()
    b = synthetic_zinc_batch(w["graphs"], seed0=1, K=w["K"], num_threads=min(16, os.cpu_count() or 1)).to(dev)
    b.build_csr()
    y = torch.randint(0, 2, (w["graphs"],), generator=torch.Generator().manual_seed(2)).to(dev)
    return model, b, y


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


def one_workload(w, dev, steps, warmup):
    import torch
    from kp_gnn_amd import _lib, ops, ops_dense
    model, b, y = build(w, dev)
    params = [p for p in model.parameters() if p.requires_grad]

    def step():
        if w["head"] == "classification":
            loss = ops_dense.classification_loss(model(b), y)
            with ops.deferred_reductions():
                grads = torch.autograd.grad(loss, params, allow_unused=True)
        else:
            score = model(b)
            loss, dscore = ops_dense.regression_loss_and_grad(score, b.y, "l1")
            with ops.deferred_reductions():
                grads = torch.autograd.grad(score, params, grad_outputs=dscore, allow_unused=True)
        return loss, grads

    ops.dropout_seed(7, dev)
    out = dict(config=w, num_nodes=b.num_nodes, native_dropout=ops.native_dropout(), loss=float(step()[0]))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    out["eager_ms"] = timed(step, steps, warmup)
    out["max_memory_allocated"] = torch.cuda.max_memory_allocated(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = step()
    out["graph_ms"] = timed(graph.replay, steps, warmup)
    out["graph_loss"] = float(keep[0])
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
    ops.set_native_dropout(args.variant == "native")
    dev = torch.device("cuda:0")
    names = sorted(WORKLOADS) if args.workload == "all" else [args.workload]
    return {"device": torch.cuda.get_device_name(0), "variant": args.variant, "steps": args.steps, "warmup": args.warmup,
            "workloads": {n: one_workload(WORKLOADS[n], dev, args.steps, args.warmup) for n in names}}


def summary(vals):
    return dict(median=statistics.median(vals), min=min(vals), max=max(vals), runs=vals)


def compare(args):
    """Fresh processes, alternating: framework, native, framework, native, ...  (this process never opens the device)."""
    variants = ["framework", "native"]
    runs = {v: [] for v in variants}
    for _ in range(args.runs):
        for v in variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--variant", v, "--workload", args.workload,
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.run_timeout, cwd=HERE)
            if r.returncode != 0:
                print(f"[dropout_step] the {v} run failed with exit status {r.returncode}; stopping", file=sys.stderr)
                sys.exit(1 if r.returncode == 1 else 3)      # (3: not an ordinary failure - the caller should start nothing more)
            runs[v].append(json.loads(r.stdout.strip().splitlines()[-1]))
    result = {"device": runs["native"][0]["device"], "steps": args.steps, "warmup": args.warmup, "runs": args.runs, "workloads": {}}
    for name in runs["native"][0]["workloads"]:
        entry = {"config": WORKLOADS[name]}
        for v in variants:
            ws = [r["workloads"][name] for r in runs[v]]
            entry[v] = dict(eager_ms=summary([x["eager_ms"] for x in ws]), graph_ms=summary([x["graph_ms"] for x in ws]),
                            max_memory_allocated=summary([x["max_memory_allocated"] for x in ws]),
                            loss=ws[0]["loss"], launches=ws[0]["launches"], launch_total=ws[0]["launch_total"],
                            num_nodes=ws[0]["num_nodes"])
        result["workloads"][name] = entry
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["all"], default="all")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--variant", choices=("native", "framework"), default=None, help="one run of this variant in this process")
    ap.add_argument("--runs", type=int, default=3, help="pairs of runs")
    ap.add_argument("--run-timeout", type=int, default=300, help="seconds one run may take")
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
