"""Training-step time (forward + loss + backward, no optimiser) of three workloads with virtual_node=True, eagerly and as one
captured hipGraph, on synthetic batches:

    zinc_b2048   KP-GIN+, K = 8, L = 8, h = 104, 2048 graphs       (bench.py's default body, plus the virtual node)
    zinc_b64     the same at 64 graphs
    qm9_b128     KP-GIN,  K = 6, L = 8, h = 120, 128 graphs         (run_qm9_targets.py's recipe: --virtual_node)

    python scripts/vn_step.py                          # this checkout: one run per workload, one JSON line
    python scripts/vn_step.py --against ../parent      # runs of that checkout and of this one, interleaved (fresh processes)
    python scripts/vn_step.py --repo ../parent         # one run of another checkout (what --against starts)

Per run: `--steps` steps after `--warmup`, each bracketed by two HIP events; the run's figure is the median step.  A checkout
without ops.virtual_node_add (the framework formulation of the virtual node: a host read-back per forward) cannot be captured
and is timed eagerly only.  Also reports the C-ABI launches of one eager step (name: count, in order of first appearance).
With --against: per side the median over the runs and their spread (min .. max)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKLOADS = {
    "zinc_b2048": dict(data="zinc", model="KPGINPlus", K=8, L=8, H=104, graphs=2048),
    "zinc_b64": dict(data="zinc", model="KPGINPlus", K=8, L=8, H=104, graphs=64),
    "qm9_b128": dict(data="qm9", model="KPGIN", K=6, L=8, H=120, graphs=128),
}


def build(w, dev):
    import torch
    from kp_gnn_amd import batch as KB, body as B
    from kp_gnn_amd.layers import make_gnn_layer
    qm9 = w["data"] == "qm9"
    ns = argparse.Namespace(model_name=w["model"], hidden_size=w["H"], K=w["K"], num_layer=w["L"], num_hop1_edge=4 if qm9 else 3,
                            max_pe_num=50, combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(0)
    enc = B.QM9InputEncoder(w["H"]) if qm9 else B.EmbeddingEncoder(21, w["H"])
    kw = dict(max_edge_count=20, max_hop_num=5, max_distance_count=15) if qm9 else \
        dict(max_edge_count=50, max_hop_num=6, max_distance_count=50)
    gnn = B.make_GNN(ns)(num_layer=w["L"], gnn_layer=make_gnn_layer(ns), JK="concat", norm_type="Batch", init_emb=enc,
                         residual=not qm9, virtual_node=True, use_rd=False, num_hop1_edge=ns.num_hop1_edge, drop_prob=0.0, **kw)
    model = B.GraphRegression(gnn, "sum").to(dev).train()
    make = KB.synthetic_qm9_batch if qm9 else KB.synthetic_zinc_batch
    b = make(w["graphs"], seed0=1, K=w["K"], num_threads=min(16, os.cpu_count() or 1)).to(dev)
    b.build_csr()
    return model, b


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
    from kp_gnn_amd import _lib, ops
    from kp_gnn_amd.ops_dense import regression_loss_and_grad
    model, b = build(w, dev)
    params = [p for p in model.parameters() if p.requires_grad]

    def step():
        score = model(b)
        loss, dscore = regression_loss_and_grad(score, b.y, "l1")
        with ops.deferred_reductions():
            grads = torch.autograd.grad(score, params, grad_outputs=dscore, allow_unused=True)
        return loss, grads

    native = hasattr(ops, "virtual_node_add")
    out = dict(config=w, num_nodes=b.num_nodes, native_virtual_node=native, loss=float(step()[0]))
    out["eager_ms"] = timed(step, steps, warmup)
    out["graph_ms"] = None
    if native:
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
    sys.path.insert(0, os.path.abspath(args.repo or HERE))
    import torch
    dev = torch.device("cuda:0")
    names = sorted(WORKLOADS) if args.workload == "all" else [args.workload]
    return {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
            "workloads": {n: one_workload(WORKLOADS[n], dev, args.steps, args.warmup) for n in names}}


def summary(vals):
    vals = [v for v in vals if v is not None]
    return None if not vals else dict(median=statistics.median(vals), min=min(vals), max=max(vals), runs=vals)


def compare(args):
    """Fresh processes, interleaved: other checkout, this one, other, this one, ...  (this process never opens the device)."""
    sides = [("parent", os.path.abspath(args.against)), ("branch", HERE)]
    runs = {s: [] for s, _ in sides}
    for _ in range(args.runs):
        for s, repo in sides:
            cmd = [sys.executable, os.path.abspath(__file__), "--repo", repo, "--workload", args.workload,
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.run_timeout, cwd=repo)
            if r.returncode != 0:
                print(f"[vn_step] the {s} run failed with exit status {r.returncode}; stopping", file=sys.stderr)
                sys.exit(1 if r.returncode == 1 else 3)      # (3: not an ordinary failure - the caller should start nothing more)
            runs[s].append(json.loads(r.stdout.strip().splitlines()[-1]))
    result = {"device": runs["branch"][0]["device"], "steps": args.steps, "warmup": args.warmup, "runs": args.runs, "workloads": {}}
    for name in runs["branch"][0]["workloads"]:
        entry = {"config": WORKLOADS[name]}
        for s, _ in sides:
            ws = [r["workloads"][name] for r in runs[s]]
            entry[s] = dict(eager_ms=summary([x["eager_ms"] for x in ws]), graph_ms=summary([x["graph_ms"] for x in ws]),
                            loss=ws[0]["loss"], launches=ws[0]["launches"], launch_total=ws[0]["launch_total"],
                            native_virtual_node=ws[0]["native_virtual_node"], num_nodes=ws[0]["num_nodes"])
        result["workloads"][name] = entry
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["all"], default="all")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repo", default=None, help="import kp_gnn_amd from this checkout instead of the script's own")
    ap.add_argument("--against", default=None, help="a built checkout of the parent commit: interleaved runs of both")
    ap.add_argument("--runs", type=int, default=3, help="runs per side with --against")
    ap.add_argument("--run-timeout", type=int, default=300, help="seconds one run may take with --against")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    result = compare(args) if args.against else one_run(args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
