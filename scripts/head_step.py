"""Training-step time (forward + loss + backward, no optimiser) of three task-head workloads, with the native head and with the
same head written in plain torch ops (--framework-head), on synthetic_zinc_batch data:

    graph_property   KP-GIN+, K = 6, L = 6, h = 96, 128 graphs, attention readout, MSE      (train_graph_property.py's default)
    tu               KP-GIN,  K = 2, L = 2, h = 32, 128 graphs, sum readout, C = 2, NLL     (train_TU.py / train_EXP.py)
    tu_max           the same with the max readout (--pooling_method max)

    python scripts/head_step.py                       # every workload, both heads, 3 interleaved runs per side, one JSON line
    python scripts/head_step.py --framework-head      # the framework head only
    python scripts/head_step.py --native-head         # the native head only

Per run: `--steps` steps after `--warmup`, each bracketed by two HIP events; the run's figure is the median step.  The head's own
time is measured the same way on the head alone (readout + Linear + loss and their backward, from a detached copy of the
body's node rows).  Reported per side: the median over the runs and their spread (min .. max).  Also prints the C-ABI launches
of one head step."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {
    "graph_property": dict(model="KPGINPlus", K=6, L=6, H=96, graphs=128, pooling="attention", task="mse"),
    "tu": dict(model="KPGIN", K=2, L=2, H=32, graphs=128, pooling="sum", task="nll", C=2),
    "tu_max": dict(model="KPGIN", K=2, L=2, H=32, graphs=128, pooling="max", task="nll", C=2),
}


def build(w, dev):
    from kp_gnn_amd import body as B
    from kp_gnn_amd.batch import synthetic_zinc_batch
    from kp_gnn_amd.layers import make_gnn_layer
    ns = argparse.Namespace(model_name=w["model"], hidden_size=w["H"], K=w["K"], num_layer=w["L"], num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(0)
    gnn = B.make_GNN(ns)(num_layer=w["L"], gnn_layer=make_gnn_layer(ns), JK="concat", norm_type="Batch",
                         init_emb=B.EmbeddingEncoder(21, w["H"]), residual=True, virtual_node=False, use_rd=False,
                         num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=0.0)
    model = B.GraphRegression(gnn, w["pooling"]) if w["task"] == "mse" else B.GraphClassification(gnn, w["pooling"], w["C"])
    model = model.to(dev).train()
    b = synthetic_zinc_batch(w["graphs"], seed0=1, K=w["K"]).to(dev)
    b.build_csr()
    g = torch.Generator().manual_seed(2)
    y = torch.randn(w["graphs"], generator=g) if w["task"] == "mse" else torch.randint(0, w["C"], (w["graphs"],), generator=g)
    return model, b, y.to(dev)


def native_head(model, w, x, b, y):
    from kp_gnn_amd import ops_dense
    pooled = model.pool(x, b.batch, b.num_graphs)
    if w["task"] == "mse":
        return ops_dense.regression_loss(ops_dense.score_head(pooled, model.regressor).squeeze(), y, "mse")
    return ops_dense.classification_loss(ops_dense.head_linear(pooled, model.classifier), y)


def framework_head(model, w, x, b, y):
    """The same head in plain torch ops: PyG's formulation of the readout, nn.Linear, the scripts' loss."""
    G, idx = b.num_graphs, b.batch
    if w["pooling"] == "attention":
        gate = F.linear(x, model.pool.gate_nn.weight, model.pool.gate_nn.bias).reshape(-1)
        mx = gate.new_full((G,), float("-inf")).scatter_reduce(0, idx, gate.detach(), reduce="amax")
        e = (gate - mx[idx]).exp()
        alpha = e / (gate.new_zeros(G).index_add_(0, idx, e)[idx] + 1e-16)
        pooled = x.new_zeros((G, x.shape[1])).index_add_(0, idx, alpha.unsqueeze(-1) * x)
    elif w["pooling"] == "max":
        pooled = x.new_full((G, x.shape[1]), float("-inf")).scatter_reduce(0, idx.view(-1, 1).expand_as(x), x, reduce="amax")
    else:
        pooled = x.new_zeros((G, x.shape[1])).index_add_(0, idx, x)
    if w["task"] == "mse":
        return F.mse_loss(F.linear(pooled, model.regressor.weight, model.regressor.bias).squeeze(), y)
    return F.nll_loss(F.log_softmax(F.linear(pooled, model.classifier.weight, model.classifier.bias), dim=-1), y)


def timed(fn, steps, warmup):
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


def one_run(model, w, b, y, head, steps, warmup):
    params = [p for p in model.parameters() if p.requires_grad]

    def step():
        loss = head(model, w, model.embedding_model(b), b, y)
        torch.autograd.grad(loss, params, allow_unused=True)
        return loss

    with torch.no_grad():
        x0 = model.embedding_model(b).detach()
    head_params = [p for n, p in model.named_parameters() if not n.startswith("embedding_model.")]

    def head_step():
        x = x0.requires_grad_(True)
        torch.autograd.grad(head(model, w, x, b, y), [x] + head_params)

    loss = float(step())
    return dict(step_ms=timed(step, steps, warmup), head_ms=timed(head_step, steps, warmup), loss=loss)


def launches_of(model, w, b, y, head):
    from kp_gnn_amd import _lib
    x = model.embedding_model(b).detach().requires_grad_(True)
    names, real = [], _lib.launch

    def spy(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)

    _lib.launch = spy
    try:
        head(model, w, x, b, y).backward()
        torch.cuda.synchronize()
    finally:
        _lib.launch = real
    return names


def summary(runs, key):
    v = [r[key] for r in runs]
    return dict(median=statistics.median(v), min=min(v), max=max(v), runs=v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["all"], default="all")
    ap.add_argument("--framework-head", action="store_true", help="only the head written in plain torch ops")
    ap.add_argument("--native-head", action="store_true", help="only the native head")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3, help="interleaved runs per side")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sides = [("native", native_head), ("framework", framework_head)]
    if args.framework_head and not args.native_head:
        sides = sides[1:]
    if args.native_head and not args.framework_head:
        sides = sides[:1]
    result = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "workloads": {}}
    for name in (sorted(WORKLOADS) if args.workload == "all" else [args.workload]):
        w = WORKLOADS[name]
        model, b, y = build(w, dev)
        runs = {s: [] for s, _ in sides}
        for _ in range(args.runs):                       # interleaved: native, framework, native, framework, ...
            for s, head in sides:
                runs[s].append(one_run(model, w, b, y, head, args.steps, args.warmup))
        out = {"config": w, "num_nodes": b.num_nodes}
        for s, head in sides:
            out[s] = dict(step_ms=summary(runs[s], "step_ms"), head_ms=summary(runs[s], "head_ms"), loss=runs[s][0]["loss"],
                          head_launches=launches_of(model, w, b, y, head))
            print(f"[head_step] {name} {s}: head launches {out[s]['head_launches']}", file=sys.stderr)
        result["workloads"][name] = out
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
