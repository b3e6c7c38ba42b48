"""Training-step time (forward + loss + backward, no optimiser) of KP-GIN+, K = 8, L = 8, h = 104 on 2048 synthetic_zinc_batch
molecules with norm_type = Layer / Instance / GraphSize / Pair, with the native norms (kpgnn_body_norm_fwd / _bwd) and with
ops.set_native_norms(False) (the framework expressions of ops.body_norm_reference) - the yardstick is the framework expression
on the same commit: no earlier commit has these norms at all.

    python scripts/norm_step.py --out profiles/norms/norm_step.json
    python scripts/norm_step.py --norm Pair --no-graph --steps 5        # e.g. under a kernel trace

ONE process, both settings ALTERNATING: per norm the model is built once, and each of `--rounds` rounds times first the
framework setting and then the native one - `--steps` eager steps after `--warmup`, each bracketed by two HIP events, then the
same number of replays of that setting's captured hipGraph (captured once, before the first round).  A round's figure is the
median step; reported per setting are the median over the rounds and their spread (min .. max).  Also per setting: the loss, the
C-ABI launches of one eager step (name: count, in order of first appearance) and torch.cuda.max_memory_allocated over the eager
steps.  norm_bytes: what the norm has to move per layer and direction, counted from the shapes (csrc/body_norm.hip).

    python scripts/norm_step.py --scope graph --out profiles/norms/norm_step_graph.json

--scope graph times the PER-GRAPH norms (norm_scope="graph", kpgnn_graph_norm_fwd / _bwd, csrc/body_norm_graph.hip): per round
the framework per-graph expression, the native per-graph route, and - a second model of the same weights with
norm_scope="batch" - the whole-batch native route, in that order.  Per setting also launch_ms: every kpgnn_*_norm_* call of
three eager steps bracketed by two HIP events (the time of one call as the stream sees it; no counters are collected)."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIG = dict(model="KPGINPlus", K=8, L=8, H=104, graphs=2048, drop=0.0)
NORMS = ("Layer", "Instance", "GraphSize", "Pair")
SETTINGS = ("framework", "native")
GRAPH_SETTINGS = SETTINGS + ("whole_batch",)      # --scope graph: the whole-batch native route of the same weights beside them


def build_batch(dev):
    from kp_gnn_amd.batch import synthetic_zinc_batch
    b = synthetic_zinc_batch(CONFIG["graphs"], seed0=1, K=CONFIG["K"], num_threads=min(16, os.cpu_count() or 1)).to(dev)
    b.build_csr()
    return b


def build_model(norm, dev, norm_scope="batch"):
    import torch
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    w = CONFIG
    ns = argparse.Namespace(model_name=w["model"], hidden_size=w["H"], K=w["K"], num_layer=w["L"], num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(0)
    gnn = B.make_GNN(ns)(num_layer=w["L"], gnn_layer=make_gnn_layer(ns), JK="concat", norm_type=norm,
                         init_emb=B.EmbeddingEncoder(21, w["H"]), residual=True, virtual_node=False, use_rd=False,
                         num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=w["drop"],
                         norm_scope=norm_scope)
    return B.GraphRegression(gnn, "sum").to(dev).train()


def norm_bytes(N, C, norm):
    """Bytes one norm moves per direction (the residual included forward): the statistics pass reads x (and gout backward),
    the apply pass reads them again and writes the result; GraphSize is the apply pass alone."""
    e = 4 * N * C
    if norm == "GraphSize":
        return dict(fwd=3 * e, bwd=2 * e)
    return dict(fwd=e + 3 * e, bwd=2 * e + 3 * e)


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


def norm_launch_ms(step, steps=3):
    """{entry: median / min / max ms and the number of calls} of the kpgnn_*_norm_* calls of `steps` eager steps, each call
    bracketed by two HIP events on its stream."""
    import torch
    from kp_gnn_amd import _lib
    real, rec = _lib.launch, {}

    def spy(name, *a, **k):
        if "_norm_" not in name:
            return real(name, *a, **k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = real(name, *a, **k)
        e1.record()
        rec.setdefault(name, []).append((e0, e1))
        return rc

    _lib.launch = spy
    try:
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
    finally:
        _lib.launch = real
    out = {}
    for name, evs in rec.items():
        ms = [a.elapsed_time(z) for a, z in evs]
        out[name] = dict(median=statistics.median(ms), min=min(ms), max=max(ms), calls=len(ms))
    return out


def summary(vals):
    return dict(median=statistics.median(vals), min=min(vals), max=max(vals), rounds=vals)


def one_norm(norm, b, dev, args):
    import torch
    from kp_gnn_amd import _lib, ops, ops_dense
    settings = GRAPH_SETTINGS if args.scope == "graph" else SETTINGS
    model = build_model(norm, dev, args.scope)
    models = {s: model for s in SETTINGS}
    if args.scope == "graph":
        models["whole_batch"] = build_model(norm, dev, "batch")        # (seeded alike: the same weights)

    def step_of(m):
        params = [p for p in m.parameters() if p.requires_grad]

        def step():
            score = m(b)
            loss, dscore = ops_dense.regression_loss_and_grad(score, b.y, "l1")
            with ops.deferred_reductions():
                grads = torch.autograd.grad(score, params, grad_outputs=dscore, allow_unused=True)
            return loss, grads
        return step

    steps = {s: step_of(models[s]) for s in settings}
    out = {s: dict(eager=[], graph=[]) for s in settings}
    graphs = {}
    prev_kind = ops.set_native_norm_exact(norm, True)     # ("GraphSize" is opt-in on exact-shape batches: here native means native)
    for s in settings:
        step = steps[s]
        ops.set_native_norms(s != "framework")
        out[s]["loss"] = float(step()[0])
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
        out[s]["launches"], out[s]["launch_total"] = counts, len(names)
        out[s]["launch_ms"] = norm_launch_ms(step)
        if not args.no_graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                keep = step()
            graphs[s] = (g, keep)
            g.replay()
            torch.cuda.synchronize()
            out[s]["graph_loss"] = float(keep[0])
    peak = {}
    for _ in range(args.rounds):
        for s in settings:                       # alternating: a drift of the machine reaches every setting alike
            ops.set_native_norms(s != "framework")
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            out[s]["eager"].append(timed(steps[s], args.steps, args.warmup))
            peak[s] = max(peak.get(s, 0), torch.cuda.max_memory_allocated(dev))
            if s in graphs:
                out[s]["graph"].append(timed(graphs[s][0].replay, args.steps, args.warmup))
    ops.set_native_norms(True)
    ops.set_native_norm_exact(norm, prev_kind)
    res = dict(num_nodes=b.num_nodes, norm_bytes=norm_bytes(b.num_nodes, CONFIG["H"], norm))
    for s in settings:
        e = dict(eager_ms=summary(out[s]["eager"]), loss=out[s]["loss"], launches=out[s]["launches"],
                 launch_total=out[s]["launch_total"], launch_ms=out[s]["launch_ms"], max_memory_allocated=peak[s])
        if out[s]["graph"]:
            e["graph_ms"] = summary(out[s]["graph"])
            e["graph_loss"] = out[s]["graph_loss"]
        res[s] = e
    del graphs
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--norm", choices=NORMS + ("all",), default="all")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds of (framework, native)")
    ap.add_argument("--no-graph", action="store_true", help="eager steps only")
    ap.add_argument("--scope", choices=("batch", "graph"), default="batch",
                    help="graph: the per-graph norms (norm_scope='graph'), with the whole-batch native route beside them")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    dev = torch.device("cuda:0")
    b = build_batch(dev)
    norms = NORMS if args.norm == "all" else (args.norm,)
    result = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
              "scope": args.scope, "config": CONFIG, "norm": {}}
    for norm in norms:
        result["norm"][norm] = one_norm(norm, b, dev, args)
        print(f"[norm_step] {norm} done", file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
