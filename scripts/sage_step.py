"""Training-step time (forward + loss + backward, no optimiser) of a KP-GraphSAGE body, K = 8, L = 8, h = 104 (the per-hop
shape of the golden layer case: dk = 13) on 2048 synthetic_zinc_batch molecules, with the tail on kpgnn_sage_tail_fwd / _bwd and
with ops_dense.set_native_sage_tail(False) (the framework expression cat -> baddbmm -> relu -> normalize -> combine ->
combine_proj).  On a commit without the switch only the framework setting exists and is what gets timed: the same arguments
there give the parent's figure.

    python scripts/sage_step.py --out profiles/sage/sage_step.json
    python scripts/sage_step.py --no-graph --steps 5        # e.g. under a kernel trace
    python scripts/sage_step.py --kernels                   # adds the device kernel list of one step (torch.profiler)

ONE process, both settings ALTERNATING: the model is built once, and each of `--rounds` rounds times first the framework
setting and then the native one - `--steps` eager steps after `--warmup`, each bracketed by two HIP events, then the same number
of replays of that setting's captured hipGraph (captured once, before the first round).  A round's figure is the median step;
reported per setting are the median over the rounds and their spread (min .. max).  Also per setting: the loss, the C-ABI
launches of one eager step (name: count, in order of first appearance), the framework ops of one step that belong to the tail
(aten name: count) and torch.cuda.max_memory_allocated over the eager steps."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIG = dict(model="KPGraphSAGE", K=8, L=8, H=104, graphs=2048, drop=0.0, combine="geometric", norm="Batch")
TAIL_OPS = ("aten::cat", "aten::baddbmm", "aten::bmm", "aten::relu", "aten::threshold_backward", "aten::linalg_vector_norm",
            "aten::clamp_min", "aten::div", "aten::mul", "aten::sum", "aten::addmm", "aten::mm", "aten::linear")


def build_batch(dev):
    from kp_gnn_amd.batch import synthetic_zinc_batch
    b = synthetic_zinc_batch(CONFIG["graphs"], seed0=1, K=CONFIG["K"], num_threads=min(16, os.cpu_count() or 1)).to(dev)
    b.build_csr()
    return b


def build_model(dev):
    import torch
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    w = CONFIG
    ns = argparse.Namespace(model_name=w["model"], hidden_size=w["H"], K=w["K"], num_layer=w["L"], num_hop1_edge=3, max_pe_num=50,
                            combine=w["combine"], eps=0., train_eps=False, aggr="add")
    torch.manual_seed(0)
    gnn = B.make_GNN(ns)(num_layer=w["L"], gnn_layer=make_gnn_layer(ns), JK="concat", norm_type=w["norm"],
                         init_emb=B.EmbeddingEncoder(21, w["H"]), residual=True, virtual_node=False, use_rd=False,
                         num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=w["drop"])
    return B.GraphRegression(gnn, "sum").to(dev).train()


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


def summary(vals):
    return dict(median=statistics.median(vals), min=min(vals), max=max(vals), rounds=vals)


def profiled(step, kernels):
    """(tail-related framework ops, device kernels) of one step: {name: count}."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    acts = [ProfilerActivity.CPU] + ([ProfilerActivity.CUDA] if kernels else [])
    with profile(activities=acts) as prof:
        step()
        torch.cuda.synchronize()
    ops, kern = {}, {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CPU:
            if e.name in TAIL_OPS:
                ops[e.name] = ops.get(e.name, 0) + 1
        else:
            kern[e.name] = kern.get(e.name, 0) + 1
    return ops, kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds of (framework, native)")
    ap.add_argument("--no-graph", action="store_true", help="eager steps only")
    ap.add_argument("--kernels", action="store_true", help="record the device kernel list of one step per setting")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    from kp_gnn_amd import _lib, ops, ops_dense
    dev = torch.device("cuda:0")
    b = build_batch(dev)
    model = build_model(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    switch = getattr(ops_dense, "set_native_sage_tail", None)
    settings = ("framework", "native") if switch is not None else ("framework",)

    def select(s):
        if switch is not None:
            switch(s == "native")

    def step():
        score = model(b)
        loss, dscore = ops_dense.regression_loss_and_grad(score, b.y, "l1")
        with ops.deferred_reductions():
            grads = torch.autograd.grad(score, params, grad_outputs=dscore, allow_unused=True)
        return loss, grads

    out = {s: dict(eager=[], graph=[]) for s in settings}
    graphs = {}
    for s in settings:
        select(s)
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
        out[s]["tail_ops"], kern = profiled(step, args.kernels)
        if args.kernels:
            out[s]["kernels"], out[s]["kernel_total"] = kern, sum(kern.values())
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
        for s in settings:                       # alternating: a drift of the machine reaches both settings alike
            select(s)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            out[s]["eager"].append(timed(step, args.steps, args.warmup))
            peak[s] = max(peak.get(s, 0), torch.cuda.max_memory_allocated(dev))
            if s in graphs:
                out[s]["graph"].append(timed(graphs[s][0].replay, args.steps, args.warmup))
    select("native")
    result = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
              "config": CONFIG, "num_nodes": b.num_nodes}
    for s in settings:
        e = dict(eager_ms=summary(out[s]["eager"]), loss=out[s]["loss"], launches=out[s]["launches"],
                 launch_total=out[s]["launch_total"], tail_ops=out[s]["tail_ops"], max_memory_allocated=peak[s])
        for k in ("kernels", "kernel_total"):
            if k in out[s]:
                e[k] = out[s][k]
        if out[s]["graph"]:
            e["graph_ms"] = summary(out[s]["graph"])
            e["graph_loss"] = out[s]["graph_loss"]
        result[s] = e
    del graphs
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
