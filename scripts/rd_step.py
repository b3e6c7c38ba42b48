"""The resistance-distance feature (`--use_rd`), measured in two places.

    python scripts/rd_step.py --out profiles/rd/rd_step.json
    python scripts/rd_step.py --part build --graphs 2000          # only (a), fewer graphs

(a) build: the time to compute the `rd` column of `--graphs` (10,000) ZINC-shaped and as many QM9-shaped synthetic molecules from
    their K-hop edge lists (K = 8 / K = 6, spd; the reference computes rd after its K-hop transform): the batched kernel through
    ops.resistance_distance (edge list already on the device, as in KHopDataset.from_collated; status read-back and host fills
    included; median of `--rounds` runs after one warm-up), the float64 numpy route khop_transform.resistance_distance_host per
    graph, and the reference's recipe restated - a scipy csgraph Laplacian of float32 ones and scipy.linalg.pinv per graph -
    where scipy imports.  Also the share of graphs per kernel status and the largest distance of the kernel from the numpy route.
(b) step: forward + MSE loss + backward (no optimiser) of the `qm9` workload's body - KP-GIN, K = 6, L = 8, h = 120, QM9 encoder -
    with use_rd=True on 128 and on 2048 QM9-shaped molecules whose batch carries rd, with the native projection
    (kpgnn_rd_proj_fwd / _bwd) and with ops.set_native_rd_proj(False) - the framework Linear(1, H), the parent commit's code path.
    ONE process, both settings ALTERNATING per round: `--steps` eager steps after `--warmup`, each bracketed by two HIP events,
    then as many replays of that setting's captured hipGraph.  A round's figure is the median step; reported are the median over
    the rounds and their spread (min .. max), the loss, and the C-ABI launches of one eager step."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEP = dict(model="KPGIN", K=6, L=8, H=120, batches=(128, 2048))
SETTINGS = ("framework", "native")
SHAPES = {"zinc": (8, 50, 6, 3, 50, 50, "spd"), "qm9": (6, 50, 5, 4, 20, 15, "spd")}


def khop_lists(shape, graphs, threads):
    """(node_ptr, K-hop edge_ptr, K-hop edge_index with global ids) of `graphs` synthetic molecules."""
    from kp_gnn_amd import khop_transform as KT
    node_ptr, edge_ptr, ei, ea, _ = KT.synth_molecules(graphs, 1, shape=KT.qm9_shape() if shape == "qm9" else None)
    out = KT.khop_batch(node_ptr, edge_ptr, ei, ea, *SHAPES[shape], num_threads=threads)
    return node_ptr, out["edge_ptr"].numpy(), out["edge_index"]


def scipy_recipe(n, ei):
    """data_utils.py:280-303 restated: float32 ones -> csgraph.laplacian -> linalg.pinv, all in float32."""
    import numpy as np
    import scipy.linalg
    import scipy.sparse as ssp
    import scipy.sparse.csgraph  # noqa: F401
    adj = ssp.coo_matrix((np.ones(ei.shape[1], dtype=np.float32), (ei[0], ei[1])), (n, n)).tocsr()
    Lp = scipy.linalg.pinv(ssp.csgraph.laplacian(adj).toarray())
    return Lp[0, 0] + np.diagonal(Lp) - Lp[0, :] - Lp[:, 0]


def build_part(args, dev):
    import numpy as np
    import torch
    from kp_gnn_amd import ops
    from kp_gnn_amd.khop_transform import resistance_distance_host
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    res = {}
    for shape in SHAPES:
        node_ptr, edge_ptr, ei = khop_lists(shape, args.graphs, args.threads)
        ei_d = ei.to(dev)
        ops.resistance_distance(node_ptr, edge_ptr, ei_d, dev)              # warm-up (library load, LDS attribute)
        torch.cuda.synchronize()
        t_kernel = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            rd, status = ops.resistance_distance(node_ptr, edge_ptr, ei_d, dev)
            torch.cuda.synchronize()
            t_kernel.append(time.perf_counter() - t0)
        ei_h = ei.numpy()
        per_graph = [(int(node_ptr[g + 1] - node_ptr[g]), ei_h[:, edge_ptr[g]:edge_ptr[g + 1]] - node_ptr[g]) for g in range(args.graphs)]
        t0 = time.perf_counter()
        host = [resistance_distance_host(n, e) for n, e in per_graph]
        t_host = time.perf_counter() - t0
        diff = float(np.abs(np.concatenate(host) - rd.cpu().reshape(-1).double().numpy()).max())
        entry = dict(graphs=args.graphs, nodes=int(node_ptr[-1]), khop_edges=int(edge_ptr[-1]), max_nodes=int(np.diff(node_ptr).max()),
                     kernel_s=dict(median=statistics.median(t_kernel), min=min(t_kernel), max=max(t_kernel), rounds=t_kernel),
                     numpy_f64_s=t_host, status_share={str(s): float((status == s).float().mean()) for s in range(5)},
                     max_abs_kernel_minus_numpy_f64=diff)
        if have_scipy:
            t0 = time.perf_counter()
            ref = [scipy_recipe(n, e) for n, e in per_graph]
            entry["scipy_f32_s"] = time.perf_counter() - t0
            entry["max_abs_scipy_f32_minus_numpy_f64"] = float(np.abs(np.concatenate(ref).astype(np.float64) - np.concatenate(host)).max())
        res[shape] = entry
        print(f"[rd_step] build {shape} done", file=sys.stderr, flush=True)
    return res


def build_model(dev):
    import torch
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    w = STEP
    ns = argparse.Namespace(model_name=w["model"], hidden_size=w["H"], K=w["K"], num_layer=w["L"], num_hop1_edge=4, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(0)
    gnn = B.make_GNN(ns)(num_layer=w["L"], gnn_layer=make_gnn_layer(ns), JK="concat", norm_type="Batch",
                         init_emb=B.QM9InputEncoder(w["H"]), residual=False, virtual_node=False, use_rd=True, num_hop1_edge=4,
                         wo_peripheral_edge=False, wo_peripheral_configuration=False, drop_prob=0.0,
                         max_edge_count=20, max_hop_num=5, max_distance_count=15)
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


def step_part(args, dev, graphs):
    import torch
    from kp_gnn_amd import _lib, ops, ops_dense
    from kp_gnn_amd.batch import synthetic_qm9_batch
    host = synthetic_qm9_batch(graphs, seed0=1, K=STEP["K"], num_threads=args.threads)
    b = host.to(dev)
    b.rd = ops.resistance_distance(host.node_ptr, host.edge_ptr, b.edge_index, dev)[0]
    b.build_csr()
    model = build_model(dev)
    params = [p for p in model.parameters() if p.requires_grad]

    def step():
        score = model(b)
        loss, dscore = ops_dense.regression_loss_and_grad(score, b.y, "mse")
        with ops.deferred_reductions():
            grads = torch.autograd.grad(score, params, grad_outputs=dscore, allow_unused=True)
        return loss, grads

    out = {s: dict(eager=[], graph=[]) for s in SETTINGS}
    captured = {}
    for s in SETTINGS:
        ops.set_native_rd_proj(s == "native")
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
        out[s]["launch_total"] = len(names)
        out[s]["rd_launches"] = [n for n in names if "rd_proj" in n]
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
            captured[s] = (g, keep)
            g.replay()
            torch.cuda.synchronize()
            out[s]["graph_loss"] = float(keep[0])
    for _ in range(args.rounds):
        for s in SETTINGS:                       # alternating: a drift of the machine reaches both settings alike
            ops.set_native_rd_proj(s == "native")
            torch.cuda.synchronize()
            out[s]["eager"].append(timed(step, args.steps, args.warmup))
            if s in captured:
                out[s]["graph"].append(timed(captured[s][0].replay, args.steps, args.warmup))
    ops.set_native_rd_proj(True)
    res = dict(graphs=graphs, num_nodes=b.num_nodes)
    for s in SETTINGS:
        e = dict(eager_ms=summary(out[s]["eager"]), loss=out[s]["loss"], launch_total=out[s]["launch_total"],
                 rd_launches=out[s]["rd_launches"])
        if out[s]["graph"]:
            e["graph_ms"] = summary(out[s]["graph"])
            e["graph_loss"] = out[s]["graph_loss"]
        res[s] = e
    del captured
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("build", "step", "all"), default="all")
    ap.add_argument("--graphs", type=int, default=10000, help="graphs per shape of the build part")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds of (framework, native); runs of the build timing")
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1), help="host threads of the K-hop transform")
    ap.add_argument("--no-graph", action="store_true", help="eager steps only")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds}
    if args.part in ("build", "all"):
        result["build"] = build_part(args, dev)
    if args.part in ("step", "all"):
        result["step_config"] = {k: v for k, v in STEP.items() if k != "batches"}
        result["step"] = {}
        for graphs in STEP["batches"]:
            result["step"][str(graphs)] = step_part(args, dev, graphs)
            print(f"[rd_step] step B={graphs} done", file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
