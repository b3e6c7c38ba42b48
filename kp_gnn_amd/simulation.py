"""The regular-graph simulation of the reference (run_simulation.py:96-178) on this project's parts: random R-regular graphs
(batch.regular_graphs from networkx, or ops.random_regular_graphs on the device), the K-hop pre-transform on the device
(ops.khop_transform), one mask-only K-hop GIN layer in eval mode (layers.KGINConv) and the collision rate of its node or graph embeddings (ops.collision_count).  The embeddings stay on the
device from the forward to the count; what comes back to the host is two integers per (n, k)."""
import time

import torch

from . import _lib, ops
from .batch import regular_graphs

_EDGE_BUDGET = 1 << 24      # K-hop edges of one forward chunk: [E,k] int64 edge_attr of 128 MiB per hop


def compute_simulation_collisions(outputs, ratio=True):
    """run_simulation.py:165-178 with the [N, D, N] tensor replaced by ops.collision_count: the number of colliding pairs
    int((2 * upper + diag - N) / 2) - the reference's own expression on its count (diff < 1e-10).sum() = 2 * upper + diag, so
    rows with a NaN or Inf (which do not even collide with themselves) give its arithmetic exactly - or, with ratio, that
    number over N (N - 1) / 2 (ZeroDivisionError for a single row, as there)."""
    epsilon = 1e-10
    N = outputs.size(0)
    upper, diag = ops.collision_count(outputs, epsilon)
    n_collision = int((2 * upper + diag - N) / 2)
    r = n_collision / (N * (N - 1) / 2)
    if ratio:
        return r
    return n_collision


def _chunk_graphs(n, R, k, N):
    """Graphs per forward chunk so that the K-hop edge tensors stay within _EDGE_BUDGET edges: a node of an R-regular graph
    reaches at most min(n - 1, R + R (R-1) + .. + R (R-1)^(k-1)) others within k hops."""
    reach, ring = 0, R
    for _ in range(k):
        reach += ring
        ring *= max(R - 1, 1)
        if reach >= n - 1:
            break
    per_graph = max(1, n * min(max(n - 1, 1), reach))
    return int(max(1, min(N, _EDGE_BUDGET // per_graph)))


class _Stage:
    """Adds the wall time of a block, fenced by device synchronises, to timings[name]; does nothing without a dict."""

    def __init__(self, timings, name, dev):
        self.t, self.name, self.dev = timings, name, dev

    def __enter__(self):
        if self.t is not None:
            torch.cuda.synchronize(self.dev)
            self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        if self.t is not None:
            torch.cuda.synchronize(self.dev)
            self.t[self.name] = self.t.get(self.name, 0.0) + time.perf_counter() - self.t0
        return False


def simulate(n_list, R=3, N=100, K=6, graph=False, hidden_size=16, seed=0, device=None, chunk_graphs=None,
             return_outputs=False, timings=None, generator="networkx"):
    """run_simulation.py:96-116: {(n, k): collision rate} for every n of n_list and k = 1 .. K.  Per n the N random R-regular
    graphs are generated once (seeds seed .. seed + N - 1, x = ones); per k they are pre-transformed with
    (k, 10, 1, 1, 1, 1, "spd") on the device (graphs of up to 2048 nodes by the kernels, larger ones by the host route of the
    same call), a fresh KGINConv(hidden_size, k, pool=graph) is built after torch.manual_seed(seed) and run in eval mode without
    gradients over chunks of `chunk_graphs` graphs (default: as many as keep a chunk's K-hop edges within 2^24), the outputs are
    concatenated on the device - node rows, or one pooled row per graph with graph=True - and counted there.
    return_outputs: (rates, {(n, k): the [rows, hidden_size] device tensor}).  timings: a dict that receives the seconds per
    stage (generate / pre_transform / forward / count), each fenced by device synchronises; None times nothing.
    generator: "networkx", the default, is the reference's generator on the host (batch.regular_graphs); "device" draws the
    graphs of each n with ops.random_regular_graphs(N, n, R, seed, route="device") - uniform random regular graphs from the
    pairing model, another draw than networkx's - and every chunk is a slice of its device edge list: no graph visits the host."""
    if generator not in ("networkx", "device"):
        raise ValueError(f"unknown generator {generator!r}: 'networkx' or 'device'")
    from .layers import KGINConv
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise _lib.KpgnnError("simulation.simulate runs the layer on the HIP kernels: it needs a device (no CPU fallback)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    results, kept = {}, {}
    for n in n_list:
        n = int(n)
        with _Stage(timings, "generate", dev):
            if generator == "device":
                node_ptr, edge_ptr, ei = ops.random_regular_graphs(N, n, R, seed, dev, first_graph=0, route="device")[:3]
            else:
                node_ptr, edge_ptr, ei = regular_graphs(N, seed, n=n, degree=R)
        for k in range(1, K + 1):
            torch.manual_seed(seed)
            model = KGINConv(hidden_size, k, pool=graph).to(dev).eval()
            step = int(chunk_graphs) if chunk_graphs else _chunk_graphs(n, R, k, N)
            outs = []
            with torch.no_grad():
                for g0 in range(0, N, step):
                    g1 = min(N, g0 + step)
                    e0, e1 = int(edge_ptr[g0]), int(edge_ptr[g1])
                    with _Stage(timings, "pre_transform", dev):
                        t, _ = ops.khop_transform(node_ptr[g0:g1 + 1] - node_ptr[g0], edge_ptr[g0:g1 + 1] - e0, ei[:, e0:e1], None,
                                                  k, 10, 1, 1, 1, 1, "spd", dev, large="device")
                    with _Stage(timings, "forward", dev):
                        x = torch.ones((int(node_ptr[g1] - node_ptr[g0]), 1), device=dev)
                        outs.append(model(x, t["edge_index"], t["edge_attr"], t["batch"]))
                    del t
                out = outs[0] if len(outs) == 1 else torch.cat(outs, 0)
            with _Stage(timings, "count", dev):
                results[(n, k)] = compute_simulation_collisions(out, ratio=True)
            if return_outputs:
                kept[(n, k)] = out
    return (results, kept) if return_outputs else results
