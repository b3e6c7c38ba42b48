"""The Layer, Instance, GraphSize and Pair norms PER GRAPH as plain torch in any dtype: tests/norm_ref.py applied to each row
block of a graph pointer on its own, which is what PyG's modules compute when they are handed a batch vector.  The reference
of tests/test_graph_norm_host.py, test_graph_norm_cabi.py and test_graph_norm.py; nothing of kp_gnn_amd is imported here.

Graph g owns the rows [ptr[g], min(ptr[g+1], live)), live = the row count unless given; a graph without rows is skipped, and
rows no graph owns come back as `fill`."""
import torch

import norm_ref as NR

EPS, KINDS = NR.EPS, NR.KINDS


def blocks(ptr, live=None):
    """[(g, r0, r1)] of the graphs that own at least one row."""
    ptr = [int(v) for v in ptr]
    live = ptr[-1] if live is None else int(live)
    out = []
    for g in range(len(ptr) - 1):
        r0, r1 = ptr[g], min(ptr[g + 1], live)
        if r1 > r0:
            out.append((g, r0, r1))
    return out


def norm(kind, x, ptr, weight=None, bias=None, residual=None, eps=EPS, live=None, fill=0.0):
    """norm_kind of every block of x [N,C] (+ residual), differentiable; rows outside every live block are `fill`."""
    parts, at = [], 0
    for _, r0, r1 in blocks(ptr, live):
        if r0 > at:
            parts.append(x.new_full((r0 - at, x.shape[1]), fill))
        parts.append(NR.norm(kind, x[r0:r1], weight, bias, None if residual is None else residual[r0:r1], eps))
        at = r1
    if at < x.shape[0]:
        parts.append(x.new_full((x.shape[0] - at, x.shape[1]), fill))
    return torch.cat(parts) if parts else x.new_full(x.shape, fill)


def batch_of(ptr, N=None):
    """The int64 batch vector of a pointer (rows beyond ptr[-1], up to N, repeat the last graph id, as a static batch pads)."""
    ptr = torch.as_tensor(ptr, dtype=torch.int64)
    G = ptr.numel() - 1
    b = torch.repeat_interleave(torch.arange(G), ptr[1:] - ptr[:-1])
    if N is not None and N > b.numel():
        b = torch.cat([b, torch.full((N - b.numel(),), G - 1, dtype=torch.int64)])
    return b
