"""Graph pointers around the places csrc/body_norm_graph.hip can go wrong, shared by the per-graph norm tests.  T is the row
count from which a block instead of a wavefront owns a graph; callers read it from the binding (_lib.GRAPH_NORM_BLOCK_ROWS)
and hand it in.  Nothing of kp_gnn_amd is imported here."""
import torch

WIDTHS = (1, 3, 33, 104, 256)


def sizes_around(T):
    return [0, 1, 2, 3, 31, 32, 33, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]


def ptr_of(sizes):
    p = [0]
    for n in sizes:
        p.append(p[-1] + int(n))
    return p


def cases(T):
    """{name: list of graph sizes}."""
    s = sizes_around(T)
    g = torch.Generator().manual_seed(11)
    shuffled = [s[i] for i in torch.randperm(len(s), generator=g).tolist()]
    return {
        "sizes": s,
        "shuffled": shuffled,
        "empty-first-middle-last": [0, 5, 37, 0, 0, T + 3, 9, 0],
        "one-graph": [T + 9],
        "one-small-graph": [23],
        "200-tiny": torch.randint(1, 5, (200,), generator=g).tolist(),
    }


def inputs(N, C, seed=0):
    """(x, gout, residual, weight, bias) on the CPU in fp32: N(0,1) plus a per-column offset of up to 3."""
    g = torch.Generator().manual_seed(7919 * seed + 1000 * N + C)
    off = 6 * torch.rand(C, generator=g) - 3
    x = torch.randn(N, C, generator=g) + off
    gout, res = torch.randn(N, C, generator=g), torch.randn(N, C, generator=g)
    return x, gout, res, 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
