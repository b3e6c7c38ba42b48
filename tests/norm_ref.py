"""The bodies' Layer, Instance, GraphSize and Pair norms as plain torch in any dtype: what PyG's modules compute when they are
called without a batch vector (the whole batch is one graph), as the bodies call them (models/GNNs.py:191,430,656,680).  The
reference of tests/test_body_norm_cabi.py and tests/test_body_norm.py; nothing of kp_gnn_amd is imported here.

With x [N,C] and eps = 1e-5:
    Layer      xc = x - mean(all N*C);  y = xc / (std_biased(all N*C) + eps) * weight + bias   (eps joins the std)
    Instance   per column: y = (x - mean_n) / sqrt(var_biased_n + eps)                         (the same in eval(): no running stats)
    GraphSize  y = x / sqrt(N)
    Pair       xc = x - mean_n per column;  y = xc / sqrt(eps + mean_n(sum_c xc^2))            (scale 1)
"""
EPS = 1e-5
KINDS = ("Layer", "Instance", "GraphSize", "Pair")


def layer_norm(x, weight, bias, eps=EPS):
    xc = x - x.mean()
    return xc / (xc.std(unbiased=False) + eps) * weight + bias


def instance_norm(x, eps=EPS):
    return (x - x.mean(0, keepdim=True)) / (x.var(0, unbiased=False, keepdim=True) + eps).sqrt()


def graph_size_norm(x):
    return x / x.shape[0] ** 0.5


def pair_norm(x, eps=EPS):
    xc = x - x.mean(0, keepdim=True)
    return xc / (eps + xc.pow(2).sum(-1).mean()).sqrt()


def norm(kind, x, weight=None, bias=None, residual=None, eps=EPS):
    """norm_kind(x) (+ residual); weight / bias [C] are Layer's."""
    if kind == "Layer":
        y = layer_norm(x, weight, bias, eps)
    elif kind == "Instance":
        y = instance_norm(x, eps)
    elif kind == "GraphSize":
        y = graph_size_norm(x)
    elif kind == "Pair":
        y = pair_norm(x, eps)
    else:
        raise ValueError(kind)
    return y if residual is None else y + residual
