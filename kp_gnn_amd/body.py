"""Caller side of the hot path: the GNN bodies and the graph-regression head that drive the K-hop layers.

The reference's models/GNNs.py (GNN :22-235, GNNPlus :238-474, GNNPrime :478-722), models/
GraphRegression.py:9-51 and the small encoders (layers/input_encoder.py:9-23, feature_encoder.py:37-67) are
the *callers* of the path this package accelerates; with PyG installed they run unchanged on top of
kp_gnn_amd.layers.  PyG is absent here and on the GPU box, so bench.py / smoke() / the body-level parity
tests need a caller of their own: this file.  It keeps the reference's constructor arguments and
state_dict key names (so reference checkpoints and the golden bodies load verbatim) but shares one base
class instead of three near-identical copies.  All five norm_type choices of the reference are built: "Batch" on the
BatchNorm kernels, "Layer", "Instance", "GraphSize" and "Pair" on ops.body_norm (PyG's modules as the bodies call them: without
a batch vector, the whole batch one graph).  One argument the reference does not have: norm_scope="graph" hands those four
the batch vector, so that every graph is normalised over its own rows; the default "batch" is the reference's behaviour.
"""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from .layers.gine import GINEConv
from .ops import (DictPeripheral, attention_pool, body_norm, dropout_add, embedding_rows, enc_tables, jk_lstm_applies, jk_lstm_score,
                  jk_native_applies, jk_reduce,
                  native_dropout_applies, rd_project, rd_project_applies, refuse_dynamic_rows, segment_max, segment_pool, table_gather_sum, virtual_node_add)
from .ops_dense import (JKConcatLinear, batch_norm_act, head_linear, jk_concat_linear_nograd, mlp_linear_bn_relu_x2,
                        prepare_mlp_splits, score_head)

MAX_DICT_ROWS = 128  # peripheral dictionaries up to this many distinct tuples use the dictionary kernels

_PIDX = "_kpgnn_packed_peripheral"


def _packed_peripheral_index(pea, pca, sizes):
    """[N,K,T,2] / [N,K,Hc] int64 -> ([N*K, C] uint16 rows, [C] int32 table offsets), cached on the source
    tensor.  Column order: (type_t, count_t) for t < T, then the Hc configuration columns; `sizes` lists
    the table heights in the order the tables are concatenated (type, count, conf_0..conf_Hc-1)."""
    anchor = pea if pea is not None else pca
    key = (None if pea is None else pea._version, None if pca is None else (id(pca), pca._version), tuple(sizes))
    rec = getattr(anchor, _PIDX, None)
    if rec is not None and rec[0] == key:
        return rec[1:]
    cols, table_of_col = [], []
    starts = [0]
    for n in sizes:
        starts.append(starts[-1] + n)
    ti = 0
    if pea is not None:
        N, K, T, two = pea.shape
        cols.append(pea.reshape(N * K, T * 2))
        table_of_col += [0, 1] * T
        ti = 2
    if pca is not None:
        N, K, Hc = pca.shape
        cols.append(pca.reshape(N * K, Hc))
        table_of_col += list(range(ti, ti + Hc))
    idx64 = torch.cat(cols, dim=1)
    limit = torch.tensor([sizes[t] for t in table_of_col], device=idx64.device)
    if idx64.numel() and bool(((idx64 < 0) | (idx64 >= limit)).any().item()):  # one sync per batch object
        raise IndexError("peripheral attribute index out of range for its embedding table")
    if max(sizes) > 65536:
        raise ValueError("peripheral embedding table too large for uint16 indices")
    idx = idx64.to(torch.int16) if max(sizes) <= 32768 else (idx64 - 65536 * (idx64 >= 32768)).to(torch.int16)
    col_offset = torch.tensor([starts[t] for t in table_of_col], dtype=torch.int32, device=idx64.device)
    idx = idx.contiguous()
    # dictionary encoding of the (node,hop) tuples (one sort per batch object)
    uidx = uid = None
    if idx64.numel():
        u64, inv = torch.unique(idx64, dim=0, return_inverse=True)
        if u64.shape[0] <= MAX_DICT_ROWS:
            uidx = (u64.to(torch.int16) if max(sizes) <= 32768 else (u64 - 65536 * (u64 >= 32768)).to(torch.int16)).contiguous()
            n_nodes = (pea if pea is not None else pca).shape[0]
            uid = inv.to(torch.int32).view(n_nodes, -1).contiguous()
            # the most frequent row of every hop (one id covers 82-99.9 % of a molecule batch's nodes per hop): the
            # dictionary-gradient kernel takes that id's sum as total minus the rest (ops.dict_grad_raw, kpgnn_dict_grad)
            uid._kp_dom = torch.mode(uid, dim=0).values.to(torch.int32).contiguous()
    rec = (key, idx, col_offset, uidx, uid)
    try:
        setattr(anchor, _PIDX, rec)
    except Exception:  # pragma: no cover
        pass
    return rec[1:]


_COL_OFFSETS = {}


def _dataset_peripheral_index(pd, use_e, use_c, sizes):
    """The same four values as _packed_peripheral_index for a batch collated from a resident dataset: the dictionary rows
    are the DATASET's distinct tuples (static), the batch carries int32 ids into them; the range check runs on the host
    against the dataset-wide column maxima (no device round trip, nothing per batch but the ids themselves)."""
    T, Hc = pd.pdict.T, pd.pdict.Hc
    rows, col_max = pd.pdict.select(use_e, use_c)
    table_of_col = ([0, 1] * T if use_e else []) + list(range(2 if use_e else 0, (2 if use_e else 0) + (Hc if use_c else 0)))
    for c, t in enumerate(table_of_col):
        if col_max[c] >= sizes[t]:
            raise IndexError("peripheral attribute index out of range for its embedding table")
    key = (tuple(sizes), tuple(table_of_col), rows.device)
    col_offset = _COL_OFFSETS.get(key)
    if col_offset is None:
        starts = [0]
        for n in sizes:
            starts.append(starts[-1] + n)
        col_offset = _COL_OFFSETS[key] = torch.tensor([starts[t] for t in table_of_col], dtype=torch.int32, device=rows.device)
    if rows.shape[0] <= MAX_DICT_ROWS:
        return None, col_offset, rows, pd.uid
    return rows[pd.uid.reshape(-1).long()].contiguous(), col_offset, None, None     # (dense rows: a dictionary too large for LDS)


# ------------------------------------------------------------------------------------------------ small pieces
def _get(data, name):
    try:
        v = getattr(data, name)
    except AttributeError:
        return None
    return v


def global_add_pool(x, batch, size=None):
    size = int(batch[-1].item()) + 1 if size is None else size
    if x.is_cuda and x.dim() == 2 and x.dtype == torch.float32:
        return segment_pool(x, batch, size)          # segmented sum in node order: one launch, bitwise reproducible
    return x.new_zeros((size,) + tuple(x.shape[1:])).index_add_(0, batch, x)


class EmbeddingEncoder(nn.Module):
    """layers/input_encoder.py:9-23."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.init_proj = nn.Embedding(input_size, hidden_size)

    def reset_parameters(self):
        self.init_proj.reset_parameters()

    def forward(self, data):
        if data.x.is_cuda:   # (host-sync-free backward: hipGraph-capturable, unlike nn.Embedding's)
            return embedding_rows(self.init_proj.weight, data.x)
        return self.init_proj(data.x)


class QM9InputEncoder(nn.Module):
    """layers/input_encoder.py:43-84: Linear over cat(Embedding(z), continuous features [, pos])."""

    def __init__(self, hidden_size, use_pos=False):
        super().__init__()
        self.use_pos = use_pos
        self.init_proj = nn.Linear(22 if use_pos else 19, hidden_size)
        self.z_embedding = nn.Embedding(1000, 8)

    def reset_parameters(self):
        self.init_proj.reset_parameters()
        self.z_embedding.reset_parameters()

    def forward(self, data):
        x, z = data.x, _get(data, "z")
        if z is not None:
            z_emb = embedding_rows(self.z_embedding.weight, z) if z.is_cuda else self.z_embedding(z)
            if z_emb.dim() == 3:
                z_emb = z_emb.sum(dim=1)
            x = torch.cat([z_emb, x], -1)
        pos = _get(data, "pos")
        if self.use_pos and pos is not None:
            x = torch.cat([x, pos], 1)
        return self.init_proj(x)


class LinearEncoder(nn.Module):
    """layers/input_encoder.py:26-40."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.init_proj = nn.Linear(input_size, hidden_size)

    def reset_parameters(self):
        self.init_proj.reset_parameters()

    def forward(self, data):
        return self.init_proj(data.x)


class FeatureConcatEncoder(nn.Module):
    """Per-column embedding -> concat -> Linear (layers/feature_encoder.py:37-67)."""

    def __init__(self, feature_dims, hidden_size, padding=False):
        super().__init__()
        self.embedding_list = nn.ModuleList(
            nn.Embedding(d, hidden_size, padding_idx=0) if padding else nn.Embedding(d, hidden_size)
            for d in feature_dims)
        self.proj = nn.Linear(len(feature_dims) * hidden_size, hidden_size)

    def reset_parameters(self):
        for e in self.embedding_list:
            e.reset_parameters()
        self.proj.reset_parameters()

    def forward(self, x):
        if x.is_cuda:
            cols = [embedding_rows(emb.weight, x[..., i].contiguous(), padding_idx=emb.padding_idx)
                    for i, emb in enumerate(self.embedding_list)]
        else:
            cols = [emb(x[..., i]) for i, emb in enumerate(self.embedding_list)]
        return self.proj(torch.cat(cols, dim=-1))


_component_masks = {}


def _projected_tables(enc, gate):
    """gate * (Emb_c.weight @ proj.weight[:, c*W:(c+1)*W]^T) for every component c of a FeatureConcatEncoder, stacked
    row-wise: [sum_c n_c, out].  One block-structured GEMM instead of one small GEMM + scale per component: the stacked
    weights [R, W] are spread to [R, C*W] with a static one-hot mask (row r of component c only fills block c), which
    keeps the whole encoder at ~5 launches forward and ~7 backward (it was 2C + 3 and ~10C: 0.65 ms of tiny launches
    per training step with the reference's nine components)."""
    embs = list(enc.embedding_list)
    C, W = len(embs), embs[0].embedding_dim
    if C == 1:
        return gate * F.linear(embs[0].weight, enc.proj.weight)
    sizes = tuple(e.num_embeddings for e in embs)
    dev = embs[0].weight.device
    key = (sizes, dev)
    mask = _component_masks.get(key)
    if mask is None:
        comp = torch.repeat_interleave(torch.arange(C, device=dev), torch.tensor(sizes, device=dev))
        mask = _component_masks[key] = F.one_hot(comp, C).to(torch.float32).unsqueeze(-1)      # [R, C, 1]
    e_all = torch.cat([e.weight for e in embs], dim=0)                                       # [R, W]
    x = (e_all.unsqueeze(1) * mask).reshape(e_all.shape[0], C * W)
    return gate * F.linear(x, enc.proj.weight)


class BatchNorm(nn.Module):
    """PyG's BatchNorm wrapper: parameters live under `.module` (state_dict key compatibility)."""

    def __init__(self, in_channels):
        super().__init__()
        self.module = nn.BatchNorm1d(in_channels)

    def reset_parameters(self):
        self.module.reset_parameters()

    def forward(self, x, residual=None, batch=None, num_graphs=None):
        # (batch / num_graphs: accepted as the other norms take them and ignored - BatchNorm's statistics are the batch's)
        return batch_norm_act(x, self.module, relu=False, residual=residual)


class LayerNorm(nn.Module):
    """PyG's LayerNorm(in_channels) (mode "graph", affine) called without a batch vector: mean and biased standard deviation
    over all N * C elements, eps added to the standard deviation.  state_dict keys weight / bias, as PyG's module yields."""

    def __init__(self, in_channels, eps=1e-5):
        super().__init__()
        self.in_channels, self.eps = in_channels, eps
        self.weight = nn.Parameter(torch.empty(in_channels))
        self.bias = nn.Parameter(torch.empty(in_channels))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.ones_(self.weight)
        nn.init.zeros_(self.bias)

    def forward(self, x, residual=None, batch=None, num_graphs=None):
        return body_norm(x, "Layer", self.weight, self.bias, residual=residual, eps=self.eps, batch=batch, num_graphs=num_graphs)


class InstanceNorm(nn.Module):
    """PyG's InstanceNorm(in_channels) (affine=False, track_running_stats=False) called without a batch vector: every column
    normalised over the N rows, the same in training and evaluation.  No parameters, no buffers."""

    def __init__(self, in_channels, eps=1e-5):
        super().__init__()
        self.in_channels, self.eps = in_channels, eps

    def reset_parameters(self):
        pass

    def forward(self, x, residual=None, batch=None, num_graphs=None):
        return body_norm(x, "Instance", residual=residual, eps=self.eps, batch=batch, num_graphs=num_graphs)


class GraphSizeNorm(nn.Module):
    """PyG's GraphSizeNorm() called without a batch vector: x / sqrt(N)."""

    def reset_parameters(self):
        pass

    def forward(self, x, residual=None, batch=None, num_graphs=None):
        return body_norm(x, "GraphSize", residual=residual, batch=batch, num_graphs=num_graphs)


class PairNorm(nn.Module):
    """PyG's PairNorm() (scale=1, scale_individually=False) called without a batch vector."""

    def __init__(self, eps=1e-5):
        super().__init__()
        self.eps = eps

    def reset_parameters(self):
        pass

    def forward(self, x, residual=None, batch=None, num_graphs=None):
        return body_norm(x, "Pair", residual=residual, eps=self.eps, batch=batch, num_graphs=num_graphs)


def _make_norm(norm_type, hidden_size):
    """One norm of models/GNNs.py:103-112."""
    if norm_type == "Batch":
        return BatchNorm(hidden_size)
    if norm_type == "Layer":
        return LayerNorm(hidden_size)
    if norm_type == "Instance":
        return InstanceNorm(hidden_size)
    if norm_type == "GraphSize":
        return GraphSizeNorm()
    if norm_type == "Pair":
        return PairNorm()
    raise ValueError("Not supported norm method")


def _vn_mlp(h):
    return nn.Sequential(nn.Linear(h, h), nn.BatchNorm1d(h), nn.ReLU(), nn.Linear(h, h), nn.BatchNorm1d(h), nn.ReLU())


def _reset(m):
    if hasattr(m, "reset_parameters"):
        m.reset_parameters()


# ------------------------------------------------------------------------------------------------ bodies
class _KHopBody(nn.Module):
    """Everything the three reference bodies have in common.  `width` is the per-hop width of the
    peripheral features (dk for GNN / GNNPrime, H for GNNPlus); `gate` their squashing (Q11)."""

    def __init__(self, num_layer, hidden_size, K, width, gate, init_emb, num_hop1_edge, max_edge_count, max_hop_num,
                 max_distance_count, JK, norm_type, virtual_node, residual, use_rd, wo_peripheral_edge,
                 wo_peripheral_configuration, drop_prob, norm_scope="batch"):
        super().__init__()
        if norm_scope not in ("batch", "graph"):
            raise ValueError(f"norm_scope must be 'batch' or 'graph', got {norm_scope!r}")
        # "batch": the reference's behaviour - its bodies hand the norms no batch vector, so the collated batch is one graph;
        # "graph": every graph on its own rows (ops.body_norm with a batch vector).  Not a parameter: state_dict does not hold it.
        self.norm_scope = norm_scope
        self.num_layer, self.hidden_size, self.K = num_layer, hidden_size, K
        self._periph_width, self._gate = width, gate
        self.dropout = nn.Dropout(drop_prob)
        self.JK, self.residual, self.use_rd, self.virtual_node = JK, residual, use_rd, virtual_node
        self.wo_peripheral_edge = wo_peripheral_edge
        self.wo_peripheral_configuration = wo_peripheral_configuration
        jk_in = (num_layer + 1) * hidden_size if JK == "concat" else hidden_size
        self.output_proj = nn.Sequential(nn.Linear(jk_in, hidden_size), nn.ReLU(), nn.Dropout(drop_prob))
        if JK == "attention":
            self.attention_lstm = nn.LSTM(hidden_size, num_layer, 1, batch_first=True, bidirectional=True, dropout=0.)
        self.init_proj = init_emb
        if use_rd:
            self.rd_projection = nn.Linear(1, hidden_size)
        if virtual_node:
            self.virtualnode_embedding = nn.Embedding(1, hidden_size)
            self.mlp_virtualnode_list = nn.ModuleList(_vn_mlp(hidden_size) for _ in range(num_layer - 1))
        if not wo_peripheral_edge:
            # the reference passes `padding=0` (GNNs.py:91), which is falsy: these tables have NO padding row
            self.peripheral_edge_embedding = FeatureConcatEncoder([num_hop1_edge + 2, max_edge_count + 1], width,
                                                                  padding=False)
            self.pew = nn.Parameter(torch.rand(1))
        if not wo_peripheral_configuration:
            self.peripheral_configuration_embedding = FeatureConcatEncoder(
                [max_distance_count + 1] * (max_hop_num + 1), width, padding=False)
            self.pcw = nn.Parameter(torch.rand(1))
        self.norms = nn.ModuleList(_make_norm(norm_type, hidden_size) for _ in range(num_layer))

    # -- parameter init shared by the three bodies (GNNs.py:122-140)
    def _reset_common(self):
        self.init_proj.reset_parameters()
        if self.JK == "attention":
            self.attention_lstm.reset_parameters()
        self.output_proj.apply(_reset)
        if self.use_rd:
            self.rd_projection.reset_parameters()
        if self.virtual_node:
            nn.init.constant_(self.virtualnode_embedding.weight.data, 0)
            self.mlp_virtualnode_list.apply(_reset)
        if not self.wo_peripheral_edge:
            self.peripheral_edge_embedding.reset_parameters()
            nn.init.normal_(self.pew)
        if not self.wo_peripheral_configuration:
            self.peripheral_configuration_embedding.reset_parameters()
            nn.init.normal_(self.pcw)

    # -- pieces of forward
    def _norm_kw(self, data, batch):
        """What every self.norms[l] call is handed besides its rows: nothing under norm_scope "batch", the batch vector and the
        graph count the heads resolve under "graph"."""
        if self.norm_scope != "graph":
            return {}
        if batch is None:
            raise ValueError("norm_scope='graph' needs data.batch")
        return {"batch": batch, "num_graphs": _num_graphs(batch, _get(data, "num_graphs"))}

    def _inputs(self, data):
        x = self.init_proj(data).squeeze()
        rd = _get(data, "rd")
        if self.use_rd and rd is not None:
            lin = self.rd_projection
            if rd_project_applies(x, rd, lin.weight, lin.bias):     # fp32 device rows, H <= 256: one native launch
                x = rd_project(x, rd, lin.weight, lin.bias)
            else:
                if x.is_cuda and x.dim() == 2:      # the framework Linear would sum its gradients over the dead rows too
                    refuse_dynamic_rows("the framework rd_projection", x.shape[0])
                x = x + lin(rd).squeeze()
        return x

    def _peripheral(self, data, num_nodes, like):
        """Peripheral-subgraph features P [N,K,width] (GNNs.py:171-179 / :392-400 / :636-644).

        Linear(cat_c Emb_c[i_c]) == sum_c (Emb_c W_c^T)[i_c] + b, so P is ONE multi-table gather-sum over
        the projected (tiny) tables, gates and biases folded in (ops.table_gather_sum).  The int64 index
        tensors are packed to uint16 once per batch object."""
        pea, pca = _get(data, "peripheral_edge_attr"), _get(data, "peripheral_configuration_attr")
        pd = _get(data, "peripheral_dict")        # dataset.BatchPeripheral: dictionary ids collated from a resident dataset
        use_e = (not self.wo_peripheral_edge) and (pea is not None or pd is not None)
        use_c = (not self.wo_peripheral_configuration) and (pca is not None or pd is not None)
        if not (use_e or use_c):
            return like.new_zeros(num_nodes, self.K, self._periph_width)
        W = self._periph_width
        kind = 1 if self._gate is torch.tanh else (0 if self._gate is torch.sigmoid else -1)
        encs, sizes = [], []
        if use_e:
            enc = self.peripheral_edge_embedding
            encs.append((enc, self.pew, pea.shape[-2] if pea is not None else pd.pdict.T))
            sizes.extend(emb.num_embeddings for emb in enc.embedding_list)
        if use_c:
            enc = self.peripheral_configuration_embedding
            encs.append((enc, self.pcw, 1))
            sizes.extend(emb.num_embeddings for emb in enc.embedding_list)
        if like.is_cuda and like.dtype == torch.float32 and kind >= 0 and W <= 256 and \
                all(e.padding_idx is None for enc, _, _ in encs for e in enc.embedding_list):
            # one launch per direction for ALL projected tables, gates and biases (csrc/enc_tables.hip)
            table, bias = enc_tables(kind, [(enc.proj.weight, enc.proj.bias, gate, mult, [e.weight for e in enc.embedding_list])
                                            for enc, gate, mult in encs])
        else:
            tables, bias = [], 0
            for enc, gate, mult in encs:
                g = self._gate(gate)
                tables.append(_projected_tables(enc, g))
                bias = bias + g * mult * enc.proj.bias
            table = torch.cat(tables, dim=0)
        if pd is not None:
            idx, col_offset, uidx, uid = _dataset_peripheral_index(pd, use_e, use_c, sizes)
        else:
            idx, col_offset, uidx, uid = _packed_peripheral_index(pea if use_e else None, pca if use_c else None, sizes)
        if uidx is not None:
            # dictionary form: the distinct index tuples are few (25 for a 2048-molecule batch), so P is a
            # [U,W] table + a static int32 uid per (node,hop); the layers' kernels read / differentiate that
            ptab = table_gather_sum(table, bias, uidx, col_offset)
            # (every layer of the stack reads this table, one after the other: its gradient is collected in one buffer -
            #  ops.KHopAggregate, dict_cell)
            ptab._kp_shared_grad = True
            return DictPeripheral(ptab, uid)
        return table_gather_sum(table, bias, idx, col_offset).view(num_nodes, -1, W)

    def _vn_init(self, data, batch):
        """The virtual node's initial rows [G,H]: the one embedding row, expanded (row stride 0 - nothing is materialised, and
        the gradient of the embedding is the framework's sum over the expand).  The graph count comes from the batch when it
        carries one (no host sync: capturable), else from the one read-back `_num_graphs` does for the readouts."""
        G = _num_graphs(batch, _get(data, "num_graphs"))
        if batch.is_cuda and torch.is_grad_enabled() and self.training:
            # (their launches are over G rows: the bf16-split route starts at 4096 of them, with splits of their own)
            prepare_mlp_splits(list(self.mlp_virtualnode_list), G)
        return self.virtualnode_embedding.weight.expand(G, -1)

    def _vn_add(self, l, h, vn, batch):
        """(h + vn[batch], global_add_pool(h + vn[batch]) + vn): one launch on the device (ops.virtual_node_add); the pooled
        sum only for a layer that updates the virtual node."""
        return virtual_node_add(h, vn, batch, vn.size(0), l < self.num_layer - 1)

    def _drop(self, h, residual=None, module=None):
        """module(h) (+ residual), module = self.dropout unless given: one launch with counter-based masks where the native
        route applies (ops.dropout_add: fp32 device rows, training mode, 0 < p < 1), else the framework module and add."""
        module = self.dropout if module is None else module
        if native_dropout_applies(h, module.p, module.training):
            return dropout_add(h, module.p, True, residual)
        h = module(h)
        return h if residual is None else h + residual

    def _vn_update(self, l, vn, tmp):
        G = tmp.size(0)
        if tmp.is_cuda:
            # the MLP's launches are over G rows and static; a dynamic_rows capacity equal to G would hand them the live NODE count
            refuse_dynamic_rows("the virtual-node MLP over as many graphs as the batch has node rows", G)
        mlp = self.mlp_virtualnode_list[l]
        # (one graph in training mode: the framework modules, whose BatchNorm1d raises as it does in the reference)
        upd = mlp(tmp) if G == 1 and mlp[1].training else mlp_linear_bn_relu_x2(mlp, tmp)
        if self.residual and native_dropout_applies(upd, self.dropout.p, self.dropout.training):
            return self._drop(upd, vn)           # (the residual rides in the dropout launch)
        upd = self._drop(upd)
        return vn + upd if self.residual else upd

    def _jk(self, h_list):
        if self.JK == "concat" and h_list[0].is_cuda and h_list[0].dtype == torch.float32 and torch.is_grad_enabled():
            lin = self.output_proj[0]
            return self._drop(JKConcatLinear.apply(lin.weight, lin.bias, *h_list), module=self.output_proj[2])
        if self.JK == "concat" and h_list[0].is_cuda and h_list[0].dtype == torch.float32:
            # no grad (evaluation): the grouped-K kernel directly - no autograd node, nothing saved
            lin = self.output_proj[0]
            y = jk_concat_linear_nograd(lin.weight, lin.bias, h_list)
            if y is not None:
                return self._drop(y, module=self.output_proj[2])
        if self.JK == "concat":
            rep = torch.cat(h_list, dim=1)
        elif self.JK == "last":
            rep = h_list[-1]
        elif self.JK == "max":
            # (fp32 device states: one kpgnn_jk_reduce_fwd launch over the states in place, ops.jk_reduce; else the stack)
            rep = jk_reduce(h_list, "max") if jk_native_applies(h_list, "max") else torch.stack(h_list, dim=-1).max(dim=-1).values
        elif self.JK == "sum":
            rep = jk_reduce(h_list, "sum") if jk_native_applies(h_list, "sum") else torch.stack(h_list, dim=0).sum(dim=0)
        elif self.JK == "attention" and jk_lstm_applies(h_list, self.attention_lstm) and jk_native_applies(h_list, "softmax"):
            # scorer and weighted sum both read the states in place: no stack, no module call (ops.jk_lstm_score, ops.jk_reduce)
            score = jk_lstm_score(h_list, self.attention_lstm)
            rep = jk_reduce(h_list, "softmax", score)
        elif self.JK == "attention":
            # the scoring LSTM as a framework module on the stacked states (CPU tensors, hidden size > 16, the switch off)
            hs = torch.stack(h_list, dim=1)
            self.attention_lstm.flatten_parameters()
            score, _ = self.attention_lstm(hs)
            if jk_native_applies(h_list, "softmax"):
                rep = jk_reduce(h_list, "softmax", score.sum(-1))
            else:
                rep = (hs * torch.softmax(score.sum(-1), dim=1).unsqueeze(-1)).sum(1)
        else:
            raise NameError(f"JK={self.JK} is not implemented (as in the reference, Q14)")
        if native_dropout_applies(rep, self.output_proj[2].p, self.output_proj[2].training):
            return self._drop(self.output_proj[1](self.output_proj[0](rep)), module=self.output_proj[2])
        return self.output_proj(rep)


class GNN(_KHopBody):
    """Body for KPGCN / KPGIN layers (reference models/GNNs.py:22-235): one layer cloned num_layer times."""

    def __init__(self, num_layer, gnn_layer, init_emb, num_hop1_edge, max_edge_count, max_hop_num, max_distance_count,
                 JK="last", norm_type="batch", virtual_node=True, residual=False, use_rd=False,
                 wo_peripheral_edge=False, wo_peripheral_configuration=False, drop_prob=0.1, norm_scope="batch"):
        super().__init__(num_layer, gnn_layer.output_size, gnn_layer.K, gnn_layer.output_dk, torch.sigmoid, init_emb,
                         num_hop1_edge, max_edge_count, max_hop_num, max_distance_count, JK, norm_type, virtual_node,
                         residual, use_rd, wo_peripheral_edge, wo_peripheral_configuration, drop_prob, norm_scope)
        self.output_dk = gnn_layer.output_dk
        self.gnns = nn.ModuleList(copy.deepcopy(gnn_layer) for _ in range(num_layer))
        self.reset_parameters()

    def reset_parameters(self):
        self._reset_common()
        for g in self.gnns:
            g.reset_parameters()

    def forward(self, data):
        edge_index, edge_attr, batch = data.edge_index, data.edge_attr, _get(data, "batch")
        pe_attr = _get(data, "pe_attr")
        x = self._inputs(data)
        _prepare_splits(self.gnns, x)
        periph = self._peripheral(data, x.size(0), x)
        vn, vn_pool = (self._vn_init(data, batch), None) if self.virtual_node else (None, None)
        nkw = self._norm_kw(data, batch)
        h_list = [x]
        for l in range(self.num_layer):
            if self.virtual_node:
                h_list[l], vn_pool = self._vn_add(l, h_list[l], vn, batch)
            # norm (+ residual) in one pass whenever no dropout mask sits between them (as in GNNPlus below)
            fuse_res = self.residual and (self.dropout.p == 0.0 or not self.training or l == self.num_layer - 1)
            # (this layer is the LAST of the state's readers to run backward - the norm's residual branch and the
            #  jumping-knowledge projection come later in the forward - so a layer that supports it may collect the state's
            #  whole gradient in one buffer: ops.khop_aggregate(x_state=...))
            if h_list[l].is_cuda:
                h_list[l]._kp_last_reader = self.gnns[l]
            h = self.norms[l](self.gnns[l](h_list[l], edge_index, edge_attr, pe_attr, periph),
                              residual=h_list[l] if fuse_res else None, **nkw)
            res = h_list[l] if self.residual and not fuse_res else None
            if l != self.num_layer - 1:
                h = self._drop(h, res)           # (with a mask between norm and residual, the add rides in the dropout launch)
            elif res is not None:
                h = h + res
            h_list.append(h)
            if self.virtual_node and l < self.num_layer - 1:
                vn = self._vn_update(l, vn, vn_pool)
        return self._jk(h_list)


class GNNPlus(_KHopBody):
    """Body for KP-GIN+ (reference models/GNNs.py:238-474): layer l sees the last min(l+1,K) states as its
    hop slots and the first k columns of edge_attr / peripheral features (:410-429)."""

    def __init__(self, num_layer, gnn_layer, init_emb, num_hop1_edge, max_edge_count, max_hop_num, max_distance_count,
                 JK="last", norm_type="batch", virtual_node=True, residual=False, use_rd=False,
                 wo_peripheral_edge=False, wo_peripheral_configuration=False, drop_prob=0.1, norm_scope="batch"):
        hidden, K = gnn_layer[-1].output_size, gnn_layer[-1].K
        assert num_layer >= K
        super().__init__(num_layer, hidden, K, hidden, torch.tanh, init_emb, num_hop1_edge, max_edge_count, max_hop_num,
                         max_distance_count, JK, norm_type, virtual_node, residual, use_rd, wo_peripheral_edge,
                         wo_peripheral_configuration, drop_prob, norm_scope)
        self.gnns = nn.ModuleList(gnn_layer)
        for g in self.gnns:
            g._kp_emit_out_stats = True      # norms[l] follows every layer: its statistics come out of the layer's last kernel
        self.reset_parameters()

    def reset_parameters(self):
        self._reset_common()
        for g in self.gnns:
            g.reset_parameters()

    def forward(self, data):
        edge_index, edge_attr, batch = data.edge_index, data.edge_attr, _get(data, "batch")
        pe_attr = _get(data, "pe_attr")
        x = self._inputs(data)
        _prepare_splits(self.gnns, x)
        periph = self._peripheral(data, x.size(0), x)
        vn, vn_pool = (self._vn_init(data, batch), None) if self.virtual_node else (None, None)
        nkw = self._norm_kw(data, batch)
        h_list, last_h = [x], x
        for l in range(self.num_layer):
            if self.virtual_node:
                h_list[l], vn_pool = self._vn_add(l, h_list[l], vn, batch)
            k = min(l + 1, self.K)
            slots = [h_list[l - m] for m in range(k)]                  # slot m = state of layer l-m
            pek = pe_attr[:, :k - 1] if pe_attr is not None else None
            fuse_res = self.residual and (self.dropout.p == 0.0 or not self.training or l == self.num_layer - 1)
            res = last_h if fuse_res else None
            if hasattr(self.gnns[l], "forward_slots") and slots[0].is_cuda:
                # (history=True: slot m is the state of layer l-m, so the layers may pool their slot gradients per state;
                #  post_norm: norms[l] (+ residual) is applied by the layer's own last autograd node, see ops_dense.FusedMLP)
                norm = self.norms[l]
                post = (norm.module, res) if isinstance(norm, BatchNorm) else None
                h = self.gnns[l].forward_slots(slots, edge_index, edge_attr[:, :k], pek, periph[:, :k], history=True,
                                               post_norm=post)
                if post is None:
                    h = norm(h, residual=res, **nkw)
            else:
                h = self.gnns[l](torch.stack(slots, dim=1), edge_index, edge_attr[:, :k], pek, periph[:, :k])
                h = self.norms[l](h, residual=res, **nkw)   # norm (+ residual) in one pass
            res = last_h if self.residual and not fuse_res else None
            if l != self.num_layer - 1:
                h = self._drop(h, res)
            elif res is not None:
                h = h + res
            if self.residual:
                last_h = h
            h_list.append(h)
            if self.virtual_node and l < self.num_layer - 1:
                vn = self._vn_update(l, vn, vn_pool)
        return self._jk(h_list)


class GNNPrime(_KHopBody):
    """Body for KP-GIN' (reference models/GNNs.py:478-722): num_l1_layer K-hop layers, then GINE layers that
    walk the same K-hop edge list masked by its hop-1 column (:676-679)."""

    def __init__(self, num_layer, gnn_layer, init_emb, num_hop1_edge, max_edge_count, max_hop_num, max_distance_count,
                 num_l1_layer=1, JK="last", norm_type="batch", virtual_node=True, residual=False, use_rd=False,
                 wo_peripheral_edge=False, wo_peripheral_configuration=False, drop_prob=0.1, norm_scope="batch"):
        assert num_l1_layer > 0
        assert num_layer >= 2
        super().__init__(num_layer, gnn_layer.output_size, gnn_layer.K, gnn_layer.output_dk, torch.sigmoid, init_emb,
                         num_hop1_edge, max_edge_count, max_hop_num, max_distance_count, JK, norm_type, virtual_node,
                         residual, use_rd, wo_peripheral_edge, wo_peripheral_configuration, drop_prob, norm_scope)
        self.output_dk = gnn_layer.output_dk
        self.num_l1_layer, self.num_l2_layer = num_l1_layer, num_layer - num_l1_layer
        self.khop_gnns = nn.ModuleList(copy.deepcopy(gnn_layer) for _ in range(num_l1_layer))
        gine = GINEConv(self.hidden_size, self.hidden_size, num_hop1_edge=num_hop1_edge)
        self.gins = nn.ModuleList(copy.deepcopy(gine) for _ in range(self.num_l2_layer))
        for g in self.gins:
            g._kp_emit_out_stats = True
        self.reset_parameters()

    def reset_parameters(self):
        self._reset_common()
        for g in list(self.khop_gnns) + list(self.gins):
            g.reset_parameters()

    def forward(self, data):
        edge_index, edge_attr, batch = data.edge_index, data.edge_attr, _get(data, "batch")
        pe_attr = _get(data, "pe_attr")
        x = self._inputs(data)
        _prepare_splits(list(self.khop_gnns) + list(self.gins), x)
        periph = self._peripheral(data, x.size(0), x)
        vn, vn_pool = (self._vn_init(data, batch), None) if self.virtual_node else (None, None)
        nkw = self._norm_kw(data, batch)
        h_list = [x]
        for l in range(self.num_layer):
            if self.virtual_node:
                h_list[l], vn_pool = self._vn_add(l, h_list[l], vn, batch)
            layer = self.khop_gnns[l] if l < self.num_l1_layer else self.gins[l - self.num_l1_layer]
            if h_list[l].is_cuda:
                h_list[l]._kp_last_reader = layer       # (as in GNN.forward: the norm's residual and the JK projection come later)
            if l < self.num_l1_layer:
                h = layer(h_list[l], edge_index, edge_attr, pe_attr, periph)
            else:
                h = layer(h_list[l], edge_index, edge_attr[:, :1])
            drops = l < self.num_l1_layer or l != self.num_layer - 1   # (:659 drops out after every K-hop layer)
            fuse_res = self.residual and (self.dropout.p == 0.0 or not self.training or not drops)
            h = self.norms[l](h, residual=h_list[l] if fuse_res else None, **nkw)
            res = h_list[l] if self.residual and not fuse_res else None
            if drops:
                h = self._drop(h, res)
            elif res is not None:
                h = h + res
            h_list.append(h)
            if self.virtual_node and l < self.num_layer - 1:
                vn = self._vn_update(l, vn, vn_pool)
        return self._jk(h_list)


def make_GNN(args):
    """models/model_utils.py:8-14."""
    return {"KPGINPlus": GNNPlus, "KPGINPrime": GNNPrime}.get(args.model_name, GNN)


def _prepare_splits(layers, x):
    """The split copies of every layer MLP's weights for the bf16-split Linear kernels, one launch per forward
    (ops_dense.prepare_mlp_splits); training mode on the device only - the fused MLP path is the only taker."""
    if x.is_cuda and torch.is_grad_enabled():
        mlps = [g.mlp for g in layers if g.training and isinstance(getattr(g, "mlp", None), nn.Sequential) and len(g.mlp) >= 5
                and isinstance(g.mlp[0], nn.Linear) and isinstance(g.mlp[3], nn.Linear)]
        if mlps:
            prepare_mlp_splits(mlps, x.size(0))


# ------------------------------------------------------------------------------------------------ readouts and task heads
def _num_graphs(batch, size):
    return int(batch[-1].item()) + 1 if size is None else size


def global_mean_pool(x, batch, size=None):
    size = _num_graphs(batch, size)
    if x.is_cuda and x.dim() == 2 and x.dtype == torch.float32:
        return segment_pool(x, batch, size, mean=True)
    cnt = x.new_zeros(size).index_add_(0, batch, x.new_ones(batch.numel()))
    return global_add_pool(x, batch, size) / cnt.clamp(min=1).unsqueeze(-1)


def global_max_pool(x, batch, size=None):
    """PyG 2.1.0's global_max_pool.  2-D fp32 device tensors run ops.segment_max: one winner per (graph, column), the lowest
    row of a tie, takes the whole gradient, as torch_scatter.scatter_max gives it.  Everything else keeps the framework's
    scatter, whose backward splits a tied column's gradient evenly - and which cannot tell the dead rows of a
    capacity-shaped batch from live ones, so on the device it refuses them."""
    size = _num_graphs(batch, size)
    if x.is_cuda and x.dim() == 2 and x.dtype == torch.float32:
        return segment_max(x, batch, size)
    if x.is_cuda:
        refuse_dynamic_rows("max readout on the framework path", x.shape[0])
    idx = batch.view(-1, 1).expand_as(x)
    return x.new_full((size, x.size(1)), float("-inf")).scatter_reduce(0, idx, x, reduce="amax")


class AttentionalAggregation(nn.Module):
    """PyG's AttentionalAggregation(gate_nn=nn.Linear(hidden, 1)) as the reference heads build it
    (models/GraphClassification.py:31-32): out[g] = sum_n softmax_g(gate_nn(x))[n] x[n].  state_dict keys gate_nn.weight /
    gate_nn.bias, as PyG's module yields; the arithmetic is ops.attention_pool (one HIP launch forward)."""

    def __init__(self, gate_nn):
        super().__init__()
        self.gate_nn = gate_nn
        self.reset_parameters()

    def reset_parameters(self):
        self.gate_nn.reset_parameters()

    def forward(self, x, batch, size=None):
        return attention_pool(x, batch, _num_graphs(batch, size), self.gate_nn)


def make_pool(pooling_method, hidden_size):
    """self.pool of the two graph-level heads (models/GraphRegression.py / GraphClassification.py:24-34): a function for
    sum / mean / max, a module with parameters for attention.  Called as pool(x, batch, num_graphs)."""
    if pooling_method == "sum":
        return global_add_pool
    if pooling_method == "mean":
        return global_mean_pool
    if pooling_method == "max":
        return global_max_pool
    if pooling_method == "attention":
        return AttentionalAggregation(gate_nn=nn.Linear(hidden_size, 1))
    raise ValueError("The pooling method not implemented")


class GraphRegression(nn.Module):
    """Pool + Linear head (reference models/GraphRegression.py:9-51); sum / mean / max / attention pooling."""

    def __init__(self, embedding_model, pooling_method):
        super().__init__()
        self.embedding_model = embedding_model
        self.JK, self.num_layer = embedding_model.JK, embedding_model.num_layer
        self.pooling_method = pooling_method
        self.pool = make_pool(pooling_method, embedding_model.hidden_size)
        self.regressor = nn.Linear(embedding_model.hidden_size, 1)
        self.reset_parameters()

    def reset_parameters(self):
        self.embedding_model.reset_parameters()
        self.regressor.reset_parameters()
        if self.pooling_method == "attention":
            self.pool.reset_parameters()

    def forward(self, data):
        x = self.embedding_model(data)
        return score_head(self.pool(x, data.batch, _get(data, "num_graphs")), self.regressor).squeeze()


class GraphClassification(nn.Module):
    """Pool + Linear classifier (reference models/GraphClassification.py:9-52): logits [num_graphs, output_size]."""

    def __init__(self, embedding_model, pooling_method, output_size):
        super().__init__()
        self.embedding_model = embedding_model
        hidden_size = embedding_model.hidden_size
        self.JK, self.num_layer = embedding_model.JK, embedding_model.num_layer
        self.pooling_method = pooling_method
        self.pool = make_pool(pooling_method, hidden_size)
        self.classifier = nn.Linear(hidden_size, output_size)
        self.reset_parameters()

    def reset_parameters(self):
        self.embedding_model.reset_parameters()
        self.classifier.reset_parameters()
        if self.pooling_method == "attention":
            self.pool.reset_parameters()

    def forward(self, data):
        x = self.embedding_model(data)
        return head_linear(self.pool(x, data.batch, _get(data, "num_graphs")), self.classifier)


class NodeClassification(nn.Module):
    """Linear classifier on the node rows (reference models/NodeClassification.py:7-35): logits [num_nodes, output_size]."""

    def __init__(self, embedding_model, output_size):
        super().__init__()
        self.embedding_model = embedding_model
        hidden_size = embedding_model.hidden_size
        self.JK, self.num_layer = embedding_model.JK, embedding_model.num_layer
        # (the reference sizes the classifier for hidden_size * (num_layer + 1) inputs under JK == "concat", although its
        #  bodies project the concatenation back to hidden_size: kept as it is so that checkpoints load)
        width = hidden_size * (self.num_layer + 1) if self.JK == "concat" else hidden_size
        self.classifier = nn.Linear(width, output_size)
        self.reset_parameters()

    def reset_parameters(self):
        self.embedding_model.reset_parameters()
        self.classifier.reset_parameters()

    def forward(self, data):
        return head_linear(self.embedding_model(data), self.classifier)


class NodeRegression(nn.Module):
    """Linear(hidden, 1) on the node rows (reference models/NodeRegression.py:7-29): one score per node."""

    def __init__(self, embedding_model):
        super().__init__()
        self.embedding_model = embedding_model
        self.JK, self.num_layer = embedding_model.JK, embedding_model.num_layer
        self.regressor = nn.Linear(embedding_model.hidden_size, 1)
        self.reset_parameters()

    def reset_parameters(self):
        self.embedding_model.reset_parameters()
        self.regressor.reset_parameters()

    def forward(self, data):
        return head_linear(self.embedding_model(data), self.regressor).squeeze()
