"""ctypes binding of libkpgnn_hip.so (include/kpgnn.h).  There is NO fallback: if the library is missing
or a call fails, an exception is raised - the product path never silently runs on the CPU."""
import ctypes
import os

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.path.join(_PKG, "libkpgnn_hip.so")

MODE_GIN, MODE_GINPLUS, MODE_GCN, MODE_SUM = 0, 1, 2, 3
ROUTE_SUBGROUP, ROUTE_NARROW, ROUTE_SMALL, ROUTE_LDS = 0, 1, 2, 3      # include/kpgnn.h KPGNN_AGG_ROUTE_*

c_i32, c_i64, c_f32p, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p


MATH_AUTO, MATH_F32 = 0, 1     # include/kpgnn.h KPGNN_MATH_*
ELIMIT = -3                    # include/kpgnn.h KPGNN_ELIMIT: the shape is not covered
DENSE_MATH = MATH_AUTO          # what new dense descriptors ask for (ops_dense.set_dense_math)


class KpgnnError(RuntimeError):
    pass


class AggFwdDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i32), ("K", c_i32), ("D", c_i32), ("K_csr", c_i32), ("mode", c_i32),
        ("n_code0", c_i32), ("n_codek", c_i32), ("use_tables", c_i32),
        ("rowptr", c_vp), ("col", c_vp), ("code", c_vp), ("dis", c_vp),
        ("x", c_vp), ("x_sn", c_i64), ("x_sk", c_i64),
        ("table0", c_vp), ("tablek", c_vp),
        ("periph", c_vp), ("p_sn", c_i64), ("p_sk", c_i64),
        ("eps", c_vp),
        ("out", c_vp), ("o_sn", c_i64), ("o_sk", c_i64),
        ("pre", c_vp), ("theta", c_vp), ("hout", c_vp), ("xbias", c_vp),
        ("ptab", c_vp), ("uid", c_vp), ("uid_stride", c_i64),
        ("x_slot", c_vp * 16), ("n_dict", c_i32), ("alphas", c_vp), ("storage", c_i32),
        ("n_dyn", c_vp),
        ("graph_ptr", c_vp), ("num_graphs", c_i32), ("max_graph_nodes", c_i32), ("hinit", c_vp), ("hinit2", c_vp),
    ]


class PullGatherDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i32), ("K", c_i32), ("D", c_i32), ("K_csr", c_i32),
        ("n_dyn", c_vp), ("rowptr", c_vp), ("col", c_vp),
        ("slab", c_vp * 16), ("slab_sn", c_i64),
        ("hinit", c_vp), ("hinit2", c_vp), ("hout", c_vp),
    ]


class AggBwdDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i32), ("K", c_i32), ("D", c_i32), ("K_csr", c_i32), ("mode", c_i32),
        ("n_code0", c_i32), ("n_codek", c_i32), ("use_tables", c_i32),
        ("rowptr_src", c_vp), ("col_src", c_vp), ("code_src", c_vp), ("dis", c_vp),
        ("g", c_vp), ("g_sn", c_i64), ("g_sk", c_i64),
        ("eps", c_vp),
        ("gx", c_vp), ("gx_sn", c_i64), ("gx_sk", c_i64),
        ("gtable0", c_vp), ("gtablek", c_vp),
        ("gx_slot", c_vp * 16), ("accumulate_mask", ctypes.c_uint32), ("storage", c_i32),
        ("n_dyn", c_vp),
    ]


class TableGradDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i32), ("K", c_i32), ("D", c_i32), ("nodes_per_tile", c_i32), ("n_code0", c_i32), ("n_codek", c_i32),
        ("n_dict", c_i32), ("dict_src", c_i32),
        ("tile_ptr", c_vp), ("tile_pack", c_vp),
        ("g", c_vp), ("g_sn", c_i64), ("g_sk", c_i64),
        ("uid", c_vp), ("uid_stride", c_i64), ("theta", c_vp), ("gh", c_vp),
        ("gtable0", c_vp), ("gtablek", c_vp), ("gdict", c_vp),
        ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t),
        ("kernel", c_i32),
        ("dict_pack", c_vp), ("dict_pack_K", c_i32),
        ("extra_slab", c_vp), ("extra_nslab", c_i32), ("extra_elems", c_i64), ("extra_out", c_vp), ("storage", c_i32),
        ("fuse_pre", c_vp), ("fuse_ptab", c_vp), ("fuse_uid", c_vp), ("fuse_uid_stride", c_i64), ("fuse_n_dict", c_i32),
        ("fuse_g", c_vp), ("fuse_gtheta", c_vp), ("fuse_alphas", c_vp), ("fuse_galphas", c_vp),
        ("fuse_workspace", c_vp), ("fuse_workspace_bytes", ctypes.c_size_t), ("accumulate_dict", c_i32),
        ("pending", c_vp),
        ("n_dyn", c_vp),
        ("max_multiplicity", c_i32),
    ]


class DictGradDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i32), ("K", c_i32), ("D", c_i32), ("n_dict", c_i32),
        ("uid", c_vp), ("uid_stride", c_i64), ("theta", c_vp), ("gh", c_vp), ("gdict", c_vp),
        ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t), ("defer_reduce", c_i32), ("dominant", c_vp),
        ("n_dyn", c_vp),
    ]


class DictGradMultiDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i32), ("D", c_i32), ("n_dict", c_i32), ("L", c_i32),
        ("uid", c_vp), ("uid_stride", c_i64),
        ("theta", c_vp * 16), ("gh", c_vp * 16), ("K", c_i32 * 16),
        ("gdict", c_vp), ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t), ("dominant", c_vp), ("n_dyn", c_vp),
    ]


class CombineBwdDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i32), ("K", c_i32), ("D", c_i32), ("mode", c_i32),
        ("pre", c_vp), ("gh", c_vp), ("theta", c_vp),
        ("gout", c_vp), ("go_sn", c_i64), ("go_sk", c_i64),
        ("periph", c_vp), ("p_sn", c_i64), ("p_sk", c_i64),
        ("ptab", c_vp), ("uid", c_vp), ("uid_stride", c_i64),
        ("g", c_vp), ("gv", c_vp), ("gtheta", c_vp),
        ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t), ("n_dict", c_i32),
        ("alphas", c_vp), ("galphas", c_vp), ("storage", c_i32),
    ]


class BnDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("C", c_i32), ("relu", c_i32), ("eps", ctypes.c_float), ("momentum", ctypes.c_float),
        ("x", c_vp), ("x_stride", c_i64), ("gamma", c_vp), ("beta", c_vp),
        ("running_mean", c_vp), ("running_var", c_vp), ("mean", c_vp), ("invstd", c_vp),
        ("z", c_vp), ("z_stride", c_i64), ("residual", c_vp), ("r_stride", c_i64),
        ("stat_slot", c_vp), ("stats_ready", c_i32), ("out_slot", c_vp), ("num_batches_tracked", c_vp),
        ("outer_gamma", c_vp), ("outer_beta", c_vp), ("outer_eps", ctypes.c_float), ("outer_momentum", ctypes.c_float),
        ("outer_running_mean", c_vp), ("outer_running_var", c_vp), ("outer_num_batches_tracked", c_vp),
        ("outer_mean", c_vp), ("outer_invstd", c_vp),
        ("n_dyn", c_vp),
    ]


class BnBwdDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("C", c_i32), ("relu", c_i32),
        ("x", c_vp), ("x_stride", c_i64), ("dz", c_vp), ("dz_stride", c_i64),
        ("gamma", c_vp), ("beta", c_vp), ("mean", c_vp), ("invstd", c_vp),
        ("dx", c_vp), ("dx_stride", c_i64), ("dgamma", c_vp), ("dbeta", c_vp),
        ("stat_slot", c_vp), ("reduce_only", c_i32), ("residual_grad", c_vp), ("rg_stride", c_i64),
        ("outer_mean", c_vp), ("outer_invstd", c_vp),
        ("n_dyn", c_vp),
    ]


class ReduceJob(ctypes.Structure):
    _fields_ = [("slab", c_vp), ("nslab", c_i32), ("elems", c_i64), ("out", c_vp * 4), ("n_out", c_i64 * 4)]


class WgradDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("O", c_i32), ("I", c_i32),
        ("dy", c_vp), ("dy_stride", c_i64), ("x", c_vp), ("x_stride", c_i64),
        ("dw", c_vp), ("db", c_vp), ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t),
        ("x_mean", c_vp), ("x_invstd", c_vp), ("x_gamma", c_vp), ("x_beta", c_vp), ("x_relu", c_i32),
        ("defer", c_vp), ("dy_mask", c_vp), ("n_dyn", c_vp), ("math", c_i32),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.math = DENSE_MATH


class LinearBnDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("O", c_i32), ("I", c_i32),
        ("x", c_vp), ("w", c_vp), ("bias", c_vp), ("y", c_vp),
        ("w_transposed", c_i32), ("pro", c_i32), ("epi", c_i32), ("pro_relu", c_i32),
        ("in_slot", c_vp), ("in_gamma", c_vp), ("in_beta", c_vp),
        ("in_eps", ctypes.c_float), ("momentum", ctypes.c_float),
        ("in_mean", c_vp), ("in_invstd", c_vp),
        ("running_mean", c_vp), ("running_var", c_vp), ("num_batches_tracked", c_vp),
        ("x2", c_vp), ("xt", c_vp), ("dgamma", c_vp), ("dbeta", c_vp),
        ("out_slot", c_vp),
        ("e_x", c_vp), ("e_mean", c_vp), ("e_invstd", c_vp), ("e_gamma", c_vp), ("e_beta", c_vp),
        ("o_mean", c_vp), ("o_invstd", c_vp), ("o_gamma", c_vp), ("o_dgamma", c_vp), ("o_dbeta", c_vp),
        ("n_dyn", c_vp), ("math", c_i32), ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t),
        ("w_split_ready", c_i32),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.math = DENSE_MATH


class SplitJob(ctypes.Structure):
    _fields_ = [("w", c_vp), ("wn", c_i64), ("wk", c_i64), ("O", c_i32), ("I", c_i32), ("frag", c_vp)]


class AttnDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i32), ("K", c_i32), ("D", c_i32),
        ("x", c_vp), ("x_sn", c_i64), ("x_sk", c_i64),
        ("gin", c_vp), ("whh", c_vp), ("acts", c_vp), ("hsum", c_vp), ("w", c_vp), ("out", c_vp),
        ("gout", c_vp), ("dx", c_vp), ("ds", c_vp), ("dgin", c_vp), ("hprev", c_vp),
    ]


class AttnScanDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i32), ("K", c_i32), ("D", c_i32),
        ("x", c_vp), ("x_sn", c_i64), ("x_sk", c_i64),
        ("w_ih", c_vp * 2), ("w_hh", c_vp * 2), ("b_ih", c_vp * 2), ("b_hh", c_vp * 2),
        ("acts", c_vp), ("hsum", c_vp), ("w", c_vp), ("out", c_vp), ("w_pad", c_vp),
        ("gout", c_vp), ("dx", c_vp), ("ds", c_vp), ("dgin", c_vp), ("whh_slab", c_vp), ("dwhh_pad", c_vp),
    ]


class LinearDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("O", c_i32), ("I", c_i32),
        ("x", c_vp), ("x_stride", c_i64), ("w", c_vp), ("bias", c_vp), ("y", c_vp), ("y_stride", c_i64),
        ("w_transposed", c_i32), ("y_block_cols", c_i32), ("y_block_stride", c_i64), ("x_mask", c_vp), ("n_dyn", c_vp),
        ("math", c_i32), ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.math = DENSE_MATH


class LinearGroupDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("O", c_i32), ("I", c_i32), ("group", c_i32),
        ("x", c_vp * 16), ("x_stride", c_i64), ("w", c_vp), ("bias", c_vp), ("y", c_vp), ("relu", c_i32), ("n_dyn", c_vp),
        ("math", c_i32), ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.math = DENSE_MATH


class BnRunning(ctypes.Structure):
    _fields_ = [("gamma", c_vp), ("beta", c_vp), ("running_mean", c_vp), ("running_var", c_vp), ("eps", ctypes.c_float)]


class MlpEvalDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("I", c_i32), ("O", c_i32),
        ("x", c_vp), ("x_stride", c_i64), ("w0", c_vp), ("b0", c_vp), ("w3", c_vp), ("b3", c_vp),
        ("bn1", BnRunning), ("bn2", BnRunning), ("outer", BnRunning),
        ("residual", c_vp), ("r_stride", c_i64), ("y", c_vp), ("y_stride", c_i64),
        ("n_dyn", c_vp), ("math", c_i32),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.math = DENSE_MATH


class BnEvalDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("C", c_i32), ("relu", c_i32),
        ("x", c_vp), ("x_stride", c_i64), ("bn", BnRunning),
        ("residual", c_vp), ("r_stride", c_i64), ("z", c_vp), ("z_stride", c_i64),
        ("n_dyn", c_vp),
    ]


class HopMlpDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("K", c_i32), ("DI", c_i32), ("DO", c_i32), ("H", c_i32),
        ("s", c_vp), ("w1", c_vp), ("b1", c_vp), ("w2", c_vp), ("b2", c_vp), ("theta", c_vp),
        ("wc", c_vp), ("bc", c_vp), ("h1", c_vp), ("h2", c_vp), ("out", c_vp), ("gout", c_vp), ("gs", c_vp), ("gflat", c_vp),
        ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t),
    ]


class SageTailDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("K", c_i32), ("DI", c_i32), ("DO", c_i32), ("H", c_i32),
        ("x", c_vp), ("xn", c_vp), ("w", c_vp), ("b", c_vp), ("theta", c_vp), ("wc", c_vp), ("bc", c_vp),
        ("y", c_vp), ("rinv", c_vp), ("out", c_vp), ("gout", c_vp), ("gx", c_vp), ("gxn", c_vp), ("gflat", c_vp),
        ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t),
    ]


class TgsDesc(ctypes.Structure):
    _fields_ = [
        ("M", c_i64), ("C", c_i32), ("D", c_i32), ("R", c_i32),
        ("idx", c_vp), ("col_offset", c_vp), ("table", c_vp), ("bias", c_vp),
        ("out", c_vp), ("out_stride", c_i64), ("gout", c_vp), ("gout_stride", c_i64), ("gtable", c_vp),
        ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t),
        ("n_dyn", c_vp),
    ]


class EncTablesDesc(ctypes.Structure):
    _fields_ = [
        ("H", c_i32), ("num_components", c_i32), ("num_encoders", c_i32),
        ("comp_emb", c_vp * 16), ("comp_rows", c_i32 * 16), ("comp_encoder", c_i32 * 16),
        ("enc_w", c_vp * 4), ("enc_b", c_vp * 4), ("enc_gate", c_vp * 4), ("enc_mult", ctypes.c_float * 4),
        ("enc_squash", c_i32 * 4),
        ("table", c_vp), ("pre", c_vp), ("bias", c_vp), ("gtable", c_vp), ("gbias", c_vp),
        ("comp_gemb", c_vp * 16), ("enc_gw", c_vp * 4), ("enc_gb", c_vp * 4), ("enc_ggate", c_vp * 4),
    ]


class PoolDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("G", c_i32), ("D", c_i32), ("mode", c_i32),
        ("graph_ptr", c_vp), ("batch", c_vp), ("x", c_vp), ("x_stride", c_i64), ("out", c_vp),
        ("gout", c_vp), ("gx", c_vp), ("gx_stride", c_i64),
        ("n_dyn", c_vp),
    ]


class PoolMaxDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("G", c_i32), ("D", c_i32),
        ("graph_ptr", c_vp), ("batch", c_vp), ("x", c_vp), ("x_stride", c_i64), ("out", c_vp), ("arg", c_vp),
        ("gout", c_vp), ("gx", c_vp), ("gx_stride", c_i64),
        ("n_dyn", c_vp),
    ]


class VnDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("G", c_i32), ("D", c_i32),
        ("graph_ptr", c_vp), ("x", c_vp), ("x_stride", c_i64), ("v", c_vp), ("v_stride", c_i64),
        ("out", c_vp), ("out_stride", c_i64), ("pooled", c_vp),
        ("n_dyn", c_vp),
    ]


class DropoutDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("C", c_i32),
        ("x", c_vp), ("x_stride", c_i64), ("out", c_vp), ("out_stride", c_i64), ("residual", c_vp), ("r_stride", c_i64),
        ("thr", ctypes.c_uint32), ("scale", ctypes.c_float),
        ("state", c_vp), ("call_io", c_vp), ("ticket", c_vp),
        ("n_dyn", c_vp),
    ]


class DropoutMaskDesc(ctypes.Structure):
    _fields_ = [("seed", c_i64), ("call", c_i64), ("N", c_i64), ("C", c_i32), ("thr", ctypes.c_uint32), ("mask", c_vp)]


JK_SUM, JK_MAX, JK_SOFTMAX = 0, 1, 2     # include/kpgnn.h KPGNN_JK_*
JK_MAX_STATES = 32


class JkDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("H", c_i32), ("S", c_i32), ("mode", c_i32),
        ("x", c_vp * JK_MAX_STATES), ("x_stride", c_i64), ("score", c_vp),
        ("out", c_vp), ("out_stride", c_i64), ("arg", c_vp), ("w", c_vp),
        ("gout", c_vp), ("gout_stride", c_i64), ("gx", c_vp), ("gscore", c_vp),
        ("n_dyn", c_vp),
    ]


class JkLstmDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("H", c_i32), ("P", c_i32), ("S", c_i32),
        ("x", c_vp * JK_MAX_STATES), ("x_stride", c_i64),
        ("w_ih", c_vp * 2), ("w_hh", c_vp * 2), ("b_ih", c_vp * 2), ("b_hh", c_vp * 2),
        ("score", c_vp), ("saved", c_vp),
        ("gscore", c_vp), ("gx", c_vp), ("dw_ih", c_vp * 2), ("dw_hh", c_vp * 2), ("db", c_vp * 2),
        ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t),
        ("n_dyn", c_vp),
    ]


JK_LSTM_MAX_P, JK_LSTM_MAX_H = 16, 256    # csrc/jk_lstm.hip kMaxP, kMaxH (S: JK_MAX_STATES)

NORM_LAYER, NORM_INSTANCE, NORM_GRAPHSIZE, NORM_PAIR = 0, 1, 2, 3     # include/kpgnn.h KPGNN_NORM_*
NORM_MAX_C = 256                                                      # csrc/body_norm.hip kMaxC


class NormDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("C", c_i32), ("kind", c_i32), ("eps", ctypes.c_float),
        ("x", c_vp), ("x_stride", c_i64), ("weight", c_vp), ("bias", c_vp), ("residual", c_vp), ("res_stride", c_i64),
        ("out", c_vp), ("out_stride", c_i64), ("saved", c_vp),
        ("gout", c_vp), ("gout_stride", c_i64), ("gx", c_vp), ("gx_stride", c_i64), ("gweight", c_vp), ("gbias", c_vp),
        ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t),
        ("n_dyn", c_vp),
    ]


GRAPH_NORM_BLOCK_ROWS = 128           # include/kpgnn.h KPGNN_GRAPH_NORM_BLOCK_ROWS: a block per graph from this many rows on


class GraphNormDesc(ctypes.Structure):
    _fields_ = NormDesc._fields_ + [("graph_ptr", c_vp), ("G", c_i32)]


RD_OK, RD_ASYMMETRIC, RD_TOO_LARGE, RD_PIVOT, RD_RANGE = 0, 1, 2, 3, 4    # include/kpgnn.h KPGNN_RD_*
RD_MAX_NODES, RD_WAVE_NODES = 128, 32                                   # KPGNN_RD_MAX_NODES, KPGNN_RD_WAVE_NODES
RD_PROJ_MAX_H = 256                                                     # csrc/rd_proj.hip kMaxH
RD_LARGE_MAX_NODES = 2048                                               # KPGNN_RD_LARGE_MAX_NODES (kpgnn_resistance_distance_large)


class RdDesc(ctypes.Structure):
    _fields_ = [
        ("G", c_i32), ("n_ids", c_i32), ("node_ptr", c_vp), ("edge_ptr", c_vp), ("edge_index", c_vp), ("E", c_i64),
        ("graph_ids", c_vp), ("max_nodes", c_i32), ("reserved", c_i32), ("out", c_vp), ("status", c_vp),
    ]


class RdLargeDesc(ctypes.Structure):
    _fields_ = RdDesc._fields_ + [("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t)]


class RdProjDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("H", c_i32), ("reserved", c_i32),
        ("x", c_vp), ("x_stride", c_i64), ("rd", c_vp), ("w", c_vp), ("b", c_vp), ("out", c_vp), ("out_stride", c_i64),
        ("dy", c_vp), ("dy_stride", c_i64), ("dw", c_vp), ("db", c_vp),
        ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t),
        ("n_dyn", c_vp),
    ]


KHOP_OK, KHOP_TOO_LARGE, KHOP_RANGE, KHOP_ENDPOINT, KHOP_TYPE, KHOP_SHAPE = 0, 1, 2, 3, 4, 5    # include/kpgnn.h KPGNN_KHOP_*
KHOP_MAX_NODES, KHOP_WAVE_NODES, KHOP_MAX_TYPE = 64, 32, 63             # KPGNN_KHOP_MAX_NODES, _WAVE_NODES, _MAX_TYPE
KHOP_MAX_K, KHOP_MAX_T, KHOP_MAX_H = 16, 8, 8                           # KPGNN_KHOP_MAX_K, _MAX_T, _MAX_H
KHOP_LARGE_MAX_NODES = 2048                                             # KPGNN_KHOP_LARGE_MAX_NODES (kpgnn_khop_large_*)


class KhopDevDesc(ctypes.Structure):
    _fields_ = [
        ("G", c_i32), ("n_ids", c_i32), ("graph_ids", c_vp), ("max_nodes", c_i32), ("reserved", c_i32), ("N", c_i64),
        ("node_ptr", c_vp), ("edge_ptr", c_vp), ("edge_index", c_vp), ("edge_attr", c_vp), ("E_in", c_i64),
        ("K", c_i32), ("max_edge_attr_num", c_i32), ("max_hop_num", c_i32), ("max_edge_type", c_i32),
        ("max_edge_count", c_i32), ("max_distance_count", c_i32), ("kernel", c_i32), ("reserved2", c_i32),
        ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t), ("status", c_vp),
        ("node_off", c_vp), ("E_out", c_i64), ("out_edge_index", c_vp), ("out_edge_attr", c_vp), ("out_pe_attr", c_vp),
        ("out_pea", c_vp), ("out_pca", c_vp), ("out_batch", c_vp),
    ]


class CollisionDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("D", c_i32), ("eps", ctypes.c_float),
        ("x", c_vp), ("x_stride", c_i64), ("out", c_vp), ("workspace", c_vp), ("workspace_bytes", c_i64),
    ]


COLLISION_MAX_D = 256                                                   # csrc/collisions.hip kMaxD

GL_OK, GL_ASYMMETRIC, GL_TOO_LARGE, GL_ENDPOINT, GL_SELF_LOOP, GL_SOURCE = 0, 1, 2, 3, 4, 5    # include/kpgnn.h KPGNN_GL_*
GL_MAX_NODES, GL_WAVE_NODES = 64, 32                                    # KPGNN_GL_MAX_NODES, KPGNN_GL_WAVE_NODES
GL_LARGE_MAX_NODES = 128                                                # KPGNN_GL_LARGE_MAX_NODES (kpgnn_graph_labels_large)


class GraphLabelsDesc(ctypes.Structure):
    _fields_ = [
        ("G", c_i32), ("n_ids", c_i32), ("node_ptr", c_vp), ("edge_ptr", c_vp), ("edge_index", c_vp), ("E", c_i64),
        ("graph_ids", c_vp), ("max_nodes", c_i32), ("reserved", c_i32), ("features", c_vp), ("source", c_vp),
        ("node_out", c_vp), ("graph_out", c_vp), ("status", c_vp),
    ]


CL_OK, CL_ASYMMETRIC, CL_SELF_LOOP, CL_TOO_LARGE, CL_ENDPOINT = 0, 1, 2, 3, 4    # include/kpgnn.h KPGNN_CL_*
CL_WAVE_NODES, CL_WORD_NODES, CL_MAX_NODES = 32, 64, 2048               # KPGNN_CL_WAVE_NODES, _WORD_NODES, _MAX_NODES


class CountLabelsDesc(ctypes.Structure):
    _fields_ = RdDesc._fields_ + [("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t)]     # (`out` is double [G,5] here)


RRG_OK, RRG_EXHAUSTED = 0, 1                                            # include/kpgnn.h KPGNN_RRG_*
RRG_MAX_DEGREE, RRG_MAX_NODES, RRG_MAX_STUBS, RRG_WAVE_STUBS = 4, 2048, 8192, 256    # KPGNN_RRG_MAX_DEGREE, _MAX_NODES, _MAX_STUBS, _WAVE_STUBS


class RrgDesc(ctypes.Structure):
    _fields_ = [
        ("G", c_i32), ("n", c_i32), ("d", c_i32), ("max_attempts", c_i32), ("seed", c_i64), ("first_graph", c_i64),
        ("edge_index", c_vp), ("attempts", c_vp), ("status", c_vp),
    ]


PG_OK, PG_EXHAUSTED = 0, 1                                              # include/kpgnn.h KPGNN_PG_*
PG_MIN_NODES, PG_MAX_NODES, PG_WAVE_NODES, PG_TREE_SWAPS = 2, 128, 64, 5000    # KPGNN_PG_MIN_NODES, _MAX_NODES, _WAVE_NODES, _TREE_SWAPS
PG_TYPES = {"RANDOM": 0, "ERDOS_RENYI": 1, "BARABASI_ALBERT": 2, "GRID": 3, "CAVEMAN": 5, "TREE": 6, "LADDER": 7, "LINE": 8,
            "STAR": 9, "CATERPILLAR": 10, "LOBSTER": 11}                # the reference's GraphType values
PG_STREAMS = {"TYPE": 0, "PARAM": 1, "PAIR": 2, "BA": 3, "TREE": 4, "ATTACH": 5, "SHUFFLE": 6, "FEATURE": 7, "SOURCE": 8}
PG_NO_SHUFFLE, PG_NO_RANDOMIZE = 1, 2                                   # KPGNN_PG_NO_SHUFFLE, _NO_RANDOMIZE (flags)


class PgDesc(ctypes.Structure):
    _fields_ = [
        ("G", c_i32), ("n_ids", c_i32), ("nodes", c_vp), ("node_ptr", c_vp), ("graph_ids", c_vp),
        ("max_nodes", c_i32), ("graph_type", c_i32), ("flags", c_i32), ("max_attempts", c_i32),
        ("force_block", c_i32), ("reserved", c_i32), ("seed", c_i64), ("first_graph", c_i64),
        ("rows", c_vp), ("features", c_vp), ("info", c_vp), ("edge_ptr", c_vp), ("edge_index", c_vp), ("E", c_i64),
    ]


class AttnPoolDesc(ctypes.Structure):
    _fields_ = [
        ("N", c_i64), ("G", c_i32), ("D", c_i32),
        ("graph_ptr", c_vp), ("x", c_vp), ("x_stride", c_i64), ("w", c_vp), ("bias", c_vp),
        ("alpha", c_vp), ("out", c_vp), ("gout", c_vp), ("gx", c_vp), ("gx_stride", c_i64), ("dw", c_vp), ("db", c_vp),
        ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t),
        ("n_dyn", c_vp),
    ]


class HeadLinearDesc(ctypes.Structure):
    _fields_ = [
        ("M", c_i64), ("O", c_i32), ("I", c_i32),
        ("x", c_vp), ("x_stride", c_i64), ("w", c_vp), ("bias", c_vp), ("y", c_vp), ("y_stride", c_i64),
        ("dy", c_vp), ("dy_stride", c_i64), ("dx", c_vp), ("dx_stride", c_i64), ("dw", c_vp), ("db", c_vp),
        ("workspace", c_vp), ("workspace_bytes", ctypes.c_size_t),
        ("n_dyn", c_vp),
    ]


class NllLossDesc(ctypes.Structure):
    _fields_ = [
        ("M", c_i64), ("C", c_i32), ("reduction", c_i32),
        ("logits", c_vp), ("logits_stride", c_i64), ("y", c_vp), ("loss", c_vp),
        ("dlogits", c_vp), ("dlogits_stride", c_i64), ("correct", c_vp),
        ("n_dyn", c_vp),
    ]


class DatasetView(ctypes.Structure):
    _fields_ = [
        ("K", c_i32), ("G", c_i32), ("node_ptr", c_vp), ("pair_ptr", c_vp), ("ent_ptr", c_vp),
        ("rowptr_dst", c_vp), ("rowptr_src", c_vp), ("col_dst", c_vp), ("col_src", c_vp),
        ("code_dst", c_vp), ("code_src", c_vp), ("ent_rel", c_vp), ("ent", c_vp),
    ]


class RowGather(ctypes.Structure):
    _fields_ = [("src", c_vp), ("dst", c_vp), ("row_bytes", c_i32)]


class CollateDesc(ctypes.Structure):
    _fields_ = [
        ("ds", DatasetView), ("B", c_i32), ("N", c_i32), ("A", c_i64), ("n_ent", c_i64), ("hdr", c_vp),
        ("rowptr_dst", c_vp), ("col_dst", c_vp), ("code_dst", c_vp),
        ("rowptr_src", c_vp), ("col_src", c_vp), ("code_src", c_vp),
        ("batch", c_vp), ("node_src", c_vp),
        ("nodes_per_tile", c_i32), ("tile_ptr", c_vp), ("tile_pack", c_vp), ("ent_node_ptr", c_vp),
        ("num_prefix", c_i32), ("prefix_ptr", c_vp), ("prefix_pack", c_vp), ("prefix_scratch", c_vp),
        ("n_node_rows", c_i32), ("node_rows", RowGather * 8),
        ("n_graph_rows", c_i32), ("graph_rows", RowGather * 8),
    ]


# name -> (restype, argtypes); every symbol include/kpgnn.h declares
SIGNATURES = {
    "kpgnn_abi_version": (ctypes.c_int, []),
    "kpgnn_last_error": (ctypes.c_char_p, []),
    "kpgnn_device_info": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 3 + [ctypes.c_char_p, ctypes.c_int]),
    "kpgnn_csr_stats": (ctypes.c_int, [c_vp, c_i64, c_vp, c_i64, c_i64, c_i32, c_vp, c_vp]),
    "kpgnn_csr_workspace_bytes": (ctypes.c_size_t, [c_i64, c_i64, c_i64, c_i32]),
    "kpgnn_csr_build": (ctypes.c_int, [c_vp, c_i64, c_vp, c_i64, c_i64, c_i32, c_i64, c_i64,
                                       c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp,
                                       c_vp, ctypes.c_size_t, c_vp]),
    "kpgnn_aggregate_fwd": (ctypes.c_int, [ctypes.POINTER(AggFwdDesc), c_vp]),
    "kpgnn_khop_pull_gather": (ctypes.c_int, [ctypes.POINTER(PullGatherDesc), c_vp]),
    "kpgnn_agg_lds_launch_count": (c_i64, []),
    "kpgnn_agg_launch_counts": (ctypes.c_int, [ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    "kpgnn_aggregate_bwd": (ctypes.c_int, [ctypes.POINTER(AggBwdDesc), c_vp]),
    "kpgnn_table_grad_workspace_bytes": (ctypes.c_size_t, [c_i32] * 7),
    "kpgnn_table_grad": (ctypes.c_int, [ctypes.POINTER(TableGradDesc), c_vp]),
    "kpgnn_table_grad_fuse_workspace_bytes": (ctypes.c_size_t, [c_i32, c_i32]),
    "kpgnn_dict_grad_workspace_bytes": (ctypes.c_size_t, [c_i32] * 4),
    "kpgnn_dict_grad": (ctypes.c_int, [ctypes.POINTER(DictGradDesc), c_vp]),
    "kpgnn_dict_grad_multi": (ctypes.c_int, [ctypes.POINTER(DictGradMultiDesc), c_vp]),
    "kpgnn_dict_grad_slabs": (c_i32, [c_i32]),
    "kpgnn_tile_pack_filter": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "kpgnn_tile_pack_prefixes": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i32, c_i64, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp]),
    "kpgnn_collate": (ctypes.c_int, [ctypes.POINTER(CollateDesc), c_vp]),
    "kpgnn_regression_loss": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "kpgnn_score_head_fwd": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_vp]),
    "kpgnn_score_head_bwd": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "kpgnn_adam_step": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_double, ctypes.c_double, c_vp]),
    "kpgnn_reduce_jobs": (ctypes.c_int, [c_vp, c_i32, c_vp]),
    "kpgnn_adam_step_device": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, ctypes.c_double, ctypes.c_double,
                                              ctypes.c_double, ctypes.c_double, ctypes.c_double, c_vp]),
    "kpgnn_multi_copy": (ctypes.c_int, [c_i32, c_vp, c_vp, c_vp, c_vp]),
    "kpgnn_dict_tile_pack": (ctypes.c_int, [c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "kpgnn_dict_tile_pack_dyn": (ctypes.c_int, [c_vp, c_i64, c_i32, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "kpgnn_combine_bwd_workspace_bytes": (ctypes.c_size_t, [c_i32] * 3),
    "kpgnn_combine_bwd": (ctypes.c_int, [ctypes.POINTER(CombineBwdDesc), c_vp]),
    "kpgnn_bn_fwd": (ctypes.c_int, [ctypes.POINTER(BnDesc), c_vp]),
    "kpgnn_bn_bwd": (ctypes.c_int, [ctypes.POINTER(BnBwdDesc), c_vp]),
    "kpgnn_wgrad_workspace_bytes": (ctypes.c_size_t, [c_i32, c_i32]),
    "kpgnn_linear_wgrad": (ctypes.c_int, [ctypes.POINTER(WgradDesc), c_vp]),
    "kpgnn_linear_wgrad_pair": (ctypes.c_int, [ctypes.POINTER(WgradDesc), ctypes.POINTER(WgradDesc), c_vp]),
    "kpgnn_linear_wgrad_many": (ctypes.c_int, [ctypes.POINTER(ctypes.POINTER(WgradDesc)), ctypes.POINTER(ctypes.POINTER(WgradDesc)),
                                               c_i32, c_vp]),
    "kpgnn_wgrad_group_workspace_bytes": (ctypes.c_size_t, [c_i32, c_i32, c_i32]),
    "kpgnn_linear_wgrad_group": (ctypes.c_int, [ctypes.POINTER(WgradDesc), c_vp, c_i32, c_vp]),
    "kpgnn_linear_bn": (ctypes.c_int, [ctypes.POINTER(LinearBnDesc), c_vp]),
    "kpgnn_mlp_eval": (ctypes.c_int, [ctypes.POINTER(MlpEvalDesc), c_vp]),
    "kpgnn_bn_eval": (ctypes.c_int, [ctypes.POINTER(BnEvalDesc), c_vp]),
    "kpgnn_enc_tables_fwd": (ctypes.c_int, [ctypes.POINTER(EncTablesDesc), c_vp]),
    "kpgnn_enc_tables_bwd": (ctypes.c_int, [ctypes.POINTER(EncTablesDesc), c_vp]),
    "kpgnn_segment_pool_fwd": (ctypes.c_int, [ctypes.POINTER(PoolDesc), c_vp]),
    "kpgnn_segment_pool_bwd": (ctypes.c_int, [ctypes.POINTER(PoolDesc), c_vp]),
    "kpgnn_segment_max_fwd": (ctypes.c_int, [ctypes.POINTER(PoolMaxDesc), c_vp]),
    "kpgnn_segment_max_bwd": (ctypes.c_int, [ctypes.POINTER(PoolMaxDesc), c_vp]),
    "kpgnn_resistance_distance": (ctypes.c_int, [ctypes.POINTER(RdDesc), c_vp]),
    "kpgnn_rd_large_workspace_bytes": (ctypes.c_size_t, [c_i32, c_i32]),
    "kpgnn_resistance_distance_large": (ctypes.c_int, [ctypes.POINTER(RdLargeDesc), c_vp]),
    "kpgnn_rd_proj_workspace_bytes": (ctypes.c_size_t, [c_i64, c_i32]),
    "kpgnn_rd_proj_fwd": (ctypes.c_int, [ctypes.POINTER(RdProjDesc), c_vp]),
    "kpgnn_rd_proj_bwd": (ctypes.c_int, [ctypes.POINTER(RdProjDesc), c_vp]),
    "kpgnn_khop_dev_workspace_bytes": (ctypes.c_size_t, [c_i64]),
    "kpgnn_khop_dev_count": (ctypes.c_int, [ctypes.POINTER(KhopDevDesc), c_vp]),
    "kpgnn_khop_dev_fill": (ctypes.c_int, [ctypes.POINTER(KhopDevDesc), c_vp]),
    "kpgnn_khop_large_workspace_bytes": (ctypes.c_size_t, [c_i64, c_i64, c_i32]),
    "kpgnn_khop_large_count": (ctypes.c_int, [ctypes.POINTER(KhopDevDesc), c_vp]),
    "kpgnn_khop_large_fill": (ctypes.c_int, [ctypes.POINTER(KhopDevDesc), c_vp]),
    "kpgnn_collision_workspace_bytes": (c_i64, [c_i64]),
    "kpgnn_collision_count": (ctypes.c_int, [ctypes.POINTER(CollisionDesc), c_vp]),
    "kpgnn_graph_labels": (ctypes.c_int, [ctypes.POINTER(GraphLabelsDesc), c_vp]),
    "kpgnn_graph_labels_large": (ctypes.c_int, [ctypes.POINTER(GraphLabelsDesc), c_vp]),
    "kpgnn_count_labels_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "kpgnn_count_labels": (ctypes.c_int, [ctypes.POINTER(CountLabelsDesc), c_vp]),
    "kpgnn_random_regular_graphs": (ctypes.c_int, [ctypes.POINTER(RrgDesc), c_vp]),
    "kpgnn_property_graphs_generate": (ctypes.c_int, [ctypes.POINTER(PgDesc), c_vp]),
    "kpgnn_property_graphs_fill": (ctypes.c_int, [ctypes.POINTER(PgDesc), c_vp]),
    "kpgnn_vn_add_pool": (ctypes.c_int, [ctypes.POINTER(VnDesc), c_vp]),
    "kpgnn_dropout_fwd": (ctypes.c_int, [ctypes.POINTER(DropoutDesc), c_vp]),
    "kpgnn_dropout_bwd": (ctypes.c_int, [ctypes.POINTER(DropoutDesc), c_vp]),
    "kpgnn_dropout_mask": (ctypes.c_int, [ctypes.POINTER(DropoutMaskDesc), c_vp]),
    "kpgnn_jk_reduce_fwd": (ctypes.c_int, [ctypes.POINTER(JkDesc), c_vp]),
    "kpgnn_jk_reduce_bwd": (ctypes.c_int, [ctypes.POINTER(JkDesc), c_vp]),
    "kpgnn_jk_lstm_saved_bytes": (ctypes.c_size_t, [c_i64, c_i32, c_i32, c_i32]),
    "kpgnn_jk_lstm_workspace_bytes": (ctypes.c_size_t, [c_i64, c_i32, c_i32, c_i32]),
    "kpgnn_jk_lstm_fwd": (ctypes.c_int, [ctypes.POINTER(JkLstmDesc), c_vp]),
    "kpgnn_jk_lstm_bwd": (ctypes.c_int, [ctypes.POINTER(JkLstmDesc), c_vp]),
    "kpgnn_body_norm_workspace_bytes": (ctypes.c_size_t, [c_i64, c_i32]),
    "kpgnn_body_norm_fwd": (ctypes.c_int, [ctypes.POINTER(NormDesc), c_vp]),
    "kpgnn_body_norm_bwd": (ctypes.c_int, [ctypes.POINTER(NormDesc), c_vp]),
    "kpgnn_graph_norm_saved_floats": (ctypes.c_size_t, [c_i32, c_i32, c_i32]),
    "kpgnn_graph_norm_workspace_bytes": (ctypes.c_size_t, [c_i64, c_i32, c_i32, c_i32]),
    "kpgnn_graph_norm_fwd": (ctypes.c_int, [ctypes.POINTER(GraphNormDesc), c_vp]),
    "kpgnn_graph_norm_bwd": (ctypes.c_int, [ctypes.POINTER(GraphNormDesc), c_vp]),
    "kpgnn_attn_pool_workspace_bytes": (ctypes.c_size_t, [c_i32, c_i32]),
    "kpgnn_attn_pool_fwd": (ctypes.c_int, [ctypes.POINTER(AttnPoolDesc), c_vp]),
    "kpgnn_attn_pool_bwd": (ctypes.c_int, [ctypes.POINTER(AttnPoolDesc), c_vp]),
    "kpgnn_head_linear_workspace_bytes": (ctypes.c_size_t, [c_i64, c_i32, c_i32]),
    "kpgnn_head_linear_fwd": (ctypes.c_int, [ctypes.POINTER(HeadLinearDesc), c_vp]),
    "kpgnn_head_linear_bwd": (ctypes.c_int, [ctypes.POINTER(HeadLinearDesc), c_vp]),
    "kpgnn_nll_loss": (ctypes.c_int, [ctypes.POINTER(NllLossDesc), c_vp]),
    "kpgnn_stat_slot_bytes": (ctypes.c_size_t, [c_i32]),
    "kpgnn_stream_capture_id": (ctypes.c_int, [c_vp, ctypes.POINTER(ctypes.c_uint64)]),
    "kpgnn_attn_fwd": (ctypes.c_int, [ctypes.POINTER(AttnDesc), c_vp]),
    "kpgnn_attn_bwd": (ctypes.c_int, [ctypes.POINTER(AttnDesc), c_vp]),
    "kpgnn_attn_scan_fwd": (ctypes.c_int, [ctypes.POINTER(AttnScanDesc), c_vp]),
    "kpgnn_attn_scan_bwd": (ctypes.c_int, [ctypes.POINTER(AttnScanDesc), c_vp]),
    "kpgnn_attn_scan_unpad": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp]),
    "kpgnn_linear_fwd": (ctypes.c_int, [ctypes.POINTER(LinearDesc), c_vp]),
    "kpgnn_linear_split_workspace_bytes": (ctypes.c_size_t, [c_i32, c_i32, c_i32]),
    "kpgnn_linear_split_many": (ctypes.c_int, [ctypes.POINTER(SplitJob), c_i32, c_vp]),
    "kpgnn_linear_group_fwd": (ctypes.c_int, [ctypes.POINTER(LinearGroupDesc), c_vp]),
    "kpgnn_geo_theta_fwd": (ctypes.c_int, [c_vp, c_i32, c_i32, c_vp, c_vp]),
    "kpgnn_geo_theta_bwd": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "kpgnn_hop_mlp_workspace_bytes": (ctypes.c_size_t, [c_i64, c_i32, c_i32, c_i32, c_i32]),
    "kpgnn_hop_mlp_fwd": (ctypes.c_int, [ctypes.POINTER(HopMlpDesc), c_vp]),
    "kpgnn_hop_mlp_bwd": (ctypes.c_int, [ctypes.POINTER(HopMlpDesc), c_vp]),
    "kpgnn_sage_tail_workspace_bytes": (ctypes.c_size_t, [c_i64, c_i32, c_i32, c_i32, c_i32]),
    "kpgnn_sage_tail_fwd": (ctypes.c_int, [ctypes.POINTER(SageTailDesc), c_vp]),
    "kpgnn_sage_tail_bwd": (ctypes.c_int, [ctypes.POINTER(SageTailDesc), c_vp]),
    "kpgnn_table_gather_sum_fwd": (ctypes.c_int, [ctypes.POINTER(TgsDesc), c_vp]),
    "kpgnn_table_gather_sum_bwd": (ctypes.c_int, [ctypes.POINTER(TgsDesc), c_vp]),
    "kpgnn_table_gather_sum_bwd_workspace_bytes": (ctypes.c_size_t, [c_i64, c_i32, c_i32]),
}

_lib = None


def load(path=None):
    """Load (once) and return the ctypes handle; raises KpgnnError when the library is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or HIP_LIB_PATH
    if not os.path.exists(path):
        raise KpgnnError(
            f"{path} not found: the HIP extension is required (no CPU fallback). "
            "Build it with `python -m kp_gnn_amd.build` (or __graft_entry__.build()).")
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:  # e.g. libamdhip64 missing
        raise KpgnnError(f"cannot load {path}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.kpgnn_abi_version() != 1:
        raise KpgnnError("libkpgnn_hip.so ABI version mismatch")
    _lib = lib
    return lib


def agg_launch_counts():
    """(fwd, bwd): per KPGNN_AGG_ROUTE_* how many kpgnn_aggregate_fwd / _bwd calls of this process each kernel served"""
    fwd, bwd = (c_i64 * 4)(), (c_i64 * 4)()
    check(load().kpgnn_agg_launch_counts(fwd, bwd), "kpgnn_agg_launch_counts")
    return list(fwd), list(bwd)


def check(rc, what):
    if rc != 0:
        msg = load().kpgnn_last_error()
        raise KpgnnError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


class LaunchTimer:
    """Opt-in per-launch timing of the aggregation kernels with HIP events recorded on the stream the
    kernel is launched on (bench.py's roofline leg).  Each record: (kind, algorithmic_bytes, start, stop)."""

    def __init__(self):
        self.records = []

    def summary(self):
        """kind -> dict(launches, avg_ms, bytes_per_launch, gbps); call after a device synchronize."""
        out = {}
        for kind, nbytes, a, b in self.records:
            d = out.setdefault(kind, {"launches": 0, "ms": 0.0, "bytes": 0})
            d["launches"] += 1
            d["ms"] += a.elapsed_time(b)
            d["bytes"] += nbytes
        for d in out.values():
            d["avg_ms"] = d["ms"] / d["launches"]
            d["bytes_per_launch"] = d["bytes"] / d["launches"]
            d["gbps"] = d["bytes"] / (d["ms"] * 1e-3) / 1e9 if d["ms"] > 0 else 0.0
        return out


_timer = None


def set_launch_timer(timer):
    global _timer
    _timer = timer


def launch(name, dev, *args, timed=None, allow=()):
    """Call the entry point `name` on the current stream of `dev` (appended as the last argument) and check its return code;
    a code listed in `allow` (e.g. ELIMIT where the caller has another path for shapes the kernel does not cover) is returned.
    timed = (kind, nbytes_fn): with a launch timer installed the call is bracketed by two events and recorded as
    (kind, nbytes_fn(), start, stop).  nbytes_fn runs only then: a byte count may synchronise with the device, which an
    untimed step (let alone a stream capture) must not."""
    fn = getattr(_lib or load(), name)
    with torch.cuda.device(dev):
        timer = _timer if timed is not None else None
        if timer is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        rc = fn(*args, torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            if rc in allow:
                return rc
            check(rc, name)
        if timer is not None:
            e1.record()
            timer.records.append((timed[0], timed[1](), e0, e1))
        return 0
