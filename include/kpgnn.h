/*
 * kpgnn.h - C ABI of libkpgnn_hip.so: the MI355X (gfx950) K-hop message-passing hot path of KP-GNN.
 *
 * This is the drop-in boundary.  The reference (JiaruiFeng/KP-GNN) is pure Python; the arithmetic of
 * this path lives in its layer files and in PyG's MessagePassing.propagate.  Each entry point below
 * names the reference code it replaces.  Signatures carry plain pointers, sizes and strides only (no
 * torch types); every pointer marked "device" is HBM memory owned by the caller; nothing is allocated,
 * freed or synchronised inside a call, so calls are HIP-graph capturable.  `stream` is a hipStream_t
 * passed as void*.  All entry points return 0 on success and a negative KPGNN_E* code on failure;
 * kpgnn_last_error() returns a thread-local message for the last failure.
 *
 * Tensor layout conventions: N nodes of the collated batch, K hop slots, D per-hop feature width.
 * Feature tensors are fp32, logical shape [N, K, D], innermost dimension contiguous, node and hop
 * strides given in ELEMENTS (so a [N,k,H] view of a history buffer or of a [N, K*dk] matrix needs no copy).
 *
 * K-hop CSR ("khop_csr"): the K-hop edge list (edge_index [2,E] int64, edge_attr [E,K] int64 where
 * attr==0 means "edge not active in this hop", reference data_utils.py:80-93) is re-laid out once per
 * batch as a CSR keyed by (node, hop): segment s = node*K + hop holds the active (edge,hop) pairs of that
 * node in ORIGINAL EDGE ORDER (stable), as parallel arrays col[] (the other endpoint, int32) and code[]
 * (the attr value = embedding row, uint16).  Two orientations are built: by destination (forward
 * aggregation) and by source (backward).
 */
#ifndef KPGNN_H_
#define KPGNN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KPGNN_ABI_VERSION 1

#define KPGNN_OK 0
#define KPGNN_EINVAL (-1)   /* bad argument (shape, stride, null pointer, limits) */
#define KPGNN_EHIP (-2)     /* a HIP runtime call or kernel launch failed */
#define KPGNN_ELIMIT (-3)   /* size exceeds an implementation limit (int32 indices, LDS) */

typedef void* kpgnn_stream_t; /* hipStream_t */

int kpgnn_abi_version(void);
const char* kpgnn_last_error(void);

/* Device facts used by the host side for launch sizing / roofline reporting (needs a GPU). */
int kpgnn_device_info(int* cu_count, int* lds_bytes_per_block, int* wavefront, char* arch, int arch_len);

/* ------------------------------------------------------------------------------------------------
 * K-hop CSR construction (device).  Replaces nothing in the reference one-to-one: the reference feeds
 * the raw edge list to PyG (`self.propagate(edge_index, ...)`, layers/KPGIN.py:100, KPGINplus.py:74,
 * KPGCN.py:110, gine.py:52) which gathers/scatters over all E*K (edge,hop) slots and multiplies the
 * inactive ones by a zero mask (message(): KPGIN.py:115-118).
 * ---------------------------------------------------------------------------------------------- */

/* Pass 1: statistics of a K-hop edge list.  stats (device, int64[8]) receives
 *   [0] A = number of active (edge,hop) pairs   [1] max attr in column 0   [2] max attr in columns 1..K-1
 *   [3] min attr over all columns               [4] min node index         [5] max node index
 * edge_index rows are `ei_stride` elements apart; edge_attr rows `attr_stride` elements apart. */
int kpgnn_csr_stats(const int64_t* edge_index, int64_t ei_stride, const int64_t* edge_attr, int64_t attr_stride,
                    int64_t E, int32_t K, int64_t* stats, kpgnn_stream_t stream);

/* Workspace (bytes, device) needed by kpgnn_csr_build for E edges, A active pairs, N nodes, K hops. */
size_t kpgnn_csr_workspace_bytes(int64_t E, int64_t A, int64_t N, int32_t K);

/* Pass 2: build both orientations.  A must be stats[0].  Outputs (device):
 *   rowptr_dst int32[N*K+1], col_dst int32[A] (= source node), code_dst uint16[A]   -- keyed by (dst,hop)
 *   rowptr_src int32[N*K+1], col_src int32[A] (= dest node),   code_src uint16[A]   -- keyed by (src,hop)
 * Entries of one segment keep the order of the input edge list (stable), which is the reference's CPU
 * summation order (index_add_ over edges in order).
 * Optional third ordering for kpgnn_table_grad (tile_ptr == NULL skips it; needs K <= 62): per tile of
 * nodes_per_tile (1..8) destination nodes, one entry per DISTINCT (node, hop, code) with its multiplicity (pairs of
 * one segment that carry the same code add the same gradient row to the same table row), sorted by
 * (tile, table, code, hop, node_in_tile):
 *   tile_ptr  int32[ceil(N/nodes_per_tile)+1]   (tile_ptr[last] = number of entries <= A)
 *   tile_pack uint32[A] (at most A entries are written) =
 *             table<<31 | code<<15 | node_in_tile<<12 | (multiplicity-1)<<6 | hop
 *   (table 0 = hop 0 -> hop1_edge_emb, table 1 = hops >= 1 -> hopk_edge_emb; codes < 2^16; multiplicity 1..64, a longer
 *   run is split every 64 pairs counted from its own first pair - the list of a tile depends on that tile's pairs only,
 *   which is what lets kpgnn_collate merge per-node lists built once per dataset into the very same list). */
int kpgnn_csr_build(const int64_t* edge_index, int64_t ei_stride, const int64_t* edge_attr, int64_t attr_stride,
                    int64_t E, int32_t K, int64_t N, int64_t A,
                    int32_t* rowptr_dst, int32_t* col_dst, uint16_t* code_dst,
                    int32_t* rowptr_src, int32_t* col_src, uint16_t* code_src,
                    int32_t nodes_per_tile, int32_t* tile_ptr, uint32_t* tile_pack,
                    void* workspace, size_t workspace_bytes, kpgnn_stream_t stream);

/* Hop-prefix copy of the table-gradient entry list: the entries of (tile_ptr, tile_pack) with hop < k, in the same
 * order.  out_ptr int32[num_tiles+1], out_pack uint32[>= tile_ptr[num_tiles]], scratch int32[num_tiles].  A layer that
 * aggregates k < K hops (models/GNNs.py:421-423) hands kpgnn_table_grad this copy: the kernel splits a tile's list
 * among its waves by position, and inactive entries would leave most waves idle.  Static per batch and k. */
int kpgnn_tile_pack_filter(const int32_t* tile_ptr, const uint32_t* tile_pack, int64_t num_tiles, int32_t k,
                           int32_t* out_ptr, uint32_t* out_pack, int32_t* scratch, kpgnn_stream_t stream);

/* All hop-prefix copies at once: for k = 1..num_prefix the entries with hop < k, in the same order (three launches in all,
 * where kpgnn_tile_pack_filter takes three per k).  out_ptr int32[num_prefix][num_tiles+1], out_pack uint32[num_prefix][
 * pack_stride] (pack_stride >= tile_ptr[num_tiles]), scratch int32[num_prefix][num_tiles]. */
int kpgnn_tile_pack_prefixes(const int32_t* tile_ptr, const uint32_t* tile_pack, int64_t num_tiles, int32_t num_prefix,
                             int64_t pack_stride, int32_t* out_ptr, uint32_t* out_pack, int32_t* scratch,
                             const int32_t* n_dyn, int32_t nodes_per_tile, kpgnn_stream_t stream);
/* (n_dyn: optional device int32[1] live NODE count - num_tiles is then a capacity and the tiles beyond
 *  ceil(*n_dyn / nodes_per_tile) count as empty; NULL: all num_tiles tiles are live) */

/* ------------------------------------------------------------------------------------------------
 * Dataset-resident K-hop CSR + per-step collate (device).  Replaces the reference's storage / batching pair:
 *   datasets/ZINC_dataset.py:139-140  `torch.save(self.collate(data_list), ...)` - PyG's (data, slices) store of the
 *                                      pre-transformed dataset (tensors concatenated over graphs + per-graph offsets), and
 *   train_ZINC.py:224,36-40            DataLoader(shuffle=True) -> Batch.from_data_list + `.to(device)` on EVERY step.
 * The dataset's CSR (both orientations) and per-node table-gradient entry lists are built once - graph by graph the
 * arrays kpgnn_csr_build emits, with node ids LOCAL to their graph and offsets RELATIVE to the graph's first pair / entry -
 * and stay in HBM.  A batch of B graphs is then their concatenation plus offsets: no sort, no host synchronisation, no
 * int64 traffic.  Result: bit-identical to kpgnn_csr_build on the PyG-collated batch of the same graphs in the same order.
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_dataset_view {
    int32_t K;                  /* hops of the CSR */
    int32_t G;                  /* graphs in the dataset */
    const int64_t* node_ptr;    /* [G+1] first node of graph g in the node-level arrays (PyG slices['x']) */
    const int64_t* pair_ptr;    /* [G+1] first active (edge,hop) pair of graph g; the same offsets serve both orientations */
    const int64_t* ent_ptr;     /* [G+1] first table-gradient entry of graph g (NULL: no entry lists) */
    const int32_t* rowptr_dst;  /* [Nd*K] first pair of segment (node, hop) keyed by destination, relative to pair_ptr[g] */
    const int32_t* rowptr_src;  /* [Nd*K] the same keyed by source */
    const int32_t* col_dst;     /* [Ad] other endpoint of a pair, node id local to its graph */
    const int32_t* col_src;
    const uint16_t* code_dst;   /* [Ad] edge code of a pair */
    const uint16_t* code_src;
    const int32_t* ent_rel;     /* [Nd] first entry of a node, relative to ent_ptr[g] */
    const uint32_t* ent;        /* per-node entry lists = kpgnn_csr_build's tile_pack with nodes_per_tile = 1 */
} kpgnn_dataset_view;

typedef struct kpgnn_row_gather { const void* src; void* dst; int32_t row_bytes; } kpgnn_row_gather;

typedef struct kpgnn_collate_desc {
    kpgnn_dataset_view ds;
    int32_t B;                  /* graphs in the batch */
    int32_t N;                  /* its nodes, pairs and entries: sums of per-graph counts the host keeps.  They size the   */
    int64_t A;                  /*   LAUNCHES only - the kernels read the real counts from the header - so they may be     */
    int64_t n_ent;              /*   CAPACITIES of static buffers: one captured call then collates any batch that fits.   */
    /* device int32[4B+3]: ids[B] (dataset graph of batch slot b) | node_base[B+1] | pair_base[B+1] | ent_base[B+1], the three
     * exclusive prefix sums of the chosen graphs' node / pair / entry counts (last element = N / A / n_ent) */
    const int32_t* hdr;
    int32_t* rowptr_dst; int32_t* col_dst; uint16_t* code_dst;    /* int32[N*K+1], int32[A], uint16[A] */
    int32_t* rowptr_src; int32_t* col_src; uint16_t* code_src;
    int64_t* batch;             /* [N] batch slot of every node (PyG's Batch.batch) */
    int32_t* node_src;          /* [N] dataset node of every batch node */
    /* table-gradient entry list of the batch (tile_ptr NULL: skipped) and its hop-prefix copies for k = 1..num_prefix
     * (as kpgnn_tile_pack_prefixes lays them out, pack_stride = n_ent) */
    int32_t nodes_per_tile; int32_t* tile_ptr; uint32_t* tile_pack;
    int32_t* ent_node_ptr;      /* [N+1] scratch (first entry of every batch node) */
    int32_t num_prefix; int32_t* prefix_ptr; uint32_t* prefix_pack; int32_t* prefix_scratch;
    /* dense per-node / per-graph attributes: dst[i] = src[node_src[i]] (node rows), dst[b] = src[ids[b]] (graph rows) */
    int32_t n_node_rows; kpgnn_row_gather node_rows[8];
    int32_t n_graph_rows; kpgnn_row_gather graph_rows[8];
} kpgnn_collate_desc;

int kpgnn_collate(const kpgnn_collate_desc* d, kpgnn_stream_t stream);

/* loss[0] = mean_i |score[i] - y[i]| (kind 0; train_ZINC.py:42) or mean_i (score[i] - y[i])^2 (kind 1; train_qm9.py:96) and,
 * when dscore != NULL, dscore[i] = d loss / d score[i].  score, y: device [n] contiguous.  One launch, one block, fixed
 * summation order (bitwise reproducible); meant for batches of graph scores (n up to ~1e5). */
int kpgnn_regression_loss(const float* score, const float* y, int64_t n, int32_t kind, float* loss, float* dscore,
                          kpgnn_stream_t stream);

/* The graph regressor nn.Linear(hidden, 1) on the pooled graph rows (reference models/GraphRegression.py:17,46-51):
 * score[g] = sum_c pooled[g][c] w[c] + bias[0] (bias may be NULL).  pooled: device [G, D] contiguous fp32; w: [D]; score: [G]. */
int kpgnn_score_head_fwd(const float* pooled, const float* w, const float* bias, int64_t G, int32_t D, float* score,
                         kpgnn_stream_t stream);
/* Its backward in one launch: dpooled[g][c] = dscore[g] w[c] (NULL: skipped), dw[c] = sum_g dscore[g] pooled[g][c],
 * db[0] = sum_g dscore[g] (NULL: skipped); fixed summation order (bitwise reproducible). */
int kpgnn_score_head_bwd(const float* pooled, const float* w, const float* dscore, int64_t G, int32_t D, float* dpooled,
                         float* dw, float* db, kpgnn_stream_t stream);

/* One torch.optim.Adam step (amsgrad off, L2 weight_decay as in train_ZINC.py:244) over a flat bucket of n fp32
 * parameters with its gradient and the two moment buffers (all device, 16-B aligned, updated in place); step = 1 for the
 * first call.  Elementwise, so stepping the flat bucket of dp.py equals stepping the ~190 tensors one by one. */
int kpgnn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t step,
                    double lr, double beta1, double beta2, double eps, double weight_decay, kpgnn_stream_t stream);

/* The same step with the step number kept on the device: state = int64[2] {steps taken so far, 0}, both zero before the
 * first call; the launch reads state[0], steps with t = state[0] + 1 and leaves state[0] = t.  Its arguments never change,
 * so it can be captured in a hipGraph together with the forward and backward passes (one process, no all-reduce between). */
int kpgnn_adam_step_device(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t* state,
                           double lr, double beta1, double beta2, double eps, double weight_decay, kpgnn_stream_t stream);

/* count contiguous fp32 tensors copied device-to-device in ceil(count / 192) launches: dst[i][0..numel[i]) = src[i][..].  The
 * pointer tables are HOST arrays read at call time and passed to the kernel by value (capturable: a hipGraph node keeps
 * them).  Used to move a step's parameter gradients into their views of the flat all-reduce bucket (train_ZINC.py:34-36
 * leaves that to DataParallel's per-tensor reduce). */
int kpgnn_multi_copy(int32_t count, const float* const* src, float* const* dst, const int64_t* numel, kpgnn_stream_t stream);

/* A reduction that a launch left for later: slab holds nslab rows of elems partial sums (block order); the finished sums
 * out[e] = sum_b slab[b][e] go, in order, to n_out[0] elements of out[0], n_out[1] of out[1], ... (sum n_out == elems).
 * kpgnn_linear_wgrad(_pair) fills one instead of launching its own reduce when desc.defer is set; the caller hands it to the
 * next call that has a finishing launch anyway (kpgnn_table_grad_desc.pending) or runs it with kpgnn_reduce_jobs.  The slab
 * (the producing call's workspace) must stay untouched until then.  Fixed summation order: the result does not depend on
 * which launch does the adding. */
typedef struct kpgnn_reduce_job {
    const float* slab; int32_t nslab; int64_t elems;
    float* out[4]; int64_t n_out[4];
} kpgnn_reduce_job;
int kpgnn_reduce_jobs(const kpgnn_reduce_job* jobs, int32_t count, kpgnn_stream_t stream);   /* ceil(count / 3) launches */

/* ------------------------------------------------------------------------------------------------
 * Fused K-hop aggregation.
 * ---------------------------------------------------------------------------------------------- */
/* Storage of the big per-(node,hop) streams.  KPGNN_STORE_BF16: the rows a launch reads or writes as marked "(storage)"
 * below hold bf16 (2 bytes per element, same shapes and ELEMENT strides); every sum, the tables, theta, P and the layer
 * outputs stay fp32.  Implemented for the KP-GIN+ training path (fused GELU + geometric combine, dictionary P, D % 4 == 0):
 * kpgnn_aggregate_fwd (x_slot rows, pre), kpgnn_combine_bwd (pre, g), kpgnn_table_grad (g), kpgnn_aggregate_bwd (g);
 * other configurations answer KPGNN_EINVAL.  (BASELINE configs[1] names bf16; tolerance 2e-2 relative) */
enum { KPGNN_STORE_F32 = 0, KPGNN_STORE_BF16 = 1 };

/* Arithmetic of the dense fp32 products that offer a choice.  AUTO: the bf16-split product where the kernel has one for the
 * shape - every fp32 operand is the exact sum of three bf16 pieces, the six leading piece products run on the bf16 matrix
 * cores with fp32 accumulation - else F32.  The three dropped piece products sum to at most 7.83 * 2^-24 |a b| per product
 * (reached when the low 16 mantissa bits of both operands are set; truncation gives them one sign, so they add up along a
 * row): per element, |y - exact| <= the error of fp32 accumulation + 8 * 2^-24 * (sum_k |x_k| |w_k| + |bias|).
 * Operand range: the bound holds for every finite operand down to pieces that are SUBNORMAL bf16 numbers - measured on
 * gfx950 with x scaled by 2^-110 (values normal, their m and l pieces subnormal) against W scaled by 2^110: the split's packed
 * subtracts and v_mfma_f32_32x32x16_bf16 keep subnormal inputs, the error is that of the unscaled product - and up to
 * |x| = 2^126 with |w| <= 2^-20.  While no piece is subnormal, scaling x, w and bias by powers of two scales the result's bits
 * exactly.  A row of x that holds an Inf or a NaN comes out non-finite and touches no other row (the ReLU of
 * kpgnn_linear_group_fwd keeps a NaN, as torch.relu does).  tests/test_bf16_split_products.py holds all of this.
 * F32: v_mfma_f32_32x32x2_f32 always. */
enum { KPGNN_MATH_AUTO = 0, KPGNN_MATH_F32 = 1 };

enum {
    KPGNN_MODE_GIN = 0,     /* out = S + P + (1+eps)*x                  KPGIN.py:100-105, gine.py:52-53 */
    KPGNN_MODE_GINPLUS = 1, /* out = gelu(S) + P                        KPGINplus.py:74-77,87-88        */
    KPGNN_MODE_GCN = 2,     /* out = relu(S_norm) + P, self loops + sym. degree norm  KPGCN.py:85-114,120-126 */
    KPGNN_MODE_SUM = 3      /* out = S (+P), no activation: building block / KGINConv run_simulation.py:73 */
};
/* where, for node i and hop k,  S[i,k,:] = sum over active pairs a of segment (i,k) of
 *      x[col[a], k, :] + table_k[code[a], :]          (table_0 = hop1_edge_emb, table_k>0 = hopk_edge_emb)
 * and for GCN each term is scaled by dis[col[a],k]*dis[i,k] and the self loop (code 1) is added,
 * dis = (segment length + 1)^-1/2  (KPGCN.py:11-25,106-109).  P = peripheral_attr (nullable). */

typedef struct kpgnn_agg_fwd_desc {
    int32_t N, K, D;            /* nodes, ACTIVE hop slots (k <= K_csr), per-hop width */
    int32_t K_csr;              /* hop slots per node in rowptr (GNNPlus layer l<K uses a prefix, GNNs.py:429) */
    int32_t mode;               /* KPGNN_MODE_* */
    int32_t n_code0, n_codek;   /* rows of table0 / tablek (codes are validated against these by the caller) */
    int32_t use_tables;         /* 0: mask-only aggregation (no edge-code embedding; run_simulation.py:87-90) */
    const int32_t* rowptr;      /* device, [N*K_csr+1]  (by destination) */
    const int32_t* col;         /* device, [A] */
    const uint16_t* code;       /* device, [A] */
    const float* dis;           /* device, [N*K_csr] deg^-1/2, GCN only (else NULL) */
    const float* x;             /* device, [N,K,D] */
    int64_t x_sn, x_sk;
    const float* table0;        /* device, [n_code0, D] contiguous */
    const float* tablek;        /* device, [n_codek, D] contiguous (NULL iff K_csr == 1) */
    const float* periph;        /* device, [N,K,D] or NULL */
    int64_t p_sn, p_sk;
    const float* eps;           /* device scalar (GIN) or NULL (== 0) */
    float* out;                 /* device, [N,K,D] */
    int64_t o_sn, o_sk;
    float* pre;                 /* device, [N,K,D] contiguous or NULL: S before the activation (saved for bwd) */
    /* Optional fused geometric hop-combine (combine.py:43-58): if theta != NULL, `out` is not written;
     * hout[i,:] = sum_k theta[k,:] * (act(S[i,k,:]) + P[i,k,:]) is.  theta: device [K, D]. */
    const float* theta;
    float* hout;                /* device, [N, D] contiguous */
    /* Optional constant row added to every x row of hops >= 1 (gathered and self terms): the reference's
     * `x[:, 1:] += hopk_node_path_emb(pe_attr)` (KPGIN.py:92-94) when pe_attr is all padding (always so for
     * the reference's own pre-transform, data_utils.py:91,123): xbias = that table's row 0.  device [D]. */
    const float* xbias;
    /* Optional DICTIONARY form of the peripheral features (used when periph == NULL): P[i,k,:] =
     * ptab[uid[i*uid_stride + k], :].  Peripheral-subgraph feature tuples repeat massively (25 distinct
     * rows among 379,600 (node,hop) slots of a 2048-molecule batch), so the [N,K,D] stream becomes an
     * L2-resident table.  ptab: device [U, D] contiguous; uid: device int32. */
    const float* ptab;
    const int32_t* uid;
    int64_t uid_stride;
    /* Per-hop inputs (used when x == NULL): hop slot k reads x_slot[k], a [N,D] matrix with row stride x_sn.
     * GNNPlus stacks the previous layers' states into [N,k,H] with torch.cat every layer (models/GNNs.py:413-418);
     * with slots the kernel reads the k states where they are and the copy disappears.  K <= 16. */
    const float* x_slot[16];
    /* Rows of ptab (0 = unknown).  When given and small, the dictionary and theta are staged in LDS next to the
     * code tables, so the per-hop epilogue has no dependent global loads left. */
    int32_t n_dict;
    /* Geometric combine computed by the launch itself: alphas [D] (device) - theta[k,d] = softmax_k(a (1-a)^k) with
     * a = sigmoid(alphas[d]) (combine.py:43-50) is then an OUTPUT, written to `theta` ([K,D]) for the backward. */
    const float* alphas;
    /* KPGNN_STORE_*: with BF16 the x_slot rows (storage) and pre (storage) are bf16 - pass them through these float
     * pointers; x_sn counts ELEMENTS. */
    int32_t storage;
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
    /* Optional graph boundaries of the collated batch (device int32[num_graphs+1] node offsets, nodes of a graph contiguous as
     * PyG's collate lays them out; max_graph_nodes >= the largest graph).  With them a mask-only aggregation (no tables, no
     * peripheral features, no fused combine) whose largest graph's hop slab x[graph, hop, :] fits LDS is gathered FROM LDS: the
     * slab is staged once per (graph, hop) block and every neighbour row comes from there - the kernel for dense K-hop
     * neighbourhoods (run_simulation.py's 3-regular n = 1280 graphs: 582 pairs per node), where the plain gather is L2-bound. */
    const int32_t* graph_ptr; int32_t num_graphs; int32_t max_graph_nodes;
    /* Optional, with a fused combine and a given theta: hout[i,:] = hinit[i,:] + sum_k ... (device [N,D] contiguous; may be hout
     * itself).  This is what makes the launch the PULL form of the backward gather: with rowptr / col keyed by (source, hop),
     * x_slot[k] = hop k's slab of dL/dS of the layer k + 1 steps later, mode SUM, theta = 1, it writes a state's whole gradient
     * in one pass - every later reader's share plus what hinit already holds - instead of one read-modify-write per reader. */
    const float* hinit;
    const float* hinit2;        /* a second addend of the same kind (the pull form: the residual branch's share) or NULL */
} kpgnn_agg_fwd_desc;

int kpgnn_aggregate_fwd(const kpgnn_agg_fwd_desc* d, kpgnn_stream_t stream);

/* The PULL form of the backward gather as an entry of its own: with rowptr / col the (source, hop)-keyed CSR and slab[k] hop
 * k's [N,D] slab (row stride slab_sn) of dL/dS of the layer that read the state at hop slot k,
 *   hout[i,:] = hinit[i,:] + hinit2[i,:] + sum_k sum_{a in segment (i,k)} slab[k][col[a],:]
 * (pairs in list order into a per-hop sum, then the hops in order, after hinit and then hinit2) - exactly what
 * kpgnn_aggregate_fwd writes for mode SUM, use_tables = 0, x_slot = slab and theta = 1, bit for bit.  Rows of 36 to 256
 * columns with D % 4 == 0, 16-byte aligned operands and K below the row's lane count (16 lanes up to D = 64, 32 up to 128,
 * 64 beyond) run a kernel specialised for this case (no epilogue, no theta: more resident waves per SIMD); every other row
 * shape runs the generic kernel with unit weights. */
typedef struct kpgnn_pull_gather_desc {
    int32_t N, K, D;            /* nodes (capacity with n_dyn), hop slabs read (<= 16, <= K_csr), row width */
    int32_t K_csr;              /* hop slots per node in rowptr */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N); NULL: all N rows.  Rows beyond it are not written */
    const int32_t* rowptr;      /* device, [N*K_csr+1], keyed by (source, hop) */
    const int32_t* col;         /* device, [A] */
    const float* slab[16];      /* device, slab[k]: [N,D] with row stride slab_sn, k < K */
    int64_t slab_sn;
    const float* hinit;         /* device [N,D] contiguous or NULL; may be hout itself */
    const float* hinit2;        /* device [N,D] contiguous or NULL */
    float* hout;                /* device [N,D] contiguous */
} kpgnn_pull_gather_desc;

int kpgnn_khop_pull_gather(const kpgnn_pull_gather_desc* d, kpgnn_stream_t stream);

/* How many kpgnn_aggregate_fwd calls of this process were served by the LDS-staged kernel (graph_ptr given and every
 * condition above met).  A host-side counter: the choice of kernel leaves no other trace, so a test of that kernel reads it
 * before and after its call. */
int64_t kpgnn_agg_lds_launch_count(void);

/* The same for every kernel behind kpgnn_aggregate_fwd / kpgnn_aggregate_bwd: which of them served a call depends on shape
 * thresholds only (narrow rows, small batches, graph boundaries given) and leaves no other trace.  fwd[r] / bwd[r] receive how
 * many calls of this process were served by route r (either array may be NULL); host-side relaxed atomics, test support only.
 * fwd[KPGNN_AGG_ROUTE_LDS] is what kpgnn_agg_lds_launch_count returns; the backward has no LDS-staged kernel, so
 * bwd[KPGNN_AGG_ROUTE_LDS] stays 0.  kpgnn_khop_pull_gather is not counted. */
enum {
    KPGNN_AGG_ROUTE_SUBGROUP = 0,   /* agg_fwd_kernel / agg_bwd_kernel: a sub-group of lanes per node */
    KPGNN_AGG_ROUTE_NARROW = 1,     /* agg_narrow_kernel: a thread per output element (D <= 32) */
    KPGNN_AGG_ROUTE_SMALL = 2,      /* agg_fwd_small_kernel / agg_bwd_small_kernel: a block per node (N <= 4096) */
    KPGNN_AGG_ROUTE_LDS = 3         /* agg_lds_fwd_kernel: a graph's hop slab staged in LDS */
};
int kpgnn_agg_launch_counts(int64_t fwd[4], int64_t bwd[4]);

/* Backward of the aggregation w.r.t. x and the two edge-code tables, given g = dL/dS [N,K,D]
 * (the caller applies the activation derivative; for GCN g already includes relu').
 *   gx[j,k,:]      = sum over pairs a of segment (j,k) of the BY-SOURCE csr of w_a * g[col[a],k,:]  (+ self terms)
 *   gtable_k[c,:] += sum over pairs with code c of w_a * g[col[a],k,:]      (fp32 atomics; caller zeroes)
 * self terms: GIN adds (1+eps)*g[j,k,:]; GCN adds dis[j,k]^2*g[j,k,:] and the same into gtable_k[1,:]. */
typedef struct kpgnn_agg_bwd_desc {
    int32_t N, K, D, K_csr, mode, n_code0, n_codek, use_tables;
    const int32_t* rowptr_src;
    const int32_t* col_src;
    const uint16_t* code_src;
    const float* dis;           /* GCN only */
    const float* g;             /* device [N,K,D] */
    int64_t g_sn, g_sk;
    const float* eps;
    float* gx;                  /* device [N,K,D] */
    int64_t gx_sn, gx_sk;
    float* gtable0;             /* device [n_code0, D], accumulated into (NULL: skip table grads) */
    float* gtablek;             /* device [n_codek, D] */
    /* Per-hop outputs (used when gx == NULL): the gradient of hop slot k goes to gx_slot[k], [N,D] with row
     * stride gx_sn (the backward of the per-hop inputs above: no [N,k,D] tensor to slice up afterwards). */
    float* gx_slot[16];
    /* Bit k set: ADD the gradient of hop slot k to what gx_slot[k] already holds (a state that several layers read as
     * a slot collects its gradient in one buffer instead of one tensor per reader plus an add each).  Two hop slots of
     * one call must not share a buffer when either accumulates (KPGNN_EINVAL).  With gx (one [N,K,D] tensor) bit k adds hop
     * k's gradient to what gx[:, k, :] already holds: a state that the bodies' jumping-knowledge projection and the next
     * norm's residual branch also read collects its whole gradient in one buffer (K <= 32). */
    uint32_t accumulate_mask;
    int32_t storage;            /* KPGNN_STORE_*: with BF16, g (storage) holds bf16 rows; g_sn / g_sk count elements */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
} kpgnn_agg_bwd_desc;

int kpgnn_aggregate_bwd(const kpgnn_agg_bwd_desc* d, kpgnn_stream_t stream);

/* Table gradients WITHOUT per-edge atomics:
 *   gtable_t[c,:] = sum over active pairs (i,k) of table t with code c of g[i,k,:]      (g = dL/dS)
 * (the reference gets them from nn.Embedding's backward of the materialised [E,K,D] embedding tensor,
 * KPGIN.py:90-96), and optionally the gradient of a peripheral-feature DICTIONARY (see kpgnn_agg_fwd_desc.ptab):
 *   gdict[u,:] = sum over (i,k) with uid[i,k] == u of  theta[k,:]*gh[i,:]   (dict_src 1, fused combine)
 *                                                  or  g[i,k,:]             (dict_src 2, g is dL/dP itself)
 * A block streams tiles of `nodes_per_tile` destination nodes of g through LDS; thread t owns feature column
 * t, walks the tile's (table,code)-sorted pair list and keeps the running sum of the current code in a
 * register, so the LDS accumulators are column-private (no atomics).  Per-block partial tables go to
 * `workspace`; a second launch adds them in block order: outputs are OVERWRITTEN and bitwise reproducible.
 * K is the number of ACTIVE hops of g (pairs with hop >= K are skipped).  tile_ptr == NULL skips the
 * edge-code part (dictionary gradient only; gtable0/gtablek may then be NULL). */
typedef struct kpgnn_table_grad_desc {
    int32_t N, K, D, nodes_per_tile, n_code0, n_codek;
    int32_t n_dict, dict_src;   /* dictionary rows (0: none) and source (1: theta*gh, 2: g rows) */
    const int32_t* tile_ptr;
    const uint32_t* tile_pack;
    const float* g;             /* device [N,K,D] */
    int64_t g_sn, g_sk;
    const int32_t* uid;         /* device [N, uid_stride]: dictionary row of (node, hop) */
    int64_t uid_stride;
    const float* theta;         /* device [K, D]  (dict_src 1) */
    const float* gh;            /* device [N, D]  (dict_src 1) */
    float* gtable0;             /* device [n_code0, D] */
    float* gtablek;             /* device [n_codek, D] or NULL when K == 1 */
    float* gdict;               /* device [n_dict, D] */
    void* workspace;            /* device, >= kpgnn_table_grad_workspace_bytes(...) */
    size_t workspace_bytes;
    /* Kernel choice: 0 = automatic (narrow rows D <= 32 and K > 8 go to the count-matrix product on the matrix cores,
     * wide rows to the register walk), 1 = force the walk, 2 = force the count-matrix kernel.  The parity tests
     * compare the two. */
    int32_t kernel;
    /* Optional (walk kernel): the dictionary entries of every tile sorted by dictionary row, from kpgnn_dict_tile_pack
     * on the same uid / nodes_per_tile with dict_pack_K >= K hops (one list serves every layer: hops >= K are skipped).
     * Equal rows then leave the registers once per run, and a row belongs to one wave at a time (no float atomics:
     * bitwise reproducible).  Without it a dictionary gradient goes to the count-matrix kernel. */
    const uint32_t* dict_pack;
    int32_t dict_pack_K;
    /* Optional: a second slab [extra_nslab][extra_elems] (e.g. the one kpgnn_dict_grad left with defer_reduce) that the
     * finishing launch adds up into extra_out[extra_elems] as well - one launch instead of two. */
    const float* extra_slab;
    int32_t extra_nslab;
    int64_t extra_elems;
    float* extra_out;
    int32_t storage;            /* KPGNN_STORE_*: with BF16, g (storage) holds bf16 rows (walk kernel, D % 8 == 0) */
    /* Fused combine backward (fuse_pre != NULL; KP-GIN+ epilogue, fp32, edge tables only, K <= 8, even D <= 128): the
     * launch COMPUTES g = theta[k] * gh[i] * gelu'(S[i,k]) per tile (kpgnn_combine_bwd's arithmetic), writes it to fuse_g
     * and walks it from LDS - `g` above is not read.  fuse_gtheta [K,D] (optional) = sum_i gh[i] * (gelu(S[i,k]) + P[i,k]) with
     * P from the dictionary (fuse_ptab, fuse_uid; NULL = no P); with fuse_alphas / fuse_galphas the finishing launch also
     * differentiates theta(alphas) as kpgnn_combine_bwd does.  fuse_workspace >= kpgnn_table_grad_fuse_workspace_bytes(K, D). */
    const float* fuse_pre;      /* device [N,K,D] contiguous: S saved by the forward */
    const float* fuse_ptab;     /* device [fuse_n_dict, D] */
    const int32_t* fuse_uid;    /* device [N, fuse_uid_stride] */
    int64_t fuse_uid_stride;
    int32_t fuse_n_dict;
    float* fuse_g;              /* device, written: element (i,k,c) at i*g_sn + k*g_sk + c (even strides >= D; [N,K,D] contiguous or hop-major [K][N][D]) */
    float* fuse_gtheta;         /* device [K,D] or NULL */
    const float* fuse_alphas;   /* device [D] or NULL */
    float* fuse_galphas;        /* device [D] or NULL */
    void* fuse_workspace;
    size_t fuse_workspace_bytes;
    /* 1: the dictionary gradient is ADDED to what gdict / extra_out already hold (gdict += ...): a
     * dictionary read by every layer collects its gradient in one buffer instead of one tensor per layer for the
     * framework to sum (7 add launches per step at L = 8). */
    int32_t accumulate_dict;
    /* Optional (host pointer): one deferred reduction of an earlier call, added up by this call's finishing launch. */
    const kpgnn_reduce_job* pending;
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
    /* Optional: an upper bound (>= 1) on the multiplicity of any single entry of tile_pack, when the caller knows it (0 = unknown).
     * Below 64 no run of equal entries was cut, i.e. every (node, hop, code) has ONE entry: the fused kernel may then take the
     * table gradients as a count-matrix product on the matrix cores (8-bit count cells, entry order irrelevant). */
    int32_t max_multiplicity;
} kpgnn_table_grad_desc;

size_t kpgnn_table_grad_workspace_bytes(int32_t N, int32_t K, int32_t D, int32_t nodes_per_tile,
                                        int32_t n_code0, int32_t n_codek, int32_t n_dict);
int kpgnn_table_grad(const kpgnn_table_grad_desc* d, kpgnn_stream_t stream);
size_t kpgnn_table_grad_fuse_workspace_bytes(int32_t K, int32_t D);
/* pack[tile*64 + j] = uid<<8 | node_in_tile<<3 | hop for the (node, hop) entries of a tile of nodes_per_tile nodes
 * (nodes_per_tile * K <= 64, K <= 8), sorted by uid; unused places hold 0xFFFFFFFF.  pack: uint32[ceil(N/npt) * 64].
 * A one-off per batch (the ids are data): the reference recomputes nothing like it - its embedding backward sorts the
 * same ids on every step (aten embedding_dense_backward under models/GNNs.py:172-179). */
int kpgnn_dict_tile_pack(const int32_t* uid, int64_t uid_stride, int32_t N, int32_t K, int32_t nodes_per_tile,
                         uint32_t* pack, kpgnn_stream_t stream);
/* The same under a dynamic row count: N is the capacity (the list still has ceil(N/npt) tiles), n_dyn the device-side live
 * count (NULL: N); the places of nodes >= *n_dyn hold 0xFFFFFFFF.  kpgnn_table_grad's walk takes every entry of a list, and
 * loads only the live rows of a tile: a list for a dynamic-row launch MUST come from this entry point with the same n_dyn. */
int kpgnn_dict_tile_pack_dyn(const int32_t* uid, int64_t uid_stride, int32_t N, const int32_t* n_dyn, int32_t K,
                             int32_t nodes_per_tile, uint32_t* pack, kpgnn_stream_t stream);

/* Peripheral-dictionary gradient under the fused geometric combine, from gh alone (no [N,K,D] operand):
 *   gdict[u,:] = sum_k theta[k,:] * sum over nodes i with uid[i,k] == u of gh[i,:]
 * (the same sums as kpgnn_table_grad's dict_src 1, which stays as the path for shapes this kernel does not take:
 * kpgnn_dict_grad_workspace_bytes returns 0 unless K <= 8, D even and <= 128 and n_dict*K*D*4 B + 32 KB fit LDS).
 * One wave per hop, accumulator rows (u, hop) private to a wave: no atomics, bitwise reproducible.
 * Replaces the embedding_dense_backward calls under models/GNNs.py:393-400 for the dictionary form of the features. */
typedef struct kpgnn_dict_grad_desc {
    int32_t N, K, D, n_dict;
    const int32_t* uid;         /* device [N, uid_stride]: dictionary row of (node, hop), values in [0, n_dict) */
    int64_t uid_stride;
    const float* theta;         /* device [K, D] */
    const float* gh;            /* device [N, D] contiguous */
    float* gdict;               /* device [n_dict, D] (overwritten) */
    void* workspace;            /* device, >= kpgnn_dict_grad_workspace_bytes(N, K, D, n_dict) */
    size_t workspace_bytes;
    /* defer_reduce != 0: leave the per-block partial sums in workspace as float[kpgnn_dict_grad_slabs(N)][n_dict*D] and
     * do not write gdict: the caller adds them up in block order (kpgnn_table_grad's extra_slab does it in its own
     * finishing launch). */
    int32_t defer_reduce;
    /* Optional, device [K]: one designated id per hop.  Its sum is taken as (sum of all gh rows) - (the hop's other ids)
     * instead of being accumulated node by node - exact for ANY choice (out-of-range values are read as 0), and 3-4x less
     * work when it is the hop's most frequent id (one id covers 82-99.9 % of the nodes of a hop in a molecule batch). */
    const int32_t* dominant;
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
} kpgnn_dict_grad_desc;

size_t kpgnn_dict_grad_workspace_bytes(int32_t N, int32_t K, int32_t D, int32_t n_dict);
int32_t kpgnn_dict_grad_slabs(int32_t N);
int kpgnn_dict_grad(const kpgnn_dict_grad_desc* d, kpgnn_stream_t stream);

/* The same gradient for ALL the layers of a sequential stack that read one dictionary (models/GNNs.py:393-400: every layer
 * adds the same peripheral rows), in one launch:
 *   gdict[u,:] = sum_l sum_{k < K[l]} theta[l][k,:] * sum over nodes i with uid[i,k] == u of gh[l][i,:]
 * A launch of kpgnn_dict_grad is mostly fixed-size passes over its [n_dict*K, D] accumulator table (one block per CU);
 * here the table is filled once, each layer's rows enter it already multiplied by that layer's theta, and the
 * designated-row fix and the final hop sum run once.  `dominant` (a designated id per hop, kpgnn_dict_grad_desc) is
 * required; K[l] <= 8, L <= 16, LDS: (n_dict*Kmax + 9 L) * D * 4 bytes <= 160 KB.  workspace as kpgnn_dict_grad's for Kmax. */
typedef struct kpgnn_dict_grad_multi_desc {
    int32_t N, D, n_dict, L;
    const int32_t* uid;         /* device [N, uid_stride] */
    int64_t uid_stride;
    const float* theta[16];     /* device [K[l], D] each */
    const float* gh[16];        /* device [N, D] contiguous each */
    int32_t K[16];
    float* gdict;               /* device [n_dict, D] (overwritten) */
    void* workspace;
    size_t workspace_bytes;
    const int32_t* dominant;    /* device [Kmax] */
    const int32_t* n_dyn;       /* optional live-row count */
} kpgnn_dict_grad_multi_desc;
int kpgnn_dict_grad_multi(const kpgnn_dict_grad_multi_desc* d, kpgnn_stream_t stream);

/* Backward pre-pass of the fused epilogue (elementwise, streaming):  with v = act(S) + P,
 *   gv[i,k,:] = theta[k,:] * gh[i,:]     (fused geometric combine)   or   gout[i,k,:]   (theta == NULL)
 *   g[i,k,:]  = gv * act'(S[i,k,:])                      act = gelu (GINPLUS) / relu (GCN) / identity
 *   gtheta[k,:] = sum_i gh[i,:] * v[i,k,:]               (only with theta)
 * Replaces a dozen framework elementwise kernels (broadcast mul, erf, exp, mul, add, einsum ...) by one pass:
 * reads S (`pre`) once, writes g once.  P comes dense (periph) or from a dictionary (ptab + uid). */
typedef struct kpgnn_combine_bwd_desc {
    int32_t N, K, D, mode;
    const float* pre;           /* device [N,K,D] contiguous (S saved by the forward) */
    const float* gh;            /* device [N,D] contiguous          (with theta) */
    const float* theta;         /* device [K,D] or NULL */
    const float* gout;          /* device [N,K,D] strided            (without theta) */
    int64_t go_sn, go_sk;
    const float* periph;        /* dense P [N,K,D] or NULL  (only read for gtheta) */
    int64_t p_sn, p_sk;
    const float* ptab;          /* dictionary P: [U,D] rows + uid, or NULL */
    const int32_t* uid;
    int64_t uid_stride;
    float* g;                   /* device [N,K,D] contiguous */
    float* gv;                  /* device [N,K,D] contiguous or NULL: dL/dP when a dense P needs its gradient */
    float* gtheta;              /* device [K,D] (overwritten) or NULL */
    void* workspace;            /* device, >= kpgnn_combine_bwd_workspace_bytes(N,K,D) when gtheta != NULL */
    size_t workspace_bytes;
    int32_t n_dict;             /* rows of ptab (0 = unknown): small dictionaries are staged in LDS */
    /* Geometric combine (theta = softmax_k(a (1-a)^k), a = sigmoid(alphas), layers/combine.py:43-50): with both given the
     * launch that adds up gtheta also writes galphas[D] = (d theta / d alphas)^T gtheta (kpgnn_geo_theta_bwd's result). */
    const float* alphas;        /* device [D] or NULL */
    float* galphas;             /* device [D] or NULL */
    int32_t storage;            /* KPGNN_STORE_*: with BF16, pre (storage) and g (storage) hold bf16 rows */
} kpgnn_combine_bwd_desc;

size_t kpgnn_combine_bwd_workspace_bytes(int32_t N, int32_t K, int32_t D);
int kpgnn_combine_bwd(const kpgnn_combine_bwd_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-table gather-sum: out[m,:] = bias + sum_c table[col_offset[c] + idx[m,c], :].
 * This is the reference's peripheral feature build (models/GNNs.py:172-179 / :393-400 / :637-644 via
 * FeatureConcatEncoder, layers/feature_encoder.py:62-67): Linear(cat_c Emb_c[idx_c]) equals a sum of rows
 * of the PROJECTED tables Emb_c @ W_c^T, so the [N,K,T,2H] concat, the Linear over it and the (sort-based)
 * embedding backward disappear.  m runs over (node,hop), C = 2*max_edge_type + max_hop_num + 1 columns.
 * The caller validates idx against the table sizes.  Tables are staged in LDS (column-split when large).
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_tgs_desc {
    int64_t M;                  /* rows */
    int32_t C, D, R;            /* index columns, feature width, total table rows */
    const uint16_t* idx;        /* device [M, C] */
    const int32_t* col_offset;  /* device [C]: first row of column c's table inside `table` */
    const float* table;         /* device [R, D] contiguous (forward) */
    const float* bias;          /* device [D] or NULL (forward) */
    float* out;                 /* device [M, D], row stride out_stride (forward) */
    int64_t out_stride;
    const float* gout;          /* device [M, D], row stride gout_stride (backward) */
    int64_t gout_stride;
    float* gtable;              /* device [R, D] contiguous, OVERWRITTEN (backward; no atomics: bitwise reproducible) */
    void* workspace; size_t workspace_bytes;   /* backward: >= kpgnn_table_gather_sum_bwd_workspace_bytes(M, D, R) */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
} kpgnn_tgs_desc;

int kpgnn_table_gather_sum_fwd(const kpgnn_tgs_desc* d, kpgnn_stream_t stream);
int kpgnn_table_gather_sum_bwd(const kpgnn_tgs_desc* d, kpgnn_stream_t stream);
size_t kpgnn_table_gather_sum_bwd_workspace_bytes(int64_t M, int32_t D, int32_t R);

/* ------------------------------------------------------------------------------------------------
 * Training-mode BatchNorm1d (+ optional ReLU, + optional residual) over [N, C] rows, forward and backward.  These
 * are the nn.BatchNorm1d calls of KPGINPlusConv.mlp (KPGINplus.py:25-30), GINEConv.mlp (gine.py:31-38) and of
 * the bodies' per-layer norm (models/GNNs.py:104,431): at C ~ 100 and N ~ 50k the framework's kernels take
 * 100-140 us per pass; these stream the tensor at HBM speed around a column-statistics slot (above):
 *   fwd:  [stats pass: sum x, sum x^2 -> stat_slot, skipped when stats_ready - the producer of x filled the slot]
 *         apply pass: mean, invstd (biased var, eps) from the slot, z = [relu]( (x-mean)*invstd*gamma + beta )
 *         (+ residual); running stats updated in place with `momentum` and the unbiased variance, exactly as
 *         nn.BatchNorm1d; with out_slot the statistics of z are accumulated for a following BatchNorm.
 *   bwd:  dy = dz * [pre-activation > 0 if relu];  reduce pass: dbeta = sum dy, dgamma = sum dy*xhat -> stat_slot
 *         (reduce_only stops here: a fused consumer applies them, kpgnn_linear_bn pro 2);
 *         apply pass: dx = gamma*invstd*(dy - dbeta/N - xhat*dgamma/N).
 * Every slot must be all zero when the call is issued and is left dirty.  C <= 256.
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_bn_desc {
    int64_t N;
    int32_t C, relu;
    float eps, momentum;
    const float* x;  int64_t x_stride;      /* device [N,C], row stride in elements */
    const float* gamma; const float* beta;  /* device [C] */
    float* running_mean; float* running_var;/* device [C], updated in place, or NULL */
    float* mean; float* invstd;             /* device [C] outputs (saved for backward) */
    float* z;  int64_t z_stride;            /* device [N,C] output */
    const float* residual; int64_t r_stride;/* optional: z += residual (after the activation) */
    double* stat_slot;                      /* device, kpgnn_stat_slot_bytes(C): statistics of x */
    int32_t stats_ready;                    /* 1: stat_slot already holds sum x / sum x^2 (no stats pass) */
    double* out_slot;                       /* optional (zeroed) slot receiving the statistics of z, or NULL */
    int64_t* num_batches_tracked;           /* device scalar, += 1 per call, or NULL (nn.BatchNorm1d's counter) */
    /* Optional SECOND BatchNorm applied to the result by the same call (the layers' MLP-tail norm followed by the bodies'
     * per-layer norm, KPGINplus.py:25-30 + models/GNNs.py:440-441):
     *   z = bn_outer([relu](bn(x))) + residual
     * with stats_ready = 1 and out_slot a zeroed slot (it receives the statistics of the intermediate).  Two launches: a
     * statistics-only pass over x and one apply pass - the intermediate is never written (one [N,C] store and load less
     * than two kpgnn_bn_fwd calls).  outer_mean / outer_invstd [C] are outputs like mean / invstd; the outer running
     * statistics are updated like the inner ones. */
    const float* outer_gamma; const float* outer_beta;   /* NULL: no second norm */
    float outer_eps, outer_momentum;
    float* outer_running_mean; float* outer_running_var; int64_t* outer_num_batches_tracked;
    float* outer_mean; float* outer_invstd;
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
} kpgnn_bn_desc;

typedef struct kpgnn_bn_bwd_desc {
    int64_t N;
    int32_t C, relu;
    const float* x;  int64_t x_stride;
    const float* dz; int64_t dz_stride;
    const float* gamma; const float* beta; const float* mean; const float* invstd;
    float* dx; int64_t dx_stride;           /* NULL with reduce_only */
    float* dgamma; float* dbeta;            /* device [C] (overwritten); NULL with reduce_only */
    double* stat_slot;                      /* device, kpgnn_stat_slot_bytes(C), zero on entry */
    int32_t reduce_only;
    /* Optional, for z = bn(x) + residual: the residual branch's gradient (= dz) is ADDED in place to this [N,C]
     * buffer by the apply pass (a state read by several layers collects its gradient in one buffer). */
    float* residual_grad; int64_t rg_stride;
    /* Optional, with reduce_only: the STACKED reduce for  x -> z = [relu](bn(x)) -> h = bn_outer(z) (+ residual)  with dz
     * the gradient of h.  outer_mean / outer_invstd [C] are the outer norm's batch statistics (of z); stat_slot is then
     * 4 * kpgnn_stat_slot_bytes(C) (eight column sums, see bn.hip) and is consumed by kpgnn_linear_bn with pro = 3, which
     * applies both norms' backward while it loads its tile.  residual_grad (if set) still receives += dz. */
    const float* outer_mean; const float* outer_invstd;
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
} kpgnn_bn_bwd_desc;

int kpgnn_bn_fwd(const kpgnn_bn_desc* d, kpgnn_stream_t stream);
int kpgnn_bn_bwd(const kpgnn_bn_bwd_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Column-statistics slots.  BatchNorm needs batch-wide column sums; instead of a reduction kernel between the
 * producer and the consumer of a tensor, the producing kernel's blocks add their partial sums (fp64 atomics) to a
 * slot and the consuming kernel finishes mean / invstd (or the backward's dbeta / dgamma) from it in its prologue.
 *   slot = double[KPGNN_STAT_REPLICAS][2][C]  (block b adds to replica b % KPGNN_STAT_REPLICAS: same-address
 *   atomics serialise on this hardware), ALL ZERO before the producing launch; the calls leave it dirty - the
 *   caller zeroes its slots in bulk (one hipMemsetAsync per training step over an arena of slots).
 * Per block the sums are formed in a fixed order; only the order of the <= grid/8 fp64 adds per address varies
 * between runs (below 2^-52 relative: invisible after rounding to fp32 except on exact ties).
 * ---------------------------------------------------------------------------------------------- */
#define KPGNN_STAT_REPLICAS 8
size_t kpgnn_stat_slot_bytes(int32_t C);   /* sizeof(double) * KPGNN_STAT_REPLICAS * 2 * C */

/* ------------------------------------------------------------------------------------------------
 * Weight / bias gradient of y = x W^T + b for tall-skinny activations (N ~ 50k rows, <= 256 features):
 *   dW[o,i] = sum_r dy[r,o] * x[r,i]      db[o] = sum_r dy[r,o]
 * i.e. the backward of the nn.Linear layers behind the aggregation (KPGINplus.py:25-30, gine.py:31-38,
 * KPGIN.py:54,112).  The BLAS library's kernel for this K = N reduction runs at ~7 TFLOP/s (139 us);
 * here each wave streams row PAIRS straight from HBM into v_mfma_f32_32x32x2_f32 (exact fp32: A = dy^T
 * fragment, B = x fragment are plain coalesced row reads, no LDS), keeps a 32 x I strip of dW in
 * accumulators, and per-block partials are added in block order (deterministic).  O, I <= 256.
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_wgrad_desc {
    int64_t N;
    int32_t O, I;               /* out / in features */
    const float* dy; int64_t dy_stride;   /* device [N,O] */
    const float* x;  int64_t x_stride;    /* device [N,I] */
    float* dw;                  /* device [O,I] contiguous (overwritten) */
    float* db;                  /* device [O] (overwritten) or NULL */
    void* workspace; size_t workspace_bytes;  /* >= kpgnn_wgrad_workspace_bytes(O, I) */
    /* Optional transform of x on load: x' = [relu]((x - x_mean) * x_invstd * x_gamma + x_beta), i.e. the Linear's real
     * input when that was a BatchNorm(+ReLU) output the forward never materialised (kpgnn_linear_bn pro 1). */
    const float* x_mean; const float* x_invstd; const float* x_gamma; const float* x_beta;   /* device [I] or all NULL */
    int32_t x_relu;
    /* Optional (host pointer): leave the per-block partials in `workspace` and describe their reduction here instead of
     * launching it (kpgnn_reduce_job above; for kpgnn_linear_wgrad_pair: a->defer, one job for all four outputs).  dw / db
     * are NOT written until the job has run. */
    kpgnn_reduce_job* defer;
    /* Optional ReLU mask of dy on load (device [N,O], rows dy_stride apart): dy' = dy where dy_mask > 0, else 0 - the gradient
     * behind a ReLU whose OUTPUT was saved (the jumping-knowledge projection), without materialising the masked gradient. */
    const float* dy_mask;
    /* Optional (device int32[1]): the number of LIVE rows, <= N.  A launch captured in a hipGraph for a batch CAPACITY of N
     * rows then serves batches of any size up to it (kpgnn_collate leaves the count in its header): rows >= *n_dyn are
     * neither read nor summed.  NULL: all N rows. */
    const int32_t* n_dyn;
    int32_t math;               /* KPGNN_MATH_* (bf16-split product: O <= 128, I <= 128, 16-B aligned operands) */
} kpgnn_wgrad_desc;

size_t kpgnn_wgrad_workspace_bytes(int32_t O, int32_t I);
int kpgnn_linear_wgrad(const kpgnn_wgrad_desc* d, kpgnn_stream_t stream);
/* Two weight gradients with the same (O, I) in ONE launch + one ordered reduction (the two Linears of a
 * Linear-BatchNorm-ReLU x2 MLP): workspace >= 2 * kpgnn_wgrad_workspace_bytes(O, I), taken from a. */
int kpgnn_linear_wgrad_pair(const kpgnn_wgrad_desc* a, const kpgnn_wgrad_desc* b, kpgnn_stream_t stream);
/* `count` such pairs (2 * count <= 16) that share N, n_dyn, O and I, in ONE launch of the bf16-split kernel: the weight
 * gradients of all the MLPs of a backward pass, which nothing reads before the pass ends.  a[p] / b[p] (HOST arrays of
 * descriptors) are what kpgnn_linear_wgrad_pair takes, each pair with its own workspace and its own a[p]->defer job; every
 * pair keeps the slicing of a launch of its own, so dw / db are bit for bit what kpgnn_linear_wgrad_pair gives.  Pairs the
 * bf16-split kernel does not take (KPGNN_MATH_F32, O or I > 128, unaligned operands, mixed shapes) run as `count` pair calls. */
int kpgnn_linear_wgrad_many(const kpgnn_wgrad_desc* const* a, const kpgnn_wgrad_desc* const* b, int32_t count,
                            kpgnn_stream_t stream);
/* Grouped-K weight gradient: the Linear's input was the CONCATENATION of `group` (<= 16) states x_l [N,I] that live in
 * separate tensors (the bodies' jumping-knowledge projection, models/GNNs.py:216-218 / :455-457: cat(h_list) -> Linear):
 * dw [O, group*I] with dw[:, l*I:(l+1)*I] = dy^T x_l, db = sum dy.  d->x is ignored (x_group is a HOST array of device
 * pointers, rows d->x_stride apart); one launch (the column blocks run side by side and share dy) + one ordered reduction.
 * workspace >= kpgnn_wgrad_group_workspace_bytes(O, I, group).  Needs 16-B aligned operands, O % 4 == I % 4 == 0, O <= 128. */
size_t kpgnn_wgrad_group_workspace_bytes(int32_t O, int32_t I, int32_t group);
int kpgnn_linear_wgrad_group(const kpgnn_wgrad_desc* d, const float* const* x_group, int32_t group, kpgnn_stream_t stream);

/* y = x W^T (+ b) for tall-skinny x ([N, I], N ~ 50k, I, O <= 256) on the fp32 matrix cores: the nn.Linear
 * forward of the layers' MLPs, and - called with W^T - their input gradient dx = dy W.  Each wave keeps its
 * 32 x I strip of W in registers as MFMA A-fragments for the whole launch; 32-row tiles of x are staged in LDS
 * (padded pitch: conflict-free transposed reads) and stream through v_mfma_f32_32x32x2_f32; x is read once
 * and y written once (the BLAS library's kernel for this shape takes 24 us, ~3x the HBM time). */
typedef struct kpgnn_linear_desc {
    int64_t N;
    int32_t O, I;
    const float* x; int64_t x_stride;     /* device [N,I] */
    const float* w;                       /* device [O,I] contiguous */
    const float* bias;                    /* device [O] or NULL */
    float* y; int64_t y_stride;           /* device [N,O] */
    int32_t w_transposed;                 /* 1: w is [I,O] (y = x w): dx = dy W needs no transposed copy of W */
    /* Optional blocked output (O > 128 only): output column o is written to block o / y_block_cols, column
     * o % y_block_cols, i.e. y is [O / y_block_cols][N][y_block_cols] with y_stride = y_block_cols and the blocks
     * y_block_stride floats apart.  The input gradient of a jumping-knowledge projection (models/GNNs.py:216-218) then
     * comes out as one contiguous [N,H] matrix per layer state instead of [N, S*H] column slices.  0: plain [N,O]. */
    int32_t y_block_cols; int64_t y_block_stride;
    /* Optional (O > 128 only) ReLU mask of x on load (device [N,I], rows x_stride apart): x' = x where x_mask > 0, else 0. */
    const float* x_mask;
    const int32_t* n_dyn;                 /* optional live-row count (device int32[1], <= N), as in kpgnn_wgrad_desc */
    int32_t math;                         /* KPGNN_MATH_* (bf16-split product: blocked output with y_block_cols <= 128, no bias, N >= 4096) */
    /* Optional device scratch for the bf16-split product (the split copy of w in matrix-fragment order), 16-B aligned,
     * >= kpgnn_linear_split_workspace_bytes(y_block_cols, I, O / y_block_cols).  NULL: the fp32 kernels. */
    void* workspace; size_t workspace_bytes;
} kpgnn_linear_desc;

int kpgnn_linear_fwd(const kpgnn_linear_desc* d, kpgnn_stream_t stream);
/* Bytes of the split copy of `group` weight blocks of [O, I] (O, I <= 128) for the bf16-split kernels; 0 for shapes they do not take. */
size_t kpgnn_linear_split_workspace_bytes(int32_t O, int32_t I, int32_t group);
/* The split copies of up to 64 weight matrices in ONE launch (a body prepares all its MLPs' Linears, both orientations, at the
 * start of a step; kpgnn_linear_bn then takes them with w_split_ready = 1 instead of splitting per call - 34 five-microsecond
 * launches per step otherwise).  Element (k, n) of job i at w[n * wn + k * wk], n < O, k < I; frag: device,
 * >= kpgnn_linear_split_workspace_bytes(O, I, 1), 16-B aligned. */
typedef struct kpgnn_split_job { const float* w; int64_t wn, wk; int32_t O, I; void* frag; } kpgnn_split_job;
int kpgnn_linear_split_many(const kpgnn_split_job* jobs, int32_t n, kpgnn_stream_t stream);

/* y = act(sum_l x_l W[:, l*I:(l+1)*I]^T + b): nn.Linear over the concatenation of `group` (<= 16) states x_l [N,I] that live
 * in SEPARATE tensors - the bodies' jumping-knowledge projection `output_proj(torch.cat(h_list, dim=-1))`
 * (models/GNNs.py:216-218, :455-457, :703-705; ReLU from the Sequential at :58-59) without the concatenated copy: the
 * GEMM's K-loop runs over the state pointers.  w: device [O, group*I] contiguous; y: device [N,O] contiguous.
 * O <= 128, O % 4 == 0, I in {32, 64, 96, 104, 128}, 16-B aligned operands. */
typedef struct kpgnn_linear_group_desc {
    int64_t N;
    int32_t O, I, group;
    const float* x[16]; int64_t x_stride;
    const float* w; const float* bias; float* y;
    int32_t relu;
    const int32_t* n_dyn;                 /* optional live-row count (device int32[1], <= N) */
    int32_t math;                         /* KPGNN_MATH_* (bf16-split product: N >= 4096) */
    void* workspace; size_t workspace_bytes;  /* optional, >= kpgnn_linear_split_workspace_bytes(O, I, group); NULL: the fp32 kernel */
} kpgnn_linear_group_desc;
int kpgnn_linear_group_fwd(const kpgnn_linear_group_desc* d, kpgnn_stream_t stream);

/* The same GEMM with BatchNorm work folded into the tile's load and store phases (csrc/lin_fused.h), so that the
 * Linear-BatchNorm-ReLU x2 MLP (KPGINplus.py:25-30, gine.py:31-38) is 3 launches forward and 5 backward instead of
 * 8 + 14, with 6 fewer passes over [N,H]:
 *   pro 0: x as is.
 *   pro 1: x' = [pro_relu]((x - mean)*invstd*in_gamma + in_beta) applied while the tile is loaded; mean / invstd are
 *          finished from in_slot (sum x, sum x^2 left there by the launch that produced x, epi 1); the launch writes
 *          in_mean / in_invstd and updates running_mean / running_var / num_batches_tracked like kpgnn_bn_fwd.
 *   pro 2: BatchNorm BACKWARD on load: x is dz, x2 the BatchNorm's forward input, in_mean / in_invstd its saved
 *          statistics, in_slot holds (sum dzm, sum dzm*xhat) (kpgnn_bn_bwd reduce_only, or epi 2 of the previous
 *          launch); the tile becomes dy = gamma*invstd*(dzm - s0/N - xhat*s1/N) with dzm = dz * [bn(x2) > 0 if
 *          pro_relu]; dy is also written to xt (the weight-gradient kernel reads it); dgamma / dbeta are written.
 *   pro 3: TWO stacked BatchNorms' backward on load, for  x2 -> z = [pro_relu](bn_in(x2)) -> h = bn_o(z) (+ residual):
 *          x is dh, in_slot the eight sums of kpgnn_bn_bwd's stacked reduce (outer_mean set), in_* the inner norm, o_mean /
 *          o_invstd / o_gamma the outer one; dz is formed in registers (never stored), the tile becomes the inner norm's
 *          dy as in pro 2 (also written to xt); dgamma / dbeta and o_dgamma / o_dbeta are written.  Only with epi 2.
 *   epi 0: y stored as is.
 *   epi 1: + (sum y, sum y^2) per column into out_slot.
 *   epi 2: y is masked by the ReLU of the BatchNorm whose input was e_x (y = 0 where bn_e(e_x) <= 0) and
 *          (sum y, sum y*xhat_e) go to out_slot: the backward reduce of that BatchNorm.
 * x, x2, xt, e_x, y contiguous and 16-B aligned; I in {32, 64, 96, 104, 128}; O % 4 == 0, O <= 128.
 * KPGNN_ELIMIT when the shape is not covered.  Slots: zero on entry (out_slot), dirty on return. */
typedef struct kpgnn_linear_bn_desc {
    int64_t N;
    int32_t O, I;
    const float* x; const float* w; const float* bias; float* y;
    int32_t w_transposed;
    int32_t pro, epi, pro_relu;
    const double* in_slot;
    const float* in_gamma; const float* in_beta;
    float in_eps, momentum;
    float* in_mean; float* in_invstd;
    float* running_mean; float* running_var; int64_t* num_batches_tracked;
    const float* x2; float* xt; float* dgamma; float* dbeta;
    double* out_slot;
    const float* e_x; const float* e_mean; const float* e_invstd; const float* e_gamma; const float* e_beta;
    const float* o_mean; const float* o_invstd; const float* o_gamma; float* o_dgamma; float* o_dbeta;   /* pro 3 */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
    int32_t math;               /* KPGNN_MATH_* (bf16-split product: N >= 4096, I <= 104, a workspace; pro >= 2 then needs xt) */
    void* workspace; size_t workspace_bytes;   /* optional, 16-B aligned, >= kpgnn_linear_split_workspace_bytes(O, I, 1); NULL: fp32 kernel */
    int32_t w_split_ready;      /* 1: workspace already holds the split copy of w in this orientation (kpgnn_linear_split_many) */
} kpgnn_linear_bn_desc;

int kpgnn_linear_bn(const kpgnn_linear_bn_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation mode (model.eval() under torch.no_grad(): the reference's val() / test() loops, train_ZINC.py:50-52,
 * train_qm9.py:103-105, train_graph_property.py:52-54).  With running statistics a BatchNorm1d is a per-column map
 *   bn(v) = (v - running_mean) * rsqrt(running_var + eps) * gamma + beta
 * so no grid-wide reduction sits between the two Linears of the layers' MLP.  The running statistics (and the module's
 * num_batches_tracked, which is not even passed) are only READ.
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_bn_running {
    const float* gamma; const float* beta;                  /* device [C] */
    const float* running_mean; const float* running_var;    /* device [C] */
    float eps;
} kpgnn_bn_running;

/* y = [outer(] relu(bn2(relu(bn1(x W0^T + b0)) W3^T + b3)) [)] [+ residual] in ONE launch (csrc/mlp_eval.hip): the
 * Linear-BatchNorm-ReLU x2 MLP of KPGINPlusConv / GINEConv (KPGINplus.py:25-30, gine.py:31-38), the body's per-layer norm
 * (models/GNNs.py:440-441) and its residual add.  x is read once, y written once; relu(bn1(.)) lives in LDS only.  Each
 * norm is applied after the bias, in the order above (the scale is NOT folded into the weights); the kernel forms the
 * per-column coefficients in its prologue.  I and O in {32, 64, 96, 104, 128}, row strides multiples of 4, 16-B aligned
 * operands: KPGNN_ELIMIT otherwise.  The outer norm is absent when outer.gamma is NULL. */
typedef struct kpgnn_mlp_eval_desc {
    int64_t N;
    int32_t I, O;
    const float* x; int64_t x_stride;       /* device [N,I], row stride in elements */
    const float* w0; const float* b0;       /* device [O,I] contiguous; [O] or NULL */
    const float* w3; const float* b3;       /* device [O,O] contiguous; [O] or NULL */
    kpgnn_bn_running bn1, bn2, outer;
    const float* residual; int64_t r_stride;/* optional device [N,O] */
    float* y; int64_t y_stride;             /* device [N,O] */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
    int32_t math;               /* KPGNN_MATH_*; both settings run the fp32 matrix instruction (there is no bf16-split route) */
} kpgnn_mlp_eval_desc;
int kpgnn_mlp_eval(const kpgnn_mlp_eval_desc* d, kpgnn_stream_t stream);

/* z = [relu](bn(x)) [+ residual] over [N, C] rows with running statistics, C <= 256 (csrc/bn_eval.hip): the bodies'
 * per-layer norm of GNN / GNNPrime and the MLP norms of widths kpgnn_mlp_eval does not take.  One streaming launch. */
typedef struct kpgnn_bn_eval_desc {
    int64_t N;
    int32_t C, relu;
    const float* x; int64_t x_stride;       /* device [N,C], row stride in elements */
    kpgnn_bn_running bn;
    const float* residual; int64_t r_stride;/* optional: z += residual (after the activation) */
    float* z; int64_t z_stride;             /* device [N,C] output */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
} kpgnn_bn_eval_desc;
int kpgnn_bn_eval(const kpgnn_bn_eval_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Graph readout over a collated batch (models/GraphRegression.py:46-51: PyG global_add_pool / global_mean_pool):
 *   out[g,:] = sum (mode 0) or mean (mode 1) of x[n,:] over the nodes n of graph g;  gx[n,:] = gout[batch[n],:] (/ count)
 * The nodes of a graph are contiguous (graph_ptr[g] .. graph_ptr[g+1]), rows are added in node order: bitwise
 * reproducible, unlike a scatter with fp32 atomics.  One launch per direction.  Rows at or beyond the live count are
 * never read, and the mean divides by a graph's live rows in both directions, even where graph_ptr runs past the count.
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_pool_desc {
    int64_t N;                  /* nodes */
    int32_t G, D, mode;         /* graphs, feature width, 0 = sum / 1 = mean */
    const int32_t* graph_ptr;   /* device [G+1], non-decreasing, graph_ptr[G] == N */
    const int64_t* batch;       /* device [N]: graph of node n (backward only) */
    const float* x; int64_t x_stride;      /* device [N,D] (forward) */
    float* out;                 /* device [G,D] contiguous (forward) */
    const float* gout;          /* device [G,D] contiguous (backward) */
    float* gx; int64_t gx_stride;          /* device [N,D] (backward, overwritten) */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
} kpgnn_pool_desc;

int kpgnn_segment_pool_fwd(const kpgnn_pool_desc* d, kpgnn_stream_t stream);
int kpgnn_segment_pool_bwd(const kpgnn_pool_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Max graph readout (csrc/pool_max.hip; models/GraphClassification.py:24-34 "max": PyG 2.1.0 global_max_pool, which is
 * torch_scatter.scatter_max).  With live = *n_dyn when given, else N:
 *   out[g,c] = max of x[n,c] over graph_ptr[g] <= n < min(graph_ptr[g+1], live)
 *   arg[g,c] = the LOWEST such row n that attains the max: the tie rule of torch_scatter's CPU kernel and of kpgnn_jk_reduce_*'s max,
 *              which gives a tie to the lowest slot.  One winner per (graph, column).
 * NaN: a NaN in a live row makes the column's result NaN (as amax does) and arg the FIRST NaN row; once a NaN is taken,
 * nothing replaces it.  An empty graph gives out = -inf, arg = -1, and no gradient flows.  Rows at or beyond graph_ptr[G]
 * and rows at or beyond the live count are never read.
 * Backward, for every live row n with g = batch[n]:  gx[n,c] = (arg[g,c] == n) ? gout[g,c] : +0.0f.  Each live row is
 * written exactly once, dead rows are not written; there is no zero-fill launch and there are no atomics, so both
 * directions are bitwise reproducible.  One launch per direction.
 * D <= 1024 and ceil(D / vec) <= 256 lanes (KPGNN_ELIMIT beyond), vec as for kpgnn_segment_pool_*.  G == 0 (forward) and
 * N == 0 (backward) return KPGNN_OK without a launch.
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_pool_max_desc {
    int64_t N;                  /* nodes */
    int32_t G, D;               /* graphs, feature width */
    const int32_t* graph_ptr;   /* device [G+1], non-decreasing (forward) */
    const int64_t* batch;       /* device [N]: graph of node n (backward only) */
    const float* x; int64_t x_stride;      /* device [N,D] (forward) */
    float* out;                 /* device [G,D] contiguous (forward) */
    int32_t* arg;               /* device [G,D] contiguous winners: row index, -1 for an empty graph; NULL in forward: not kept */
    const float* gout;          /* device [G,D] contiguous (backward) */
    float* gx; int64_t gx_stride;          /* device [N,D] (backward, live rows overwritten) */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
} kpgnn_pool_max_desc;

int kpgnn_segment_max_fwd(const kpgnn_pool_max_desc* d, kpgnn_stream_t stream);
int kpgnn_segment_max_bwd(const kpgnn_pool_max_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Virtual node (csrc/virtual_node.hip; models/GNNs.py:196-199,227-230: h + vn[batch], global_add_pool(h) + vn):
 *   out[n,:]    = x[n,:] + v[g,:]               for the nodes n of graph g (graph_ptr[g] .. graph_ptr[g+1])
 *   pooled[g,:] = sum_n out[n,:] + v[g,:]       (optional; an empty graph gives v[g,:])
 * One launch, x read once, out written once, rows added in node order (bitwise reproducible, no atomics).  The work is driven
 * by graph_ptr: a row at or beyond graph_ptr[G] (and beyond *n_dyn when given) is neither read nor written.
 * The backward is the same entry: with gout = dL/dout and gp = dL/dpooled, gx[n] = gout[n] + gp[g] and
 * gv[g] = sum_n gx[n] + gp[g], i.e. (x := gout, v := gp) -> (out := gx, pooled := gv).  D <= 256 (KPGNN_ELIMIT beyond).
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_vn_desc {
    int64_t N;                  /* node rows of x / out */
    int32_t G, D;               /* graphs, feature width */
    const int32_t* graph_ptr;   /* device [G+1], non-decreasing, graph_ptr[G] == the live node count */
    const float* x; int64_t x_stride;      /* device [N,D] */
    const float* v; int64_t v_stride;      /* device [G,D]; stride 0: one row for every graph */
    float* out; int64_t out_stride;        /* device [N,D]; must not overlap x */
    float* pooled;              /* device [G,D] contiguous, or NULL: not wanted */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
} kpgnn_vn_desc;

int kpgnn_vn_add_pool(const kpgnn_vn_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Attention readout (csrc/attn_pool.hip): PyG's AttentionalAggregation(gate_nn = nn.Linear(D, 1)) over the contiguous node
 * ranges of graph_ptr (models/GraphClassification.py:31-32, models/GraphRegression.py "attention"):
 *   gate[n] = x[n] . w + bias[0]      alpha[n] = exp(gate[n] - max_g) / (sum_{m in g} exp(gate[m] - max_g) + 1e-16)
 *   out[g,:] = sum_{n in g} alpha[n] x[n,:]          (an empty graph gives a zero row)
 * Forward: one launch, x read once; alpha [N] is kept for the backward.  Backward (s_g = gout[g] . out[g]):
 *   dgate[n] = alpha[n] (gout[g] . x[n] - s_g)   gx[n,:] = alpha[n] gout[g,:] + dgate[n] w   dw = sum_n dgate[n] x[n,:]
 *   db = sum_n dgate[n]
 * in one launch plus one fixed-order reduce of the per-block partial sums (none when one block covers the batch).  Rows are
 * added in node order, blocks in block order: bitwise reproducible.  D <= 256 (KPGNN_ELIMIT beyond).
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_attn_pool_desc {
    int64_t N;                  /* nodes */
    int32_t G, D;               /* graphs, feature width */
    const int32_t* graph_ptr;   /* device [G+1], non-decreasing, graph_ptr[G] == the live node count */
    const float* x; int64_t x_stride;      /* device [N,D] */
    const float* w;             /* device [D]: gate_nn.weight (the caller checks that it has D entries) */
    const float* bias;          /* device [1]: gate_nn.bias, or NULL (forward only) */
    float* alpha;               /* device [N]: written by the forward, read by the backward */
    float* out;                 /* device [G,D] contiguous: written by the forward, read by the backward */
    const float* gout;          /* device [G,D] contiguous (backward) */
    float* gx; int64_t gx_stride;          /* device [N,D] (backward, overwritten; NULL: skipped) */
    float* dw;                  /* device [D] (backward, overwritten) */
    float* db;                  /* device [1] (backward, overwritten; NULL: skipped) */
    void* workspace; size_t workspace_bytes;   /* backward: kpgnn_attn_pool_workspace_bytes(G, D) */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
} kpgnn_attn_pool_desc;

size_t kpgnn_attn_pool_workspace_bytes(int32_t G, int32_t D);
int kpgnn_attn_pool_fwd(const kpgnn_attn_pool_desc* d, kpgnn_stream_t stream);
int kpgnn_attn_pool_bwd(const kpgnn_attn_pool_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * nn.Linear with a narrow output (csrc/head_linear.hip): the classifiers and node-level regressors of
 * models/GraphClassification.py:37, NodeClassification.py:21-24 and NodeRegression.py:18.
 *   y[M,O] = x[M,I] W^T + bias          dx = dy W      dw = dy^T x      db = sum_m dy[m,:]
 * 1 <= O <= 32 and I <= 1024 (O < 1 or I < 1: KPGNN_EINVAL; O > 32 or I > 1024: KPGNN_ELIMIT); M is any row count, 0 included.
 * I is the width of x AND of w: a caller holding an nn.Linear checks in_features against x before the call.  Forward: one launch.  Backward: one launch in
 * which every block covers a tile of rows and leaves a partial [O, I] (+ [O]) slab, plus one fixed-order reduce of the slabs
 * (none when one block covers all rows): bitwise reproducible.
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_head_linear_desc {
    int64_t M;                  /* rows */
    int32_t O, I;               /* out_features, in_features */
    const float* x; int64_t x_stride;      /* device [M,I] */
    const float* w;             /* device [O,I] contiguous */
    const float* bias;          /* device [O] or NULL (forward) */
    float* y; int64_t y_stride;            /* device [M,O] (forward) */
    const float* dy; int64_t dy_stride;    /* device [M,O] (backward) */
    float* dx; int64_t dx_stride;          /* device [M,I] (backward, overwritten; NULL: skipped) */
    float* dw;                  /* device [O,I] contiguous (backward, overwritten) */
    float* db;                  /* device [O] (backward, overwritten; NULL: skipped) */
    void* workspace; size_t workspace_bytes;   /* backward: kpgnn_head_linear_workspace_bytes(M, O, I) */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= M; kpgnn_wgrad_desc explains); NULL: all M rows */
} kpgnn_head_linear_desc;

size_t kpgnn_head_linear_workspace_bytes(int64_t M, int32_t O, int32_t I);
int kpgnn_head_linear_fwd(const kpgnn_head_linear_desc* d, kpgnn_stream_t stream);
int kpgnn_head_linear_bwd(const kpgnn_head_linear_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Classification loss (csrc/class_loss.hip): F.nll_loss(F.log_softmax(logits, -1), y), which F.cross_entropy and
 * nn.CrossEntropyLoss() reduce to (train_TU.py:45-46, train_EXP.py:81-82, train_CSL.py:41, train_SR.py:38).  One launch:
 *   loss[0] = sum (reduction 1) or mean (reduction 0) over the counted rows of  logsumexp(logits[m,:]) - logits[m, y[m]]
 *   dlogits[m,:] = (softmax(logits[m,:]) - onehot(y[m])) * (1 or 1 / count)         (NULL: skipped)
 *   correct[0] = number of counted rows whose arg-max is y[m]                         (NULL: skipped)
 * A row whose label is outside [0, C) is NOT counted, the way ignore_index = -100 is: no loss term, a zero gradient row, not
 * in the mean's denominator, and the label is never used as an index.  This is deliberate: the framework asserts on the
 * device for such a label, which takes the process down; here it is data.  Max-subtracted, one block, fixed summation order:
 * bitwise reproducible.  C <= 1024 (KPGNN_ELIMIT beyond).
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_nll_loss_desc {
    int64_t M;                  /* rows (0: loss = 0 for sum, 0 / 0 for mean) */
    int32_t C;                  /* classes */
    int32_t reduction;          /* 0 = mean, 1 = sum */
    const float* logits; int64_t logits_stride;   /* device [M,C] */
    const int64_t* y;           /* device [M] labels */
    float* loss;                /* device [1] */
    float* dlogits; int64_t dlogits_stride;       /* device [M,C] (overwritten; NULL: skipped) */
    int32_t* correct;           /* device [1] (NULL: skipped) */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= M; kpgnn_wgrad_desc explains); NULL: all M rows */
} kpgnn_nll_loss_desc;

int kpgnn_nll_loss(const kpgnn_nll_loss_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Projected peripheral-feature tables (csrc/enc_tables.hip): for every encoder e (a FeatureConcatEncoder: per-column
 * nn.Embedding -> concat -> Linear, layers/feature_encoder.py:37-67, gated by squash(pew / pcw), models/GNNs.py:172-179 /
 * :393-400 / :637-644) and every component c of it
 *     table[rows of c, :] = squash(gate_e) * Emb_c.weight @ W_e[:, cH:(c+1)H]^T        bias = sum_e squash(gate_e)*mult_e*b_e
 * so that the features are one gather-sum over `table` (kpgnn_table_gather_sum).  One launch per direction instead of
 * ~14 + ~28 framework launches on tiny tensors.  Components are listed encoder by encoder; H <= 256; <= 16 components,
 * <= 4 encoders.  enc_squash: 0 sigmoid (GNN, GNNPrime), 1 tanh (GNNPlus).  enc_mult: how many index columns share the
 * encoder's bias (T edge types for the edge encoder, 1 for the configuration encoder).
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_enc_tables_desc {
    int32_t H, num_components, num_encoders;
    const float* comp_emb[16]; int32_t comp_rows[16]; int32_t comp_encoder[16];
    const float* enc_w[4]; const float* enc_b[4]; const float* enc_gate[4]; float enc_mult[4]; int32_t enc_squash[4];
    float* table; float* pre; float* bias;       /* forward outputs: [R,H], [R,H] (un-gated, kept for backward), [H] */
    const float* gtable; const float* gbias;     /* backward inputs (plus pre) */
    float* comp_gemb[16];                        /* backward outputs: like comp_emb */
    float* enc_gw[4]; float* enc_gb[4]; float* enc_ggate[4];
} kpgnn_enc_tables_desc;

int kpgnn_enc_tables_fwd(const kpgnn_enc_tables_desc* d, kpgnn_stream_t stream);
int kpgnn_enc_tables_bwd(const kpgnn_enc_tables_desc* d, kpgnn_stream_t stream);

/* Identifier of the capture the stream is part of (hipStreamGetCaptureInfo), 0 when it is not capturing: lets a
 * caller that zeroes its statistics slots once per step put that memset into every graph it captures. */
int kpgnn_stream_capture_id(kpgnn_stream_t stream, uint64_t* id);

/* ------------------------------------------------------------------------------------------------
 * Attention hop-combine (reference layers/combine.py:8-27): a 1-layer bidirectional LSTM with hidden size K
 * over the K hop slots scores each slot, softmax over slots, weighted sum of the slots:
 *     score[n,t] = sum_c ( h_fwd[n,t,c] + h_bwd[n,t,c] ),  w = softmax_t(score),  out[n,:] = sum_t w[n,t] x[n,t,:]
 * The input projection  gin = x W_ih^T + b_ih + b_hh  ([N*K, D] x [D, 8K], both directions side by side) is a plain
 * GEMM and stays on the matrix-core library; these entry points do the rest:
 *   fwd: the K-step recurrence, one thread per (node, direction), W_hh wave-uniform, state in registers; then
 *        softmax + weighted sum.  Saves the gate activations and cell states (5K floats per step) for backward.
 *   bwd: d(out) -> dw, dx (direct part), softmax backward, BPTT in registers -> dgin [N*K, 8K] and h_prev [N*K,2,K]
 *        (dW_ih, db, dW_hh are then weight-gradient GEMMs of dgin: kpgnn_linear_wgrad; dx += dgin W_ih).
 * K <= 16.
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_attn_desc {
    int32_t N, K, D;
    const float* x; int64_t x_sn, x_sk;     /* device [N,K,D] */
    const float* gin;                       /* device [N,K,2,4K] contiguous: input projections incl. both biases */
    const float* whh;                       /* device [2,4K,K] contiguous: weight_hh_l0, weight_hh_l0_reverse */
    float* acts;                            /* device [2,N,K,5K]: i,f,g,o (activated), c per step (fwd: out, bwd: in) */
    float* hsum;                            /* device [2,N,K] workspace: sum_c h */
    float* w;                               /* device [N,K] softmax weights (fwd: out, bwd: in) */
    float* out;                             /* device [N,D] (fwd) */
    /* backward only */
    const float* gout;                      /* device [N,D] */
    float* dx;                              /* device [N,K,D] contiguous: receives the DIRECT part w[n,t]*gout[n,:] */
    float* ds;                              /* device [N,K] workspace: d(score) */
    float* dgin;                            /* device [N,K,2,4K] */
    float* hprev;                           /* device [N,K,2,K]: h_{t-1} of each step, for dW_hh */
} kpgnn_attn_desc;

int kpgnn_attn_fwd(const kpgnn_attn_desc* d, kpgnn_stream_t stream);
int kpgnn_attn_bwd(const kpgnn_attn_desc* d, kpgnn_stream_t stream);

/* The same operator for K <= 8 and D % 4 == 0, D <= 128 with the input projection inside (no gin tensor, no library
 * GEMM in the forward): a wave owns 32 nodes of one direction, takes the projection W_ih x_t and the recurrent
 * product W_hh h_{t-1} transposed (gates x nodes) on the fp32 matrix instruction - the accumulator layout then IS
 * "the four gates of four hidden units of my node" - and runs the recurrence / BPTT on its accumulators
 * (csrc/attention.hip, "scan form").  Takes the nn.LSTM parameters as they are ([4K,D], [4K,K], [4K] per direction;
 * index 0 = forward, 1 = reverse; reference layers/combine.py:17).
 *   fwd: hsum, w, out as kpgnn_attn_fwd; acts in the kernel's own lane-contiguous layout; w_pad [64, D] = the two
 *        W_ih with the hidden size padded to 8 (row dir*32 + gate*8 + unit, zero rows for unit >= K).
 *   bwd: ds as kpgnn_attn_bwd; dgin [N*K, 64] in the padded layout (column dir*32 + gate*8 + unit, zeros in the padding);
 *        dwhh_pad [2,32,8] = the recurrent weight gradient sum dg h_prev^T, taken inside the walk (the one product that contracts
 *        over nodes: operands transposed through LDS per wave); then the COMPLETE dx[n,t,:] = w[n,t] gout[n,:] +
 *        dgin[(n,t),:] w_pad in one launch (w_pad from the forward).  dW_pad = dgin^T x and db_pad = sum dgin are a plain
 *        weight-gradient product (kpgnn_linear_wgrad); kpgnn_attn_scan_unpad drops the padding:
 *        dw [2,4K,D], db [2,4K], dwhh [2,4K,K] from dw_pad [64,D], db_pad [64], dwhh_pad [2,32,8]. */
typedef struct kpgnn_attn_scan_desc {
    int32_t N, K, D;
    const float* x; int64_t x_sn, x_sk;     /* device [N,K,D], 16-byte aligned, strides multiples of 4 */
    const float* w_ih[2];                   /* device [4K,D] weight_ih_l0, weight_ih_l0_reverse */
    const float* w_hh[2];                   /* device [4K,K] */
    const float* b_ih[2];                   /* device [4K] */
    const float* b_hh[2];                   /* device [4K] */
    float* acts;                            /* device [ceil(N/32)*2*K*20*64] (fwd: out, bwd: in) */
    float* hsum;                            /* device [2,N,K] workspace */
    float* w;                               /* device [N,K] softmax weights (fwd: out, bwd: in) */
    float* out;                             /* device [N,D] (fwd) */
    float* w_pad;                           /* device [64,D] (fwd: out, bwd: in) */
    /* backward only */
    const float* gout;                      /* device [N,D] */
    float* dx;                              /* device [N,K,D] contiguous, complete */
    float* ds;                              /* device [N,K] workspace */
    float* dgin;                            /* device [N*K,64] */
    float* whh_slab;                        /* device workspace, ceil(N/32) * 512 floats: per-tile partials of dW_hh */
    float* dwhh_pad;                        /* device [2,32,8] out: dW_hh of both directions, hidden size padded to 8 */
} kpgnn_attn_scan_desc;

int kpgnn_attn_scan_fwd(const kpgnn_attn_scan_desc* d, kpgnn_stream_t stream);
int kpgnn_attn_scan_bwd(const kpgnn_attn_scan_desc* d, kpgnn_stream_t stream);
int kpgnn_attn_scan_unpad(const float* dw_pad, const float* db_pad, const float* dwhh_pad, float* dw, float* db, float* dwhh,
                          int32_t K, int32_t D, kpgnn_stream_t stream);

/* Geometric hop-combine weights (reference layers/combine.py:43-50, GeometricCombine.geometric_distribution):
 *     a = sigmoid(alpha[d]);  theta[k,d] = softmax_k( a (1-a)^k )            theta: device [K,D], alpha: device [D]
 * and the backward  galpha[d] = d/dalpha sum_k gtheta[k,d] theta[k,d].  One launch each (the op-by-op version is
 * 6 + 20 launches per layer on a ~100-element tensor). */
int kpgnn_geo_theta_fwd(const float* alpha, int32_t K, int32_t D, float* theta, kpgnn_stream_t stream);
int kpgnn_geo_theta_bwd(const float* alpha, const float* theta, const float* gtheta, int32_t K, int32_t D,
                        float* galpha, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * KP-GIN per-hop MLP + geometric hop-combine + combine_proj (reference layers/KPGIN.py:106-112, combine.py:52-58):
 *     h1[n,k,:] = relu( s[n,k,:] W1[k] + b1[k] )      h2[n,k,:] = relu( h1[n,k,:] W2[k] + b2[k] )
 *     comb[n,:] = sum_k theta[k,:] * h2[n,k,:]        (only with theta; otherwise h2 [N,K,DO] is the result)
 *     out[n,:]  = comb[n,:] Wc^T + bc                 (only with wc: H outputs; otherwise comb [N,DO] is the result)
 * The reference runs this as two batched matmuls over [K, N, dk] with dk = hidden/K (13 for ZINC, 20 for QM9,
 * 6 for K=16), a broadcast multiply + sum and an nn.Linear(dk, hidden) - all far too narrow for a BLAS tile.  Here a
 * block stages a 32-node tile of s in LDS, every wave runs v_mfma_f32_16x16x4_f32 (exact fp32) over hop slots with
 * the zero-padded weights in LDS, and the activations, the combine, the projection and (backward) every weight, bias
 * and theta gradient plus d(s) come out of the same tile residency: s, h1, h2, out cross HBM once per direction.
 *   fwd: writes h1, h2 (saved for backward) and out ([N,H] with wc, [N,DO] with theta only).
 *   bwd: gout is [N,H] with wc, [N,DO] with theta only, [N,K,DO] otherwise; writes gs [N,K,DI] and
 *        gflat = [ dW1 (K*DI*DO) | db1 (K*DO) | dW2 (K*DO*DO) | db2 (K*DO) | dtheta (K*DO, with theta) |
 *                  dWc (H*DO) | dbc (H) (with wc) ],  per-block partials added in block order (deterministic).
 * Limits (KPGNN_ELIMIT beyond): DI, DO <= 32; K * ceil(max(DI,DO)/16)^2 <= 32; H <= 1024 and
 * ceil(H/16) * ceil(max(DI,DO)/16) <= 32; K*max(DI,DO) <= 1024; the LDS footprint (<= 160 KB).
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_hop_mlp_desc {
    int64_t N;
    int32_t K, DI, DO;
    int32_t H;                              /* combine_proj outputs; 0 = no projection */
    const float* s;                         /* device [N,K,DI] contiguous */
    const float* w1; const float* b1;       /* device [K,DI,DO], [K,DO] */
    const float* w2; const float* b2;       /* device [K,DO,DO], [K,DO] */
    const float* theta;                     /* device [K,DO] or NULL */
    const float* wc; const float* bc;       /* device [H,DO], [H] (bc may be NULL); wc needs theta */
    float* h1; float* h2;                   /* device [N,K,DO] contiguous (fwd: out, bwd: in) */
    float* out;                             /* device [N,H] / [N,DO] (fwd, with theta) */
    /* backward only */
    const float* gout;                      /* device [N,H] / [N,DO] / [N,K,DO] */
    float* gs;                              /* device [N,K,DI] */
    float* gflat;                           /* device, layout above */
    void* workspace; size_t workspace_bytes;  /* >= kpgnn_hop_mlp_workspace_bytes(N, K, DI, DO, H) */
} kpgnn_hop_mlp_desc;

/* 0 = the shape is not covered (the caller keeps its BLAS path). */
size_t kpgnn_hop_mlp_workspace_bytes(int64_t N, int32_t K, int32_t DI, int32_t DO, int32_t H);
int kpgnn_hop_mlp_fwd(const kpgnn_hop_mlp_desc* d, kpgnn_stream_t stream);
int kpgnn_hop_mlp_bwd(const kpgnn_hop_mlp_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * KP-GraphSAGE tail: per-hop projection of [x | x_n], ReLU, L2-normalise (+ geometric hop-combine (+ combine_proj))
 * (reference layers/KPGraphSAGE.py:88-96, combine.py:52-58).  With W [K, 2*DI, DO]:
 *     z[n,k,:]  = x[n,k,:] W[k][:DI] + xn[n,k,:] W[k][DI:] + b[k]      (the concatenation is never materialised)
 *     r = max(z, 0);  nrm[n,k] = sqrt(sum_j r[n,k,j]^2);  rinv[n,k] = 1 / max(nrm, 1e-12)
 *     y[n,k,:]  = r[n,k,:] / max(nrm[n,k], 1e-12)                      (F.normalize(relu(z), p=2, dim=-1); by division:
 *                                                                       a row with one positive entry is exactly 1)
 *     comb[n,:] = sum_k theta[k,:] * y[n,k,:]        (only with theta; otherwise y [N,K,DO] is the result)
 *     out[n,:]  = comb[n,:] Wc^T + bc                (only with wc: H outputs; otherwise comb [N,DO] is the result)
 * The same plan as kpgnn_hop_mlp_*: a block keeps a 32-node tile of x and of xn in LDS next to the zero-padded weights,
 * every product is v_mfma_f32_16x16x4_f32 (exact fp32), the row norm is summed in the accumulator registers, and x, xn, y,
 * out cross HBM once per direction.
 *   fwd: writes y and rinv (saved for backward) and out ([N,H] with wc, [N,DO] with theta only).  With theta, y and rinv
 *        may both be NULL (evaluation: nothing is written but out; out has the same bits either way).
 *   bwd: gout is [N,H] with wc, [N,DO] with theta only, [N,K,DO] otherwise.  With gy = d(y):
 *            gr = rinv * (gy - y <gy, y>)  where nrm > 1e-12,   gr = gy * 1e12  where the clamp was active
 *            gz = gr * [y > 0]             (a slot whose ReLU output is all zero: y = 0 and gz = 0, no NaN / Inf)
 *        writes gx = gz W[k][:DI]^T and gxn = gz W[k][DI:]^T (two [N,K,DI] tensors) and
 *        gflat = [ dW (K*2DI*DO) | db (K*DO) | dtheta (K*DO, with theta) | dWc (H*DO) | dbc (H) (with wc) ],
 *        per-block partials added in block order (deterministic, no atomics).
 * Every row's y / out / gx / gxn depends on that row alone (not on N or the grid).
 * Limits (KPGNN_ELIMIT beyond): DI, DO <= 32; K * ceil(max(DI,DO)/16)^2 <= 32; H <= 1024 and
 * ceil(H/16) * ceil(max(DI,DO)/16) <= 32; K*max(DI,DO) <= 1024; the LDS footprint (<= 160 KB).
 * N == 0: fwd launches nothing, bwd zero-fills gflat.  No dynamic row count (n_dyn).
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_sage_tail_desc {
    int64_t N;
    int32_t K, DI, DO;
    int32_t H;                              /* combine_proj outputs; 0 = no projection (H > 0 exactly when wc is given) */
    const float* x; const float* xn;        /* device [N,K,DI] contiguous: the (path-encoded) input and its aggregation */
    const float* w; const float* b;         /* device [K,2*DI,DO], [K,DO] */
    const float* theta;                     /* device [K,DO] or NULL */
    const float* wc; const float* bc;       /* device [H,DO], [H] (bc may be NULL); wc needs theta */
    float* y;                               /* device [N,K,DO] contiguous (fwd: out, bwd: in) */
    float* rinv;                            /* device [N,K] (fwd: out, bwd: in) */
    float* out;                             /* device [N,H] / [N,DO] (fwd, with theta) */
    /* backward only */
    const float* gout;                      /* device [N,H] / [N,DO] / [N,K,DO] */
    float* gx; float* gxn;                  /* device [N,K,DI] each */
    float* gflat;                           /* device, layout above */
    void* workspace; size_t workspace_bytes;  /* >= kpgnn_sage_tail_workspace_bytes(N, K, DI, DO, H) */
} kpgnn_sage_tail_desc;

/* Backward grid x slab width x 4 bytes, the slab width counted with the dtheta block:
 * K*2*DI*DO + 2*K*DO + H*DO + H floats.  0 = the shape is not covered (the caller keeps the framework tail). */
size_t kpgnn_sage_tail_workspace_bytes(int64_t N, int32_t K, int32_t DI, int32_t DO, int32_t H);
int kpgnn_sage_tail_fwd(const kpgnn_sage_tail_desc* d, kpgnn_stream_t stream);
int kpgnn_sage_tail_bwd(const kpgnn_sage_tail_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Dropout (+ residual) with counter-based masks (csrc/dropout.hip; models/GNNs.py, the self.dropout sites):
 *   fwd:  out[n,c] = keep ? fmaf(x[n,c], scale, residual[n,c]) : residual[n,c]      (no residual: x * scale / 0)
 *   bwd:  out[n,c] = keep ? x[n,c] * scale : 0         with x := dL/dout, out := dL/dx; the residual branch's gradient is
 *         dL/dout itself and is nobody's launch
 * Mask: the LOGICAL element e = n * C + c (int64: independent of strides and of the capacity N) is kept iff
 *   word (e & 3) of Philox4x32-10(counter = (lo32(e >> 2), hi32(e >> 2), lo32(call), hi32(call)), key = (lo32(seed), hi32(seed)))
 *   >= thr (unsigned), with the standard constants (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
 *   0xBB67AE85).  The host forms thr = (uint32) min(4294967295, floor(p * 2^32)) and scale = (float)(1 / (1 - p)) in double.
 * Call ids live on the device.  fwd reads (seed, calls) from `state`, uses `calls` as its call id, leaves that id in call_io
 * and advances state[1] by one once every block has read it (the block that finishes last does it: `ticket` counts the
 * arrivals and is zero again when the launch ends).  Nothing about the id travels through the arguments, so a replayed
 * hipGraph draws a fresh mask on every replay.  bwd recomputes the mask from state[0] and call_io[0] and leaves state alone.
 * Launches that share a `state` must be ordered on the device (one stream, or one captured graph without parallel branches
 * through them).  Rows at or beyond *n_dyn are neither read nor written; N == 0 launches nothing and consumes no id.
 * No limit on C: 16-byte accesses when C % 4 == 0, every stride is a multiple of 4 and every pointer is 16-byte aligned; a
 * scalar path otherwise (one Philox call per element there: four times the arithmetic, correct but not tuned).  out may be x (or the residual) itself.
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_dropout_desc {
    int64_t N; int32_t C;                          /* rows (capacity with n_dyn), row width (>= 1) */
    const float* x; int64_t x_stride;              /* device [N,C], row stride in floats (>= C) */
    float* out; int64_t out_stride;                /* device [N,C] */
    const float* residual; int64_t r_stride;       /* device [N,C] or NULL (fwd only; bwd ignores it) */
    uint32_t thr; float scale;
    int64_t* state;                                /* device int64[2]: seed, calls */
    int64_t* call_io;                              /* device int64[1]: fwd writes its call id, bwd reads it */
    int64_t* ticket;                               /* device int64[1] (fwd only): the arrival counter of the call-id advance.  The
                                                    * caller zeroes it once; every completed launch leaves it zero again.  A launch
                                                    * that was aborted leaves it non-zero: zero it again before the next one
                                                    * (kp_gnn_amd.ops.dropout_seed does) */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
} kpgnn_dropout_desc;

int kpgnn_dropout_fwd(const kpgnn_dropout_desc* d, kpgnn_stream_t stream);
int kpgnn_dropout_bwd(const kpgnn_dropout_desc* d, kpgnn_stream_t stream);

/* The keep mask (1 = kept) of an explicit (seed, call) as uint8 [N,C] contiguous; consumes no call id.  The test and debug
 * surface of the definition above. */
typedef struct kpgnn_dropout_mask_desc {
    int64_t seed, call;
    int64_t N; int32_t C;
    uint32_t thr;
    uint8_t* mask;                                 /* device [N,C] */
} kpgnn_dropout_mask_desc;

int kpgnn_dropout_mask(const kpgnn_dropout_mask_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Jumping-knowledge reduce over the S = num_layer + 1 states of a body (csrc/jk_reduce.hip; models/GNNs.py, the JK branches
 * "sum", "max" and the weighted sum of "attention").  The states are S separate [N,H] tensors read IN PLACE through a pointer
 * table: nothing of [S,N,H] size is formed in the forward.  All fp32.
 *   KPGNN_JK_SUM      out[n,c] = x[0][n,c] + x[1][n,c] + ... + x[S-1][n,c], added in slot order (deterministic, independent of
 *                     the launch geometry).  No backward entry: every state's gradient is dL/dout itself.
 *   KPGNN_JK_MAX      out[n,c] = max_l x[l][n,c].  Slots are walked upwards and compared with `>`: among equal values (+0 and -0
 *                     are equal) the LOWEST slot wins, and arg[n,c] records the winner.  A NaN in any slot gives NaN, as
 *                     torch.max does; which slot arg then names is unspecified.
 *                     bwd: gx[l][n,c] = arg[n,c] == l ? gout[n,c] : 0 - every live element of all S blocks is written.
 *   KPGNN_JK_SOFTMAX  w[n,:] = softmax_l(score[n,:]) (max-subtracted), out[n,c] = sum_l w[n,l] x[l][n,c] in slot order.
 *                     bwd: gx[l][n,c] = w[n,l] gout[n,c];  gscore[n,l] = w[n,l] (d_l - sum_m w[n,m] d_m) with
 *                     d_l = <gout[n,:], x[l][n,:]>, summed per lane over its columns and then across the row's lanes (fixed
 *                     order: a function of H alone).
 * arg / w are written by fwd when given (they may be NULL when no backward follows) and read by bwd, which needs them.
 * Rows at or beyond *n_dyn are neither read nor written, in either direction and in every output; N == 0 launches nothing.
 * No limit on H: 16-byte accesses when H % 4 == 0, every stride is a multiple of 4 and every pointer is 16-byte aligned (arg:
 * 4-byte); a scalar path otherwise.
 * ---------------------------------------------------------------------------------------------- */
#define KPGNN_JK_MAX_STATES 32
enum { KPGNN_JK_SUM = 0, KPGNN_JK_MAX = 1, KPGNN_JK_SOFTMAX = 2 };

typedef struct kpgnn_jk_desc {
    int64_t N; int32_t H, S, mode;                 /* rows (capacity with n_dyn), row width (>= 1), states (1 .. 32), KPGNN_JK_* */
    const float* x[KPGNN_JK_MAX_STATES];           /* device [N,H] each; entries l < S (fwd; bwd: SOFTMAX only) */
    int64_t x_stride;                              /* the one row stride of every state, in floats (>= H) */
    const float* score;                            /* device [N,S] contiguous (SOFTMAX fwd) */
    float* out; int64_t out_stride;                /* device [N,H] (fwd) */
    uint8_t* arg;                                  /* device uint8 [N,H] contiguous: the winning slot (MAX; fwd: optional out, bwd: in) */
    float* w;                                      /* device [N,S] contiguous: the softmax weights (SOFTMAX; fwd: optional out, bwd: in) */
    /* backward only */
    const float* gout; int64_t gout_stride;        /* device [N,H] */
    float* gx;                                     /* device [S,N,H] contiguous: block l is state l's gradient */
    float* gscore;                                 /* device [N,S] contiguous (SOFTMAX) */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
} kpgnn_jk_desc;

int kpgnn_jk_reduce_fwd(const kpgnn_jk_desc* d, kpgnn_stream_t stream);
int kpgnn_jk_reduce_bwd(const kpgnn_jk_desc* d, kpgnn_stream_t stream);     /* MAX and SOFTMAX; SUM is KPGNN_EINVAL */

/* ------------------------------------------------------------------------------------------------
 * The scoring LSTM of the attention jumping-knowledge readout (csrc/jk_lstm.hip; models/GNNs.py, the JK == "attention"
 * branches): nn.LSTM(H, P, bidirectional=True) over the S states, summed over its 2P outputs.  With x[l] the S states [N,H]:
 *   for dir in {forward, reverse}, t walked 0..S-1 (forward) or S-1..0 (reverse), h = c = 0 at the start:
 *       (i,f,g,o) = W_ih[dir] x[t][n,:] + b_ih[dir] + W_hh[dir] h + b_hh[dir]       (torch's gate order: rows q, P+q, 2P+q, 3P+q)
 *       c = sigmoid(f) c + sigmoid(i) tanh(g);   h = sigmoid(o) tanh(c)
 *   score[n,t] = sum_q h_fwd[n,t,q] + sum_q h_rev[n,t,q]
 * which is what kpgnn_jk_reduce_* consumes as `score` in mode KPGNN_JK_SOFTMAX.  The states are read in place through the
 * pointer table (nothing of [N,S,H] size is formed in the forward); the input projection - 8P gate columns, both directions
 * side by side, over N*S rows of H - runs on the fp32 matrix instruction, the recurrence and its BPTT one thread per
 * (node, direction) with the state in registers.  All fp32, no atomics: the parameter gradients are per-tile partial sums
 * over FIXED ranges of 64 rows added in tile order, so the same live rows give the same bits at any capacity N.
 *   fwd: writes score; with `saved` != NULL also what bwd needs (kpgnn_jk_lstm_saved_bytes), in the kernels' own layout.
 *        saved == NULL is the evaluation forward: nothing is kept (the pre-activations then pass through the workspace).
 *   bwd: reads saved, gscore, the states and the weights; overwrites gx (block l = state l's gradient; NULL: skipped) and
 *        dw_ih / dw_hh / db (db is the gradient of b_ih and of b_hh alike).
 * Both need `workspace` of kpgnn_jk_lstm_workspace_bytes (16-byte aligned, as is saved).  Rows at or beyond *n_dyn are
 * neither read nor written in any per-row output and contribute nothing to the parameter gradients (skipped, not multiplied
 * by zero).  Limits: 1 <= P <= 16, 1 <= S <= 32, 1 <= H <= 256 (KPGNN_ELIMIT above, KPGNN_EINVAL below); N == 0 launches nothing.
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_jk_lstm_desc {
    int64_t N; int32_t H, P, S;                    /* rows (capacity with n_dyn), row width, LSTM hidden size, states */
    const float* x[KPGNN_JK_MAX_STATES];           /* device [N,H] each; entries l < S */
    int64_t x_stride;                              /* the one row stride of every state, in floats (>= H) */
    const float* w_ih[2]; const float* w_hh[2];    /* device [4P,H], [4P,P]; index 0 = forward, 1 = reverse (nn.LSTM's own) */
    const float* b_ih[2]; const float* b_hh[2];    /* device [4P] (fwd only) */
    float* score;                                  /* device [N,S] contiguous (fwd) */
    void* saved;                                   /* device, kpgnn_jk_lstm_saved_bytes: fwd optional out, bwd in */
    /* backward only */
    const float* gscore;                           /* device [N,S] contiguous */
    float* gx;                                     /* device [S,N,H] contiguous or NULL */
    float* dw_ih[2]; float* dw_hh[2]; float* db[2];/* device [4P,H], [4P,P], [4P] */
    void* workspace; size_t workspace_bytes;       /* >= kpgnn_jk_lstm_workspace_bytes(N, H, P, S) */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
} kpgnn_jk_lstm_desc;

/* 0 = the shape is not covered. */
size_t kpgnn_jk_lstm_saved_bytes(int64_t N, int32_t H, int32_t P, int32_t S);
size_t kpgnn_jk_lstm_workspace_bytes(int64_t N, int32_t H, int32_t P, int32_t S);
int kpgnn_jk_lstm_fwd(const kpgnn_jk_lstm_desc* d, kpgnn_stream_t stream);
int kpgnn_jk_lstm_bwd(const kpgnn_jk_lstm_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The bodies' norms other than BatchNorm (csrc/body_norm.hip; models/GNNs.py:103-112, norm_type "Layer", "Instance",
 * "GraphSize", "Pair").  The bodies call every norm WITHOUT a batch vector, so PyG's modules take the whole batch as one
 * graph; with x [N,C], n the live row count and eps added as PyG adds it:
 *   KPGNN_NORM_LAYER      mu, sd = mean and biased standard deviation over all n*C elements;
 *                         out = (x - mu) / (sd + eps) * weight[c] + bias[c]                  (eps joins the std, not the variance)
 *   KPGNN_NORM_INSTANCE   per column: out = (x - mean_n) / sqrt(var_biased_n + eps)          (no affine, no running statistics)
 *   KPGNN_NORM_GRAPHSIZE  out = x / sqrt(n)
 *   KPGNN_NORM_PAIR       xc = x - mean_n per column; out = xc / sqrt(eps + mean_n(sum_c xc^2))
 * each (+ residual[n,c] when given).  None has running statistics: training and evaluation compute the same.
 *   fwd: column sums of x and x^2 in DOUBLE as per-block partials in `workspace`, added in block order by a one-block finalize
 *        that leaves the fp32 coefficients in `saved`, then one streaming pass out = (x - m[c]) * s[c] (centred: a constant
 *        column and n == 1 give exact zeros).  saved: [0,C) m[c], [C,2C) s[c], then {mu, s, sd, n} (LAYER) / {0, r, 0, n}.
 *        Three launches; GRAPHSIZE one.
 *   bwd: the same three steps over the column sums of gout and gout*x: writes gx, and for LAYER gweight / gbias where given.
 *        The residual's gradient is gout itself - the caller returns it, nothing is launched for it.
 * No atomics: the same inputs and capacity give the same bits.  Rows at or beyond *n_dyn are not read, written or summed, in
 * any output of either direction; n is *n_dyn where given.  1 <= C <= 256 (KPGNN_EINVAL below, KPGNN_ELIMIT above); N == 0
 * launches nothing.  `workspace` (kpgnn_body_norm_workspace_bytes, 16-byte aligned) need not be zeroed.
 * Both entries validate one way for every kind: x, saved and workspace must be non-NULL (x_stride >= C) also where a kind
 * does not read them - the GRAPHSIZE backward reads gout alone and writes gx alone; any valid pointer serves as its x.
 * ---------------------------------------------------------------------------------------------- */
enum { KPGNN_NORM_LAYER = 0, KPGNN_NORM_INSTANCE = 1, KPGNN_NORM_GRAPHSIZE = 2, KPGNN_NORM_PAIR = 3 };

typedef struct kpgnn_norm_desc {
    int64_t N; int32_t C, kind; float eps;         /* rows (capacity with n_dyn), row width (1 .. 256), KPGNN_NORM_*, 1e-5 */
    const float* x; int64_t x_stride;              /* device [N,C], row stride in floats (>= C); both directions */
    const float* weight; const float* bias;        /* device [C]: LAYER (weight required, bias optional); NULL elsewhere */
    const float* residual; int64_t res_stride;     /* optional device [N,C] added to out (fwd) */
    float* out; int64_t out_stride;                /* device [N,C] (fwd) */
    float* saved;                                  /* device float [2C + 4]: fwd out, bwd in */
    /* backward only */
    const float* gout; int64_t gout_stride;        /* device [N,C] */
    float* gx; int64_t gx_stride;                  /* device [N,C] */
    float* gweight; float* gbias;                  /* device [C], optional (LAYER) */
    void* workspace; size_t workspace_bytes;       /* >= kpgnn_body_norm_workspace_bytes(N, C) */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
} kpgnn_norm_desc;

/* 0 = the shape is not covered. */
size_t kpgnn_body_norm_workspace_bytes(int64_t N, int32_t C);
int kpgnn_body_norm_fwd(const kpgnn_norm_desc* d, kpgnn_stream_t stream);
int kpgnn_body_norm_bwd(const kpgnn_norm_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The same four norms PER GRAPH (csrc/body_norm_graph.hip): what PyG's modules compute when they ARE handed a batch vector.
 * Graph g owns the contiguous rows [r0, r1), r0 = graph_ptr[g], r1 = min(graph_ptr[g+1], live), live = *n_dyn where given,
 * else N, n = r1 - r0; the formulas above apply to those rows alone, with that n (+ residual[row,c] when given).  A graph with
 * n <= 0 is skipped entirely; rows at or beyond `live`, and rows at or beyond graph_ptr[G], are never read, written or summed,
 * in any output of either direction.
 *   One team owns one graph from its statistics to its apply pass: a 64-lane wavefront where n < KPGNN_GRAPH_NORM_BLOCK_ROWS
 *   (eight graphs per 512-thread block), a whole block from there on; the class is chosen by n alone.  A lane owns the columns
 *   lane, lane + 64, ... whatever the alignment of the operands.  Every sum is taken in DOUBLE in an order fixed by the graph
 *   alone (rows in row order per column - per wave, then the waves in order, for a block team - and the columns by one
 *   butterfly), the coefficients stay in double, the apply pass is centred and done in double with contraction off, and the
 *   result is rounded to fp32 once: THE BITS OF A GRAPH'S ROWS OF out AND gx DEPEND ON THAT GRAPH'S ROWS, C, kind, eps (weight,
 *   bias, residual) AND ON NOTHING ELSE - not on G, the graph's position, the other graphs or the capacity N.  A constant
 *   column and n == 1 give exact zeros (INSTANCE, PAIR); a constant block gives exactly bias (LAYER).
 *   fwd: one launch.  `saved` (optional, float [G,4]) receives {mu, 1/(sd+eps), sd, n} (LAYER), {0, r, 0, n} (PAIR),
 *        {0, 1/sqrt(n), 0, n} (GRAPHSIZE), {0, 0, 0, n} (INSTANCE) for the record; a skipped graph's row is left alone.
 *   bwd: one launch.  It does NOT read `saved`: it recomputes the statistics of x in double in the same pass that sums gout
 *        and gout * x (the rows are read once either way), because coefficients rounded to fp32 cannot hold a two-row graph's
 *        gradient - a difference of nearly equal terms - to the tolerance of a float64 reference.  Where LAYER's block is
 *        constant (sd == 0) the term through the standard deviation is dropped (K = 0), as body_norm.hip does for a constant
 *        batch.  LAYER's gweight / gbias, where given, are sums over the live rows of ALL graphs: every team leaves a double
 *        partial [2][C] in `workspace` and ONE more launch adds them in a fixed order.  GRAPHSIZE reads gout alone.
 * No atomics.  1 <= C <= 256 (KPGNN_EINVAL below, KPGNN_ELIMIT above); N == 0 or G == 0 launches nothing.  x (x_stride >= C)
 * and graph_ptr must be non-NULL for every kind; `workspace` (kpgnn_graph_norm_workspace_bytes, 8-byte aligned, need not be
 * zeroed) is read by the LAYER backward with a gweight or gbias alone and may be NULL elsewhere.
 * ---------------------------------------------------------------------------------------------- */
#define KPGNN_GRAPH_NORM_BLOCK_ROWS 128     /* n >= this: a block per graph; below: a wavefront per graph */

typedef struct kpgnn_graph_norm_desc {
    int64_t N; int32_t C, kind; float eps;         /* rows (capacity with n_dyn), row width (1 .. 256), KPGNN_NORM_*, 1e-5 */
    const float* x; int64_t x_stride;              /* device [N,C], row stride in floats (>= C); both directions */
    const float* weight; const float* bias;        /* device [C]: LAYER (weight required, bias optional); NULL elsewhere */
    const float* residual; int64_t res_stride;     /* optional device [N,C] added to out (fwd) */
    float* out; int64_t out_stride;                /* device [N,C] (fwd) */
    float* saved;                                  /* optional device float [G,4]: fwd out; bwd does not read it */
    /* backward only */
    const float* gout; int64_t gout_stride;        /* device [N,C] */
    float* gx; int64_t gx_stride;                  /* device [N,C] */
    float* gweight; float* gbias;                  /* device [C], optional (LAYER) */
    void* workspace; size_t workspace_bytes;       /* >= kpgnn_graph_norm_workspace_bytes(N, G, C, kind) */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
    const int32_t* graph_ptr;                      /* device [G+1], non-decreasing */
    int32_t G;
} kpgnn_graph_norm_desc;

/* 0 = the shape is not covered. */
size_t kpgnn_graph_norm_saved_floats(int32_t G, int32_t C, int32_t kind);
size_t kpgnn_graph_norm_workspace_bytes(int64_t N, int32_t G, int32_t C, int32_t kind);
int kpgnn_graph_norm_fwd(const kpgnn_graph_norm_desc* d, kpgnn_stream_t stream);
int kpgnn_graph_norm_bwd(const kpgnn_graph_norm_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Resistance-distance node feature (csrc/resistance.hip; data_utils.py:280-303, `--use_rd`).  For each graph g of
 * n = node_ptr[g+1] - node_ptr[g] nodes, with A the summed adjacency of its edges (ones; duplicates add, the diagonal is
 * ignored as scipy's csgraph.laplacian ignores it) and L+ the pseudo-inverse of the Laplacian D - A:
 *   out[node_ptr[g] + y] = (float)(((L+[0,0] + L+[y,y]) - L+[0,y]) - L+[y,0])            in double, in that order: out[.. + 0] == 0.0f
 * L+ is not computed by an SVD: with the connected components c of sizes m_c, M = D - A + sum_c (1/m_c) 1_c 1_c^T is
 * symmetric positive definite, M^-1 comes from an in-place Gauss-Jordan sweep without pivoting (double, in LDS), and
 * L+ = M^-1 - sum_c (1/m_c) 1_c 1_c^T.  A node in another component than node 0 gets L+[0,0] + L+[y,y], as pinv gives.
 * status[g] (written for every graph of `graph_ids`; out is written only where it is 0):
 *   KPGNN_RD_OK 0          served
 *   KPGNN_RD_ASYMMETRIC 1  A != A^T: a directed list, the host route's job
 *   KPGNN_RD_TOO_LARGE 2   n > max_nodes of this launch (the cap of any launch is 128: one 128 x 129 double matrix in LDS;
 *                          kpgnn_resistance_distance_large below serves up to 2048 nodes from a workspace)
 *   KPGNN_RD_PIVOT 3       a pivot <= 0 or not finite
 *   KPGNN_RD_RANGE 4       an edge endpoint outside [node_ptr[g], node_ptr[g+1])
 * One launch serves the graphs `graph_ids[0 .. n_ids)`.  max_nodes <= 32: one wavefront per graph, four graphs per block, no
 * block barrier; above: one block per graph with dynamic LDS for max_nodes.  The caller buckets its graphs by size and makes
 * one call per class.  The count matrix is built with LDS integer atomics, so the result does not depend on the edge order;
 * no atomics to global memory, one workgroup per graph in a fixed order: bitwise reproducible.  n_ids == 0 returns KPGNN_OK
 * without a launch, n == 0 writes status 0 alone.  Ids outside [0, G) in graph_ids are skipped; edges are read from
 * [edge_ptr[g], edge_ptr[g+1]) clipped to [0, E).
 * ---------------------------------------------------------------------------------------------- */
enum { KPGNN_RD_OK = 0, KPGNN_RD_ASYMMETRIC = 1, KPGNN_RD_TOO_LARGE = 2, KPGNN_RD_PIVOT = 3, KPGNN_RD_RANGE = 4 };
#define KPGNN_RD_MAX_NODES 128
#define KPGNN_RD_WAVE_NODES 32

typedef struct kpgnn_rd_desc {
    int32_t G, n_ids;           /* graphs of the call; graphs this launch serves */
    const int64_t* node_ptr;    /* device [G+1] */
    const int64_t* edge_ptr;    /* device [G+1] */
    const int64_t* edge_index;  /* device [2,E] contiguous: global ids within the call, edges grouped by graph */
    int64_t E;                  /* edges of the call (the row length of edge_index) */
    const int32_t* graph_ids;   /* device [n_ids] */
    int32_t max_nodes, reserved;/* largest n this launch is sized for, 1 .. 128; 0 */
    float* out;                 /* device [N] */
    int32_t* status;            /* device [G] */
} kpgnn_rd_desc;

int kpgnn_resistance_distance(const kpgnn_rd_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The same feature for graphs of up to KPGNN_RD_LARGE_MAX_NODES nodes (csrc/resistance_large.hip).  The mathematics, the
 * output and the status codes are those of kpgnn_resistance_distance; KPGNN_RD_TOO_LARGE is n > max_nodes of this launch, whose
 * cap is 2048.  One workgroup of 1024 threads per graph of `graph_ids`; the graph's matrix lives in a slab of `workspace` that
 * only this workgroup touches (slot i of graph_ids owns slab i), not in LDS: integer counts by global integer atomics,
 * connected components by hooking over the edge list, M^-1 in place by a BLOCKED Gauss-Jordan sweep without pivoting (panel
 * width 32, the diagonal block inverted in LDS, plain double FMAs in a fixed order).  No float atomics, no communication between
 * workgroups: a graph's bits depend on the graph alone, not on the batch, the chunking or the workspace around it.
 * kpgnn_rd_large_workspace_bytes(max_nodes, n_ids): the bytes a launch of n_ids graphs sized for max_nodes needs - n_ids slabs
 * of the matrix (rows padded to the panel width) and two panels; 0 for max_nodes outside 1 .. 2048 or n_ids < 0.  `workspace`
 * (8-byte aligned) need not be zeroed.  The argument checks are those of kpgnn_resistance_distance, then max_nodes > 2048 is
 * KPGNN_ELIMIT and a NULL or too small workspace KPGNN_EINVAL, all before any device call.
 * ---------------------------------------------------------------------------------------------- */
#define KPGNN_RD_LARGE_MAX_NODES 2048

typedef struct kpgnn_rd_large_desc {
    int32_t G, n_ids;           /* graphs of the call; graphs this launch serves */
    const int64_t* node_ptr;    /* device [G+1] */
    const int64_t* edge_ptr;    /* device [G+1] */
    const int64_t* edge_index;  /* device [2,E] contiguous: global ids within the call, edges grouped by graph */
    int64_t E;                  /* edges of the call (the row length of edge_index) */
    const int32_t* graph_ids;   /* device [n_ids] */
    int32_t max_nodes, reserved;/* largest n this launch is sized for, 1 .. 2048; 0 */
    float* out;                 /* device [N] */
    int32_t* status;            /* device [G] */
    void* workspace;            /* device, >= kpgnn_rd_large_workspace_bytes(max_nodes, n_ids) */
    size_t workspace_bytes;
} kpgnn_rd_large_desc;

size_t kpgnn_rd_large_workspace_bytes(int32_t max_nodes, int32_t n_ids);
int kpgnn_resistance_distance_large(const kpgnn_rd_large_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The bodies' resistance-distance projection (csrc/rd_proj.hip; models/GNNs.py `x = x + self.rd_projection(rd)`, an
 * nn.Linear(1, H)):   out[n,h] = x[n,h] + rd[n] * w[h] + b[h]                  one launch
 * Backward: dx is dy itself (the caller returns it, nothing is launched); dw[h] = sum_n rd[n] dy[n,h], db[h] = sum_n dy[n,h]:
 * per-block partial sums in DOUBLE in `workspace`, added in block order by a one-block finalize.  Row r always belongs to
 * block (r / rows-per-block) mod 256 and a block without live rows contributes +0.0, so the sums do not depend on the
 * capacity N, only on the live rows: no atomics, bitwise reproducible.  Rows at or beyond *n_dyn are not read, written or
 * summed.  1 <= H <= 256 (KPGNN_EINVAL below, KPGNN_ELIMIT above); N == 0: fwd launches nothing, bwd writes zeros.
 * `workspace` (kpgnn_rd_proj_workspace_bytes, 16-byte aligned) need not be zeroed.
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_rd_proj_desc {
    int64_t N; int32_t H, reserved;                /* rows (capacity with n_dyn), row width (1 .. 256); 0 */
    const float* x; int64_t x_stride;              /* device [N,H], row stride in floats (>= H) (fwd) */
    const float* rd;                               /* device [N] contiguous (both directions) */
    const float* w; const float* b;                /* device [H] each (fwd) */
    float* out; int64_t out_stride;                /* device [N,H] (fwd; may be x itself) */
    /* backward only */
    const float* dy; int64_t dy_stride;            /* device [N,H] */
    float* dw; float* db;                          /* device [H] each */
    void* workspace; size_t workspace_bytes;       /* >= kpgnn_rd_proj_workspace_bytes(N, H) */
    const int32_t* n_dyn;       /* optional live-row count (device int32[1], <= N; kpgnn_wgrad_desc explains); NULL: all N rows */
} kpgnn_rd_proj_desc;

/* 0 = the shape is not covered. */
size_t kpgnn_rd_proj_workspace_bytes(int64_t N, int32_t H);
int kpgnn_rd_proj_fwd(const kpgnn_rd_proj_desc* d, kpgnn_stream_t stream);
int kpgnn_rd_proj_bwd(const kpgnn_rd_proj_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The K-hop pre-transform on the device (csrc/khop_transform.hip; data_utils.py:20-241, extract_multi_hop_neighbors).  A
 * restatement of transform_graph / peripheral_stats of csrc/khop_host.cpp (kpgnn_host.h, kpgnn_khop_plan_*), which is the
 * specification, quirks Q1 - Q8 of SURVEY.md included: raw graphs in, the collated K-hop tensors of the host plan out, bit
 * for bit.  Integer only, one workgroup (or wavefront) per graph, two passes over the graphs `graph_ids[0 .. n_ids)`:
 *   kpgnn_khop_dev_count   adjacency (multiplicity and summed type, LDS integer atomics: COO duplicates add, no dependence on
 *                          the edge order; self loops stay for the recurrence), walk counts W_1 = mult, W_{k+1} = W_k A,
 *                          the hop sets (spd: targets not reached at an earlier hop; gd: every positive count), and per node
 *                          its any-hop mask and K-hop out-degree into `workspace`; status[g] for every graph of the launch.
 *   kpgnn_khop_dev_fill    the same walk again for the graphs whose status is 0, now writing: the K-hop edge list in
 *                          (src, dst ascending) order with GLOBAL ids (+ node_ptr[g]) at node_off[i] + rank of dst in the
 *                          any-hop mask, edge_attr [E,K] (column 0 the summed type of the 1-hop edge or 0, hop k > 0
 *                          min(count, max_edge_attr_num) + 1, zeros in inactive slots), pe_attr zeros (Q1), batch, and the
 *                          peripheral statistics per (node, hop) when max_hop_num > 0 and max_edge_type > 0.
 * Between the two the caller scans the degrees: workspace is int64[2 N] - [0, N) the any-hop mask of each node (one bit per
 * local target), [N, 2 N) its K-hop out-degree, 0 for every node of a graph whose status is not 0 - and node_off[i] is the
 * exclusive running sum of the degrees (plus whatever the caller adds for graphs it serves by another route), E_out the
 * total.  Every write of the fill pass is checked against E_out / N.
 * status[g] (count pass; outputs of a graph are written only where it is 0):
 *   KPGNN_KHOP_OK 0          served
 *   KPGNN_KHOP_TOO_LARGE 1   n > max_nodes of this launch (the cap of any launch is KPGNN_KHOP_MAX_NODES: a row is one 64-bit word)
 *   KPGNN_KHOP_RANGE 2       a walk count >= 2^31 off the diagonal within K hops (the host's KPGNN_HOST_ERANGE)
 *   KPGNN_KHOP_ENDPOINT 3    an edge endpoint outside [0, n)
 *   KPGNN_KHOP_TYPE 4        an edge type below 0, or a summed type above KPGNN_KHOP_MAX_TYPE (the histogram's width)
 *   KPGNN_KHOP_SHAPE 5       K > 16, max_edge_type > 8 or max_hop_num > 8
 * Walk counts saturate at 2^32 - 1 where the host saturates at 2^40: min(cap, true count) is what either keeps, every use
 * is "below 2^31, then exact" or "RANGE", so any cap >= 2^31 gives the same answer.  max_nodes <= KPGNN_KHOP_WAVE_NODES: one
 * wavefront per graph, four graphs per block, no block barrier; above: one block per graph; dynamic LDS for max_nodes and
 * K either way (75,280 bytes per graph at n = 64, K = 16).  No global atomics, no float, one workgroup per graph in a fixed
 * order: bitwise reproducible.  G == 0 or n_ids == 0 return KPGNN_OK without a launch; ids outside [0, G) are skipped; edges
 * are read from [edge_ptr[g], edge_ptr[g+1]) clipped to [0, E_in).
 * ---------------------------------------------------------------------------------------------- */
enum { KPGNN_KHOP_OK = 0, KPGNN_KHOP_TOO_LARGE = 1, KPGNN_KHOP_RANGE = 2, KPGNN_KHOP_ENDPOINT = 3, KPGNN_KHOP_TYPE = 4,
       KPGNN_KHOP_SHAPE = 5 };
#define KPGNN_KHOP_MAX_NODES 64
#define KPGNN_KHOP_WAVE_NODES 32
#define KPGNN_KHOP_MAX_TYPE 63
#define KPGNN_KHOP_MAX_K 16
#define KPGNN_KHOP_MAX_T 8
#define KPGNN_KHOP_MAX_H 8

typedef struct kpgnn_khop_dev_desc {
    int32_t G, n_ids;           /* graphs of the call; graphs this launch serves */
    const int32_t* graph_ids;   /* device [n_ids] */
    int32_t max_nodes, reserved;/* largest n this launch is sized for, 1 .. KPGNN_KHOP_MAX_NODES (kpgnn_khop_large_*: 1 ..
                                   KPGNN_KHOP_LARGE_MAX_NODES); 0 */
    int64_t N;                  /* nodes of the call, node_ptr[G] */
    const int64_t* node_ptr;    /* device [G+1] */
    const int64_t* edge_ptr;    /* device [G+1] */
    const int64_t* edge_index;  /* device [2,E_in] contiguous: LOCAL ids (0 .. n-1 within each graph), edges grouped by graph */
    const int64_t* edge_attr;   /* device [E_in] edge types, or NULL = every edge has type 2 */
    int64_t E_in;               /* input edges of the call (the row length of edge_index), < 2^31 */
    /* the seven fields of kpgnn_khop_args (kpgnn_host.h) */
    int32_t K, max_edge_attr_num, max_hop_num, max_edge_type, max_edge_count, max_distance_count, kernel, reserved2;   /* kernel: 0 = spd, 1 = gd; 0 */
    void* workspace; size_t workspace_bytes;       /* >= kpgnn_khop_dev_workspace_bytes(N) (kpgnn_khop_large_*: >=
                                                      kpgnn_khop_large_workspace_bytes(N, E_in, max_nodes)), 8-byte aligned;
                                                      count writes, fill reads */
    int32_t* status;            /* device [G]; count writes, fill reads */
    /* fill pass only */
    const int64_t* node_off;    /* device [N]: first K-hop edge of each node */
    int64_t E_out;              /* K-hop edges of the call (the row length of out_edge_index) */
    int64_t* out_edge_index;    /* device [2,E_out] */
    int64_t* out_edge_attr;     /* device [E_out,K] */
    int64_t* out_pe_attr;       /* device [N,K-1], or NULL */
    int64_t* out_pea;           /* device [N,K,max_edge_type,2]; required when max_hop_num > 0 and max_edge_type > 0 */
    int64_t* out_pca;           /* device [N,K,max_hop_num+1]; likewise */
    int64_t* out_batch;         /* device [N], or NULL */
} kpgnn_khop_dev_desc;

size_t kpgnn_khop_dev_workspace_bytes(int64_t N);
int kpgnn_khop_dev_count(const kpgnn_khop_dev_desc* d, kpgnn_stream_t stream);
int kpgnn_khop_dev_fill(const kpgnn_khop_dev_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The same pre-transform for graphs above KPGNN_KHOP_MAX_NODES nodes (csrc/khop_large.hip): the same descriptor (layout
 * unchanged, reserved fields 0), the same input contract (raw COO with local ids, grouped by graph, any order within a graph;
 * duplicates add; self loops stay for the recurrence; directed lists allowed), the same status codes where the pair above
 * reports them (TOO_LARGE: n > max_nodes of THIS launch), the same K / max_edge_type / max_hop_num limits 16 / 8 / 8 and
 * summed-type limit 63, and bit for bit the tensors of the host route for a graph of 1 .. KPGNN_KHOP_LARGE_MAX_NODES nodes -
 * one of 64 nodes or fewer included.  max_nodes above KPGNN_KHOP_LARGE_MAX_NODES answers KPGNN_ELIMIT.
 * The unit of work is a SOURCE NODE (row i of W_k depends only on row i of W_{k-1}): one wavefront walks one row with two
 * uint32 count rows in LDS, W_{k+1}[i][j] a pull sum over the raw edges into j (duplicates supply the multiplicity; summed in
 * 64 bits and clamped to 2^32 - 1, so the order of the terms cannot matter), node sets as ceil(n / 64) words, the rank of a
 * target in the any-hop mask a prefix popcount over words, the edge-type histogram of the peripheral statistics in 32 bits.
 *   kpgnn_khop_large_count  per graph of the launch: status[g]; the adjacency into the workspace by two stable counting sorts
 *                           of its edge slice (positions are counted, never raced for: the workspace is the same bits on
 *                           every run); per node the any-hop words and the K-hop out-degree.  A node of a graph whose status
 *                           is not 0 gets degree 0; a graph outside the launch is not written.
 *   kpgnn_khop_large_fill   the graphs whose status is 0, from the adjacency the count pass left: the outputs of
 *                           kpgnn_khop_dev_fill, every global write checked against E_out / N; other slices are left alone.
 * Workspace (kpgnn_khop_large_workspace_bytes(N, E_in, max_nodes); W = ceil(max_nodes / 64); every launch between a count
 * pass and its fill pass that shares one workspace passes the SAME max_nodes, since W is the stride of the word arrays):
 *   int64  deg[N]            the K-hop out-degree of each node - what the caller scans, exactly as for the pair above
 *   uint64 any[N][W]         the any-hop mask of each node, one bit per local target
 *   uint64 nzt[N][W]         the targets of a node's edges whose summed type is not 0
 *   int32  in_start[N], in_cnt[N], out_start[N], out_cnt[N]     a node's range in the edge arrays below (positions of the call)
 *   int32  in_src[E_in]      edges sorted by destination (stable): the source of each
 *   int32  s_dst[E_in]       ... its destination (scratch of the second sort)
 *   int32  m_typ[E_in]       edges sorted by (source, destination): the summed type of (u, v) on the first edge of its run of
 *                            duplicates, 0 on the others (first: the types in the order of in_src)
 *   int32  o_src[E_in], o_dst[E_in], o_typ[E_in]                edges sorted by (source, destination): source, destination, type
 * No global atomics, no float, bitwise reproducible.  G == 0 or n_ids == 0 return KPGNN_OK without a launch; ids outside
 * [0, G) are skipped; edges are read from [edge_ptr[g], edge_ptr[g+1]) clipped to [0, E_in).
 * ---------------------------------------------------------------------------------------------- */
#define KPGNN_KHOP_LARGE_MAX_NODES 2048

size_t kpgnn_khop_large_workspace_bytes(int64_t N, int64_t E_in, int32_t max_nodes);
int kpgnn_khop_large_count(const kpgnn_khop_dev_desc* d, kpgnn_stream_t stream);
int kpgnn_khop_large_fill(const kpgnn_khop_dev_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Embedding collisions of the regular-graph simulation (csrc/collisions.hip; run_simulation.py:165-178,
 * compute_simulation_collisions).  For the rows o[i,:] of x [N,D] fp32, d2(i,j) = sum_d (o[i,d] - o[j,d])^2 evaluated in fp32
 * in the difference form (never |a|^2 + |b|^2 - 2 a.b), and a pair collides iff d2 < eps by the plain IEEE compare:
 *   out[0] = upper = #{ i < j : d2(i,j) < eps }
 *   out[1] = diag  = #{ i : d2(i,i) < eps }        (the rows without a NaN or Inf, since x - x is 0 or NaN; 0 when eps == 0)
 * so the reference's (diff < eps).sum() is 2 * upper + diag.  Both are exact integers; the order of the partial sums cannot
 * matter.  A pair whose exact d2 lies outside [eps (1 - delta), eps (1 + delta)], delta = (D + 2) 2^-23, is classified as exact
 * arithmetic classifies it (derivation: csrc/collisions.hip).  The pair matrix is walked as 128 x 128 tiles of its upper
 * triangle by a persistent grid; every block leaves one pair of 64-bit partial counts in the workspace and a second, one-block
 * launch adds them into `out`: two launches, no atomics, nothing read back.  Rows are read in place through x_stride.
 * 1 <= D <= 256, eps finite and >= 0, workspace 8-byte aligned (KPGNN_EINVAL otherwise).  N == 0 returns KPGNN_OK without a
 * launch and leaves `out` alone.
 * ---------------------------------------------------------------------------------------------- */
typedef struct kpgnn_collision_desc {
    int64_t N;                  /* rows */
    int32_t D;                  /* columns, 1 .. 256 */
    float eps;                  /* threshold on the squared distance (the reference's 1e-10) */
    const float* x; int64_t x_stride;      /* device [N,D], unit column stride, x_stride >= D floats between rows */
    int64_t* out;               /* device int64[2]: upper, diag */
    void* workspace; int64_t workspace_bytes;      /* device, >= kpgnn_collision_workspace_bytes(N) */
} kpgnn_collision_desc;

int64_t kpgnn_collision_workspace_bytes(int64_t N);
int kpgnn_collision_count(const kpgnn_collision_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Labels of the synthetic graph- and node-property dataset (csrc/graph_labels.hip; datasets/GraphPropertyDataset.py
 * genereate_dataset, datasets/graph_algorithms.py).  For each graph g of n = node_ptr[g+1] - node_ptr[g] <= 64 nodes, with A
 * the 0/1 adjacency of its edges (duplicates collapse), F = features[node_ptr[g] ..] and s = source[g]:
 *   node_out[node_ptr[g] + i, 0] = sssp          BFS distance from s to i; 0 for s itself and for an unreachable node
 *   node_out[.., 1]              = eccentricity  the largest finite distance from i (within its component; 0 when isolated)
 *   node_out[.., 2]              = laplacian     (float)(deg(i) F[i] - sum_{j in adj(i)} F[j]), in double, ascending j
 *   graph_out[g, 0] = is_connected    1.0f iff every ordered pair (i, j), i == j included, has a walk of length exactly 2^m,
 *                                     m = 1 + ceil(log2 n): the reference's repeated squaring, not true connectivity (a
 *                                     connected bipartite graph answers 0, so does n == 1), as m boolean squarings
 *   graph_out[g, 1] = diameter        the largest finite distance of the graph (0 when it has no edge)
 *   graph_out[g, 2] = spectral_radius (float) of the largest eigenvalue of A in double: Householder tridiagonalisation in LDS
 *                                     and Sturm-count multisection (64 probes a round); exactly 0 when the graph has no edge
 * status[g] (written for every graph of `graph_ids`; node_out / graph_out are written only where it is 0):
 *   KPGNN_GL_OK 0          served
 *   KPGNN_GL_ASYMMETRIC 1  A != A^T: a directed list, the host route's job
 *   KPGNN_GL_TOO_LARGE 2   n > max_nodes of this launch (the cap of any launch is KPGNN_GL_MAX_NODES: a row is one 64-bit word)
 *   KPGNN_GL_ENDPOINT 3    an edge endpoint outside [0, n)
 *   KPGNN_GL_SELF_LOOP 4   an edge (i, i): the reference asserts there is none
 *   KPGNN_GL_SOURCE 5      source[g] outside [0, n)
 * (3 wins over 4, 4 over 5, 5 over 1; every range is checked before anything is indexed with it.)  One launch serves the
 * graphs `graph_ids[0 .. n_ids)`.  max_nodes <= KPGNN_GL_WAVE_NODES: one wavefront per graph, four graphs per block, no block
 * barrier; above: one block per graph.  The caller buckets its graphs by size and makes one call per class.  No global
 * atomics, no float atomics, every cross-lane sum in index order: the bits of a graph depend on that graph alone - not on
 * the edge order, the other graphs of the launch, graph_ids or the size class.  G == 0 or n_ids == 0 return KPGNN_OK without
 * a launch; n == 0 writes status 0 and a zero graph_out row; ids outside [0, G) are skipped; edges are read from
 * [edge_ptr[g], edge_ptr[g+1]) clipped to [0, E).  max_nodes < 1 is KPGNN_EINVAL and > 64 KPGNN_ELIMIT, before any device call.
 * ---------------------------------------------------------------------------------------------- */
enum { KPGNN_GL_OK = 0, KPGNN_GL_ASYMMETRIC = 1, KPGNN_GL_TOO_LARGE = 2, KPGNN_GL_ENDPOINT = 3, KPGNN_GL_SELF_LOOP = 4,
       KPGNN_GL_SOURCE = 5 };
#define KPGNN_GL_MAX_NODES 64
#define KPGNN_GL_WAVE_NODES 32

typedef struct kpgnn_graph_labels_desc {
    int32_t G, n_ids;           /* graphs of the call; graphs this launch serves */
    const int64_t* node_ptr;    /* device [G+1] */
    const int64_t* edge_ptr;    /* device [G+1] */
    const int64_t* edge_index;  /* device [2,E] contiguous: LOCAL ids (0 .. n-1 within each graph), edges grouped by graph */
    int64_t E;                  /* edges of the call (the row length of edge_index) */
    const int32_t* graph_ids;   /* device [n_ids] */
    int32_t max_nodes, reserved;/* largest n this launch is sized for, 1 .. KPGNN_GL_MAX_NODES; 0 */
    const double* features;     /* device [N] */
    const int32_t* source;      /* device [G]: the local id of each graph's source node */
    float* node_out;            /* device [N,3]: sssp, eccentricity, laplacian */
    float* graph_out;           /* device [G,3]: is_connected, diameter, spectral_radius */
    int32_t* status;            /* device [G] */
} kpgnn_graph_labels_desc;

int kpgnn_graph_labels(const kpgnn_graph_labels_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The same six labels for graphs of up to KPGNN_GL_LARGE_MAX_NODES nodes (csrc/graph_labels.hip, W = 2): the third size class.
 * The descriptor, the labels, the six status codes with their precedence and the output contract are kpgnn_graph_labels's:
 * status is written for every graph of `graph_ids`, node_out / graph_out only where it is 0, n == 0 writes status 0 and a zero
 * graph_out row, n > max_nodes of the launch is KPGNN_GL_TOO_LARGE.  One 256-thread block per graph, whatever max_nodes; a row
 * is TWO 64-bit words in LDS (bit 64 is bit 0 of the second), the n x n double matrix of the spectral radius lives in LDS too
 * (128 x 129 doubles next to 11.5 KB of rows and vectors: one block per CU at max_nodes = 128, the launch's dynamic LDS is
 * sized by max_nodes).  Any n from 1 to the cap is served; the caller sends the graphs of 65 nodes and more.
 * is_connected is m = 1 + ceil(log2 n) BOOLEAN squarings here too.  For 65 <= n <= 128, m = 8 and every entry of A^(2^7) is at
 * most 127^128 < 2^895, so the reference's last float64 squaring multiplies no inf by 0: it makes no nan and rounds no positive
 * integer to zero.  Hence its min > 0 holds iff the eighth boolean squaring has no zero - exactly, dense graphs included (K128
 * overflows to inf, which is > 0); at n = 129, m = 9 and stage 8 can hold inf next to zeros, which is why the cap is 128.
 * No global atomics, no float atomics, every cross-lane sum in index order: the bits of a graph depend on that graph alone.
 * G == 0 or n_ids == 0 return KPGNN_OK without a launch.  max_nodes < 1 is KPGNN_EINVAL and > 128 KPGNN_ELIMIT, before any
 * device call.
 * ---------------------------------------------------------------------------------------------- */
#define KPGNN_GL_LARGE_MAX_NODES 128

int kpgnn_graph_labels_large(const kpgnn_graph_labels_desc* d, kpgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Labels of the synthetic substructure-counting dataset (csrc/count_labels.hip; datasets/GraphCountDataset.py process).  For
 * each graph g of n = node_ptr[g+1] - node_ptr[g] nodes, with A the symmetric 0/1 adjacency of its edges (duplicates
 * collapse), d_i the degree of node i, c_ij = popcount(row_i & row_j) = (A^2)_ij and T_i = sum_{j in N(i)} c_ij = (A^3)_ii:
 *   out[g, 0] = tri     trace(A^3) / 6                                  = (sum_i T_i) / 6
 *   out[g, 1] = tailed  sum_i (A^3)_ii / 2 * (d_i - 2)                  = sum_i (T_i / 2) (d_i - 2)
 *   out[g, 2] = star    sum_i C(d_i, 3)                                 = sum_i d_i (d_i - 1) (d_i - 2) / 6
 *   out[g, 3] = cyc4    (trace(A^4) + trace(A^2) - 2 sum(A^2)) / 8      = (sum_ij c_ij^2 + sum_i d_i - 2 sum_i d_i^2) / 8,
 *                                                                         over all ordered pairs, c_ii = d_i included
 *   out[g, 4] = cus     sum(A diag(exp(-rowsum(A^2))) A)                = sum_k d_k^2 exp(-s_k), s_k = sum_{j in N(k)} d_j
 * The first four are sums of 64-bit integers (every division is exact; at 2048 nodes every intermediate stays below 2^53)
 * converted to double once.  cus is a double sum taken by ONE lane in ascending k, one exp and one product per node, with
 * floating-point contraction off.
 * status[g] (written for every graph of `graph_ids`; out[g] is written only where it is 0):
 *   KPGNN_CL_OK 0          served
 *   KPGNN_CL_ASYMMETRIC 1  A != A^T: a directed list, the host route's job
 *   KPGNN_CL_SELF_LOOP 2   an edge (i, i): the host route's job too (the reference's expressions apply literally)
 *   KPGNN_CL_TOO_LARGE 3   n > max_nodes of this launch (the cap of any launch is KPGNN_CL_MAX_NODES)
 *   KPGNN_CL_ENDPOINT 4    an edge endpoint outside [0, n), or node_ptr decreasing at g
 * (3 is decided before the edges are read; then 4 wins over 2 and 2 over 1; every range is checked before anything is indexed
 * with it.)  One launch serves the graphs `graph_ids[0 .. n_ids)` and is sized by max_nodes:
 *   max_nodes <= KPGNN_CL_WAVE_NODES  one wavefront per graph, four graphs per 256-thread block, no block barrier; a row of
 *                                     the adjacency is ONE 64-bit word in LDS, set by LDS atomic OR
 *   max_nodes <= KPGNN_CL_WORD_NODES  one 256-thread block per graph, the same one-word rows
 *   max_nodes <= KPGNN_CL_MAX_NODES   one 1024-thread block per graph; the rows are ceil(n / 64) words in the graph's slab of
 *                                     `workspace` (slab s, of kpgnn_count_labels_workspace_bytes(max_nodes) bytes, belongs to
 *                                     graph_ids[s]); the kernel zeroes its slab and sets the bits by 64-bit integer atomic OR;
 *                                     workspace_bytes >= n_ids * kpgnn_count_labels_workspace_bytes(max_nodes), 8-byte aligned.
 *                                     A smaller graph may be served by a larger class; the two smaller classes ignore workspace.
 * The caller buckets its graphs by size and makes one call per class.  No float atomics; no global atomics but that OR; the
 * bits of a graph depend on that graph alone - not on the edge order, duplicated edges, the size class, graph_ids or the other
 * graphs of the launch.  G == 0 or n_ids == 0 return KPGNN_OK without a launch; n == 0 writes status 0 and five zeros; ids
 * outside [0, G) are skipped; edges are read from [edge_ptr[g], edge_ptr[g+1]) clipped to [0, E).  max_nodes < 1 is
 * KPGNN_EINVAL and > KPGNN_CL_MAX_NODES KPGNN_ELIMIT, before any device call.
 * ---------------------------------------------------------------------------------------------- */
enum { KPGNN_CL_OK = 0, KPGNN_CL_ASYMMETRIC = 1, KPGNN_CL_SELF_LOOP = 2, KPGNN_CL_TOO_LARGE = 3, KPGNN_CL_ENDPOINT = 4 };
#define KPGNN_CL_WAVE_NODES 32
#define KPGNN_CL_WORD_NODES 64
#define KPGNN_CL_MAX_NODES 2048

typedef struct kpgnn_count_labels_desc {
    int32_t G, n_ids;           /* graphs of the call; graphs this launch serves */
    const int64_t* node_ptr;    /* device [G+1] */
    const int64_t* edge_ptr;    /* device [G+1] */
    const int64_t* edge_index;  /* device [2,E] contiguous: LOCAL ids (0 .. n-1 within each graph), edges grouped by graph */
    int64_t E;                  /* edges of the call (the row length of edge_index) */
    const int32_t* graph_ids;   /* device [n_ids] */
    int32_t max_nodes, reserved;/* largest n this launch is sized for, 1 .. KPGNN_CL_MAX_NODES; 0 */
    double* out;                /* device [G,5]: tri, tailed, star, cyc4, cus */
    int32_t* status;            /* device [G] */
    void* workspace; size_t workspace_bytes;       /* device; needed only when max_nodes > KPGNN_CL_WORD_NODES */
} kpgnn_count_labels_desc;

/* Bytes of ONE graph's slab in a launch sized for max_nodes: 0 up to KPGNN_CL_WORD_NODES (the rows live in LDS), else
 * max_nodes * ceil(max_nodes / 64) * 8.  Never decreases with max_nodes; no device call. */
size_t kpgnn_count_labels_workspace_bytes(int max_nodes);
int kpgnn_count_labels(const kpgnn_count_labels_desc* d, kpgnn_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * Uniform random simple d-regular graphs: the pairing model with rejection (csrc/regular_graphs.hip; the same bits from
 * kp_gnn_amd/regular_graphs.py on the host).  The definition, which no launch geometry enters: graph g of a call is a
 * function of (seed, first_graph + g, n, d) alone.
 *   stubs     m = n * d of them; stub s belongs to node s / d.
 *   words     pairing number a = 0, 1, .. draws one 64-bit word r(s) per stub: with (w0, w1, w2, w3) the output of
 *             Philox4x32-10 (ten rounds, multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85 - the
 *             function behind kpgnn_dropout_*) under the key (seed & 0xFFFFFFFF, seed >> 32) at the counter
 *             (s >> 1, a, id & 0xFFFFFFFF, id >> 32), id = (uint64_t)(first_graph + g):
 *             r(s) = w[2 (s & 1)] | w[2 (s & 1) + 1] << 32.
 *   key       (r(s) & ~0x1FFF) | s: 51 random bits above the 13-bit stub index, so no two keys are equal and the order is
 *             total whatever sorts them.
 *   pairing   sort the m keys ascending; the stubs at the sorted positions 2 i and 2 i + 1 are partners.
 *   accepted  when no stub's partner lies in the stub's own node (no self loop) and no node has two stubs whose partners lie
 *             in one node (no double edge).  Every simple d-regular graph on n labelled nodes then comes out with the same
 *             probability.  Otherwise a increases by one; after max_attempts pairings the graph is EXHAUSTED.
 *   output    node u's d neighbours ascending, as the directed edges (u, v) at the columns g * m + u * d + j of
 *             edge_index [2, G * m] (LOCAL ids): the (src, dst)-sorted list of batch.regular_graphs, with
 *             node_ptr[g] = g * n and edge_ptr[g] = g * m.  attempts[g] = the pairings drawn (max_attempts when exhausted).
 * status[g]: KPGNN_RRG_OK 0, or KPGNN_RRG_EXHAUSTED 1 - the columns of such a graph are NOT written.
 * One team per graph for its whole rejection loop: the keys, padded with all-ones keys to the next power of two P >= m, are
 * sorted by a bitonic network in LDS (8 P bytes, and 2 m for the partner table: 80 KiB at the limit), the two checks end in a
 * team-wide vote, and the accepted rows are written by one thread per node.  m <= KPGNN_RRG_WAVE_STUBS: a wavefront per
 * graph, four graphs per 256-thread block, no block barrier; else a block per graph of P / 2 threads, at least 256 and at
 * most 1024.  Integer arithmetic only, no atomics, no workspace.
 * Limits, answered before any device call: G < 0, n < 1, d < 1, d >= n, n * d odd, max_attempts < 1, first_graph < 0 or a
 * NULL output (G > 0) are KPGNN_EINVAL; d > KPGNN_RRG_MAX_DEGREE, n > KPGNN_RRG_MAX_NODES or n * d > KPGNN_RRG_MAX_STUBS
 * are KPGNN_ELIMIT (d >= 5 accepts fewer than 3 pairings in 1000: DESIGN.md 5.31).  G == 0 returns KPGNN_OK without a launch.
 * ---------------------------------------------------------------------------------------------- */
enum { KPGNN_RRG_OK = 0, KPGNN_RRG_EXHAUSTED = 1 };
#define KPGNN_RRG_MAX_DEGREE 4
#define KPGNN_RRG_MAX_NODES 2048     /* (the bound of kpgnn_khop_large_*) */
#define KPGNN_RRG_MAX_STUBS 8192     /* n * d: the 13 index bits of a key */
#define KPGNN_RRG_WAVE_STUBS 256     /* n * d up to which a wavefront owns a graph */

typedef struct kpgnn_rrg_desc {
    int32_t G, n, d, max_attempts;  /* graphs of the call; nodes and degree of each; pairings tried per graph */
    int64_t seed, first_graph;      /* the Philox key; the id of the call's graph 0 */
    int64_t* edge_index;            /* device [2, G * n * d] contiguous */
    int32_t* attempts;              /* device [G] */
    int32_t* status;                /* device [G] */
} kpgnn_rrg_desc;

int kpgnn_random_regular_graphs(const kpgnn_rrg_desc* d, kpgnn_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * The random graphs of the graph- and node-property dataset (csrc/property_graphs.hip; the same bits from
 * kp_gnn_amd/property_graphs.py on the host): the reference's datasets/graph_generation.py generate_graph - ten graph types,
 * a uniform relabelling, `randomize`, and a retry while a node has no neighbour - as a function of Philox words.  Graph g of
 * a call is a function of (seed, first_graph + g, n_g, graph_type, flags) alone; no launch geometry enters.  The laws are the
 * reference's; the stream is not (numpy's and Python's Mersenne Twister there), so the graphs are another draw.
 *   words     W(stream, a, i) = the output (w0, w1, w2, w3) of Philox4x32-10 (as for kpgnn_random_regular_graphs) under the
 *             key (seed & 0xFFFFFFFF, seed >> 32) at the counter (i, a << 4 | stream, id & 0xFFFFFFFF, id >> 32),
 *             id = (uint64_t)(first_graph + g), a the attempt.  "Word i" of a stream is w0 of W(stream, a, i); PAIR also
 *             uses w1 and w2 and SHUFFLE w1.  Streams: TYPE 0 (always a = 0), PARAM 1, PAIR 2, BA 3, TREE 4, ATTACH 5,
 *             SHUFFLE 6, FEATURE 7, SOURCE 8.
 *   below     below(w, L) = ((uint64_t)w * L) >> 32: uniform in [0, L) with a bias below L / 2^32 (L <= 8192 here).
 *   No floating point enters a decision: every comparison is one of integers of at most 64 bits.
 * Attempt a = 0, 1, .. of a graph of n nodes:
 *   1 type      graph_type, or for KPGNN_PG_RANDOM (once per graph, kept over the attempts) x = below(TYPE word 0, 20) against
 *               the reference's MIXTURE in twentieths: x < 4 ERDOS_RENYI, < 8 BARABASI_ALBERT, < 9 GRID, < 10 CAVEMAN,
 *               < 13 TREE, < 14 LADDER, < 15 LINE, < 16 STAR, < 18 CATERPILLAR, else LOBSTER.
 *   2 structure on canonical labels 0 .. n-1 (the position of a node in list(G) of the networkx constructor the reference calls).
 *     ERDOS_RENYI      p = PARAM word 0; pair (i, j), i > j, numbered q = i (i - 1) / 2 + j, is an edge iff w2 of
 *                      W(PAIR, a, q) < p (p as a 32-bit fraction is uniform, as the reference's degree / N).
 *     BARABASI_ALBERT  m = 1 + below(PARAM word 0, n - 1).  A star with centre 0 and leaves 1 .. m; the list `repeated` =
 *                      m times 0, then 1 .. m.  Node s = m + 1 .. n - 1 draws x = repeated[below(BA word t, len(repeated))],
 *                      t = 0, 1, .. counting on across the whole graph, until it holds m DISTINCT targets x, joins them, and
 *                      appends its targets in ASCENDING order and then m copies of s (networkx 3.x's procedure).
 *     GRID             r = the largest divisor of n with r * r <= n, c = n / r: node i * c + j joins its right (j + 1 < c)
 *                      and its lower (i + 1 < r) neighbour.
 *     CAVEMAN          the same r: r cliques of n / r consecutive nodes (a prime n: the complete graph).
 *     LADDER           h = n / 2: the paths 0 .. h-1 and h .. 2h-1, the rungs (i, i + h); an odd n adds node n - 1 joined to 0.
 *     LINE             the path 0 - 1 - .. - n-1.            STAR  node 0 joined to every other.
 *     TREE             degree(v) of a word v = the smallest k >= 1 with v * (2k+1)^2 < 2^32 * ((2k+1)^2 - 4), at most n
 *                      (round(paretovariate(2)): P(1) = 5/9, P(k) = 4 / (2k-1)^2 - 4 / (2k+1)^2).  deg[i] = degree(TREE word
 *                      i), i < n.  For s = 0, 1, ..: stop when sum(deg) == 2n - 2; the attempt is REJECTED when
 *                      s == KPGNN_PG_TREE_SWAPS; else deg[below(TREE word n + 2s, n)] = degree(TREE word n + 2s + 1).  The
 *                      graph is nx.degree_sequence_tree(deg): with I the number of degrees above 1, a path 0 .. I+1; its
 *                      inner nodes 1 .. I take those degrees in ascending order and node b of degree k gets the next k - 2
 *                      unused labels, from I + 2 on, as leaves.
 *     CATERPILLAR      B = 1 + below(PARAM word 0, n - 1): the path 0 .. B-1; node i >= B joins below(ATTACH word i, B).
 *     LOBSTER          B as above, F = B + 1 + below(PARAM word 1, n - B); node i in [B, F) joins below(ATTACH word i, B),
 *                      node i in [F, n) joins B + below(ATTACH word i, F - B).
 *   3 relabel   node i becomes the rank of its key ((w1 << 32 | w0) & ~127) | i of W(SHUFFLE, a, i) among the n keys: a
 *               uniform permutation (no ties: the index is in the low 7 bits).  Skipped under KPGNN_PG_NO_SHUFFLE.
 *   4 randomize the reference's `randomize`, with its sum of two uniforms: with e the edges so far, r = n (n - 1) / 2 - e and,
 *               for the pair u > v of the NEW labels, t = w0 + w1 of W(PAIR, a, u (u - 1) / 2 + v) (33 bits),
 *                 e <= r: an edge stays iff 10 t < 9 * 2^33;              a missing one appears iff 10 t r < e * 2^33;
 *                 e >  r: an edge stays iff 10 t e < (10 e - r) * 2^33;   a missing one appears iff 10 t < 2^33.
 *               Skipped under KPGNN_PG_NO_RANDOMIZE.
 *   5 accept    iff every node has a neighbour; otherwise (or after a rejected TREE) a increases by one, and after
 *               max_attempts attempts the graph is EXHAUSTED.
 *   6 output    of the accepted attempt a: source = below(SOURCE word 0, n); feature[i] = (FEATURE word i >> 8) * 2^-24 as
 *               float (exact); row u of the adjacency as two 64-bit words, bit v & 63 of word v >> 6.
 * kpgnn_property_graphs_generate serves the n_ids graphs `graph_ids` of a call of G graphs and writes, for graph g with
 * node_ptr[g] = its first row: rows [N, 2], features [N] and the columns g of info [5, G]: the DIRECTED edge count 2 e, the
 * source, the type, the attempts made and the status.  An EXHAUSTED graph (and, so that a wrong plan cannot write out of
 * bounds, a graph of fewer than 2 nodes or more than the launch's class holds, with attempts 0) gets the edge count 0, the
 * source 0 and no rows or features.  max_nodes <= KPGNN_PG_WAVE_NODES and force_block == 0: a wavefront per graph, four
 * graphs per 256-thread block, no block barrier; else a 256-thread block per graph (up to 128 nodes).  The class changes no bit.
 * kpgnn_property_graphs_fill expands the rows of the same graphs into edge_index [2, E] int64, LOCAL ids, (src, dst)-sorted,
 * graph g at the columns [edge_ptr[g], edge_ptr[g + 1]) of the caller's cumulative sum of info[0]; a graph whose status is
 * not OK or whose count does not fill its columns exactly is skipped.  A wavefront per row, popcount prefixes, no atomics.
 * Limits, answered before any device call: a NULL descriptor, G < 0, n_ids < 0 or > G, max_attempts < 1 or > 2^27,
 * first_graph < 0, an unknown graph_type, unknown flag bits, max_nodes outside [1, 128] or a NULL array with G > 0 are
 * KPGNN_EINVAL; any nodes[g] outside [KPGNN_PG_MIN_NODES, KPGNN_PG_MAX_NODES] is KPGNN_ELIMIT; G == 0 or n_ids == 0 returns
 * KPGNN_OK without a launch.  No atomics, no workspace, and no floating point but the feature conversion.
 * ---------------------------------------------------------------------------------------------- */
enum { KPGNN_PG_OK = 0, KPGNN_PG_EXHAUSTED = 1 };
#define KPGNN_PG_MIN_NODES 2
#define KPGNN_PG_MAX_NODES 128       /* (the bound of kpgnn_graph_labels_large; the reference's splits go to 99) */
#define KPGNN_PG_WAVE_NODES 64       /* nodes up to which a wavefront owns a graph */
#define KPGNN_PG_TREE_SWAPS 5000     /* (the reference's tries=10000 is 5,000 swaps and then an exception) */
enum { KPGNN_PG_RANDOM = 0, KPGNN_PG_ERDOS_RENYI = 1, KPGNN_PG_BARABASI_ALBERT = 2, KPGNN_PG_GRID = 3, KPGNN_PG_CAVEMAN = 5,
       KPGNN_PG_TREE = 6, KPGNN_PG_LADDER = 7, KPGNN_PG_LINE = 8, KPGNN_PG_STAR = 9, KPGNN_PG_CATERPILLAR = 10,
       KPGNN_PG_LOBSTER = 11 };                                          /* the reference's GraphType values */
enum { KPGNN_PG_STREAM_TYPE = 0, KPGNN_PG_STREAM_PARAM = 1, KPGNN_PG_STREAM_PAIR = 2, KPGNN_PG_STREAM_BA = 3,
       KPGNN_PG_STREAM_TREE = 4, KPGNN_PG_STREAM_ATTACH = 5, KPGNN_PG_STREAM_SHUFFLE = 6, KPGNN_PG_STREAM_FEATURE = 7,
       KPGNN_PG_STREAM_SOURCE = 8 };
#define KPGNN_PG_NO_SHUFFLE 1        /* flags: keep the canonical labels */
#define KPGNN_PG_NO_RANDOMIZE 2      /* flags: keep the structure's edges */

typedef struct kpgnn_pg_desc {
    int32_t G, n_ids;               /* graphs of the call; graphs of this launch */
    const int32_t* nodes;           /* HOST [G]: the node counts, checked before any device call */
    const int64_t* node_ptr;        /* device [G+1]: their cumulative sum */
    const int32_t* graph_ids;       /* device [n_ids], or NULL for the graphs 0 .. n_ids-1 */
    int32_t max_nodes;              /* the launch's size class holds graphs up to this many nodes */
    int32_t graph_type, flags, max_attempts;
    int32_t force_block, reserved;  /* nonzero: the block class whatever max_nodes (the same bits; for tests) */
    int64_t seed, first_graph;      /* the Philox key; the id of the call's graph 0 */
    uint64_t* rows;                 /* device [N, 2] */
    float* features;                /* device [N]           (_generate) */
    int32_t* info;                  /* device [5, G]: edges | source | type | attempts | status */
    const int64_t* edge_ptr;        /* device [G+1]         (_fill) */
    int64_t* edge_index;            /* device [2, E]        (_fill) */
    int64_t E;
} kpgnn_pg_desc;

int kpgnn_property_graphs_generate(const kpgnn_pg_desc* d, kpgnn_stream_t stream);
int kpgnn_property_graphs_fill(const kpgnn_pg_desc* d, kpgnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KPGNN_H_ */
