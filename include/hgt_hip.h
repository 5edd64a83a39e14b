/*
 * hgt_hip.h -- C ABI of libhgt_hip.so: MI355X (gfx950) kernels for the forward pass of the
 * Heterogeneous Graph Transformer convolution (acbull/pyHGT, pyHGT/conv.py::HGTConv).
 *
 * Boundary conventions:
 *   - extern "C", plain pointers and sizes, no torch / C++ types in any signature;
 *   - every pointer is a DEVICE pointer unless the parameter name ends in _host;
 *   - every call enqueues work on the given hipStream_t (passed as void*) and returns; nothing
 *     here synchronises the stream, allocates or frees device memory (the caller owns every
 *     buffer, sized with the *_sizes() helpers);
 *   - return value 0 = HGT_OK, negative = error (hgt_strerror()); nothing throws or exits;
 *   - re-entrant and thread-safe as long as concurrent calls use distinct workspaces.
 *
 * Each entry point cites the reference code (file:line under /root/reference) it replaces.
 * The Python binding that calls these through ctypes is pyhgt_amd/_lib.py; the binding a
 * maintainer of the reference would add is shown in INTEGRATION.md.
 */
#ifndef HGT_HIP_H_
#define HGT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HGT_ABI_VERSION 8

/* error codes */
#define HGT_OK 0
#define HGT_ERR_INVALID_ARG (-1)   /* null pointer, negative size, d % n_heads != 0, ... */
#define HGT_ERR_UNSUPPORTED (-2)   /* shape outside what the kernels are instantiated for */
#define HGT_ERR_WORKSPACE (-3)     /* caller-provided buffer too small */
#define HGT_ERR_TOO_LARGE (-4)     /* N or E beyond 32-bit plan indices */
#define HGT_ERR_LAUNCH (-5)        /* HIP runtime reported a launch error */

/* length of the relative-temporal-encoding table, conv.py:287 (max_len = 240) */
#define HGT_RTE_LEN 240

const char* hgt_strerror(int code);
int hgt_abi_version(void);
/* Bit mask of optional parts compiled into this library.  Bit 0 is retired (it announced two experimental kernels that no shipped
 * library ever contained) and is never set.
 * ABI note: with those kernels the export hgt_edge_single_pass_items left the library while HGT_ABI_VERSION stayed 8 -- in a
 * shipped library it answered HGT_ERR_UNSUPPORTED for every call with edges, so no working caller loses anything, and a stale one
 * fails at link time.
 * Bit 1: the atomic-free training entry points (hgt_*_det below): every reduction of the backward pass in an order fixed by the
 * problem sizes alone. */
#define HGT_FEATURE_DETERMINISTIC_TRAINING 2
int hgt_build_features(void);

/* ----------------------------------------------------------------------------------------------
 * Internal "head-padded" feature layout.  Q/K/V/agg rows hold n_heads blocks of dk_pad floats
 * (dk_pad >= d_k = d_out / n_heads, extra columns are zero) so that one 64-lane wavefront covers
 * a row with `vec` contiguous floats per lane and every head maps to dk_pad / vec adjacent lanes.
 * Replaces the .view(-1, n_heads, d_k) of conv.py:96-97,103.
 * Requires: d_out % n_heads == 0, n_heads <= 16.  A head count that does not divide 64 (3, 5, 6, 12: legal in the reference,
 * conv.py:21) runs in the layout of the next power of two `heads`: the extra heads are all-zero and never reach an output.
 * Every kernel-level entry point below takes the LAYOUT head count (`heads`) as its n_heads; hgt_conv_forward, the workspace
 * helpers, hgt_relation_pack and hgt_att_export take the model's real head count as well.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hgt_layout {
    int32_t d_k;     /* d_out / n_heads                         */
    int32_t dk_pad;  /* padded head width                       */
    int32_t d_pad;   /* heads * dk_pad = 64 * vec               */
    int32_t vec;     /* floats per lane (1,2,4,8,16)            */
    int32_t heads;   /* head count of the layout: n_heads rounded up to a power of two (ABI 3) */
} hgt_layout;
int hgt_layout_for(int32_t d_out, int32_t n_heads, hgt_layout* out_host);

/* ----------------------------------------------------------------------------------------------
 * Graph plan: everything that depends only on (edge_index, edge_type, edge_time, node_type).
 * Built once per sampled subgraph and shared by all layers (the reference reuses the same graph
 * tensors for every layer, model.py:78-79).  Replaces, for the whole layer, PyG's per-call
 * index_select gathers (MessagePassing.propagate, called at conv.py:57), the T*T*R boolean mask
 * cube and its host syncs (conv.py:71-84) and the per-type masks of update() (conv.py:121-123):
 *   - edges stably sorted by (dst / TD, relation, dst % TD) (TD = tile size, hgt_plan_constants), ids int64 -> int32,
 *     source-type*240 + edge_time folded into one uint16 per edge;
 *   - a segment table over (dst tile, relation, dst) and a list of wavefront work items
 *     (a bounded run of consecutive edges of one (dst tile, relation));
 *   - nodes stably sorted by type (row lists for the typed linears) + per-type offsets.
 * Edges whose relation id or endpoint node types fall outside [0,R) / [0,T) go to an extra
 * "unclaimed" relation bucket: logit 0, message 0, still part of the softmax -- the behaviour of
 * the reference's zero-initialised res_att / res_msg (conv.py:68-69).
 * ---------------------------------------------------------------------------------------------- */
typedef struct hgt_plan_sizes {
    uint64_t plan_bytes;   /* persistent plan buffer                         */
    uint64_t tmp_bytes;    /* scratch needed only during hgt_plan_build      */
    int64_t  max_items;    /* upper bound on wavefront work items            */
    int64_t  n_bins;       /* (dst tiles) * (R+1) * tile size                */
} hgt_plan_sizes;

int hgt_plan_sizes_for(int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                       hgt_plan_sizes* out_host);
/* build-time constants of the plan: destination tile size and the edge cap of one work item */
int hgt_plan_constants(int32_t* tile_nodes_host, int32_t* item_edges_host);
/* edges per logits work item for a graph of n_edges edges (<= the maximum hgt_plan_constants reports; smaller for small
 * graphs so that enough wavefronts exist) */
int hgt_plan_item_edges(int64_t n_edges, int32_t* item_edges);

/* Row lists exported by a built plan (device pointers INTO the plan buffer), for hgt_typed_linear:
 *   rows_all / off_all : all n_nodes nodes stably sorted by type, int32[n_nodes] / int32[T+2]
 *   rows_q   / off_q   : the target nodes [0, n_q_rows) sorted by type (identical to the above
 *                        when n_q_rows == n_nodes); group T holds nodes with an out-of-range type. */
typedef struct hgt_plan_rows {
    const int32_t* rows_all; const int32_t* off_all;
    const int32_t* rows_q;   const int32_t* off_q;
} hgt_plan_rows;
int hgt_plan_row_lists(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types,
                       int32_t n_relations, hgt_plan_rows* out_host);

/* ABI 6: the per-tile item table of a plan: int32[*n_tiles + 1] at byte offset *offset of the plan buffer; the logits work items of
 * destination tile t (tile_nodes targets each, hgt_plan_constants) are [table[t], table[t + 1]).  pyhgt_amd.dist reads it once per
 * graph to launch the edge phase of ONE target block (hgt_conv_forward stage 5). */
int hgt_plan_tile_items_offset(int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations, uint64_t* offset_host,
                               int64_t* n_tiles_host);

/* edge_index: int64, element (row, e) at edge_index[row * stride_row + e * stride_col]; row 0 =
 * source j, row 1 = target i (conv.py:60-63, data.py:245,254 -- the reference hands over the
 * (1,2)-strided transpose of an [E,2] tensor).  edge_time may be NULL (use_RTE = False).
 * n_q_rows: nodes [0, n_q_rows) are targets that get Q / aggregation / update; nodes beyond are
 * source-only halo rows (multi-GPU destination partitioning); pass n_nodes on a single GPU.
 * Every edge target must be < n_q_rows. */
int hgt_plan_build(const int64_t* edge_index, int64_t stride_row, int64_t stride_col,
                   const int64_t* edge_type, const int64_t* edge_time, const int64_t* node_type,
                   int64_t n_nodes, int64_t n_q_rows, int64_t n_edges, int32_t n_types, int32_t n_relations,
                   void* plan, uint64_t plan_bytes, void* tmp, uint64_t tmp_bytes, void* stream);

/* ABI 5: the first 16 bytes of a plan (int32 n_items, bad_index, n_hubs, n_unknown_q) copied to PINNED host memory without a
 * synchronisation (one hipMemcpyAsync on `stream`): how the host learns "no hub target / no unknown rows / malformed ids". */
int hgt_plan_header_to_host(const void* plan, void* host_dst_pinned, void* stream);

/* Plan from a graph that is ALREADY in the order the reference's sampler produces (data.py:183-209,
 * 227-246): nodes type-contiguous with ascending types (type t = ids [type_off[t], type_off[t+1])), edges grouped by relation
 * (relation r = positions [rel_ptr[r], rel_ptr[r+1]) of src / dst / edge_time) with NON-DECREASING target ids inside a
 * relation, ids already int32.  Builds the same plan as hgt_plan_build (bit-identical arrays; eid = position in the given
 * order) without its radix sorts: seven small launches, no 64-bit index traffic.  pyhgt_amd.sampled.to_device_graph is the
 * sibling of to_torch (data.py:212-256) that emits this form.  Same buffer sizes as hgt_plan_build (hgt_plan_sizes_for).
 * edge_time may be NULL.  All arrays are DEVICE arrays. */
int hgt_plan_from_sorted(const int32_t* src, const int32_t* dst, const int32_t* edge_time, const int32_t* rel_ptr,
                         const int32_t* type_off, int64_t n_nodes, int64_t n_q_rows, int64_t n_edges, int32_t n_types,
                         int32_t n_relations, void* plan, uint64_t plan_bytes, void* tmp, uint64_t tmp_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Typed (grouped) linear layer on MFMA: for every node type t and every row n of that type
 *     y[n, :] = prologue(x[n, :]) @ W[t]^T + b[t]
 * Replaces the per-meta-relation, per-EDGE nn.Linear calls of conv.py:96-97,103 (Q, K, V) and
 * the per-type a_linear of conv.py:125, plus RelTemporalEncoding.lin (conv.py:297-299) when
 * building the temporal tables.  Row lists come from the plan (or any caller-made row list).
 *   x         [*, ldx] fp32 rows, gathered through rows[] (node ids)
 *   rows      int32[n_rows] row ids grouped by type; group g = rows[group_off[g] .. group_off[g+1])
 *   group_off int32[n_groups+1] (device)
 *   W         fp32 [n_groups][n_out][k] with stride w_group_stride floats between groups
 *   bias      fp32 [n_groups][n_out] with stride b_group_stride, or NULL
 *   out0..2   the n_out columns are split into blocks of block_cols columns, block c is written
 *             to out{c}[row * block_cols + col]; row = rows[p] (out_by_position = 0) or p (= 1)
 *   prologue  0 = none, 1 = exact (erf) GELU applied to x on load (conv.py:119); split variants only (ABI 6): 2 = x holds rows in the
 *             24-bit transport format of the multi-GPU exchange (hgt_gather_rows_c24; ldx = 3 k / 4 dwords, k <= 256, k % 4 == 0),
 *             decoded by the kernel's loader -- the halo rows a rank receives are projected straight off the wire buffer.
 *             Split variants: | HGT_LINEAR_FORCE_XS takes the x-stationary kernel (hgt_gemm_xs.hip) for every shape it covers
 *             whatever the row count (default: from 262 144 rows, K = 512 from 65 536), | HGT_LINEAR_NO_XS never takes it -- the
 *             two kernels are bit-identical; the bits exist for tests and A/B timings (no environment variable is read)
 *   precision must be 0 (fp32 MFMA, exact fp32 FMA chain); the split-bf16 variant is below
 * ---------------------------------------------------------------------------------------------- */
#define HGT_LINEAR_FORCE_XS 0x100
#define HGT_LINEAR_NO_XS 0x200
#define HGT_LINEAR_TANH 0x1000     /* ABI 7, split variants: tanh applied to the output (model.py:70-76: the GNN's typed adapter + tanh in one kernel).
                                    * Only the latency-regime tile kernel and the K > 256 slab kernel carry it: HGT_ERR_UNSUPPORTED otherwise (and
                                    * nothing launched) -> plain call + hgt_tanh_inplace */
#define HGT_LINEAR_NO_TILE 0x400   /* ABI 7: never the latency-regime tile kernel (hgt_gemm_tile.hip; the default for up to HGT_TILE_MAX_ROWS = 16 384
                                    * rows and at most 64 groups: K <= 256 with at most 1 024 workgroups, K > 256 when all tiles are resident at
                                    * once) -- bit-identical to the slab kernels; the bit exists for tests and A/B timings.  (Not covered by
                                    * this: k_merge_update16, a merge update of hgt_edge_aggregate_items_update, whose sums differ from its
                                    * 32 x 32 form's in the last bits.) */
int hgt_typed_linear(const float* x, int64_t ldx, const int32_t* rows, const int32_t* group_off,
                     int32_t n_groups, int64_t n_rows, int32_t k, int32_t n_out,
                     const float* W, int64_t w_group_stride, const float* bias, int64_t b_group_stride,
                     float* out0, float* out1, float* out2, int32_t block_cols,
                     int32_t out_by_position, int32_t prologue, int32_t precision, void* stream);

/* Split-bf16 x3 variant of the typed linear layer (same contract as hgt_typed_linear): operands are
 * split into bf16 hi+mid terms and a product is evaluated as mid*hi + hi*mid + hi*hi on the bf16 matrix
 * cores with fp32 accumulation (relative error of a product <= ~3*2^-18).  W is split and tiled once per
 * forward by hgt_split_weights into a caller-owned buffer of hgt_split_weights_bytes() bytes. */
int hgt_split_weights_bytes(int32_t n_groups, int32_t k, int32_t n_out, uint64_t* out_host);
int hgt_split_weights(const float* W, int64_t w_group_stride, int32_t n_groups, int32_t k, int32_t n_out,
                      void* w_split, void* stream);
int hgt_typed_linear_bf16x3(const float* x, int64_t ldx, const int32_t* rows, const int32_t* group_off,
                            int32_t n_groups, int64_t n_rows, int32_t k, int32_t n_out, const void* w_split,
                            const float* bias, int64_t b_group_stride, float* out0, float* out1, float* out2,
                            int32_t block_cols, int32_t out_by_position, int32_t prologue, void* stream);

/* fp16 hi / lo variant of the split products (ABI 5, precision "f16x3"): the same three MFMAs per step with 11 + 11 mantissa bits
 * per operand instead of 8 + 8 (relative error of a product ~2^-22: the layer's output is within ~3e-7 of the fp64 result), at the
 * same cost.  fp16 has 5 exponent bits, so every x row is scaled by a power of two (found on the fly) and every weight group by
 * one (found by hgt_split_weights_f16, kept in the image's tail); the inverse scales go onto the fp32 accumulators.  Same
 * arguments and the same image size (hgt_split_weights_bytes) as the bf16 functions; an image must be used with its own kind. */
int hgt_split_weights_f16(const float* W, int64_t w_group_stride, int32_t n_groups, int32_t k, int32_t n_out,
                          void* w_split, void* stream);
int hgt_typed_linear_f16x3(const float* x, int64_t ldx, const int32_t* rows, const int32_t* group_off,
                           int32_t n_groups, int64_t n_rows, int32_t k, int32_t n_out, const void* w_split,
                           const float* bias, int64_t b_group_stride, float* out0, float* out1, float* out2,
                           int32_t block_cols, int32_t out_by_position, int32_t prologue, void* stream);

/* Introspection (host only, no GPU): the work decomposition of the x-stationary kernel behind hgt_typed_linear_bf16x3 / _f16x3 on
 * large inputs (csrc/hgt_gemm_xs.hip), enumerated with the kernel's own scheduling helpers.  group_off_host = the [n_groups + 1]
 * offsets as a HOST array, n_cu = number of workgroups the launch may use (the device's CU count), k selects the form (512: four
 * wavefronts per workgroup, otherwise eight).  items[i] = {workgroup, round, wavefront, group, first position in the row list,
 * rows (1..32)}; *n_items = number of entries the schedule has; HGT_ERR_TOO_LARGE (with *n_items set) if max_items is smaller.
 * Replaces nothing in the reference (its Linear layers have no decomposition to inspect); it exists so that the partition of the row
 * list -- every position exactly once, no round mixing two groups -- is tested on the CPU (tests/test_xs_schedule.py). */
int hgt_typed_linear_xs_schedule(const int32_t* group_off_host, int32_t n_groups, int64_t n_rows, int32_t k, int32_t n_cu,
                                 int32_t* items_host, int64_t max_items, int64_t* n_items_host);

/* a_linear (conv.py:125) with the node update (conv.py:129-133, see hgt_node_update) fused into its epilogue:
 *   out[n] = LN_t( (agg[n] @ W_a[t]^T + b_a[t]) * sigmoid(skip[t]) + x_skip[n] * (1 - sigmoid(skip[t])) )
 * for the rows of every group; split-bf16 x3 MFMA; needs n_out % 4 == 0 and n_out <= 256, or n_out <= 512 with k <= 512 (round 5:
 * both 256-column passes of a row tile stay in registers, LayerNorm over the two together) -- HGT_ERR_UNSUPPORTED otherwise -> use
 * hgt_typed_linear[_bf16x3] + hgt_node_update.  Rows of no group are not written: hgt_zero_rows. */
int hgt_linear_update_bf16x3(const float* agg, int64_t ld_agg, const int32_t* rows, const int32_t* group_off,
                             int32_t n_groups, int64_t n_rows, int32_t k, int32_t n_out, const void* w_split,
                             const float* bias, int64_t b_group_stride, const float* x_skip, int64_t ld_skip,
                             const float* skip, const float* ln_w, const float* ln_b, int32_t use_norm, float* out,
                             void* stream);
/* the same on an fp16 hi / lo image (hgt_split_weights_f16) */
int hgt_linear_update_f16x3(const float* agg, int64_t ld_agg, const int32_t* rows, const int32_t* group_off,
                            int32_t n_groups, int64_t n_rows, int32_t k, int32_t n_out, const void* w_split,
                            const float* bias, int64_t b_group_stride, const float* x_skip, int64_t ld_skip,
                            const float* skip, const float* ln_w, const float* ln_b, int32_t use_norm, float* out,
                            void* stream);
/* out[rows[i]][0..d) = 0 for i in [range[0], range[1]) -- range is a DEVICE array of two int32 */
int hgt_zero_rows(const int32_t* rows, const int32_t* range, int32_t d, float* out, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Relation parameter packing (per forward, R*H*dk*dk elements):
 *   att_t[r][h][c][k] = relation_att[r][h][k][c] * relation_pri[r][h] / sqrt(d_k)   (zero padded; heads >= n_heads: zero)
 *   msg_p[r][h][k][c] = relation_msg[r][h][k][c]                                     (zero padded)
 * both [R][H][dk_pad][dk_pad].  Folds conv.py:99's "* relation_pri / sqrt_dk" into the matrix and
 * transposes relation_att so that  q . (k A) = (A q) . k  can be evaluated on the target side.
 * ---------------------------------------------------------------------------------------------- */
int hgt_relation_pack(const float* relation_att, const float* relation_msg, const float* relation_pri,
                      int32_t n_relations, int32_t n_heads, int32_t n_heads_layout, int32_t d_k, int32_t dk_pad,
                      float* att_t, float* msg_p, void* stream);
/* n_heads = heads of the parameter tensors, n_heads_layout >= n_heads = heads of att_t / msg_p (extra heads: zero matrices) */

/* ----------------------------------------------------------------------------------------------
 * Edge phase (replaces conv.py:98-99,104,108-111 and PyG's scatter-add, conv.py:13 aggr='add').
 * All feature rows are in the head-padded layout, row stride d_pad.
 *   hgt_edge_logits    s[p][h] = (A'[rel] q[dst])_h . (K[src] + rte_k[src_type, dt])_h  for every
 *                      sorted edge position p (conv.py:98-99); unclaimed edges get 0
 *   hgt_edge_softmax   in place: s -> exp(s - max_i) / (sum_i exp(s - max_i) + 1e-16) over all
 *                      in-edges of each target, per head (PyG softmax, conv.py:108)
 *   hgt_edge_aggregate takes the RAW logits of hgt_edge_logits and evaluates the per-target softmax
 *                      online (same formula as above) while aggregating:
 *                      agg[i] = sum_rel (sum_{e in (i,rel)} att_e (V[src] + rte_v[...])) M[rel]
 *                      (conv.py:104,108-111 + scatter-add) for every target i < n_q_rows (isolated
 *                      targets get 0); apply_gelu != 0 stores gelu(agg) instead (conv.py:119).
 *                      hgt_edge_softmax is only needed to materialise att for hgt_att_export.
 *   hgt_att_export     att_out[original edge id][h] = att[p][h]   (self.att, conv.py:108)
 * rte_k / rte_v: [n_types*240][d_pad] tables or NULL.
 * n_edges == 0: the per-edge arrays (logits, logits_att, att_sorted, att_out; in the backward pass att, d_att, d_logits,
 * by_edge_id, sorted; the weights of hgt_edge_spmm / hgt_relation_outer) may be NULL -- an empty array has no address -- and
 * hgt_edge_logits*, hgt_edge_softmax, hgt_att_export, hgt_edge_softmax_bwd and hgt_edge_gather_sorted launch nothing.  With edges a
 * NULL per-edge array is HGT_ERR_INVALID_ARG, and every other argument is checked with or without edges.
 * ---------------------------------------------------------------------------------------------- */
int hgt_edge_logits(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                    int32_t n_heads, int32_t dk_pad, const float* Q, const float* K, const float* rte_k,
                    const float* att_t, float* logits, void* stream);
/* ABI 5: the same logits with the target-side transform  q~ = q A'[r]  on the matrix cores: att_frag = hgt_relation_frag_pack(att_t)
 * (frag_f16 = 0) or hgt_relation_frag_pack_f16(att_t) (frag_f16 = 1), 16 distinct targets of a work item at a time, 3-term split
 * products like the aggregation's.  The form for d_k >= 64 (the reference's own widths: n_hid 400 / 512 with 8 heads), where the
 * vector-ALU kernel needs a 4-way head-group split and is instruction-bound; layouts it does not cover fall through to
 * hgt_edge_logits (att_t is required for that).
 * frag_f16 bits (ABI 7, here and in hgt_edge_aggregate_items[_update]): bit 0 = the fp16 images; for d_k >= 64 (the runs kernel of the
 * item-parallel aggregation: >= 32) and the 16-edge work items of a sampled batch the four wavefronts of a workgroup SHARE the relation transform (a quarter of the fragment image each, kept
 * in registers while consecutive items share the relation; same result bit for bit): bit 1 = never, bit 2 = for larger items too. */
int hgt_edge_logits_mfma(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                         int32_t n_heads, int32_t dk_pad, const float* Q, const float* K, const float* rte_k,
                         const float* att_t, const void* att_frag, int32_t frag_f16, float* logits, void* stream);
/* The same logits with the relation transform on the SOURCE operand, per edge, on the matrix cores:
 *   s_e,h = < q_i,h , A'[r,h]^T k_j,h >,  32 edges of a work item x one head = one v_mfma_f32_32x32x16_f16 product (two k-steps, three
 *   fp16 hi / lo terms), the edge on the lane; no target segments (csrc/hgt_edge_logits_kside.hip).  The form for graphs with short
 *   (target, relation) segments at d_k <= 32.
 * att_kside = hgt_relation_kside_pack(att_t): hgt_relation_kside_bytes bytes (0: the layout is not covered), the A operands of every
 *   (relation, head) block as fp16 hi / lo of att_t * 2^s with one power-of-two scale per block, and the blocks' exponents behind them.
 *   The K rows are scaled per (row, head) and the Q rows per (row, head) by exact powers of two inside the kernel, so the result is
 *   finite whenever the fp32 logit is, whatever the magnitudes; the same image and arithmetic serve both split precisions
 *   (att_t is not read; of frag_f16 only bit 3 is: the per-lane gather of HGT_FLAG_KSIDE_LANE_GATHER, same logits bit for bit).
 * Covered: dk_pad == 32, n_heads (layout heads) 2, 4 or 8 (rows of at most 256 padded columns), rte_k == NULL, and
 *   n_nodes * n_heads * dk_pad * 4 < 2^32 (every Q / K row below 4 GiB from its base).  HGT_ERR_UNSUPPORTED otherwise: the caller
 *   takes hgt_edge_logits / hgt_edge_logits_mfma.  Edges of the unclaimed bucket get logit 0.  No atomics: bit-reproducible. */
int hgt_relation_kside_bytes(int32_t n_relations, int32_t n_heads, int32_t dk_pad, uint64_t* out_host);
int hgt_relation_kside_pack(const float* att_t, int32_t n_relations, int32_t n_heads, int32_t dk_pad, void* att_kside, void* stream);
int hgt_edge_logits_kside(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                          int32_t n_heads, int32_t dk_pad, const float* Q, const float* K, const float* rte_k,
                          const float* att_t, const void* att_kside, int32_t frag_f16, float* logits, void* stream);
/* Host only (no GPU): the index maps of that image and of the kernel's lanes (csrc/hgt_kside_map.h), for tests.
 *   image_map[p][4] = {block, term (0 hi, 1 lo), output, k} of f16 element p, p < n_blocks * 2048 (block = relation * n_heads + head);
 *   b_col[k-step 2][lane 64][8] = the column of the head a lane supplies as element j of the B operand;
 *   c_out[lane 64][16] = the output a lane receives in accumulator register reg.  Any of the three may be NULL. */
int hgt_kside_image_map(int32_t n_blocks, int32_t* image_map, int32_t* b_col, int32_t* c_out);
/* Host only (no GPU): how the kernel's lanes gather a batch of 32 edges x one 128-byte head line through LDS (4 pieces of 1 KB).
 *   dma_map[piece 4][lane 64][2] = {edge of the batch, 16-byte chunk of the head line} a lane fetches; it lands at 1024 piece + 16 lane;
 *   read_map[read 4][lane 64][3] = {LDS byte offset, edge, chunk}: where the lane's i-th 16-byte read goes and what it must find.
 * Either may be NULL. */
int hgt_kside_gather_map(int32_t* dma_map, int32_t* read_map);
/* ABI 6: the work items [item_begin, item_end) only = the items of a range of destination tiles (hgt_plan_tile_items_offset): the
 * logits of ONE target block of the multi-GPU path.  att_frag may be NULL (vector-ALU kernel). */
int hgt_edge_logits_range(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                          int32_t n_heads, int32_t dk_pad, const float* Q, const float* K, const float* rte_k,
                          const float* att_t, const void* att_frag, int32_t frag_f16, float* logits, int32_t item_begin,
                          int32_t item_end, void* stream);
int hgt_edge_softmax(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                     int32_t n_heads, float* logits_att, void* stream);
int hgt_edge_aggregate(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                       int32_t n_heads, int32_t dk_pad, const float* logits, const float* V, const float* rte_v,
                       const float* msg_p, const void* msg_frag, float* agg, int64_t n_q_rows, int32_t apply_gelu,
                       void* hub_ws, void* stream);
/* ABI 5, latency regime (sampled sub-graphs): the same aggregate (after it agg equals hgt_edge_aggregate's up to fp32 rounding), item-
 * parallel: one wavefront per logits work item sums the runs of consecutive same-target edges, transforms 16 runs per matrix-core
 * round and writes them to `scratch` (hgt_edge_aggregate_items_bytes); a second kernel combines every target's runs in (relation,
 * position) order like softmax partials.  No atomics, fixed order: bit-reproducible; hub targets need no hub_ws.  msg_frag is
 * required (frag_f16: which of hgt_relation_frag_pack / _f16 made it); apply_gelu 0 / 1; n_relations < 64. */
int hgt_edge_aggregate_items_bytes(int64_t n_edges, int32_t n_heads, int32_t dk_pad, uint64_t* out_host);
int hgt_edge_aggregate_items(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                             int32_t n_heads, int32_t dk_pad, const float* logits, const float* V, const float* rte_v,
                             const void* msg_frag, int32_t frag_f16, float* agg, int64_t n_q_rows, int32_t apply_gelu,
                             void* scratch, uint64_t scratch_bytes, void* stream);
/* ABI 7: hgt_edge_aggregate_items whose merge pass IS the node update (sampled batches: one of the layer's five dependent kernels less and the
 * merged rows never written): per target the runs are merged exactly like hgt_edge_aggregate_items merges them (apply_gelu = 1), the row is
 * multiplied with W_a[type] on the matrix cores (split x3 like hgt_linear_update_*; w_a_split = hgt_split_weights[_f16](W_a) with
 * k = n_heads * dk_pad; frag_f16 selects the fp16 images of BOTH msg_frag and w_a_split) and the gated skip + LayerNorm of conv.py:129-133
 * is applied: out[n] for every row n of rows[] (rows / group_off: target rows grouped by node type, hgt_plan_row_lists rows_q / off_q).
 * Output identical to hgt_edge_aggregate_items + hgt_linear_update_*.  HGT_ERR_UNSUPPORTED: rows wider than 512 padded columns,
 * n_out > 512 or > the padded row, n_out % 4 != 0, ld_skip % 4 != 0 -> use the two-call form. */
int hgt_edge_aggregate_items_update(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                                    int32_t n_heads, int32_t dk_pad, const float* logits, const float* V, const float* rte_v,
                                    const void* msg_frag, int32_t frag_f16, int64_t n_q_rows, void* scratch, uint64_t scratch_bytes,
                                    const int32_t* rows, const int32_t* group_off, int32_t n_groups, const void* w_a_split,
                                    const float* b_a, const float* x_skip, int64_t ld_skip, const float* skip, const float* ln_w,
                                    const float* ln_b, int32_t use_norm, int32_t n_out, float* out, void* stream);
/* ABI 4: one slice [rel_lo, rel_hi) of the plan's n_relations + 1 relation buckets (bucket n_relations = unclaimed edges).
 * hgt_edge_logits_slice writes the logits of the slice's edges only.  hgt_edge_aggregate_slice (matrix-core kernel: msg_frag
 * required) aggregates the slice and combines it with what earlier slices left: state = f32[n_q_rows][n_heads][2] (softmax
 * reference, exp-sum) and the un-normalised rows in agg; has_prev = 0 for the first slice; more != 0: leave state + raw rows
 * for the next slice, more = 0: normalise (+ gelu) -- after it agg equals hgt_edge_aggregate's over all slices (partials merge as
 * m = max(m_a, m_b), x = x_a e^(m_a - m) + x_b e^(m_b - m): exact up to fp32 rounding).  Hub targets are processed with the
 * last slice, over all relations. */
int hgt_edge_logits_slice(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                          int32_t n_heads, int32_t dk_pad, const float* Q, const float* K, const float* rte_k,
                          const float* att_t, float* logits, int32_t rel_lo, int32_t rel_hi, void* stream);
int hgt_edge_aggregate_slice(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                             int32_t n_heads, int32_t dk_pad, const float* logits, const float* V, const float* rte_v,
                             const float* msg_p, const void* msg_frag, float* agg, int64_t n_q_rows, int32_t apply_gelu,
                             void* hub_ws, int32_t rel_lo, int32_t rel_hi, float* state, int32_t has_prev, int32_t more,
                             void* stream);
/* hgt_edge_aggregate_slice with hub_deterministic != 0: the hub targets (last slice) take the deterministic hub mode of
 * HGT_FLAG_DETERMINISTIC_HUBS (hub_ws of hgt_hub_workspace_bytes_ex(.., deterministic = 1) bytes); hgt_conv_forward stage 4 uses it */
int hgt_edge_aggregate_slice_ex(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                                int32_t n_heads, int32_t dk_pad, const float* logits, const float* V, const float* rte_v,
                                const float* msg_p, const void* msg_frag, float* agg, int64_t n_q_rows, int32_t apply_gelu,
                                void* hub_ws, int32_t rel_lo, int32_t rel_hi, float* state, int32_t has_prev, int32_t more,
                                int32_t hub_deterministic, void* stream);
/* msg_frag (ABI 3): hgt_relation_frag_pack(msg_p) = the relation message matrices as bf16 hi/mid MFMA fragments.  Non-NULL:
 * the per-(target, relation) transforms  (sum att_e v_e) M[rel]  run on the matrix cores, 16 targets x one relation at a time,
 * as 3-term split-bf16 products with fp32 accumulation (relative error of a product <= ~3*2^-18, like the split-bf16 typed
 * linears).  NULL: exact fp32 mat-vecs on the vector ALU (the round-1 kernel; also taken for a head wider than 256 columns). */
int hgt_relation_frag_bytes(int32_t n_relations, int32_t n_heads, int32_t dk_pad, uint64_t* out_host);
int hgt_relation_frag_pack(const float* msg_p, int32_t n_relations, int32_t n_heads, int32_t dk_pad, void* msg_frag, void* stream);
/* fp16 hi / lo variant (ABI 5, precision "f16x3"; see hgt_split_weights_f16): the fragments hold M * s with ONE power-of-two s for
 * all relations (everything summed into one accumulator must share it; 1/s sits behind the fragments, hgt_relation_frag_bytes
 * counts it), the rows  sum att_e v_e  of a target are scaled by one power of two per target, chosen when its first row is
 * formed (2^7 of headroom, moved with an exact rescale of the accumulator column if a later relation needs more), and both
 * inverses join the softmax normalisation.  Relative error of a transform ~2^-22.  hgt_edge_aggregate_f16x3 takes the f16 image
 * (required); slices, hgt_edge_spmm and the hub path (exact fp32) are unchanged. */
int hgt_relation_frag_pack_f16(const float* msg_p, int32_t n_relations, int32_t n_heads, int32_t dk_pad, void* msg_frag, void* stream);
int hgt_edge_aggregate_f16x3(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                             int32_t n_heads, int32_t dk_pad, const float* logits, const float* V, const float* rte_v,
                             const float* msg_p, const void* msg_frag, float* agg, int64_t n_q_rows, int32_t apply_gelu,
                             void* hub_ws, void* stream);
/* hub_ws: scratch of hgt_hub_workspace_bytes() bytes for targets with more than 1024 in-edges ("hubs"): their edge
 * ranges are split over many wavefronts (max / sum-exp / weighted sum accumulated with atomics) instead of being
 * walked by the one wavefront that owns their 16-target sub-tile.  NULL = no hub path (correct, slow on hubs). */
int hgt_hub_workspace_bytes(int64_t n_edges, int32_t n_heads, int32_t dk_pad, uint64_t* out_host);
/* ABI 6: deterministic != 0 adds one partial slot per piece, (n_relations + 1) x 32 pieces per possible hub (n_edges / 1024 + 1 of them):
 * about 0.28 * n_edges * (H * dk_pad + H) * 4 bytes.  hgt_edge_aggregate_ex / hgt_edge_aggregate_update_range take such a buffer with
 * hub_deterministic = 1. */
int hgt_hub_workspace_bytes_ex(int64_t n_edges, int32_t n_heads, int32_t dk_pad, int32_t n_relations, int32_t deterministic,
                               uint64_t* out_host);
int hgt_edge_aggregate_ex(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                          int32_t n_heads, int32_t dk_pad, const float* logits, const float* V, const float* rte_v,
                          const float* msg_p, const void* msg_frag, int32_t frag_f16, float* agg, int64_t n_q_rows, int32_t apply_gelu,
                          void* hub_ws, int32_t hub_deterministic, void* stream);
int hgt_att_export(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                   int32_t n_heads, const float* att_sorted, float* att_out, int32_t n_heads_out, void* stream);
/* att_sorted [E][n_heads] (layout heads) -> att_out [E][n_heads_out] (the first n_heads_out heads; the model's real heads) */

/* ----------------------------------------------------------------------------------------------
 * Node update epilogue (conv.py:129-133): per node n of type t (rows with a type outside [0,T)
 * are written as zeros, like the reference's zero-initialised `res`, conv.py:120):
 *     y = trans[n] * sigmoid(skip[t]) + x[n] * (1 - sigmoid(skip[t]));
 *     out[n] = use_norm ? LayerNorm(y; ln_w[t], ln_b[t], eps 1e-5) : y
 * ---------------------------------------------------------------------------------------------- */
int hgt_node_update(const float* trans, const float* x, int64_t ldx, const int64_t* node_type,
                    const float* skip, const float* ln_w, const float* ln_b, int32_t use_norm,
                    int64_t n_nodes, int32_t d, int32_t n_types, float* out, void* stream);

/* Generalised form used by DenseHGTConv (conv.py:250-274): skip == NULL -> plain residual y = trans[n] + x[n]
 * (conv.py:259,271); ln_shared != 0 -> one LayerNorm for every type (out_norm, conv.py:272), ln_w/ln_b are [d].
 * out may alias x (every row is read completely before it is written). */
int hgt_node_update_ex(const float* trans, const float* x, int64_t ldx, const int64_t* node_type,
                       const float* skip, const float* ln_w, const float* ln_b, int32_t use_norm, int32_t ln_shared,
                       int64_t n_nodes, int32_t d, int32_t n_types, float* out, void* stream);

/* x[i] = tanh(x[i]) in place: the activation of the typed input adapter of model.GNN (model.py:70-76) */
int hgt_tanh_inplace(float* x, int64_t n, void* stream);

/* Task heads of model.py, used by pyhgt_amd.Classifier / Matcher on the seed rows:
 *   hgt_log_softmax_rows: out[r] = log_softmax(x[r])   (torch.log_softmax(..., dim=-1), model.py:11)
 *   hgt_row_dot:          out[r] = scale * <x[r], y[r]> (Matcher pair=True, model.py:41,44) */
int hgt_log_softmax_rows(const float* x, int64_t n_rows, int32_t n_cols, float* out, void* stream);
int hgt_row_dot(const float* x, const float* y, int64_t n_rows, int32_t d, float scale, float* out, void* stream);

/* row gather used to pack halo rows for the multi-GPU exchange: out[i] = x[idx[i]] */
int hgt_gather_rows(const float* x, int64_t ldx, const int32_t* idx, int64_t n, int32_t d, float* out, void* stream);
/* The inverse of hgt_gather_rows with an addition: gradients of halo rows return to the rows' owners (pyhgt_amd.dist,
 * HaloPlan.return_grads).  src [*, ld_src] holds the received rows in the order of the rank's send list; rows int32[n_rows] the
 * DISTINCT destination rows that receive something, ptr int32[n_rows + 1] / pos int32[ptr[n_rows]] the CSR list of the source rows of
 * each (HaloPlan.return_index):
 *   dst[rows[i]][0..d) += src[pos[ptr[i]]] + ... + src[pos[ptr[i+1]-1]], added one after the other in that order, starting
 * from dst's value; rows[] holds DISTINCT row ids, so no two wavefronts write one row: no atomics, bits fixed by the lists.
 * Plain fp32 adds.  Any d >= 1 (ld_src, ld_dst >= d): 16-byte accesses where d, both leading dimensions and both pointers allow it,
 * scalar ones otherwise.  Rows not listed (and listed rows with an empty range) are not touched.  No allocation, no synchronisation;
 * n_rows == 0 returns HGT_OK without a launch (additive export at ABI 8). */
int hgt_scatter_add_rows(const float* src, int64_t ld_src, const int32_t* rows, const int32_t* ptr, const int32_t* pos,
                         int64_t n_rows, int32_t d, float* dst, int64_t ld_dst, void* stream);
/* The same rows in a 24-bit transport format (sign, 8 exponent, 15 mantissa bits, round to nearest: relative error <= 2^-16;
 * 3*d bytes per row, d % 4 == 0) and its inverse: the multi-GPU exchange is bound by the links, and halo rows only feed the
 * K/V projections. */
int hgt_gather_rows_c24(const float* x, int64_t ldx, const int32_t* idx, int64_t n, int32_t d, void* out, void* stream);
int hgt_unpack_rows_c24(const void* in, int64_t n, int32_t d, float* out, int64_t ld_out, void* stream);

/* hgt_edge_aggregate with HGTConv's node update (conv.py:119-133) fused in: the workgroup that aggregated 64 targets
 * multiplies their gelu'd rows with W_a on the matrix cores (split-bf16 x3, w_a_split = hgt_split_weights(W_a,
 * k = H*dk_pad, n_out)) and writes
 *     out[i] = LN_t( (gelu(agg_i) W_a[t]^T + b_a[t]) * sigmoid(skip[t]) + x_skip[i] * (1 - sigmoid(skip[t])) ),
 * rows of unknown type = 0, so agg never goes through HBM.  Needs H*dk_pad <= 256, n_out % 4 == 0 and a layout without
 * head-group split (HGT_ERR_UNSUPPORTED otherwise -> hgt_edge_aggregate + hgt_linear_update_bf16x3).
 * `agg` [n_q_rows][H*dk_pad] and `pending` [(n_q_rows+63)/64] int32 are scratch: workgroups that contain a hub target
 * (hub_ws != NULL) finish through agg and the hub kernels, exactly like hgt_edge_aggregate, and are updated last. */
int hgt_edge_aggregate_update(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                              int32_t n_heads, int32_t dk_pad, const float* logits, const float* V, const float* rte_v,
                              const float* msg_p, const void* msg_frag, float* agg, int64_t n_q_rows, void* hub_ws, int32_t* pending,
                              const int64_t* node_type, const void* w_a_split, const float* b_a, const float* x_skip,
                              int64_t ld_skip, const float* skip, const float* ln_w, const float* ln_b, int32_t use_norm,
                              int32_t n_out, float* out, void* stream);
/* the same with the fp16 hi / lo images: msg_frag = hgt_relation_frag_pack_f16, w_a_split = hgt_split_weights_f16 (both required) */
int hgt_edge_aggregate_update_f16x3(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                                    int32_t n_heads, int32_t dk_pad, const float* logits, const float* V, const float* rte_v,
                                    const float* msg_p, const void* msg_frag, float* agg, int64_t n_q_rows, void* hub_ws,
                                    int32_t* pending, const int64_t* node_type, const void* w_a_split, const float* b_a,
                                    const float* x_skip, int64_t ld_skip, const float* skip, const float* ln_w, const float* ln_b,
                                    int32_t use_norm, int32_t n_out, float* out, void* stream);

/* ABI 6: hgt_edge_aggregate_update for the targets [q_begin, q_end) only (q_begin a multiple of the plan tile, q_end <= n_q_rows):
 * one TARGET BLOCK of the multi-GPU path, whose in-edges only reference source rows that have already arrived.  `pending` must hold
 * (n_q_rows + 63) / 64 entries like in the whole-graph call: the kernels index it by ABSOLUTE 64-row tile (q_begin / 64 + workgroup),
 * so that target blocks of one layer may run concurrently.  Matrix-core kernel only (msg_frag required).  frag_f16: msg_frag / w_a_split are the fp16 images;
 * hub_deterministic: see HGT_FLAG_DETERMINISTIC_HUBS. */
int hgt_edge_aggregate_update_range(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                                    int32_t n_heads, int32_t dk_pad, const float* logits, const float* V, const float* rte_v,
                                    const float* msg_p, const void* msg_frag, float* agg, int64_t n_q_rows, void* hub_ws,
                                    int32_t* pending, const int64_t* node_type, const void* w_a_split, const float* b_a,
                                    const float* x_skip, int64_t ld_skip, const float* skip, const float* ln_w, const float* ln_b,
                                    int32_t use_norm, int32_t n_out, float* out, void* stream, int64_t q_begin, int64_t q_end,
                                    int32_t frag_f16, int32_t hub_deterministic);

/* ----------------------------------------------------------------------------------------------
 * Backward pass (the reference gets it from autograd: OAG/train_paper_field.py:249,
 * ogbn-mag/train_ogbn_mag.py:172).  The chain rule on the node-level algebra of the forward needs three more edge
 * primitives, all of them "forward kernels in disguise" (pyhgt_amd/autograd.py strings them together):
 *   hgt_edge_spmm        out[i] = sum_rel ( sum_{e in (i,rel)} w_e (rows[src_e] + rte_rows[..]) ) F[rel]   -- the aggregation
 *                        kernel with GIVEN edge weights (sorted edge order of `plan`) instead of the softmax; F = f_p
 *                        (hgt_relation_pack layout, [R][H][dk_pad][dk_pad], out = in . F) and its MFMA image f_frag
 *                        (hgt_relation_frag_pack).  dQ = spmm(plan, ds, K, A'), dK = spmm(plan^T, ds, Q, A'^T),
 *                        dV = spmm(plan^T, att, dagg, M^T) where plan^T is the plan of the reversed edges.
 *   hgt_edge_logits      (existing) with (Q, K, att_t) := (dagg, V, M^T) yields d att_e = <dagg_i M^T, v_e>
 *   hgt_edge_softmax_bwd d s_e = att_e (d att_e - rho[dst_e]),  rho = hgt_head_dot(dagg, agg)
 *   hgt_relation_outer   out[r][h][k][c] += sum_{e of relation r} w_e a[src_e][h][k] b[dst_e][h][c]  (d relation_msg, d A')
 *   hgt_edge_gather_sorted  values given per ORIGINAL edge id -> sorted edge order of a plan (inverse of hgt_att_export)
 * and the dense pieces:
 *   hgt_node_update_bwd  reverse of hgt_node_update (+ the dropout mask of conv.py:125): d_trans, dx (skip path, overwritten),
 *                        d_alpha[t] += sum dy (o - x) (d skip = d_alpha * a (1 - a)), d_ln_w / d_ln_b [T][d] += ...
 *   hgt_gelu_bwd         out = dg * gelu'(agg)           hgt_mul_inplace   x *= m (dropout mask)
 *   hgt_typed_wgrad      out[g][m][n] += sum_{rows p of group g} A[rows[p]][m] B[rows[p]][n]   (exact fp32 MFMA; fp32 atomics)
 *   hgt_typed_colsum     out[g][c]    += sum_{rows p of group g} A[rows[p]][c]                  (bias gradients)
 * Accumulating outputs (+=) must be zeroed by the caller.
 * n_edges == 0 (a sampled batch without edges): att / d_att / d_logits of hgt_edge_softmax_bwd and by_edge_id / sorted of
 * hgt_edge_gather_sorted may be NULL like the weights of hgt_edge_spmm and hgt_relation_outer; both return HGT_OK without a launch
 * (rho is per node and required).
 * ---------------------------------------------------------------------------------------------- */
int hgt_edge_spmm(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations, int32_t n_heads,
                  int32_t dk_pad, const float* weights, const float* rows, const float* rte_rows, const float* f_p,
                  const void* f_frag, float* out, int64_t ld_out, int64_t n_q_rows, void* hub_ws, void* stream);
/* ABI 7: the same sums on the item-parallel kernels of the latency regime (hgt_edge_aggregate_items with the edge weights given): one
 * wavefront per <= 16-edge work item + a fixed-order merge per target, no atomics; scratch = hgt_edge_aggregate_items_bytes().  What
 * pyhgt_amd/autograd.py takes below 65 536 nodes (the sub-tile kernel's wavefronts walk sixteen targets' edges one after the other:
 * 285 us per call on the transposed plan of a 3 200-node sampled batch against ~25 us).  HGT_ERR_UNSUPPORTED: > 63 relations, rows wider
 * than 512 padded columns, ld_out % 4 != 0, out not 16-byte aligned -> hgt_edge_spmm. */
int hgt_edge_spmm_items(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations, int32_t n_heads,
                        int32_t dk_pad, const float* weights, const float* rows, const float* rte_rows, const void* f_frag, float* out,
                        int64_t ld_out, int64_t n_q_rows, void* scratch, uint64_t scratch_bytes, void* stream);
int hgt_edge_softmax_bwd(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations, int32_t n_heads,
                         const float* att, const float* d_att, const float* rho, int64_t ld_rho, float* d_logits, void* stream);
int hgt_edge_gather_sorted(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations, int32_t n_heads,
                           const float* by_edge_id, float* sorted, void* stream);
int hgt_head_dot(const float* a, const float* b, int64_t n_rows, int32_t n_heads, int32_t dk_pad, float* out, void* stream);
int hgt_relation_outer(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations, int32_t n_heads,
                       int32_t dk_pad, const float* weights, const float* a_src, const float* rte_a, const float* b_dst, float* out,
                       void* stream);
/* ABI 8: the same sums for heads of 128 or 256 padded columns (n_hid 768 / 1024 with 8 heads, 512 with 4 or 2, 256 with 1): one
 * workgroup per 128 x 128 block of a head's matrix, exact fp32 products on the matrix cores (v_mfma_f32_32x32x2_f32).  Same arguments
 * and contract as hgt_relation_outer (+= into out, a relation without edges is left untouched, rte_a optional; a_src / rte_a /
 * b_dst 16-byte aligned); HGT_ERR_UNSUPPORTED for every other dk_pad -- hgt_relation_outer covers heads of up to 64 columns. */
int hgt_relation_outer_wide(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations, int32_t n_heads,
                            int32_t dk_pad, const float* weights, const float* a_src, const float* rte_a, const float* b_dst,
                            float* out, void* stream);
/* d <= 1024 (rows of up to 512 columns and wider ones run two instantiations of one kernel: 8 / 16 columns per lane) */
int hgt_node_update_bwd(const float* grad_out, const float* trans, const float* x, int64_t ldx, const int64_t* node_type,
                        const float* skip, const float* ln_w, int32_t use_norm, const float* drop_mask, int64_t n_rows, int32_t d,
                        int32_t n_types, float* d_trans, float* dx, int64_t ld_dx, float* d_alpha, float* d_ln_w, float* d_ln_b,
                        void* stream);
/* the reverse of hgt_node_update_ex (DenseHGTConv.update, conv.py:250-274): skip == NULL = plain residual y = o + x (no gate;
 * d_alpha unused), shared_norm != 0 = one LayerNorm for every type (row 0 of ln_w / d_ln_w / d_ln_b) */
int hgt_node_update_bwd_ex(const float* grad_out, const float* trans, const float* x, int64_t ldx, const int64_t* node_type,
                           const float* skip, const float* ln_w, int32_t use_norm, int32_t shared_norm, const float* drop_mask,
                           int64_t n_rows, int32_t d, int32_t n_types, float* d_trans, float* dx, int64_t ld_dx, float* d_alpha,
                           float* d_ln_w, float* d_ln_b, void* stream);
/* off2[0..1] = {0, group_off[n_groups]}: the rows of every valid group as one group (shared dense layer of DenseHGTConv) */
int hgt_single_group_offsets(const int32_t* group_off, int32_t n_groups, int32_t* off2, void* stream);
int hgt_gelu_bwd(const float* dg, const float* agg, float* out, int64_t n, void* stream);
int hgt_mul_inplace(float* x, const float* m, int64_t n, void* stream);
int hgt_typed_wgrad(const float* A, int64_t lda, const float* B, int64_t ldb, const int32_t* rows, const int32_t* group_off,
                    int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols, float* out, int64_t out_group_stride, void* stream);
/* hgt_typed_wgrad as 3-term split-bf16 products (relative error of a product ~3*2^-18, like the forward typed linears); colsum
 * (optional, [n_groups][colsum_group_stride]) += the column sums of A per group (the bias gradient) from the same pass. */
int hgt_typed_wgrad_bf16x3(const float* A, int64_t lda, const float* B, int64_t ldb, const int32_t* rows, const int32_t* group_off,
                           int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols, float* out, int64_t out_group_stride,
                           float* colsum, int64_t colsum_group_stride, void* stream);
int hgt_typed_colsum(const float* A, int64_t lda, const int32_t* rows, const int32_t* group_off, int32_t n_groups, int64_t n_rows,
                     int32_t m, float* out, int64_t out_group_stride, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Bit-reproducible training (hgt_build_features() & HGT_FEATURE_DETERMINISTIC_TRAINING): a `_det` form of every entry point above
 * that sums with fp32 atomics (the reference's `loss.backward()`, OAG/train_paper_field.py:249, leaves the order to autograd's
 * scatter-adds; a seeded run here repeats bit for bit).  Two launches on the stream instead of atomics: stage one writes each
 * slot's partial result with plain stores into `ws`, stage two (one small kernel) sums the slots in slot order.  The number of
 * slots and the rows / work items of a slot are a function of the ARGUMENTS of the matching `*_det_bytes` call alone (never of the
 * device, the occupancy or the launch order; DESIGN.md section 10 has the formulas), `*_det_bytes` = the bytes `ws` must have
 * (possibly 0: one slot per output tile, written directly).  Contract differences to the atomic forms: the outputs are
 * OVERWRITTEN (no caller-side zeroing; groups without rows and relations without edges get zeros), `ws` must be 16-byte aligned;
 * ws_bytes too small -> HGT_ERR_WORKSPACE, bad arguments -> HGT_ERR_INVALID_ARG, and neither launches anything.  The results are
 * within rounding of the atomic forms', not bit-equal to them.
 * ---------------------------------------------------------------------------------------------- */
/* conv.py:125-133 in reverse (both hgt_node_update_bwd and hgt_node_update_bwd_ex: skip may be NULL) */
int hgt_node_update_bwd_det_bytes(int64_t n_rows, int32_t d, int32_t n_types, uint64_t* out);
int hgt_node_update_bwd_det(const float* grad_out, const float* trans, const float* x, int64_t ldx, const int64_t* node_type,
                            const float* skip, const float* ln_w, int32_t use_norm, int32_t shared_norm, const float* drop_mask,
                            int64_t n_rows, int32_t d, int32_t n_types, float* d_trans, float* dx, int64_t ld_dx, float* d_alpha,
                            float* d_ln_w, float* d_ln_b, void* ws, uint64_t ws_bytes, void* stream);
/* weight / bias gradients of the typed linears (conv.py:96-97,103,125; model.py:70-76): out_group_stride >= m * n_cols */
int hgt_typed_wgrad_det_bytes(int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols, uint64_t* out);
int hgt_typed_wgrad_det(const float* A, int64_t lda, const float* B, int64_t ldb, const int32_t* rows, const int32_t* group_off,
                        int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols, float* out, int64_t out_group_stride, void* ws,
                        uint64_t ws_bytes, void* stream);
int hgt_typed_wgrad_bf16x3_det_bytes(int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols, uint64_t* out);
int hgt_typed_wgrad_bf16x3_det(const float* A, int64_t lda, const float* B, int64_t ldb, const int32_t* rows,
                               const int32_t* group_off, int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols, float* out,
                               int64_t out_group_stride, float* colsum, int64_t colsum_group_stride, void* ws, uint64_t ws_bytes,
                               void* stream);
int hgt_typed_colsum_det_bytes(int32_t n_groups, int64_t n_rows, int32_t m, uint64_t* out);
int hgt_typed_colsum_det(const float* A, int64_t lda, const int32_t* rows, const int32_t* group_off, int32_t n_groups, int64_t n_rows,
                         int32_t m, float* out, int64_t out_group_stride, void* ws, uint64_t ws_bytes, void* stream);
/* d relation_msg / d relation_att (conv.py:98-99,104): partials per slice of the plan's item list */
int hgt_relation_outer_det_bytes(int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations, int32_t n_heads,
                                 int32_t dk_pad, uint64_t* out);
int hgt_relation_outer_det(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations, int32_t n_heads,
                           int32_t dk_pad, const float* weights, const float* a_src, const float* rte_a, const float* b_dst,
                           float* out, void* ws, uint64_t ws_bytes, void* stream);
int hgt_relation_outer_wide_det_bytes(int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations, int32_t n_heads,
                                      int32_t dk_pad, uint64_t* out);
int hgt_relation_outer_wide_det(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations,
                                int32_t n_heads, int32_t dk_pad, const float* weights, const float* a_src, const float* rte_a,
                                const float* b_dst, float* out, void* ws, uint64_t ws_bytes, void* stream);
/* hgt_edge_spmm with the hub targets summed per piece in piece order (the hub mode of HGT_FLAG_DETERMINISTIC_HUBS); the
 * workspace is the hub workspace: hgt_edge_spmm_det_bytes == hgt_hub_workspace_bytes_ex(.., 1) */
int hgt_edge_spmm_det_bytes(int64_t n_edges, int32_t n_heads, int32_t dk_pad, int32_t n_relations, uint64_t* out);
int hgt_edge_spmm_det(const void* plan, int64_t n_nodes, int64_t n_edges, int32_t n_types, int32_t n_relations, int32_t n_heads,
                      int32_t dk_pad, const float* weights, const float* rows, const float* rte_rows, const float* f_p,
                      const void* f_frag, float* out, int64_t ld_out, int64_t n_q_rows, void* ws, uint64_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * One whole HGTConv.forward (conv.py:56-134, eval mode) as a single enqueue of the kernels above.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hgt_conv_args {
    /* problem */
    int64_t n_nodes, n_edges;
    int32_t in_dim, out_dim, n_types, n_relations, n_heads;
    int32_t use_norm, use_rte, precision, want_att;   /* precision: 0 exact fp32 MFMA chain, 1 split-bf16 x3, 2 fp16 hi/lo x3
                                                       * (every matrix-core product of the layer; stage 0 only: staged calls
                                                       * return HGT_ERR_UNSUPPORTED) */
    int64_t n_q_rows;            /* nodes [0, n_q_rows) get Q/aggregate/update; others only K,V (halo) */
    /* inputs */
    const float* x;              /* [n_nodes][in_dim]                          */
    const int64_t* node_type;    /* [n_nodes]                                  */
    const void* plan;            /* hgt_plan_build output                      */
    /* parameters (packed by the caller, see pyhgt_amd/conv.py::_pack_parameters) */
    const float* w_qkv;          /* [T][3*d_pad][in_dim] head-padded rows      */
    const float* b_qkv;          /* [T][3*d_pad]                               */
    const float* w_a;            /* [T][out_dim][d_pad] head-padded columns    */
    const float* b_a;            /* [T][out_dim]                               */
    const float* relation_att;   /* [R][H][d_k][d_k]                           */
    const float* relation_msg;   /* [R][H][d_k][d_k]                           */
    const float* relation_pri;   /* [R][H]                                     */
    const float* skip;           /* [T]                                        */
    const float* ln_w;           /* [T][out_dim] or NULL                       */
    const float* ln_b;           /* [T][out_dim] or NULL                       */
    const float* rte_emb;        /* [240][in_dim]   (use_rte)                  */
    const float* rte_w;          /* [in_dim][in_dim]                           */
    const float* rte_b;          /* [in_dim]                                   */
    /* workspace + outputs */
    void* workspace;             /* hgt_conv_workspace_bytes()                 */
    uint64_t workspace_bytes;
    float* out;                  /* [n_nodes][out_dim]                         */
    float* att_out;              /* [n_edges][n_heads] or NULL                 */
    /* optional instrumentation: HOST array of HGT_N_PHASE_EVENTS hipEvent_t handles, recorded on the
     * stream at the phase boundaries listed below (NULL = no events)           */
    void* const* phase_events;
    /* ABI 2: update_mode 0 = HGTConv.update (conv.py:114-134); 1 = DenseHGTConv.update (conv.py:250-274):
     *   y1 = LN_t(a_linear_t(agg) + x)   (no gelu on agg, no gate; `skip` is ignored)
     *   out = out_norm(out_linear(gelu(mid_linear(y1))) + y1)      (weights shared by all types)   */
    int32_t update_mode;
    const float* mid_w;          /* [2*out_dim][out_dim]                       */
    const float* mid_b;          /* [2*out_dim]                                */
    const float* out_w;          /* [out_dim][2*out_dim]                       */
    const float* out_b;          /* [out_dim]                                  */
    const float* out_ln_w;       /* [out_dim]                                  */
    const float* out_ln_b;       /* [out_dim]                                  */
    /* Staged execution for the multi-GPU path (pyhgt_amd/dist.py), so that the halo exchange overlaps the projections.
     * All stages of one forward use the same args (same workspace) on the same stream:
     *   0  the whole layer (default)
     *   1  parameter packing + Q|K|V projections of the rows [0, n_q_rows) only (+ temporal tables)
     *   2  K|V projections of the rows listed in proj_rows (typed row list: group t = proj_rows[proj_off[t] ..
     *      proj_off[t+1]), device arrays, n_types+1 offsets) -- call once per received chunk of halo rows
     *   3  edge phase + update (needs K,V of every source row: stages 1 and 2 done)
     *   4  (ABI 4) edge phase over slice `slice_index` of `slice_count` equal slices of the relation ids, softmax state carried
     *      from slice to slice in the workspace; the LAST slice also takes the unclaimed edges and runs the update.  For
     *      source-bucketed graphs: the caller numbers relations bucket * R' + relation (n_relations = slice_count * R', the
     *      relation parameters repeated slice_count times), so slice b = the edges whose source rows arrived with bucket b
     *      and the edge phase overlaps the exchange of the later buckets.  bf16x3 precision, HGTConv update only.
     *   5  (ABI 6) edge phase + fused node update of the TARGET BLOCK [q_begin, q_end) (q_begin a multiple of the plan tile; its
     *      logits work items are [item_begin, item_end), hgt_plan_tile_items_offset).  pyhgt_amd.dist orders a rank's halo rows by
     *      the first target block that needs them, so block b can run as soon as halo chunks 0..b have been projected (stage 2):
     *      no state is carried between blocks, every block is the single-GPU kernel pair on a tile range.  Split precisions, HGTConv
     *      update, padded row <= 256 columns (HGT_ERR_UNSUPPORTED otherwise: the caller falls back to stages 1/2/3).          */
    int32_t stage;
    const int32_t* proj_rows;
    const int32_t* proj_off;
    int64_t proj_n;              /* number of rows in proj_rows (host value)   */
    /* Weight-only preprocessing kept across calls (inference with fixed parameters: the reference re-derives nothing
     * per call either): packed relation matrices, split-bf16 tiles of W_qkv and W_a, temporal tables RTE_K / RTE_V.
     * `prepared` = caller-owned device buffer of hgt_conv_prepared_bytes() bytes that belongs to ONE parameter set;
     * prepared_valid = 0 -> this call fills it, 1 -> this call trusts it (the caller resets it to 0 whenever a
     * parameter, the precision or the buffer changed).  NULL = recompute into the workspace every call. */
    void* prepared;
    uint64_t prepared_bytes;
    int32_t prepared_valid;
    /* What the caller KNOWS about the plan (from the plan header, read back asynchronously -- pyhgt_amd.GraphPlan), as a bit set;
     * 0 = nothing known: every kernel is enqueued.
     *   bit 0: the plan found no hub target, so the hub kernels of the aggregation (4-5 launches that would exit at once)
     *          are not enqueued;
     *   bit 1: every target row has a valid node type, so hgt_zero_rows (output rows of unknown type := 0) is not enqueued. */
    int32_t plan_no_hubs;
    /* ABI 3: bit set of HGT_FLAG_* (0 = the default kernel selection) */
    int32_t flags;
    /* ABI 4: stage 4 only */
    int32_t slice_index;
    int32_t slice_count;
    /* ABI 6: stage 5 only */
    int64_t q_begin, q_end;
    int32_t item_begin, item_end;
    /* ABI 6: stage 2 only, optional: the rows of proj_rows are read from this buffer of 24-bit wire rows (hgt_gather_rows_c24 format,
     * 3 * in_dim bytes per row) instead of from x -- wire row = node row - proj_c24_row0 (the chunk's first local row).  Needs
     * in_dim <= 256, in_dim % 4 == 0 and a split precision (HGT_ERR_UNSUPPORTED otherwise -> hgt_unpack_rows_c24 + plain stage 2). */
    const void* proj_c24;
    int64_t proj_c24_row0;
} hgt_conv_args;

/* hgt_conv_args.flags: explicit kernel-selection switches (A/B measurements, tests); never read from the environment */
#define HGT_FLAG_NO_FUSED_UPDATE 1   /* aggregation writes agg, the node update runs as its own kernel(s) */
#define HGT_FLAG_VALU_AGGREGATE  2   /* relation transforms of the aggregation on the vector ALU (round-1 kernel) instead of MFMA */
#define HGT_FLAG_MFMA_LOGITS     4   /* hgt_edge_logits_mfma for every layout it covers (default: d_k >= 64 only) */
#define HGT_FLAG_VALU_LOGITS     8   /* never hgt_edge_logits_mfma */
#define HGT_FLAG_KSIDE_LOGITS 65536  /* hgt_edge_logits_kside wherever it is covered (see there), whatever the size of the work items (default: whole-layer,
                                      * plain staged and target-block (stage 5) calls with a split precision whose work items have at least 64 edges, and neither of the
                                      * two flags above) */
#define HGT_FLAG_NO_KSIDE_LOGITS 131072 /* never hgt_edge_logits_kside */
#define HGT_FLAG_KSIDE_LANE_GATHER 262144 /* wherever hgt_edge_logits_kside runs (the stage-5 item ranges included): every lane loads its own 16-byte
                                      * pieces of K[src] and Q[dst] instead of the gather of whole head lines through LDS.  Same logits bit
                                      * for bit; tests / A/B timings.  Bit 3 of `frag_f16` of hgt_edge_logits_kside.  ABI note: added while
                                      * HGT_ABI_VERSION stayed 8 (earlier libraries ignore the bit, as they ignore every unknown one); the
                                      * bit and the lane form are to be retired once the LDS form has held for a while -- do not reuse it */
#define HGT_FLAG_ITEM_AGGREGATE 16   /* hgt_edge_aggregate_items wherever it applies.  It applies -- and is the default -- when ALL of these hold: a split
                                      * precision; fewer than 65536 NODES (n_nodes: the workspace only then holds its scratch) and fewer than 65536
                                      * targets (n_q_rows); a scratch of at most 1 GiB (hgt_edge_aggregate_items_bytes <= 1 << 30: ~986 k edges at
                                      * 256 padded columns); fewer than 64 relations; a workspace that was sized with the scratch (options bit 0 of
                                      * hgt_conv_workspace_bytes_ex).  Rows wider than 512 padded columns are refused by the kernel itself and take
                                      * the sub-tile kernel.  Below 16384 targets it runs alone, from there on only where the fused kernel does not
                                      * (rows wider than 256 padded columns, DenseHGTConv, HGT_FLAG_NO_FUSED_UPDATE).  With both size defaults at
                                      * 65536 the flag changes nothing today. */
#define HGT_FLAG_NO_ITEM_AGGREGATE 32 /* never hgt_edge_aggregate_items */
#define HGT_FLAG_FUSED_ANY_SIZE 64   /* hgt_edge_aggregate_update below its default size too (default: n_q_rows >= 16384 -- targets, not nodes --, a
                                      * split precision, HGTConv, rows of at most 256 padded columns, fewer than 64 relations) */
/* (bits 256 and 512, like feature bit 0, are retired: hgt_conv_forward ignores them, as every shipped library always did; do not reuse them) */
#define HGT_FLAG_XS_GEMM_ALWAYS 1024 /* ABI 6: the x-stationary split GEMM (hgt_gemm_xs.hip) for every typed linear of the layer it covers, whatever
                                      * the row count (HGT_LINEAR_FORCE_XS); */
#define HGT_FLAG_XS_GEMM_NEVER 2048  /* ... never (HGT_LINEAR_NO_XS): the slab kernels.  Bit-identical results either way: tests / A/B timings */
#define HGT_FLAG_NO_TILE_GEMM 4096   /* ABI 7: the typed linears of a small layer on the persistent / slab kernels instead of the latency-regime tile
                                      * kernel (HGT_LINEAR_NO_TILE): bit-identical results; tests / A/B timings */
#define HGT_FLAG_NO_MERGE_UPDATE 8192 /* ABI 7: sampled batches: hgt_edge_aggregate_items + hgt_linear_update_* as two calls instead of
                                      * hgt_edge_aggregate_items_update (identical output; tests / A/B timings) */
#define HGT_FLAG_NO_COOP_EDGE 16384  /* ABI 7: d_k >= 64 (logits) / >= 32 (runs): the one-wavefront-per-item forms of hgt_edge_logits_mfma / the runs kernel of
                                      * hgt_edge_aggregate_items instead of the forms that share the relation transform across the workgroup
                                      * (identical output bit for bit; tests / A/B timings).  The same switch is bit 1 of `frag_f16` of those calls */
#define HGT_FLAG_COOP_EDGE_ALWAYS 32768 /* ... the shared-transform forms for work items of more than 16 edges too (default: the 16-edge items
                                      * of sampled batches only; larger items measured slower in lock-step rounds).  Bit 2 of `frag_f16` */
#define HGT_FLAG_DETERMINISTIC_HUBS 128 /* ABI 6: targets with more than 1024 in-edges ("hubs") are aggregated WITHOUT atomics: every piece of a
                                      * (hub, relation) range writes its partial row / exp-sum to its own slot and the finalize kernel sums
                                      * the slots in (relation, piece) order, so two forwards are bit-identical on every row (the default
                                      * hub path adds fp32 partials atomically: hub rows then differ in the last bits from run to run).
                                      * Every edge phase honours it: whole-layer calls and stages 3, 4 (source buckets) and 5.
                                      * Costs workspace: hgt_conv_workspace_bytes_ex(options bit 1) */

/* phase boundaries at which hgt_conv_forward records phase_events[i]:
 *   0 start | 1 relation pack + Q/K/V (+ temporal tables) done | 2 logits done | 3 softmax done |
 *   4 aggregate (+ att export) done | 5 a_linear done | 6 node update done                      */
#define HGT_N_PHASE_EVENTS 7

int hgt_conv_workspace_bytes(int64_t n_nodes, int64_t n_edges, int32_t in_dim, int32_t out_dim,
                             int32_t n_types, int32_t n_relations, int32_t n_heads, int32_t use_rte,
                             uint64_t* out_host);
/* ABI 6: options bit 0 = include the scratch of hgt_edge_aggregate_items (E*d*4 + E*H*8 + E bytes, up to 1 GiB, on graphs below 65536
 * nodes; calls that cannot take that kernel -- exact fp32, HGT_FLAG_NO_ITEM_AGGREGATE, staged multi-GPU calls -- leave it out, and
 * hgt_conv_forward accepts either size); bit 1 = the partial slots of HGT_FLAG_DETERMINISTIC_HUBS (required when that flag is set). */
int hgt_conv_workspace_bytes_ex(int64_t n_nodes, int64_t n_edges, int32_t in_dim, int32_t out_dim,
                                int32_t n_types, int32_t n_relations, int32_t n_heads, int32_t use_rte, int32_t options,
                                uint64_t* out_host);
int hgt_conv_prepared_bytes(int32_t in_dim, int32_t out_dim, int32_t n_types, int32_t n_relations, int32_t n_heads,
                            int32_t use_rte, uint64_t* out_host);
int hgt_conv_forward(const hgt_conv_args* args_host, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Counter-based dropout (csrc/hgt_dropout.hip; the recompute mode of the training step, pyhgt_amd/autograd.py): the mask of
 * nn.Dropout (conv.py:125 / 261,273) as a pure function of (seed, offset, keep, element index), so that a training step keeps a
 * seed instead of a float mask and writes the mask again in its backward.  Added under ABI 8 (new symbols only).
 *   generator Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = the 64-bit value offset + i / 4 in counter words 0 and
 *   1 (words 2, 3 zero); element i takes output word i % 4 and is kept iff word < (uint32)(keep * 2^32).
 *   hgt_dropout_mask   m[i] = kept ? 1.0f / keep : 0
 *   hgt_dropout_apply  x[i] *= that float: bit-identical to hgt_mul_inplace(x, m)
 * keep >= 1: every element kept with factor 1; keep <= 0: zeros (Dropout(p = 1)).  Any alignment of the pointer (16-byte aligned
 * arrays move 16 bytes per lane).  n == 0 -> HGT_OK without a runtime call; NULL pointer, n < 0, keep NaN -> HGT_ERR_INVALID_ARG.
 * ---------------------------------------------------------------------------------------------- */
int hgt_dropout_mask(float* m, int64_t n, uint64_t seed, uint64_t offset, float keep, void* stream);
int hgt_dropout_apply(float* x, int64_t n, uint64_t seed, uint64_t offset, float keep, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Stacking sampled batches (csrc/hgt_stack.hip; pyhgt_amd.sampled.stack_device_graphs): B graphs that are each in
 * hgt_plan_from_sorted form become one block-diagonal graph in the same form.  Added under ABI 8 (new symbols only).
 *   in   src / dst / edge_time   int32[E_tot], the pieces' arrays one after the other, ids LOCAL to the piece (edge_time may be NULL;
 *                                then edge_time_out must be NULL too)
 *        rel_ptr                 int32[B][R+1], piece-relative;   type_off  int32[B][T+1]
 *        edge_off_host / node_off_host   HOST int64[B+1]: where piece b starts in the concatenation ([0] = 0, [B] = E_tot / N_tot);
 *                                they travel as kernel arguments (B <= HGT_STACK_MAX_PIECES, HGT_ERR_UNSUPPORTED beyond)
 *   out  src_out / dst_out / edge_time_out int32[E_tot], rel_ptr_out int32[R+1], type_off_out int32[T+1]: the stacked graph.
 *        Stacked node id = type_off_out[t] + (nodes of type t in the pieces before b) + serial inside the piece's type t;
 *        inside a relation the edges are ordered by target type, then piece, then the piece's own order (targets non-decreasing).
 *        node_map int32[N_tot] / edge_map int32[E_tot]: stacked position -> position in the concatenation (permutations; node_map
 *        is a row list for hgt_gather_rows).
 *   tmp  hgt_stack_tmp_bytes(B, T, R) bytes of device scratch (HGT_ERR_WORKSPACE if smaller).
 * Three launches, no sort, no atomic, no allocation, no synchronisation.  Every store is bounds-checked and the maps are permutations
 * whatever the arrays hold; a piece that is not in the required form (targets not sorted inside a relation, ids outside the piece,
 * rel_ptr / type_off not spanning it) yields a stacked graph on which hgt_plan_from_sorted sets bad_index (ids written as -1,
 * rel_ptr_out[R] = -1).  Bad arguments -> a negative code and no launch.
 * ---------------------------------------------------------------------------------------------- */
#define HGT_STACK_MAX_PIECES 256
int hgt_stack_tmp_bytes(int32_t n_pieces, int32_t n_types, int32_t n_relations, uint64_t* bytes_host);
int hgt_stack_sorted(const int32_t* src, const int32_t* dst, const int32_t* edge_time, const int32_t* rel_ptr,
                     const int32_t* type_off, const int64_t* edge_off_host, const int64_t* node_off_host, int32_t n_pieces,
                     int32_t n_types, int32_t n_relations, int32_t* src_out, int32_t* dst_out, int32_t* edge_time_out,
                     int32_t* rel_ptr_out, int32_t* type_off_out, int32_t* node_map, int32_t* edge_map, void* tmp,
                     uint64_t tmp_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Device sampler (csrc/hgt_sampler.hip; pyhgt_amd/sampler.py): HGSampling, pyHGT/data.py:87-210, over a graph that is resident in
 * device memory.  One entry point per step of the reference so that each can be tested on its own; the host loop that strings them
 * together is sample_subgraph_device.  Added under ABI 8 (new symbols only).
 *
 * hgt_sampler_triple  one meta triple (target type, source type, relation) as a CSR by target id: indptr int32[n_tgt + 1], src and
 *                     time int32[indptr[n_tgt]], neighbours in the order of the reference's adjacency dict; time ==
 *                     HGT_SAMPLER_TIME_NONE stands for None (data.py:125: the neighbour inherits the target's time).  rel_id is the
 *                     relation's id in the result (edge_dict of data.py:237); the induce calls need the triples ordered by
 *                     (rel_id, tgt_type) and every rel_id below n_relations - 1, which is `self`.
 * hgt_sampler_type    the state of one node type: score u64[n_nodes] (32.32 fixed point), stamp u64[n_nodes] ((step << 32) |
 *                     (time ^ 0x80000000)), serial int32[n_nodes] (-1 = not sampled), sampled int32[cap_sampled] (ids in serial
 *                     order), cand int32[cap_cand] (budget keys), counts int32[4] = {sampled, first serial of the newest batch,
 *                     candidates, overflow flag}.  Before the first call: score = stamp = counts = 0, serial = -1;
 *                     hgt_sampler_reset restores that by walking the two lists.  cap_sampled, cap_cand <= n_nodes.
 * Both tables are HOST arrays of at most HGT_SAMPLER_MAX_TYPES / HGT_SAMPLER_MAX_TRIPLES entries (they travel as kernel
 * arguments) whose pointer members are device pointers.  Random words: Philox4x32-10 under key = seed (the generator of
 * hgt_dropout_*, other counter words).  `step` numbers the calls of one batch; it enters the stamps (a later step's time replaces an
 * earlier one's, inside a step the largest time wins) and the random words.
 *
 *   hgt_sampler_seed        data.py:135-137: nodes ids[0..n) with times[0..n) become serials 0..n-1 of `type`.
 *   hgt_sampler_add_budget  data.py:112-130 for the newest batch of `type` (at most max_new nodes) over every triple into it.  A row
 *                           of more than sampled_number neighbours keeps those with the smallest (word, position), word keyed by
 *                           (position, target id, step, 0x10000 + index of the triple in the table).  A kept neighbour is skipped
 *                           when its (inherited) time exceeds max_time (has_max_time != 0) or when it is sampled; otherwise
 *                           score += round(2^32 / min(degree, sampled_number)), stamp = max(stamp, (step, time)), and its first
 *                           touch appends it to cand.  One wavefront per row up to HGT_SAMPLER_HUB_DEG neighbours, one
 *                           1024-thread workgroup per longer row.  hub: int32[hub_entries >= max_new * triples into type + 1].
 *   hgt_sampler_select      data.py:151-172: the min(sampled_number, candidates) candidates of `type` with the smallest
 *                           (key, node id), key = -log(u) / s^2 in fp32, s = score * 2^-32, u = ((word >> 8) + 0.5) * 2^-24, word
 *                           keyed by (node id, type, step, 0x20000); they get the next serials in that order and leave cand.
 *                           keys: u64[cap_cand], tmp: int32[tmp_entries >= cap_cand].  sampled_number <= HGT_SAMPLER_MAX_NUMBER.
 *   hgt_sampler_induce_slots  HOST only: the number of row slots of the induce calls = sum over the triples of their target type's
 *                           cap_sampled.
 *   hgt_sampler_induce_count  data.py:183-209, first pass: rowoff int32[n_entries >= slots + 1] and hub (same size) are scratch that
 *                           the fill call reads again; out: type_off_out int32[T + 1], rel_ptr_out int32[R + 1] and sizes_out
 *                           int32[T + M + 2] = {nodes per type, edges per triple, overflow flag, non-self edges} -- the one array
 *                           the host reads per batch.
 *   hgt_sampler_induce_fill   second pass: src_out / dst_out / time_out int32[n_edges] (n_edges = non-self edges + n_nodes),
 *                           relation-major, inside a relation by global target id, a target's neighbours in adjacency order, the
 *                           `self` edges last; edge time = time[tgt] - time[src] + 120 (data.py:250).  node_time_out and
 *                           node_id_out int32[n_nodes]: time and original id of every sampled node in global order.
 *   hgt_sampler_reset       clears the state entries that the sampled and candidate lists name, then the counts.
 * No float atomics; every store is bounds-checked against the capacities in the tables.  Bad arguments -> a negative code and no
 * launch (NULL table or array, negative size: HGT_ERR_INVALID_ARG; scratch too small: HGT_ERR_WORKSPACE; more types, triples or
 * a larger sampled_number than the limits: HGT_ERR_UNSUPPORTED).
 * ---------------------------------------------------------------------------------------------- */
#define HGT_SAMPLER_MAX_TYPES 16
#define HGT_SAMPLER_MAX_TRIPLES 48
#define HGT_SAMPLER_MAX_NUMBER 1024
#define HGT_SAMPLER_HUB_DEG 512
#define HGT_SAMPLER_TIME_NONE INT32_MIN
typedef struct hgt_sampler_type {
    uint64_t* score;
    uint64_t* stamp;
    int32_t* serial;
    int32_t* sampled;
    int32_t* cand;
    int32_t* counts;
    int32_t n_nodes, cap_sampled, cap_cand, reserved;
} hgt_sampler_type;
typedef struct hgt_sampler_triple {
    const int32_t* indptr;
    const int32_t* src;
    const int32_t* time;
    int32_t tgt_type, src_type, rel_id, reserved;
} hgt_sampler_triple;
int hgt_sampler_seed(const hgt_sampler_type* types_host, int32_t n_types, int32_t type, const int32_t* ids, const int32_t* times,
                     int32_t n, int32_t step, void* stream);
int hgt_sampler_add_budget(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                           int32_t n_triples, int32_t type, int32_t step, int32_t sampled_number, int32_t max_new,
                           int32_t has_max_time, int32_t max_time, uint64_t seed, int32_t* hub, int64_t hub_entries, void* stream);
int hgt_sampler_select(const hgt_sampler_type* types_host, int32_t n_types, int32_t type, int32_t step, int32_t sampled_number,
                       uint64_t seed, uint64_t* keys, int32_t* tmp, int64_t tmp_entries, void* stream);
int hgt_sampler_induce_slots(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                             int32_t n_triples, int64_t* n_slots_host);
int hgt_sampler_induce_count(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                             int32_t n_triples, int32_t n_relations, int32_t* rowoff, int32_t* hub, int64_t n_entries,
                             int32_t* type_off_out, int32_t* rel_ptr_out, int32_t* sizes_out, void* stream);
int hgt_sampler_induce_fill(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                            int32_t n_triples, int32_t n_relations, const int32_t* rowoff, const int32_t* hub, int64_t n_entries,
                            const int32_t* type_off, int64_t n_nodes, int64_t n_edges, int32_t* src_out, int32_t* dst_out,
                            int32_t* time_out, int32_t* node_time_out, int32_t* node_id_out, void* stream);
int hgt_sampler_reset(const hgt_sampler_type* types_host, int32_t n_types, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Task batches (csrc/hgt_sampler.hip, csrc/hgt_sampler_labels.hip): what the reference's training scripts do between sample_subgraph
 * and to_torch (OAG/train_paper_field.py:109-137 and its siblings) -- take the edges of the label relation at the output nodes out of
 * the batch and build the labels from the same relation of the full graph.  Added under ABI 8 (new symbols only).
 *
 *   hgt_sampler_induce_count_masked / _fill_masked   the induce calls with one hgt_sampler_mask per triple (HOST array of n_triples
 *                           entries; the thresholds travel as kernel arguments next to the tables).  The rule: an edge of triple m
 *                           between the sampled target of serial i and a sampled source of serial ser is left out iff
 *                           i < masks[m].tgt_below or ser < masks[m].src_below.  Serials are per type, and the seeds of a type are
 *                           its first serials in the order given, so a threshold equal to the number of seeds names exactly the
 *                           edges at the seeds.  `self` edges are never masked.  Count pass (rowoff, rel_ptr, sizes_out) and fill
 *                           pass apply the same rule, in wavefront rows and in hub rows; the order of the surviving edges, the edge
 *                           times and the node outputs are those of the unmasked calls; a relation may come out empty.  All-zero
 *                           masks give the arrays of the unmasked calls bit for bit.  masks_host == NULL or a negative threshold:
 *                           HGT_ERR_INVALID_ARG, no launch.  Both passes of one batch must be given the same masks.
 *   hgt_sampler_labels      labels of n nodes of the triple's target type from the resident CSR.  For row r, v = ids[r]: a neighbour
 *                           (in adjacency order) qualifies iff col_of[src] >= 0 and, with has_window != 0, its edge time is not
 *                           HGT_SAMPLER_TIME_NONE and lies in [t_min, t_max].  C = the set of distinct columns of the qualifying
 *                           neighbours.  dist_out[r * ld + c] = 1.0f / (float)|C| for c in C and 0 for every other c < n_cols (the
 *                           whole row is written, the padding ld - n_cols is not touched); index_out[r] = the column of the first
 *                           qualifying neighbour or -1; count_out[r] = |C|.  An id outside [0, n_tgt_nodes) gives a zero row, -1
 *                           and 0.  ids, col_of (int32[n_src_nodes], -1 = no class) and the outputs are device arrays; any of the
 *                           three outputs may be NULL.  One launch, one workgroup per row, no float atomics, the result does not
 *                           depend on the launch geometry.  NULL table or array with n > 0, a negative size, ld < n_cols (with
 *                           dist_out), t_min > t_max with a window: HGT_ERR_INVALID_ARG, no launch.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hgt_sampler_mask {
    int32_t tgt_below, src_below;
} hgt_sampler_mask;
int hgt_sampler_induce_count_masked(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                    int32_t n_triples, int32_t n_relations, int32_t* rowoff, int32_t* hub, int64_t n_entries,
                                    int32_t* type_off_out, int32_t* rel_ptr_out, int32_t* sizes_out, const hgt_sampler_mask* masks_host,
                                    void* stream);
int hgt_sampler_induce_fill_masked(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                   int32_t n_triples, int32_t n_relations, const int32_t* rowoff, const int32_t* hub, int64_t n_entries,
                                   const int32_t* type_off, int64_t n_nodes, int64_t n_edges, int32_t* src_out, int32_t* dst_out,
                                   int32_t* time_out, int32_t* node_time_out, int32_t* node_id_out, const hgt_sampler_mask* masks_host,
                                   void* stream);
int hgt_sampler_labels(const hgt_sampler_triple* triple_host, int32_t n_tgt_nodes, int32_t n_src_nodes, const int32_t* ids, int32_t n,
                       const int32_t* col_of, int32_t n_cols, int32_t has_window, int32_t t_min, int32_t t_max, float* dist_out,
                       int64_t ld, int32_t* index_out, int32_t* count_out, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Batched device sampler (csrc/hgt_sampler.hip; sample_subgraphs_device): n_batch independent batches (replicas) that share the
 * resident graph and nothing else, drawn by ONE pass of the launches of a single batch -- replica b of every launch is blockIdx.y = b.
 * Added under ABI 8 (new symbols only); the single entry points above keep their signatures, their kernels and their bits.
 *
 * Form: explicit arguments.  Every entry point is its single sibling with n_batch behind the tables and these rules:
 *   state        the tables are those of ONE replica (replica 0) and travel as kernel arguments as before; replica b's arrays are
 *                the table's pointers shifted by b strides, and every stride is a field of the tables: score / stamp / serial by
 *                n_nodes, sampled by cap_sampled, cand by cap_cand, counts by 4 * n_types.  So score is u64[n_batch][n_nodes],
 *                sampled int32[n_batch][cap_sampled], counts of type t int32[n_batch][n_types][4] + 4 * t, and so on.
 *   scratch      sizes (hub_entries, tmp_entries, n_entries) are PER REPLICA, exactly the single call's requirement, and the arrays
 *                hold n_batch times as much: keys u64[n_batch][tmp_entries], tmp int32[n_batch][tmp_entries], rowoff
 *                int32[n_batch][n_entries].  hub int32[n_batch * hub_entries]: the n_batch queue counters first (one memset),
 *                then replica b's queue entries at hub + n_batch + b * (hub_entries - 1) -- every replica's queue is its own.
 *   inputs       ids / times int32[n_batch][n]; seeds_host: HOST array of n_batch Philox keys, which ride in the kernel-argument
 *                space next to the tables (that is what bounds HGT_SAMPLER_MAX_BATCH: tables + parameters + 8 bytes per replica
 *                within the 4 KB of arguments of a launch).  type, step, sampled_number, max_new, max_time and the masks are shared.
 *   count pass   type_off_out int32[n_batch][T + 1], rel_ptr_out int32[n_batch][R + 1], sizes_out int32[n_batch][T + M + 2]: the one
 *                array the host reads per batched call.  Replica b raises its own overflow flag, sizes_out[b][T + M].
 *   fill pass    n_nodes / n_edges are the totals over the replicas; src_out / dst_out / time_out int32[n_edges] and node_time_out /
 *                node_id_out int32[n_nodes] hold the replicas one after the other, indices local to each piece exactly as a single
 *                call writes them.  offs_out int32[2 * (n_batch + 1)] receives the node prefix sums over b, then the edge prefix sums
 *                (one more launch, from `sizes`, the array of the count pass); a replica whose range does not lie inside the totals
 *                writes nothing.  The masked forms take the one mask table for all replicas.
 *   hgt_sampler_gather_features   the feature rows of the whole call in one launch, one wavefront per output row: row g finds its
 *                replica in the node prefix sums (offs), its type in that replica's type_off, and copies `width` floats of row
 *                node_id[g] of features_host[type] (HOST array of n_types device pointers, NULL for a type without a matrix;
 *                type_nodes_host: rows per matrix) -- a pure copy, bit-equal to hgt_gather_rows.  A row whose type has no matrix or
 *                whose id is outside it is left untouched.
 * One workgroup per replica in the selection and the scan, the hub launches loop over their replica's queue; row logic, bounds checks
 * and the absence of float atomics are those of the single entry points (the same device functions under a replica view).  Bad
 * arguments -> a negative code and no launch: n_batch < 1, a NULL per-replica array with n > 0, a negative size: HGT_ERR_INVALID_ARG;
 * scratch below the single requirement per replica: HGT_ERR_WORKSPACE; n_batch > HGT_SAMPLER_MAX_BATCH: HGT_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------------- */
#define HGT_SAMPLER_MAX_BATCH 64
int hgt_sampler_seed_batched(const hgt_sampler_type* types_host, int32_t n_types, int32_t n_batch, int32_t type, const int32_t* ids,
                             const int32_t* times, int32_t n, int32_t step, void* stream);
int hgt_sampler_add_budget_batched(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                   int32_t n_triples, int32_t n_batch, int32_t type, int32_t step, int32_t sampled_number,
                                   int32_t max_new, int32_t has_max_time, int32_t max_time, const uint64_t* seeds_host, int32_t* hub,
                                   int64_t hub_entries, void* stream);
int hgt_sampler_select_batched(const hgt_sampler_type* types_host, int32_t n_types, int32_t n_batch, int32_t type, int32_t step,
                               int32_t sampled_number, const uint64_t* seeds_host, uint64_t* keys, int32_t* tmp, int64_t tmp_entries,
                               void* stream);
int hgt_sampler_induce_count_batched(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                     int32_t n_triples, int32_t n_batch, int32_t n_relations, int32_t* rowoff, int32_t* hub,
                                     int64_t n_entries, int32_t* type_off_out, int32_t* rel_ptr_out, int32_t* sizes_out, void* stream);
int hgt_sampler_induce_count_masked_batched(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                            int32_t n_triples, int32_t n_batch, int32_t n_relations, int32_t* rowoff, int32_t* hub,
                                            int64_t n_entries, int32_t* type_off_out, int32_t* rel_ptr_out, int32_t* sizes_out,
                                            const hgt_sampler_mask* masks_host, void* stream);
int hgt_sampler_induce_fill_batched(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                    int32_t n_triples, int32_t n_batch, int32_t n_relations, const int32_t* rowoff, const int32_t* hub,
                                    int64_t n_entries, const int32_t* type_off, const int32_t* sizes, int32_t* offs_out, int64_t n_nodes,
                                    int64_t n_edges, int32_t* src_out, int32_t* dst_out, int32_t* time_out, int32_t* node_time_out,
                                    int32_t* node_id_out, void* stream);
int hgt_sampler_induce_fill_masked_batched(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                           int32_t n_triples, int32_t n_batch, int32_t n_relations, const int32_t* rowoff,
                                           const int32_t* hub, int64_t n_entries, const int32_t* type_off, const int32_t* sizes,
                                           int32_t* offs_out, int64_t n_nodes, int64_t n_edges, int32_t* src_out, int32_t* dst_out,
                                           int32_t* time_out, int32_t* node_time_out, int32_t* node_id_out,
                                           const hgt_sampler_mask* masks_host, void* stream);
int hgt_sampler_reset_batched(const hgt_sampler_type* types_host, int32_t n_types, int32_t n_batch, void* stream);
int hgt_sampler_gather_features(const float* const* features_host, const int32_t* type_nodes_host, int32_t n_types, int32_t n_batch,
                                int32_t width, const int32_t* type_off, const int32_t* offs, const int32_t* node_id, int64_t n_nodes,
                                float* out, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Scoring task batches (csrc/hgt_task_metrics.hip): what the reference's training scripts do with the model's output -- NDCG and MRR of
 * every scored row (OAG/train_paper_field.py:272-275 and :303-308 and the same lines of train_paper_venue.py and
 * train_author_disambiguation.py:335-345, 391-398, which take one argsort row at a time to the host and run pyHGT/utils.py:5-20 on it)
 * and the pair-ranking loss mask_softmax (train_author_disambiguation.py:90-96).  Added under ABI 8 (new symbols only).
 *
 *   hgt_rank_metrics        per row of C scores s (float32) with relevances l >= 0: 0-based ranks, a tie goes to the lower position,
 *                             score rank of p = #{ j : s_j > s_p or (s_j == s_p and j < p) }
 *                             ideal rank of p = #{ j : l_j > l_p or (l_j == l_p and j < p) }
 *                           and with w(0) = 1, w(i) = 1 / log2(i + 1), K = k > 0 ? k : C, over the positives (l_p > 0):
 *                             DCG = sum of l_p * w(rank_p) where rank_p < K, IDCG the same over the ideal ranks,
 *                             ndcg_out[r] = DCG / IDCG (0 when IDCG == 0), rr_out[r] = 1 / (1 + min rank_p) (0 without a positive).
 *                           A NaN score in a row makes both of its results NaN; -inf is an ordinary score.
 *                           Relevances: `labels` (float32, laid out like the scores) as given; or `index` (int64[n_rows]): l = 1 at
 *                           that position, a value outside [0, C) = no positive; or neither: l = 1 at position 0.  Both: an error.
 *                           Rows: row_ptr == NULL: n_rows rows of n_cols positions, row r at scores + r * ld_scores (labels + r *
 *                           ld_labels), ld >= n_cols, any alignment (16-byte loads where the row's base allows).  row_ptr
 *                           (int64[n_rows + 1], device): row r is scores[row_ptr[r] .. row_ptr[r + 1]) (and labels likewise; index is
 *                           relative to the row), n_cols is the longest row and the leading dimensions are not read; a row the pointers
 *                           make longer than n_cols, or negative, gives NaN.  Rows of at most 64 positions take a wavefront each,
 *                           longer ones a workgroup each; the positives of a row go through an LDS list of HGT_RANK_LIST_CAP entries,
 *                           a row with more takes further passes (no cap on their number).  Ranks are integer counts, the l * w terms
 *                           fp64, summed in an order fixed by the row alone: no float atomic, and a row's bits do not depend on
 *                           n_rows, the other rows or the launch geometry.  No allocation, no synchronisation; n_rows == 0: HGT_OK
 *                           without a launch.  scores, labels, index, row_ptr and the two outputs (double[n_rows]) are device arrays.
 *                           Negative n_rows / n_cols / k, labels and index together, NULL outputs or NULL scores with n_cols > 0,
 *                           ld < n_cols: HGT_ERR_INVALID_ARG; n_cols > INT32_MAX - 1024: HGT_ERR_UNSUPPORTED; no launch.
 *   hgt_segment_first_nll   segments s = scores[row_ptr[s] .. row_ptr[s + 1]) of lengths 2 .. max_len: with m = max and
 *                           ls = log(sum exp(x - m)) in fp32 as torch.log_softmax forms them, loss_out[s] = (ls - (x_0 - m)) / ln(len)
 *                           (ln(len) = the fp32 value nearest to it) and lse_out[2 s] = m, lse_out[2 s + 1] = ls -- the logsumexp in
 *                           its two parts, so that the backward forms x - m - ls exactly as the forward did.  A segment the pointers
 *                           make shorter than 2 or longer than max_len gives NaN.  A wavefront per segment up to 64 entries, a
 *                           workgroup above; no atomics.
 *   hgt_segment_first_nll_bwd   grad_scores[j] = grad_loss[s] * (exp(x_j - m - ls) - [j is the first of s]) / ln(len) for every j of
 *                           every segment, each element written exactly once (grad_loss: float32[n_seg]).
 *                           Both: n_seg == 0: HGT_OK without a launch; a negative size, max_len < 2 or a NULL array with n_seg > 0:
 *                           HGT_ERR_INVALID_ARG, no launch.
 * ---------------------------------------------------------------------------------------------- */
#define HGT_RANK_LIST_CAP 1024
int hgt_rank_metrics(const float* scores, const float* labels, const int64_t* index, const int64_t* row_ptr, int32_t n_rows,
                     int32_t n_cols, int64_t ld_scores, int64_t ld_labels, int32_t k, double* ndcg_out, double* rr_out, void* stream);
int hgt_segment_first_nll(const float* scores, const int64_t* row_ptr, int32_t n_seg, int32_t max_len, float* loss_out, float* lse_out,
                          void* stream);
int hgt_segment_first_nll_bwd(const float* scores, const int64_t* row_ptr, int32_t n_seg, int32_t max_len, const float* lse,
                              const float* grad_loss, float* grad_scores, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Classification losses (csrc/hgt_task_loss.hip, csrc/hgt_sampler_labels.hip): what the reference's paper-venue, ogbn-mag and
 * paper-field scripts do with the Classifier's output -- log_softmax followed by nll_loss (OAG/train_paper_venue.py:86,
 * ogbn-mag/train_ogbn_mag.py:116) or KLDivLoss(reduction='batchmean') (OAG/train_paper_field.py:87) -- on the raw logits, and the
 * paper-field labels as a short list of class columns per row in place of a dense [n, C] distribution (train_paper_field.py:133-137).
 * Added under ABI 8 (new symbols only).
 *
 *   hgt_class_loss          per row x of n_cols logits (float32): m = max x, ls = log(sum exp(x - m)), logp_j = (x_j - m) - ls, in fp32
 *                           as torch.log_softmax forms them.  lse_out[2 r] = m, lse_out[2 r + 1] = ls (the logsumexp in its two parts,
 *                           so that the backward forms the same difference).  Exactly one label form is given:
 *                             index (int64[n_rows])     loss_out[r] = -logp_y, wsum_out[r] = 1;  y < 0: the row is ignored -- term 0,
 *                                                       W 0;  y >= n_cols: NaN, and nothing out of range is read
 *                             labels (float32, row r at labels + r * ld_labels)   loss_out[r] = sum over l_j > 0 of
 *                                                       l_j (log l_j - logp_j), the rows of kl_div(reduction='none').sum(1);
 *                                                       wsum_out[r] = sum l_j;  an entry < 0 or NaN: NaN
 *                             columns (int32[n_rows, width], -1 = padding)   with c = the number of entries >= 0 of the row (distinct
 *                                                       by contract): -log c - (1 / c) sum logp_col, the dense form with l = 1 / c on
 *                                                       those columns; W = 1;  c = 0: term 0, W 0;  an entry >= n_cols: NaN;  with
 *                                                       `count` (int32[n_rows], optional: the true number of classes of the row)
 *                                                       count[r] > width: NaN -- a truncated list is never scored silently
 *                           A NaN term is saved with W = NaN.  The label-weighted terms are summed in fp64 in an order fixed by the
 *                           row alone and rounded once to float32.
 *   hgt_class_loss_bwd      grad_logits[r * ld_grad + j] = grad_loss[r] * (W_r * exp((x_j - m) - ls) - l_rj) for j < n_cols, l the
 *                           row's label distribution (1 at the index, the dense entries, 1 / c on the listed columns); the columns
 *                           n_cols .. ld_grad of a row are left untouched.  A row with W = 0 and no dense labels gets exact zeros, a
 *                           row with W = NaN gets NaN.  One launch, no float atomic.
 *                           Both: row r is at logits + r * ld, ld >= n_cols, any alignment (16-byte loads where the row's base
 *                           allows).  Rows of at most HGT_CLASS_LOSS_WAVE_COLS columns take a wavefront each, longer ones a workgroup
 *                           each, streamed twice; a position always belongs to the same thread, so a row's bits do not depend on its
 *                           alignment, n_rows, the other rows or the launch geometry.  No allocation, no synchronisation.  All arrays
 *                           are device arrays.  n_rows == 0: HGT_OK without a launch.  No label form or more than one, count without
 *                           columns, a negative size, ld (ld_labels, ld_grad) < n_cols, width < 1 with columns, a NULL output or
 *                           NULL logits with n_cols > 0: HGT_ERR_INVALID_ARG; n_cols > INT32_MAX - 1024: HGT_ERR_UNSUPPORTED; no launch.
 *   hgt_sampler_label_columns   hgt_sampler_labels's arguments and row rule; the set C of row r is written as a list:
 *                           columns_out[r * width + i] = the i-th smallest column of C for i < min(|C|, width), -1 behind it;
 *                           count_out[r] = |C| whether it fitted or not (count_out may be NULL).  One launch, one workgroup per row:
 *                           a prefix popcount over the LDS bitmap of hgt_sampler_labels, chunk after chunk.  The argument errors of
 *                           hgt_sampler_labels, and width < 1 or columns_out == NULL with n > 0: HGT_ERR_INVALID_ARG, no launch.
 * ---------------------------------------------------------------------------------------------- */
#define HGT_CLASS_LOSS_WAVE_COLS 256
int hgt_class_loss(const float* logits, int64_t ld, int32_t n_rows, int32_t n_cols, const float* labels, int64_t ld_labels,
                   const int64_t* index, const int32_t* columns, int32_t width, const int32_t* count, float* loss_out, float* lse_out,
                   float* wsum_out, void* stream);
int hgt_class_loss_bwd(const float* logits, int64_t ld, int32_t n_rows, int32_t n_cols, const float* labels, int64_t ld_labels,
                       const int64_t* index, const int32_t* columns, int32_t width, const int32_t* count, const float* lse,
                       const float* wsum, const float* grad_loss, float* grad_logits, int64_t ld_grad, void* stream);
int hgt_sampler_label_columns(const hgt_sampler_triple* triple_host, int32_t n_tgt_nodes, int32_t n_src_nodes, const int32_t* ids,
                              int32_t n, const int32_t* col_of, int32_t n_cols, int32_t has_window, int32_t t_min, int32_t t_max,
                              int32_t* columns_out, int32_t width, int32_t* count_out, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Voted evaluation (csrc/hgt_task_vote.hip): what the reference's ogbn-mag scripts do with the Classifier's output besides the
 * loss -- the train / valid / test accuracies of a step, argmax of each split's rows against y (ogbn-mag/train_ogbn_mag.py:165-191),
 * and the vote of ogbn-mag/eval_ogbn_mag.py:128-191: every test paper owns a vector of n_cols sums, each sampled sub-graph adds the
 * log-probabilities of the test papers it contains, the answer is the argmax of the sums.  Added under ABI 8 (new symbols only).
 *
 *   hgt_class_predict       pred_out[r] (int64) = np.argmax of row r of the scores (float32): the lowest position among the maxima;
 *                           a NaN beats every number, so the first NaN wins; -inf and +inf are ordinary values.  The prediction is
 *                           taken on the scores as given.  The scripts take argmax of log-probabilities; on the raw logits that
 *                           is the same position except where the float32 rounding of (x - m) - ls makes two log-probabilities
 *                           equal that come from different logits (the script then answers the lower position of the two).
 *                           Scoring (optional): `label` (int64) and `split` (int32, needs label) are per-row arrays when
 *                           ids == NULL; with `ids` (int64[n_rows]) they are resident tables of n_table entries read at ids[r] --
 *                           graph.y and the split id of a batch's papers without per-batch label tensors.  A row is scored in
 *                           split s iff label >= 0 and 0 <= split < n_splits; without `split` every row with label >= 0 goes to
 *                           split 0 and n_splits must be 1; with it 1 <= n_splits <= HGT_PREDICT_MAX_SPLITS.
 *                           counts_out[2 s] = rows scored in split s, counts_out[2 s + 1] = those with pred == label (a label
 *                           >= n_cols is scored and never correct).  counts_out (int32[2 n_splits]) needs no initialisation: it
 *                           is zeroed on the stream inside the call and filled with integer atomics, whose sum has no order.  A row
 *                           whose ids[r] lies outside [0, n_table) is not scored and nothing out of range is read; it, and a row
 *                           with split < 0, still gets its pred_out.  pred_out or counts_out may be NULL, not both.
 *                           n_rows == 0: HGT_OK, counts_out zeroed if given.  NULL scores with n_rows > 0, NULL pred_out and NULL
 *                           counts_out, counts_out or split without label, n_cols < 1 with n_rows > 0, ld < n_cols, a negative
 *                           size, n_splits out of range: HGT_ERR_INVALID_ARG; n_cols > INT32_MAX - 1024: HGT_ERR_UNSUPPORTED; no launch.
 *   hgt_vote_add            rows piece_ptr_host[b] .. piece_ptr_host[b + 1] of the logits form piece b (a host array of
 *                           n_pieces + 1 entries).  For row r with s = slot_of[ids[r]]: if ids[r] is in [0, n_nodes) and
 *                           0 <= s < n_slots, votes[s * ld_votes + j] += logp_j for j < n_cols and count[s] += 1, logp the float32
 *                           log-softmax of hgt_class_loss: m = max x, ls = log(sum exp(x - m)), (x_j - m) - ls.  Any other row is
 *                           skipped, nothing out of range is read or written, and the columns n_cols .. ld_votes of the table are
 *                           left untouched.  One launch per piece, in piece order on the stream; an empty piece gets none.  Within a
 *                           piece the ids that map to a slot are distinct BY CONTRACT (the sampler returns each node of a type
 *                           once): no two threads of a launch touch the same slot, so there are no atomics.  Different pieces may
 *                           carry the same node; stream order fixes the order of the additions into its slot, so the bits of
 *                           `votes` depend only on the sequence of calls and their inputs.  NaN and infinite logits propagate into
 *                           the slot, as they do in the script.  slot_of: int32[n_nodes], count: int32[n_slots].
 *                           No rows: HGT_OK without a launch.  A NULL array with work to do, n_pieces < 0, piece_ptr_host not
 *                           non-decreasing from a non-negative start, ld or ld_votes < n_cols, n_cols < 1 with rows, a negative
 *                           size: HGT_ERR_INVALID_ARG; n_cols > INT32_MAX - 1024: HGT_ERR_UNSUPPORTED; no launch.
 *                           Both: row r is at base + r * ld, ld >= n_cols, any alignment (16-byte loads where the row's base
 *                           allows).  Rows of at most HGT_CLASS_LOSS_WAVE_COLS columns take a wavefront each, longer ones a
 *                           workgroup each; a position always belongs to the same thread, so a row's result does not depend on its
 *                           alignment, the other rows, n_rows or the launch geometry.  No float atomics, no allocation, no
 *                           synchronisation.  Every array is a device array unless its name ends in _host.
 * ---------------------------------------------------------------------------------------------- */
#define HGT_PREDICT_MAX_SPLITS 8
int hgt_class_predict(const float* scores, int64_t ld, int32_t n_rows, int32_t n_cols, const int64_t* ids, int64_t n_table,
                      const int64_t* label, const int32_t* split, int32_t n_splits, int64_t* pred_out, int32_t* counts_out,
                      void* stream);
int hgt_vote_add(const float* logits, int64_t ld, int32_t n_cols, const int64_t* ids, const int32_t* piece_ptr_host, int32_t n_pieces,
                 const int32_t* slot_of, int64_t n_nodes, float* votes, int64_t ld_votes, int32_t* count, int32_t n_slots,
                 void* stream);

/* ----------------------------------------------------------------------------------------------
 * The optimizer step (csrc/hgt_optim.hip): the line every training script of the reference ends a step with --
 *   torch.nn.utils.clip_grad_norm_(model.parameters(), args.clip); optimizer.step()     (OAG/train_paper_field.py:251-252,
 *   OAG/train_paper_venue.py:249-250, OAG/train_author_disambiguation.py:292-293, ogbn-mag/train_ogbn_mag.py:225-226)
 * with optimizer = torch.optim.AdamW (OAG/train_paper_field.py:194, ogbn-mag/train_ogbn_mag.py:169) -- global-norm clip and the
 * AdamW update of torch/optim/adamw.py (single-tensor form, amsgrad off) over all parameter tensors of a model in three launches,
 * whatever their number.  Added under ABI 8 (new symbols only).  float32 parameters, gradients and moments.
 *
 * Tables.  tensors: one hgt_optim_tensor per parameter tensor, the device pointers of its p, g, exp_avg, exp_avg_sq (dense,
 *   numel elements each), its group, its own step count (the count INCLUDING this step, >= 1) and `aligned` = all four bases are
 *   16-byte aligned (16-byte loads and stores then, scalar ones otherwise; element i gets the same bits on either path).  A row
 *   whose g is NULL has no gradient this step: it adds 0 to the norm and nothing of it is read or written.
 *   groups: one hgt_optim_group per parameter group: the hyper-parameters as the doubles Python holds, maximize, and clip = the
 *   group's tensors count in the norm and get the coefficient.  chunks: chunk c covers elements [first, min(first +
 *   HGT_OPTIM_CHUNK, numel)) of tensor `row`; a chunk never spans two tensors, chunks are in tensor order, a tensor of 4 elements is
 *   a chunk of its own (hgt_optim_chunk_table writes the table; it depends on the numels alone).  All three tables are DEVICE
 *   arrays; tensors and groups may be two parts of one buffer (hgt_optim_tables_bytes gives the sizes and the offset of the groups),
 *   so that a step needs one host-to-device copy.
 *
 *   hgt_optim_constants     *chunk_host = HGT_OPTIM_CHUNK as this library was built (host only; NULL: HGT_ERR_INVALID_ARG).
 *   hgt_optim_chunk_table   host only, no device call: *n_chunks_host = the number of chunks of tensors of numel_host[0 .. n_tensors);
 *                           with chunks_host != NULL the table is written there (capacity entries; fewer than needed:
 *                           HGT_ERR_WORKSPACE).  A negative numel or size, NULL n_chunks_host: HGT_ERR_INVALID_ARG; more than
 *                           INT32_MAX chunks: HGT_ERR_UNSUPPORTED.
 *   hgt_optim_tables_bytes  step_bytes = tensors + groups in one buffer, the groups at groups_offset; chunk_bytes; partials_bytes
 *                           (one double per chunk).
 *   hgt_grad_sqnorm         partials[c] = the fp64 sum of g^2 over chunk c -- per thread over its quads in element order, a shuffle
 *                           tree, then wavefront after wavefront; 0 where the row has no gradient or its group has clip == 0.
 *                           One workgroup per chunk, no atomics.
 *   hgt_grad_norm_join      *total_norm = (float)sqrt(sum of partials[0 .. n_chunks)), one workgroup, a fixed order (thread t adds
 *                           partials t, t + 256, ..., then the tree of hgt_grad_sqnorm); n_chunks == 0 writes 0.
 *   hgt_adamw_step          with total_norm != NULL: coef = min(1, max_norm / (*total_norm + 1e-6f)) in fp32 as clip_grad_norm_ forms
 *                           it (a NaN or infinite norm gives what torch's expression gives: no special case); NULL: no clipping.
 *                           Per element of a row with a gradient, in fp32:
 *                             g *= coef (groups with clip);  g = -g (maximize);  p *= 1 - lr wd;  m = b1 m + (1 - b1) g;
 *                             v = b2 v + (1 - b2) g g;  p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
 *                           bc1 = 1 - b1^step, bc2 = 1 - b2^step, 1 - lr wd, lr / bc1 and sqrt(bc2) are formed in fp64 once per
 *                           workgroup and rounded to fp32 once.  p, exp_avg and exp_avg_sq are written; g is NOT (the clipped
 *                           gradient is never stored).  One workgroup per chunk.
 *                           All three: no allocation, no synchronisation.  n_chunks == 0: HGT_OK without a launch (the join still
 *                           writes its 0).  A negative size, a NULL table or fewer than one tensor or group with chunks, NULL
 *                           partials / total_norm where written, max_norm negative or NaN with total_norm: HGT_ERR_INVALID_ARG;
 *                           n_chunks > INT32_MAX: HGT_ERR_UNSUPPORTED; no launch.  A chunk whose row, group or first element lies
 *                           outside the tables is skipped (its partial is 0); the pointers of a row are trusted.  The 16-byte path is taken only where
 *                           `aligned` is set AND the chunk's first element is a multiple of 4 (always so in the table of
 *                           hgt_optim_chunk_table); any other chunk of a caller-built table takes the scalar path.
 * ---------------------------------------------------------------------------------------------- */
#define HGT_OPTIM_CHUNK 4096
typedef struct hgt_optim_tensor {
    void* p;
    const void* g;
    void* exp_avg;
    void* exp_avg_sq;
    int64_t numel;
    int32_t group;
    int32_t step;
    int32_t aligned;
    int32_t reserved[3];
} hgt_optim_tensor;
typedef struct hgt_optim_group {
    double lr, beta1, beta2, eps, weight_decay;
    int32_t maximize;
    int32_t clip;
    int64_t reserved[2];
} hgt_optim_group;
typedef struct hgt_optim_chunk {
    int64_t first;
    int32_t row;
    int32_t reserved;
} hgt_optim_chunk;
int hgt_optim_constants(int32_t* chunk_host);
int hgt_optim_chunk_table(const int64_t* numel_host, int32_t n_tensors, hgt_optim_chunk* chunks_host, int64_t capacity,
                          int64_t* n_chunks_host);
int hgt_optim_tables_bytes(int32_t n_tensors, int32_t n_groups, int64_t n_chunks, uint64_t* step_bytes_host,
                           uint64_t* groups_offset_host, uint64_t* chunk_bytes_host, uint64_t* partials_bytes_host);
int hgt_grad_sqnorm(const hgt_optim_tensor* tensors, int32_t n_tensors, const hgt_optim_group* groups, int32_t n_groups,
                    const hgt_optim_chunk* chunks, int64_t n_chunks, double* partials, void* stream);
int hgt_grad_norm_join(const double* partials, int64_t n_chunks, float* total_norm, void* stream);
int hgt_adamw_step(const hgt_optim_tensor* tensors, int32_t n_tensors, const hgt_optim_group* groups, int32_t n_groups,
                   const hgt_optim_chunk* chunks, int64_t n_chunks, const float* total_norm, float max_norm, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Building the resident graph from raw edge lists (csrc/hgt_graph_build.hip): what ogbn-mag/preprocess_ogbn_mag.py:29-42 does with
 * nested dicts, one Python step per edge -- `elist[t_id][s_id] = year` -- and the row means of its lines 69-99.  Added under ABI 8
 * (new symbols only).  pyhgt_amd.graph_build.np_edge_lists_to_csr / np_neighbour_mean are the definitions.
 *
 *   hgt_graph_csr_bytes   *ws_bytes_host = the device scratch hgt_graph_csr_build needs for E entries (E < 0, NULL: HGT_ERR_INVALID_ARG;
 *                         E >= 2^31 - 1: HGT_ERR_TOO_LARGE).  Host arithmetic on E alone, no device call: about 52 bytes per entry,
 *                         16 of them reserved for rocPRIM's sorts (a rocPRIM that wants more: HGT_ERR_UNSUPPORTED from the build,
 *                         before its first launch).
 *   hgt_graph_csr_build   one direction of one relation.  Entry e (0 <= e < E) says "row rows[e * row_stride] has the neighbour
 *                         nbrs[e * nbr_stride]"; strides in elements, ids of id_bytes = 4 (int32) or 8 (int64) bytes, read in place.
 *                         The dict rule: inside a row the neighbours stand in the order of their FIRST entry; a repeated (row,
 *                         neighbour) pair keeps that position and takes the time of its LAST entry.  The time of entry e is
 *                         edge_time[e], else node_time[row id] (node_time_by == HGT_GRAPH_TIME_BY_ROW) or node_time[neighbour id]
 *                         (HGT_GRAPH_TIME_BY_NBR), else HGT_SAMPLER_TIME_NONE's value (both NULL); giving both is
 *                         HGT_ERR_INVALID_ARG.
 *                         Out: indptr int32[n_rows + 1], nbr_out / time_out int32[E] of which the first indptr[n_rows] are written,
 *                         status int32[2] = {entries kept, error flag}.  Flag bit 0: an id outside [0, n_rows) / [0, n_nbrs) -- such
 *                         an entry is built as id 0, so every index of the output stays in range, and the caller reads the flag with
 *                         the count and discards the result.
 *                         How: a stable radix sort (rocPRIM) by (row, neighbour) brings the copies of a pair together in entry
 *                         order; the head of a run marks its entry as kept, the tail hands it its time; a second stable sort of the
 *                         entries by row, a scan over the kept marks and one compaction give the three arrays.  Integers only, no
 *                         atomics but the OR into the flag.  Nothing synchronises; E == 0 writes a zero indptr and status.
 *                         NULL output / scratch, NULL ids with E > 0, a negative size or stride, id_bytes not 4 or 8, n_rows or n_nbrs
 *                         < 1 with E > 0: HGT_ERR_INVALID_ARG; E, n_rows or n_nbrs >= 2^31 - 1: HGT_ERR_TOO_LARGE; ws_bytes below
 *                         hgt_graph_csr_bytes: HGT_ERR_WORKSPACE; no launch in any of these.
 *   hgt_neighbour_mean_bytes  *ws_bytes_host = the scratch of hgt_neighbour_mean for n_entries = the summed lengths of the CSRs'
 *                         neighbour arrays and rows of d columns.
 *   hgt_neighbour_mean    out[r, 0:d] = (sum of x[nbr]) / count over the neighbours of row r in n_csr CSRs (host table, at most
 *                         HGT_SAMPLER_MAX_TRIPLES) that share the row type and the neighbour type: fp32, the CSRs in table order, a
 *                         CSR's neighbours in its order -- one sequence of `count` terms per row, a pair that two CSRs hold counts
 *                         twice (coo_matrix sums duplicates, preprocess_ogbn_mag.py:83).  count == 0: a row of zeros (normalize's
 *                         1 / 0 -> 0).  A sequence of up to HGT_GRAPH_MEAN_CHUNK terms is added term by term by one wavefront;
 *                         a longer one is cut into chunks of HGT_GRAPH_MEAN_CHUNK terms, one wavefront each, whose sums are joined
 *                         in chunk order: the bits of a row depend on its own sequence alone, not on the other rows or the launch.
 *                         No float atomics.  x: [n_nbrs, d] float32 with row stride ldx >= d (a column slice is fine), out: [n_rows,
 *                         d] with ldo >= d; any d >= 1.  Ids in the CSRs are trusted (hgt_graph_csr_build made them).
 *                         NULL table / x / out / scratch where read, n_csr < 1, d < 1, ld below d, a negative size:
 *                         HGT_ERR_INVALID_ARG; n_csr > HGT_SAMPLER_MAX_TRIPLES: HGT_ERR_UNSUPPORTED; n_rows or n_entries >= 2^31 - 1:
 *                         HGT_ERR_TOO_LARGE; scratch too small: HGT_ERR_WORKSPACE; no launch.  n_rows == 0: HGT_OK, no launch.
 * ---------------------------------------------------------------------------------------------- */
#define HGT_GRAPH_MEAN_CHUNK 256
#define HGT_GRAPH_TIME_BY_ROW 0
#define HGT_GRAPH_TIME_BY_NBR 1
#define HGT_GRAPH_BAD_ID 1
typedef struct hgt_graph_csr {
    const int32_t* indptr;
    const int32_t* nbr;
} hgt_graph_csr;
int hgt_graph_csr_bytes(int64_t E, uint64_t* ws_bytes_host);
int hgt_graph_csr_build(const void* rows, int64_t row_stride, const void* nbrs, int64_t nbr_stride, int32_t id_bytes,
                        const int32_t* edge_time, const int32_t* node_time, int32_t node_time_by, int64_t E, int64_t n_rows,
                        int64_t n_nbrs, int32_t* indptr, int32_t* nbr_out, int32_t* time_out, int32_t* status, void* ws,
                        uint64_t ws_bytes, void* stream);
int hgt_neighbour_mean_bytes(int64_t n_entries, int32_t d, uint64_t* ws_bytes_host);
int hgt_neighbour_mean(const hgt_graph_csr* csrs_host, int32_t n_csr, const float* x, int64_t ldx, int64_t n_rows, int64_t n_entries,
                       int32_t d, float* out, int64_t ldo, void* ws, uint64_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Seed-trimmed graphs (csrc/hgt_trim.hip): the rows and edges each layer of an n_layers stack needs for the seed rows, in hop-major
 * order.  Added under ABI 8 (new symbols only).  pyhgt_amd.trim.np_trim_to_seeds / np_trim_graph are the definitions: hop[v] = the
 * shortest directed distance from v to a seed along source -> target edges over EVERY edge (0 at a seed; -1 beyond n_layers); rows
 * kept iff hop <= L, ordered by (hop, old row); edges kept iff hop[target] <= L - 1, ordered by (hop[target], old position).
 *
 *   hgt_trim_tmp_bytes    *tmp_bytes_host = the device scratch of the two calls below (host arithmetic: 4 bytes per node and about
 *                         (L + 2) / 512 bytes per node and per edge).
 *   hgt_trim_hops         edge_index int64 read in place (source of edge e at [e * stride_col], target at [stride_row + e *
 *                         stride_col], as hgt_plan_build takes it), seeds int64[n_seeds] in any order, with repeats.  Leaves the hops
 *                         and the bad-index flag in tmp: 2 + n_layers launches (one per hop round: the launch boundary is the only
 *                         global synchronisation; atomicMin on hop, where every writer of a round writes the same value).
 *   hgt_trim_fill         same graph, seeds, n_layers and tmp, after hgt_trim_hops on the same stream.  Out: hop int32[N] (-1 = out),
 *                         order int64[N] (the first n_rows[0] written), new_id int64[N] (-1 = dropped), edge_order int64[E] (the first
 *                         n_edges[1] written), node_type_out int64[N] = node_type[order], edge_index_out int64[2][E] contiguous =
 *                         new_id[edge_index[:, edge_order]], edge_type_out / edge_time_out int64[E] (edge_time NULL: none, and
 *                         edge_time_out is not touched), out_rows int64[n_seeds] = new_id[seeds], counts int32[2 L + 2] on the device
 *                         = {n_rows[0..L], n_edges[1..L], flag} and the same 8 L + 8 bytes in counts_host_pinned (one hipMemcpyAsync
 *                         on `stream`: the caller waits for the stream before it reads them).  n_rows[k] = #{hop <= L - k},
 *                         n_edges[l] = #{kept edges with hop[target] <= L - l}.  Flag bit 0 (HGT_TRIM_BAD_ID): a seed or an edge end
 *                         outside [0, N); such a seed / edge is left out, every index written stays in range, and the caller discards
 *                         the result.  6 launches: positions come from per-tile counts, one single-workgroup scan and wavefront
 *                         ballots, never from an atomic -- every array is a function of the inputs alone.
 *   All three: n_layers outside [1, HGT_TRIM_MAX_LAYERS], a negative size, N, E or n_seeds >= 2^31, a NULL pointer where the sizes say it
 *   is read or written: HGT_ERR_INVALID_ARG; tmp_bytes too small: HGT_ERR_WORKSPACE; no launch.  N, E or n_seeds == 0 are valid.
 * ---------------------------------------------------------------------------------------------- */
#define HGT_TRIM_MAX_LAYERS 8
#define HGT_TRIM_BAD_ID 1
int hgt_trim_tmp_bytes(int64_t n_nodes, int64_t n_edges, int32_t n_layers, uint64_t* tmp_bytes_host);
int hgt_trim_hops(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, int64_t n_nodes, int64_t n_edges,
                  const int64_t* seeds, int64_t n_seeds, int32_t n_layers, void* tmp, uint64_t tmp_bytes, void* stream);
int hgt_trim_fill(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, const int64_t* edge_type, const int64_t* edge_time,
                  const int64_t* node_type, int64_t n_nodes, int64_t n_edges, const int64_t* seeds, int64_t n_seeds, int32_t n_layers,
                  void* tmp, uint64_t tmp_bytes, int32_t* hop_out, int64_t* order, int64_t* new_id, int64_t* edge_order,
                  int64_t* node_type_out, int64_t* edge_index_out, int64_t* edge_type_out, int64_t* edge_time_out, int64_t* out_rows,
                  int32_t* counts, void* counts_host_pinned, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Whole-graph view of a resident graph (csrc/hgt_graph_view.hip): the CSRs of every meta triple -> the wire format of to_torch
 * (pyHGT/data.py:212-256) over all nodes and all, or the kept, edges.  Added under ABI 8 (new symbols only).
 * pyhgt_amd.view.np_whole_graph is the definition.
 *
 *   the table             hgt_view_triple[n_triples + 1] in DEVICE memory, built by the caller: the triples ordered by (relation id,
 *                         target type), then one entry for the self run.  Per triple: the CSR (indptr int32[n_rows + 1], src, time with
 *                         HGT_SAMPLER_TIME_NONE = none; time may be NULL = all none), the leave-out flags over the target / source
 *                         type's nodes (uint8, non-zero = the entries at that node are dropped; NULL = none), the node times of the two
 *                         types (int32; both NULL or both set), `first` = the entries of the triples in front, n_rows = the target type's
 *                         nodes, the two types' first global rows and the relation id in [0, n_relations).  The last entry has first =
 *                         the CSR entries of all triples, n_rows = N and rel_id = the id of `self`; its pointers are not read.
 *                         n_entries = all CSR entries + N with self loops, = all CSR entries without.  The CSRs are trusted (rows
 *                         ascending, ids in range), as the sampler trusts them.
 *   the order             entry e of triple m is position p = e - first of its CSR: source src_off + src[p] -> target tgt_off + row(p);
 *                         the self run is i -> i for i in [0, N).  The kept entries keep this order.  A wavefront owns
 *                         HGT_VIEW_TILE consecutive entries (a workgroup four such tiles); it finds a row by one binary search of indptr
 *                         per triple it enters and walks from there.
 *   the filter            (filtered != 0) an entry with stored time t is kept iff t <= max_time (has_max_time != 0; a TIME_NONE entry
 *                         takes tgt_time[row] under the same test, and is kept where there is none) and neither flag is set; self entries
 *                         are always kept.  filtered == 0: nothing is tested, positions = entry indices, ONE launch.  filtered: count
 *                         per tile, one single-workgroup scan, fill -- positions from the scan and wavefront ballots, never from an
 *                         atomic.
 *   hgt_view_tmp_bytes    *tmp_bytes_host = the device scratch of a filtered build (4 bytes per tile; host arithmetic).
 *   hgt_view_build        Out: src32 / dst32 int32[n_entries] and, with has_time, time32 = tgt_time[row] - src_time[src] + 120 (120
 *                         on a self entry; NOT clamped to [0, 240), only saturated to int32).  Every output array has room for
 *                         n_entries elements; a filtered build writes only the first rel_ptr[n_relations] elements of each.  With
 *                         edge_index != NULL the reference's int64 tensors come out of the same pass: sources at edge_index[pos],
 *                         targets at edge_index[edge_index_stride + pos], edge_type, edge_time (has_time).  rel_ptr int32[n_relations
 *                         + 2]: rel_ptr[r] = the first kept position of relation id r, rel_ptr[n_relations] = the kept entries, then
 *                         the flag word; head_host_pinned (may be NULL) receives the same 4 (n_relations + 2) bytes by one
 *                         hipMemcpyAsync on `stream`.  Flag bit 0 (HGT_VIEW_BAD_TIME): a kept entry's time difference is outside
 *                         [0, 240); the value stands in time32 / edge_time as it is, so hgt_plan_from_sorted and hgt_plan_build flag
 *                         the same edges in the plan header (the reference's IndexError).
 *   Both: NULL table / rel_ptr, a NULL output that n_entries > 0 (and has_time) says is written, edge_index without edge_type (or
 *   without edge_time under has_time) or with a stride below n_entries, NULL tmp for a filtered build, a negative size, n_entries
 *   >= 2^31 - 1, n_triples > HGT_SAMPLER_MAX_TRIPLES, n_relations outside [1, HGT_SAMPLER_MAX_TRIPLES + 1]: HGT_ERR_INVALID_ARG;
 *   tmp_bytes too small: HGT_ERR_WORKSPACE; no launch.  n_entries == 0, empty triples and types without nodes are valid.
 * ---------------------------------------------------------------------------------------------- */
#define HGT_VIEW_TILE 512
#define HGT_VIEW_BAD_TIME 1
typedef struct hgt_view_triple {
    const int32_t* indptr;
    const int32_t* src;
    const int32_t* time;
    const uint8_t* tgt_flags;
    const uint8_t* src_flags;
    const int32_t* tgt_time;
    const int32_t* src_time;
    int64_t first;
    int32_t n_rows;
    int32_t tgt_off;
    int32_t src_off;
    int32_t rel_id;
} hgt_view_triple;
int hgt_view_tmp_bytes(int64_t n_entries, uint64_t* tmp_bytes_host);
int hgt_view_build(const hgt_view_triple* table_dev, int32_t n_triples, int32_t n_relations, int64_t n_entries, int32_t filtered,
                   int32_t has_max_time, int32_t max_time, int32_t has_time, int32_t* src32, int32_t* dst32, int32_t* time32,
                   int64_t* edge_index, int64_t edge_index_stride, int64_t* edge_type, int64_t* edge_time, int32_t* rel_ptr, void* tmp,
                   uint64_t tmp_bytes, void* head_host_pinned, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Exact L-hop neighbourhood of a seed set from the resident graph (csrc/hgt_neighbourhood.hip): a frontier walk over the in-edge
 * CSRs whose result stands in the seed trim's hop-major order.  Added under ABI 8 (new symbols only).
 * pyhgt_amd.neighbourhood.np_neighbourhood is the definition: array for array the whole-graph view, trimmed to the seeds.
 *
 *   the tables            hgt_nb_type[n_types] and hgt_nb_triple[n_triples] in DEVICE memory (the triples ordered by (relation id,
 *                         target type), as in the view); hgt_nb_expand / hgt_nb_fill take the triple table once more in HOST memory,
 *                         of which they read only tgt_type / src_type.  Per type: the RESIDENT mark array (int32[n_nodes], -1
 *                         everywhere between calls; during a call HGT_NB_CLAIMED, then the node's new row), the type's first view
 *                         row, its feature matrix (float32, leading dimension ld; read by hgt_nb_finish only).  Per triple: the CSR,
 *                         the leave-out flags and the node times as in hgt_view_triple.  The CSRs are trusted.
 *   the head              int64[HGT_NB_HEAD_WORDS] in device memory: [HGT_NB_HEAD_N] the size of the level that was numbered last, [_DEG] / [_CHUNKS] the CSR entries / the chunks of that level's
 *                         rows over the triples into their types (summed only under `expand`), [_KEPT] the kept entries of the
 *                         level that was expanded last, [_FLAGS] HGT_NB_BAD_SEED | HGT_NB_BAD_TIME, [_TYPE_BEGIN + t, _TYPE_END + t)
 *                         the rows of type t inside the level that was numbered last (both 0 for a type without rows).  The
 *                         caller copies it to the host once per level: that is the only synchronisation of a call, L + 1 reads at
 *                         the most for L layers.
 *   a call                hgt_nb_seeds; hgt_nb_number (level 0); read.  Then per level h < L with rows: hgt_nb_expand (h);
 *                         hgt_nb_number (h + 1, capacity = the level's CSR entries, skipped when there are none); hgt_nb_fill (h);
 *                         read.  Then hgt_nb_finish and, per level, hgt_nb_reset.  All on one stream.  Calls on one graph are NOT
 *                         reentrant: they share the marks.  Launches, the radix sort's own kernels aside (one sort per numbered
 *                         level): 5 for level 0 (head reset, memset, claim, head reset, numbering), 11 per expanded level (head reset,
 *                         memset, chunks and entries per item, two scans, count + claim, scan, head reset, numbering, fill, self
 *                         loops), 2 for hgt_nb_finish, 1 reset per numbered level (at most L + 1): 8 + 12 L at the most.  No grid, loop
 *                         or scratch size is proportional to the graph's N or E.
 *   hgt_nb_seeds          zeroes the head; a seed (seed_type int32, seed_id int64) outside its type's nodes sets HGT_NB_BAD_SEED and
 *                         claims nothing; every other seed claims its node (integer compare-and-swap -1 -> HGT_NB_CLAIMED), the
 *                         winner writes its key (type << 32 | id) to cand[s], its own slot of cand[n_seeds] (filled with all-ones
 *                         keys first): no counter.
 *   hgt_nb_number         radix-sorts cand[capacity] into keys_out[capacity] (rocPRIM; sort_tmp of hgt_nb_sort_bytes); the keys that
 *                         are not all-ones are the level, their count goes to head[_N], and row i of them gets mark = row_base + i, order_out[i] = the node's view row,
 *                         node_type_out[i], row_id_out[i]; the type ranges and, with expand != 0, the entry and chunk totals go to the
 *                         head.  The ORDER of a level is the sort's, never an atomic's.
 *   hgt_nb_expand         level h: chunks per item (an item = (row of the level, triple into its type), triple-major; a row of d
 *                         entries has ceil(d / HGT_NB_CHUNK) chunks) and entries per item, their single-workgroup scans into
 *                         item_chunks[n_items + 1] / item_entries[n_items + 1], then one wavefront per chunk: the kept entries of the
 *                         chunk into chunk_cnt, the sources of the kept entries claimed, a winner's key written to the slot of its
 *                         own entry in cand[capacity] (entries in front of the item + place in the row; all-ones keys elsewhere);
 *                         chunk_cnt[n_chunks + 1] scanned, its total in head[_KEPT].
 *                         n_chunks must be head[_CHUNKS] as read, capacity >= head[_DEG], type_begin / type_end (host, int64[n_types])
 *                         the head's ranges.  n_chunks == 0: only head[_N] = head[_KEPT] = 0.
 *   hgt_nb_fill           level h again, after hgt_nb_number of level h + 1: the kept entries in (triple, row, stored) order to
 *                         src_out (the source's new row, from its mark) / dst_out (row_base + the row's place in its level) /
 *                         edge_type_out / edge_time_out (has_time: tgt_time - src_time + 120; outside [0, 240) sets
 *                         HGT_NB_BAD_TIME), positions from the scan and wavefront ballots; with self_loops the level's loops follow
 *                         at [head[_KEPT], + n_level).  Every output has edge_capacity >= head[_DEG] (+ n_level) elements.
 *   hgt_nb_finish         feature_out[n_rows, width] = the rows' feature rows (node_type / row_id as hgt_nb_number wrote them);
 *                         out_rows[s] = the mark of seed s.
 *   hgt_nb_reset          mark = -1 at every key of keys[n] that is not all-ones: the end of a call and its error paths.
 *   All: a NULL table or head, n_types outside [1, HGT_SAMPLER_MAX_TYPES], n_triples outside [0, HGT_SAMPLER_MAX_TRIPLES], a
 *   negative size or one >= 2^31 - 1, a NULL array the sizes say is read or written, type ranges outside the level, a triple type
 *   outside [0, n_types): HGT_ERR_INVALID_ARG; sort_bytes too small: HGT_ERR_WORKSPACE; no launch.  hgt_nb_sort_bytes asks rocPRIM,
 *   which answers by the device's architecture: without a device it (and hgt_nb_number with valid arguments and sort_bytes >= 256)
 *   returns HGT_ERR_LAUNCH; sort_bytes < 256 is refused as HGT_ERR_WORKSPACE before the question.
 * ---------------------------------------------------------------------------------------------- */
#define HGT_NB_CHUNK 1024          /* entries of a row one wavefront takes; a longer row is split */
#define HGT_NB_WAVE_ROWS 64        /* rows of a level whose entry and chunk totals one wavefront of the numbering kernel sums (the
                                    * wavefront width: one atomic add per that many rows) */
#define HGT_NB_CLAIMED (-2)
#define HGT_NB_BAD_SEED 1
#define HGT_NB_BAD_TIME 2
#define HGT_NB_HEAD_N 0
#define HGT_NB_HEAD_DEG 1
#define HGT_NB_HEAD_CHUNKS 2
#define HGT_NB_HEAD_KEPT 3
#define HGT_NB_HEAD_FLAGS 4
#define HGT_NB_HEAD_TYPE_BEGIN 8
#define HGT_NB_HEAD_TYPE_END 24
#define HGT_NB_HEAD_WORDS 40
typedef struct hgt_nb_type {
    int32_t* mark;
    const float* feat;
    int64_t ld;
    int64_t row_off;
    int32_t n_nodes;
    int32_t reserved;
} hgt_nb_type;
typedef struct hgt_nb_triple {
    const int32_t* indptr;
    const int32_t* src;
    const int32_t* time;
    const uint8_t* tgt_flags;
    const uint8_t* src_flags;
    const int32_t* tgt_time;
    const int32_t* src_time;
    int32_t tgt_type;
    int32_t src_type;
    int32_t rel_id;
    int32_t reserved;
} hgt_nb_triple;
int hgt_nb_constants(int32_t* chunk, int32_t* wave_rows, int32_t* head_words);
int hgt_nb_sort_bytes(int64_t capacity, int32_t n_types, uint64_t* bytes_host);
int hgt_nb_seeds(const hgt_nb_type* types_dev, int32_t n_types, const int32_t* seed_type, const int64_t* seed_id, int64_t n_seeds,
                 uint64_t* cand, int64_t* head, void* stream);
int hgt_nb_number(const hgt_nb_type* types_dev, int32_t n_types, const hgt_nb_triple* triples_dev, int32_t n_triples,
                  const uint64_t* cand, int64_t capacity, uint64_t* keys_out, void* sort_tmp, uint64_t sort_bytes, int64_t row_base,
                  int32_t expand, int64_t* order_out, int64_t* node_type_out, int64_t* row_id_out, int64_t* head, void* stream);
int hgt_nb_expand(const hgt_nb_type* types_dev, int32_t n_types, const hgt_nb_triple* triples_dev, const hgt_nb_triple* triples_host,
                  int32_t n_triples, const uint64_t* keys, const int64_t* type_begin_host, const int64_t* type_end_host, int64_t n_level,
                  int64_t n_chunks, int32_t has_max_time, int32_t max_time, int32_t* item_chunks, int32_t* item_entries, int32_t* chunk_cnt,
                  uint64_t* cand, int64_t capacity, int64_t* head, void* stream);
int hgt_nb_fill(const hgt_nb_type* types_dev, int32_t n_types, const hgt_nb_triple* triples_dev, const hgt_nb_triple* triples_host,
                int32_t n_triples, const uint64_t* keys, const int64_t* type_begin_host, const int64_t* type_end_host, int64_t n_level,
                int64_t n_chunks, int32_t has_max_time, int32_t max_time, int32_t has_time, int32_t self_loops, int32_t rel_self,
                int64_t row_base, const int32_t* item_chunks, int32_t* chunk_cnt, int64_t* src_out, int64_t* dst_out,
                int64_t* edge_type_out, int64_t* edge_time_out, int64_t edge_capacity, int64_t* head, void* stream);
int hgt_nb_finish(const hgt_nb_type* types_dev, int32_t n_types, const int64_t* node_type, const int64_t* row_id, int64_t n_rows,
                  int32_t width, float* feature_out, const int32_t* seed_type, const int64_t* seed_id, int64_t n_seeds, int64_t* out_rows,
                  void* stream);
int hgt_nb_reset(const hgt_nb_type* types_dev, int32_t n_types, const uint64_t* keys, int64_t n, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Matcher retrieval (csrc/hgt_matcher_topk.hip): the k best candidates of every query and the exact rank of one candidate per query
 * over ALL candidates, without the [n_cand, n_query] score matrix that Matcher.forward(infer=True) returns (pyHGT/model.py:16-49:
 * "we will consider millions or even billions of nodes as candidates").  Added under ABI 8 (new symbols only).
 *
 *   score   s(c, q) = (row c of tx . row q of ty, a k-ordered fp32 fma chain on v_mfma_f32_32x32x2_f32) * scale, the scale applied
 *           once to the finished sum (hgt_row_dot's convention).  The bits of s(c, q) are a function of the two rows, d and scale
 *           alone: the same in both calls, for every n_cand, n_query, chunk_rows and position of the rows.
 *   order   scores compare as floats, -0 == +0, every NaN is one value above +inf; among equal scores the lower candidate position
 *           comes first (hgt_rank_metrics's tie rule).
 *
 *   hgt_matcher_topk_bytes  *bytes_host = the device scratch either call needs (the rank call asks with k = 1).  Host arithmetic only.
 *   hgt_matcher_topk        values_out float32 [n_query, k], indices_out int64 [n_query, k]: the first min(k, n_cand) candidates of
 *                           every query in that order; slots beyond n_cand hold -inf and -1.  A returned -0 reads +0 and a NaN reads
 *                           the positive quiet NaN (values are decoded from the selection key).  chunk_rows == 0: the library cuts the
 *                           candidates into chunks itself; > 0: chunks of at most that many rows, rounded up to 128 (the rows a
 *                           workgroup takes per step).  The output is the same bits for every chunk_rows.
 *   hgt_matcher_rank        rank_out[q] (int64) = #{ c : c comes before index[q] in the order of query q }, 0-based; index[q] (int64,
 *                           device) outside [0, n_cand): -1.  rank < k  <=>  index[q] is among hgt_matcher_topk's first k of query q.
 *
 *   tx [n_cand, d] and ty [n_query, d] float32 device arrays with leading dimensions ld_x, ld_y >= d (rows 16-byte aligned take
 *   16-byte loads).  Supported: d % 4 == 0, 4 <= d <= 1024, 1 <= k <= HGT_TOPK_MAX_K, n_cand < 2^31 - 1.  Caller-owned scratch, no
 *   allocation, no synchronisation, no float atomics; n_query == 0: HGT_OK without a launch; n_cand == 0 writes the padding (-1 ranks).
 *   Refusals, all before a launch: a NULL array that would be read or written, NULL bytes_host, a negative size, ld < d, k < 1, a NaN or
 *   infinite scale: HGT_ERR_INVALID_ARG; k > HGT_TOPK_MAX_K, d % 4 != 0, d < 4, d > 1024, n_query >= 2^31 - 1: HGT_ERR_UNSUPPORTED;
 *   n_cand >= 2^31 - 1 (or a chunk_rows so small that the chunks' lists pass 2^62 bytes or 2^31 - 1 workgroups): HGT_ERR_TOO_LARGE;
 *   ws NULL or ws_bytes below hgt_matcher_topk_bytes: HGT_ERR_WORKSPACE.
 * ---------------------------------------------------------------------------------------------- */
#define HGT_TOPK_MAX_K 128
int hgt_matcher_topk_bytes(int64_t n_cand, int64_t n_query, int32_t k, int64_t chunk_rows, uint64_t* bytes_host);
int hgt_matcher_topk(const float* tx, int64_t ld_x, int64_t n_cand, const float* ty, int64_t ld_y, int64_t n_query, int32_t d, float scale,
                     int32_t k, int64_t chunk_rows, float* values_out, int64_t* indices_out, void* ws, uint64_t ws_bytes, void* stream);
int hgt_matcher_rank(const float* tx, int64_t ld_x, int64_t n_cand, const float* ty, int64_t ld_y, int64_t n_query, int32_t d, float scale,
                     int64_t chunk_rows, const int64_t* index, int64_t* rank_out, void* ws, uint64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HGT_HIP_H_ */
