// C-ABI glue: error strings, layout helper and the whole-layer entry point that enqueues every
// kernel of one HGTConv.forward (conv.py:56-134, eval mode) on the caller's stream.
#include "hgt_common.h"

#ifndef HGT_FUSED_MIN_NODES
#define HGT_FUSED_MIN_NODES 16384         // targets from which the aggregation + update run as ONE kernel (hgt_edge_aggregate_update):
                                          // 10 edges per node, d = 256: 154 vs 125 us (item-parallel + update kernel) at 8k nodes, 181 vs
                                          // 191 at 16k, 229 vs 285 at 24k, 252 vs 365 at 32k, 474 vs 677 at 60k
#endif
#ifndef HGT_ITEM_AGG_MAX_NODES
#define HGT_ITEM_AGG_MAX_NODES 65536      // graphs below this CAN take the item-parallel aggregation (its scratch is part of the workspace)
#endif
#ifndef HGT_ITEM_AGG_DEFAULT_NODES
#define HGT_ITEM_AGG_DEFAULT_NODES 65536  // ... and below this they do by default (hgt_edge_agg_items.hip; measured with 10 edges per
                                          // node: 127 vs 173 us at 8k nodes, 191 vs 194 at 16k, 369 vs 383 at 32k, 708 vs 745 at 64k, d = 256 (unfused);
                                          // 330 vs 356 at 8k ... 1409 vs 1501 at 48k, d = 512)
#endif

// hgt_edge_logits_kside.hip: that kernel on the work items [item_lo, item_hi) (a target block of the multi-GPU path), or all of them (0, -1)
int hgt_edge_logits_kside_items(const void* plan, int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, int32_t dk_pad, const float* Q,
                                const float* K, const float* rte_k, const void* att_kside, float* logits, int item_lo, int item_hi, int lane_gather,
                                void* stream);

namespace {

struct ConvWorkspace {
    uint64_t off_q, off_k, off_v, off_logits, off_agg, off_trans, off_att_t, off_msg_p, off_msg_f, off_att_f, off_att_k, off_hub;
    uint64_t off_rte_lin, off_rte_k, off_rte_v, off_rte_rows, off_rte_off, off_ws_qkv, off_ws_a, off_ws_rte, off_off2, off_pending, off_state, off_zitems, zitems_bytes, total;
    // the same layout without the item-aggregation scratch: it is the last region, every other offset stays
    void drop_item_scratch() { zitems_bytes = 0; total = off_zitems; }
};

static ConvWorkspace conv_workspace(int64_t N, int64_t NQ, int64_t E, int in_dim, int out_dim, int T, int R, int /*n_heads*/, int use_rte,
                                    const hgt_layout& lay, bool item_scratch = true, bool det_hubs = false) {
    const int H = lay.heads;     // layout heads (n_heads rounded up to a power of two)
    ConvWorkspace w;
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { uint64_t r = o; o = hgt_align_up(o + bytes, 256); return r; };
    const uint64_t dp = (uint64_t)lay.d_pad;
    w.off_q = take((uint64_t)NQ * dp * 4);
    w.off_k = take((uint64_t)N * dp * 4);
    w.off_v = take((uint64_t)N * dp * 4);
    w.off_logits = take((uint64_t)E * H * 4);
    w.off_agg = take((uint64_t)NQ * dp * 4);
    w.off_trans = take((uint64_t)NQ * out_dim * 4);
    w.off_att_t = take((uint64_t)R * H * lay.dk_pad * lay.dk_pad * 4);
    w.off_msg_p = take((uint64_t)R * H * lay.dk_pad * lay.dk_pad * 4);
    uint64_t fb = 0;
    hgt_relation_frag_bytes(R, H, lay.dk_pad, &fb);
    w.off_msg_f = take(fb);
    w.off_att_f = take(fb);
    uint64_t kb = 0;
    hgt_relation_kside_bytes(R, H, lay.dk_pad, &kb);      // (0: a layout hgt_edge_logits_kside does not cover)
    w.off_att_k = take(kb);
    uint64_t hb = 0;
    hgt_hub_workspace_bytes_ex(E, H, lay.dk_pad, R, det_hubs ? 1 : 0, &hb);
    w.off_hub = take(hb);
    if (use_rte) {
        w.off_rte_lin = take((uint64_t)HGT_RTE_LEN * in_dim * 4);
        w.off_rte_k = take((uint64_t)T * HGT_RTE_LEN * dp * 4);
        w.off_rte_v = take((uint64_t)T * HGT_RTE_LEN * dp * 4);
        w.off_rte_rows = take((uint64_t)T * HGT_RTE_LEN * 4);
        w.off_rte_off = take((uint64_t)(T + 1) * 4);
    } else {
        w.off_rte_lin = w.off_rte_k = w.off_rte_v = w.off_rte_rows = w.off_rte_off = 0;
    }
    // split-bf16 weight tiles (precision = 1); sized unconditionally, they are small
    uint64_t b = 0;
    hgt_split_weights_bytes(T, in_dim, 3 * lay.d_pad, &b);
    w.off_ws_qkv = take(b);
    // shared by the a_linear / Q-only / temporal K|V splits (used one after the other on the stream)
    hgt_split_weights_bytes(T, in_dim > lay.d_pad ? in_dim : lay.d_pad, 2 * lay.d_pad > out_dim ? 2 * lay.d_pad : out_dim, &b);
    {   // ... and by the shared dense layer of DenseHGTConv (one group; its out_linear has K = 2*out_dim, which the typed
        // shapes above do not cover when T == 1 and d_pad <= 128 -- found by tools/fuzz_parity.py)
        uint64_t b2 = 0;
        hgt_split_weights_bytes(1, 2 * out_dim, out_dim, &b2);
        if (b2 > b) b = b2;
        hgt_split_weights_bytes(1, out_dim, 2 * out_dim, &b2);
        if (b2 > b) b = b2;
    }
    w.off_ws_a = take(b);
    hgt_split_weights_bytes(1, in_dim, in_dim, &b);
    w.off_ws_rte = take(use_rte ? b : 0);
    w.off_off2 = take(256);
    w.off_pending = take((uint64_t)(NQ / 64 + 1) * 4);
    w.off_state = take((uint64_t)NQ * H * 2 * 4);   // softmax state carried between relation slices (stage 4)
    // scratch of the item-parallel aggregation (hgt_edge_aggregate_items): only for graphs in the latency regime
    w.zitems_bytes = 0;
    if (item_scratch && N < HGT_ITEM_AGG_MAX_NODES) {
        uint64_t zb = 0;
        hgt_edge_aggregate_items_bytes(E, H, lay.dk_pad, &zb);
        if (zb <= ((uint64_t)1 << 30)) w.zitems_bytes = zb;
    }
    w.off_zitems = take(w.zitems_bytes);
    w.total = o;
    return w;
}

struct PreparedLayout {
    uint64_t off_att_t, off_msg_p, off_msg_f, off_att_f, off_att_k, off_ws_qkv, off_ws_upd, off_rte_k, off_rte_v, total;
};

static PreparedLayout prepared_layout(int in_dim, int out_dim, int T, int R, int /*n_heads*/, int use_rte, const hgt_layout& lay) {
    const int H = lay.heads;
    PreparedLayout p;
    uint64_t o = 0, b = 0;
    auto take = [&](uint64_t bytes) { uint64_t r = o; o = hgt_align_up(o + bytes, 256); return r; };
    p.off_att_t = take((uint64_t)R * H * lay.dk_pad * lay.dk_pad * 4);
    p.off_msg_p = take((uint64_t)R * H * lay.dk_pad * lay.dk_pad * 4);
    hgt_relation_frag_bytes(R, H, lay.dk_pad, &b);
    p.off_msg_f = take(b);
    p.off_att_f = take(b);
    hgt_relation_kside_bytes(R, H, lay.dk_pad, &b);
    p.off_att_k = take(b);
    hgt_split_weights_bytes(T, in_dim, 3 * lay.d_pad, &b);
    p.off_ws_qkv = take(b);
    hgt_split_weights_bytes(T, lay.d_pad, out_dim, &b);
    p.off_ws_upd = take(b);
    p.off_rte_k = take(use_rte ? (uint64_t)T * HGT_RTE_LEN * lay.d_pad * 4 : 0);
    p.off_rte_v = take(use_rte ? (uint64_t)T * HGT_RTE_LEN * lay.d_pad * 4 : 0);
    p.total = o;
    return p;
}

// rows[i] = i % 240 for i < T*240 ; off[g] = g*240
__global__ void k_rte_row_lists(int T, int32_t* __restrict__ rows, int32_t* __restrict__ off) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < T * HGT_RTE_LEN) rows[i] = i % HGT_RTE_LEN;
    if (i <= T) off[i] = i * HGT_RTE_LEN;
}

// The kernels of one call, decided once (Conv::route).  AGG_FUSED and AGG_ITEMS_UPDATE run the update themselves.
enum LogitsForm { LOGITS_VALU, LOGITS_MFMA, LOGITS_SLICE, LOGITS_RANGE, LOGITS_KSIDE };
enum AggForm { AGG_FUSED, AGG_ITEMS_UPDATE, AGG_ITEMS, AGG_SLICE, AGG_SUBTILE };
enum UpdateForm { UPDATE_IN_AGGREGATION, UPDATE_LINEAR_FUSED, UPDATE_LINEAR_NODE, UPDATE_DENSE };
struct ConvRoute {
    LogitsForm logits;
    bool kside_range;        // (the range form of stage 5 takes hgt_edge_logits_kside where the one-call layer of the same graph does:
                             //  its blocks are bit-identical to that layer)
    bool mfma_logits;        // (the range form of stage 5 takes the fragment image of att_t when set)
    // aggregation forms in the order they are tried: a kernel that answers HGT_ERR_UNSUPPORTED (a head-group layout it is not
    // instantiated for -- the kernels decide that themselves) hands over to the next.  The last one is the slice or sub-tile form.
    AggForm agg[4];
    int n_agg;
    UpdateForm update;
};

// One hgt_conv_forward call: its checks, shapes, buffers and route, and the steps its stages are made of
struct Conv {
    const hgt_conv_args* a;
    hipStream_t stream;
    hgt_layout lay;
    ConvWorkspace w;
    PreparedLayout pl;
    hgt_plan_rows pr;
    int64_t N, E, NQ;
    int T, R, H, din, dout, dp, dkp, stage, fmode, sl_lo, sl_hi, sl_more;
    bool f16, split, dense, det_hubs, no_unknown_rows, have_frags, have_kside, mfma_agg;
    decltype(&hgt_split_weights) split_weights;
    bool fresh;              // this call derives the weight images (written where they live, below)
    bool wa_prepared;        // the image of W_a lives in the prepared buffer (see wa_written)
    char* wb;
    float *Q, *K, *V, *logits, *agg, *trans, *att_t, *msg_p, *rte_k, *rte_v;
    void *msg_f_buf, *att_f_buf, *att_k_buf, *msg_f, *hub_ws, *ws_qkv, *ws_upd, *ws_a;
    ConvRoute r;

    // Every check of the arguments, in the order that decides which code a call with several faults returns; nothing is
    // enqueued before it passes.  An empty graph (N == 0) passes before the stage checks: the call does nothing.
    int check(const hgt_conv_args* args) {
        if (!(a = args)) return HGT_ERR_INVALID_ARG;
        N = a->n_nodes, E = a->n_edges;
        NQ = (a->n_q_rows > 0 && a->n_q_rows <= N) ? a->n_q_rows : N;
        T = a->n_types, R = a->n_relations, din = a->in_dim, dout = a->out_dim, stage = a->stage;
        if (!a->x || !a->node_type || !a->plan || !a->w_qkv || !a->b_qkv || !a->w_a || !a->b_a || !a->relation_att ||
            !a->relation_msg || !a->relation_pri || (!a->skip && a->update_mode == 0) || !a->workspace || !a->out)
            return HGT_ERR_INVALID_ARG;
        if (din != dout) return HGT_ERR_INVALID_ARG;   // the skip connection of conv.py:131 needs in_dim == out_dim
        if (a->use_norm && (!a->ln_w || !a->ln_b)) return HGT_ERR_INVALID_ARG;
        if (a->use_rte && (!a->rte_emb || !a->rte_w || !a->rte_b)) return HGT_ERR_INVALID_ARG;
        if (a->want_att && E > 0 && !a->att_out) return HGT_ERR_INVALID_ARG;
        dense = (a->update_mode == 1);
        if (a->update_mode != 0 && a->update_mode != 1) return HGT_ERR_INVALID_ARG;
        if (a->precision < 0 || a->precision > 2) return HGT_ERR_INVALID_ARG;
        // precision 2 (fp16 hi/lo split, include/hgt_hip.h): whole-layer calls only -- the staged multi-GPU calls share one prepared
        // image between a sliced edge phase (whose state does not carry the fp16 row scales) and the rest, and stay on precision 1
        f16 = (a->precision == 2), split = (a->precision >= 1);
        if (f16 && stage != 0) return HGT_ERR_UNSUPPORTED;
        if (dense && (!a->mid_w || !a->mid_b || !a->out_w || !a->out_b || !a->out_ln_w || !a->out_ln_b)) return HGT_ERR_INVALID_ARG;
        int rc = hgt_layout_for(dout, a->n_heads, &lay);
        if (rc != HGT_OK) return rc;
        H = lay.heads;     // the kernels run with the layout's head count (extra heads are all-zero)
        dp = lay.d_pad, dkp = lay.dk_pad;
        det_hubs = (a->flags & HGT_FLAG_DETERMINISTIC_HUBS) != 0;       // needs the larger hub region: options bit 1
        w = conv_workspace(N, N, E, din, dout, T, R, H, a->use_rte, lay, true, det_hubs);   // sized for NQ == N (upper bound)
        if (a->workspace_bytes < w.total) w.drop_item_scratch();   // a workspace sized without it (hgt_conv_workspace_bytes_ex)
        if (a->workspace_bytes < w.total) return HGT_ERR_WORKSPACE;
        if (N == 0) return HGT_OK;
        pl = prepared_layout(din, dout, T, R, H, a->use_rte, lay);
        if (a->prepared && a->prepared_bytes < pl.total) return HGT_ERR_WORKSPACE;
        if (stage < 0 || stage > 5) return HGT_ERR_INVALID_ARG;
        // relation transforms of the aggregation: matrix cores (split-bf16 x3) with the split precision, exact fp32 mat-vecs otherwise
        uint64_t frag_bytes = 0;
        hgt_relation_frag_bytes(R, H, dkp, &frag_bytes);
        have_frags = split && frag_bytes > 0;
        uint64_t kside_bytes = 0;
        hgt_relation_kside_bytes(R, H, dkp, &kside_bytes);
        have_kside = kside_bytes > 0;      // (the image of hgt_edge_logits_kside: made for every precision, like the fragment images for the split ones)
        mfma_agg = have_frags && !(a->flags & HGT_FLAG_VALU_AGGREGATE);
        if (stage == 5) {   // one target block: the fused kernel pair of the single-GPU layer on a range of destination tiles
            if (a->q_begin < 0 || a->q_end < a->q_begin || a->q_end > NQ || (a->q_begin % HGT_TD) != 0 || a->item_begin < 0 ||
                a->item_end < a->item_begin)
                return HGT_ERR_INVALID_ARG;
            if (!mfma_agg || dense || a->want_att) return HGT_ERR_UNSUPPORTED;
            if (!(split && dp <= 256 && dout <= dp && (dout & 3) == 0 && (din & 3) == 0)) return HGT_ERR_UNSUPPORTED;
        }
        // stage 4: the edge phase over ONE slice of the relation buckets (multi-GPU path: relation id = source bucket * R' + relation)
        sl_lo = 0, sl_hi = R + 1, sl_more = 0;
        if (stage == 4) {
            const int S = a->slice_count, si = a->slice_index;
            if (S <= 0 || R % S != 0 || si < 0 || si >= S) return HGT_ERR_INVALID_ARG;
            if (!mfma_agg || dense) return HGT_ERR_UNSUPPORTED;      // the slice merge lives in the matrix-core aggregation kernel
            sl_lo = si * (R / S);
            sl_hi = (si + 1) * (R / S) + (si == S - 1 ? 1 : 0);       // the last slice also takes the bucket of unclaimed edges
            sl_more = (si < S - 1);
        }
        if (stage == 2 && (a->proj_n < 0 || (a->proj_n > 0 && (!a->proj_rows || !a->proj_off)))) return HGT_ERR_INVALID_ARG;
        if (stage == 2 && a->proj_n > 0 && a->proj_c24 && !split) return HGT_ERR_UNSUPPORTED;   // wire rows: split kernels only
        return HGT_OK;
    }

    void setup(hipStream_t s) {
        stream = s;
        split_weights = f16 ? hgt_split_weights_f16 : hgt_split_weights;
        fmode = (f16 ? 1 : 0) | ((a->flags & HGT_FLAG_NO_COOP_EDGE) ? 2 : 0) | ((a->flags & HGT_FLAG_COOP_EDGE_ALWAYS) ? 4 : 0);      // `frag_f16` of the item kernels
        no_unknown_rows = (a->plan_no_hubs & 2) != 0;     // the caller knows that every target row has a valid type
        wb = (char*)a->workspace;
        Q = (float*)(wb + w.off_q), K = (float*)(wb + w.off_k), V = (float*)(wb + w.off_v);
        logits = (float*)(wb + w.off_logits), agg = (float*)(wb + w.off_agg), trans = (float*)(wb + w.off_trans);
        hub_ws = (a->plan_no_hubs & 1) ? nullptr : (void*)(wb + w.off_hub);
        // weight-only preprocessing: in the caller's `prepared` buffer (kept across calls) or in the workspace (every call)
        char* pb = (char*)a->prepared;
        fresh = !(pb && a->prepared_valid);
        att_t = (float*)(pb ? pb + pl.off_att_t : wb + w.off_att_t);
        msg_p = (float*)(pb ? pb + pl.off_msg_p : wb + w.off_msg_p);
        msg_f_buf = pb ? pb + pl.off_msg_f : wb + w.off_msg_f;
        att_f_buf = pb ? pb + pl.off_att_f : wb + w.off_att_f;
        att_k_buf = pb ? pb + pl.off_att_k : wb + w.off_att_k;
        rte_k = a->use_rte ? (float*)(pb ? pb + pl.off_rte_k : wb + w.off_rte_k) : nullptr;
        rte_v = a->use_rte ? (float*)(pb ? pb + pl.off_rte_v : wb + w.off_rte_v) : nullptr;
        ws_qkv = pb ? (void*)(pb + pl.off_ws_qkv) : (void*)(wb + w.off_ws_qkv);   // tiles of the full [Q|K|V] weight
        ws_a = wb + w.off_ws_a;                                                     // scratch tiles (Q-only, K|V, temporal, dense layer)
        // The image of W_a: in the prepared buffer (HGTConv's update) or in ws_a.  ws_a is shared scratch that the Q-only projection,
        // the temporal K|V split and the dense layer also write, so an image there is split right in front of its consumer (wa_image
        // where it is read), never earlier in stream order: a split hoisted to the start of the call would be overwritten.
        wa_prepared = pb && !dense;
        ws_upd = wa_prepared ? (void*)(pb + pl.off_ws_upd) : ws_a;
        msg_f = mfma_agg ? msg_f_buf : nullptr;      // (the kernel argument; the images are made whatever the flags select)
    }

    void route() {
        const int fl = a->flags;
        const bool sliced = (stage == 4);
        // logits: the target-side transforms on the matrix cores where the vector-ALU kernel is instruction-bound (d_k >= 64)
        r.mfma_logits = have_frags && !(fl & HGT_FLAG_VALU_LOGITS) && stage != 4 && (dkp >= 64 || (fl & HGT_FLAG_MFMA_LOGITS));
        r.logits = stage == 5 ? LOGITS_RANGE : sliced ? LOGITS_SLICE : r.mfma_logits ? LOGITS_MFMA : LOGITS_VALU;
        // ... and the transform on the source side, per edge (hgt_edge_logits_kside), where that kernel is covered: 32-column heads in
        // one head group, no temporal rows, rows below 4 GiB; whole-layer and plain staged calls with a split precision.  By default
        // from 64-edge work items on (the 16- and 32-edge items of sampled batches are ragged batches of 32 lanes) and only when neither
        // logits flag names another kernel; HGT_FLAG_KSIDE_LOGITS: whatever the item size, HGT_FLAG_NO_KSIDE_LOGITS: never
        const bool kside_covered = have_kside && split && !a->use_rte && stage != 4 &&
                                   (uint64_t)N * (uint64_t)H * (uint64_t)dkp * 4u < (1ull << 32);
        const bool kside = kside_covered && !(fl & HGT_FLAG_NO_KSIDE_LOGITS) &&
                           ((fl & HGT_FLAG_KSIDE_LOGITS) || (hgt_item_edges(E) >= 64 && !(fl & (HGT_FLAG_MFMA_LOGITS | HGT_FLAG_VALU_LOGITS))));
        r.kside_range = kside && stage == 5;
        if (kside && stage != 5) r.logits = LOGITS_KSIDE;
        // (graphs below HGT_FUSED_MIN_NODES targets take the unfused kernels: the latency regime, see items)
        const bool fused = split && !dense && dp <= 256 && dout <= dp && (dout & 3) == 0 && (din & 3) == 0 &&
                           (NQ >= HGT_FUSED_MIN_NODES || (fl & HGT_FLAG_FUSED_ANY_SIZE)) &&
                           !(fl & HGT_FLAG_NO_FUSED_UPDATE) && !sliced &&
                           !(f16 && !mfma_agg);   // the vector-ALU kernel's fused epilogue only reads the bf16 image of W_a
        // latency regime: the item-parallel form (hgt_edge_agg_items.hip), where a sub-tile wavefront's chain of edge batches and
        // relation ends is the kernel time (c3: 80 -> 66 us per layer, c5: 195 -> 147 us); flags force / forbid it
        const bool items = mfma_agg && !sliced && w.zitems_bytes > 0 && NQ < HGT_ITEM_AGG_MAX_NODES && R < 64 &&
                           !(fl & HGT_FLAG_NO_ITEM_AGGREGATE) &&
                           (NQ < HGT_ITEM_AGG_DEFAULT_NODES || (fl & HGT_FLAG_ITEM_AGGREGATE));
        r.n_agg = 0;
        if (fused) r.agg[r.n_agg++] = AGG_FUSED;   // preferred form: one kernel that never writes agg (hgt_edge_aggregate_update)
        // sampled batches (round 6): the merge pass of the item-parallel aggregation IS the node update (k_merge_update) -- two of the
        // layer's five dependent kernels become one and `agg` is never written
        if (items && !dense && !(fl & HGT_FLAG_NO_MERGE_UPDATE) && dp <= 512 && dout <= 512 && dout <= dp && (dout & 3) == 0 && (din & 3) == 0)
            r.agg[r.n_agg++] = AGG_ITEMS_UPDATE;
        if (items) r.agg[r.n_agg++] = AGG_ITEMS;
        r.agg[r.n_agg++] = sliced ? AGG_SLICE : AGG_SUBTILE;
        // (257..512 columns, e.g. n_hid 400 / 512: k_typed_linear_update_wide, round 5)
        const bool fuse_update = !dense && split && (dout <= 256 || (dout <= 512 && dp <= 512)) && (dout & 3) == 0 && (din & 3) == 0;
        r.update = dense ? UPDATE_DENSE : fuse_update ? UPDATE_LINEAR_FUSED : UPDATE_LINEAR_NODE;
    }

    void mark(int i) const {
        if (a->phase_events && a->phase_events[i]) (void)hipEventRecord((hipEvent_t)a->phase_events[i], stream);
    }

    // The one rule for the image of W_a: in ws_a, every call that reads it writes it; in the prepared buffer, fresh calls write it
    // where they read it, except the stage-5 blocks: stage 1 of their forward writes it `ahead` for every width that a consumer
    // takes from a prepared buffer (rows of up to 512 padded columns), and B blocks share that one split.
    bool wa_written(bool ahead = false) const {
        if (ahead) return stage == 1 && wa_prepared && fresh && split && dp <= 512 && dout <= dp && (dout & 3) == 0;
        return !wa_prepared || (fresh && stage != 5);
    }
    int wa_image(bool ahead = false) const {
        return wa_written(ahead) ? split_weights(a->w_a, (int64_t)dout * dp, T, dp, dout, ws_upd, stream) : HGT_OK;
    }

    // typed linear dispatch: exact fp32 MFMA, or split-bf16 x3 with weights split+tiled into `wsplit`
    int linear(const float* xin, int64_t ldx, const int32_t* rws, const int32_t* goff, int ng, int64_t nrows, int kk, int nout,
               const float* Wp, int64_t wgs, const float* bp, int64_t bgs, float* o0, float* o1, float* o2, int bcols,
               int by_pos, void* wsplit, int prologue = 0, bool tiles_ready = false) const {
        if (!split)
            return hgt_typed_linear(xin, ldx, rws, goff, ng, nrows, kk, nout, Wp, wgs, bp, bgs, o0, o1, o2, bcols, by_pos, prologue, 0, stream);
        if (((nout | bcols) & 3) != 0)   // the split kernel stores 16 B per lane: odd widths take the exact fp32 kernel
            return hgt_typed_linear(xin, ldx, rws, goff, ng, nrows, kk, nout, Wp, wgs, bp, bgs, o0, o1, o2, bcols, by_pos, prologue, 0, stream);
        if (!tiles_ready) {
            int r2 = split_weights(Wp, wgs, ng, kk, nout, wsplit, stream);
            if (r2 != HGT_OK) return r2;
        }
        // (kernel-selection bits of the split linears: HGT_FLAG_XS_GEMM_ALWAYS / _NEVER -- tests and A/B runs)
        const int sel = ((a->flags & HGT_FLAG_XS_GEMM_NEVER) ? HGT_LINEAR_NO_XS : ((a->flags & HGT_FLAG_XS_GEMM_ALWAYS) ? HGT_LINEAR_FORCE_XS : 0)) |
                        ((a->flags & HGT_FLAG_NO_TILE_GEMM) ? HGT_LINEAR_NO_TILE : 0);
        return f16 ? hgt_typed_linear_f16x3(xin, ldx, rws, goff, ng, nrows, kk, nout, wsplit, bp, bgs, o0, o1, o2, bcols, by_pos, prologue | sel, stream)
                   : hgt_typed_linear_bf16x3(xin, ldx, rws, goff, ng, nrows, kk, nout, wsplit, bp, bgs, o0, o1, o2, bcols, by_pos, prologue | sel,
                                             stream);
    }

    // relation matrices: fold pri/sqrt(dk), transpose att, zero-pad heads (conv.py:98-99,104).  BOTH fragment images are made
    // whenever the split precision has them, whatever kernels this call's flags select: a `prepared` buffer outlives the call and a
    // later call with other flags trusts it (round-3 advisor finding: a flag change on a live layer read an image that was never written)
    int relation_images() const {
        if (!fresh) return HGT_OK;
        int rc = hgt_relation_pack(a->relation_att, a->relation_msg, a->relation_pri, R, a->n_heads, H, lay.d_k, dkp, att_t, msg_p, stream);
        auto frag_pack = f16 ? hgt_relation_frag_pack_f16 : hgt_relation_frag_pack;
        if (rc == HGT_OK && have_kside) rc = hgt_relation_kside_pack(att_t, R, H, dkp, att_k_buf, stream);
        if (rc != HGT_OK || !have_frags || (rc = frag_pack(msg_p, R, H, dkp, msg_f_buf, stream)) != HGT_OK) return rc;
        return frag_pack(att_t, R, H, dkp, att_f_buf, stream);
    }

    // typed projections once per NODE (conv.py:96-97,103 did them per edge)
    int project() const {
        const int64_t wstride = (int64_t)3 * dp * din;
        if (stage == 2) {   // K|V of one received chunk of halo rows (the K|V split tiles are re-made each time: tiny)
            if (a->proj_n == 0) return HGT_OK;
            // proj_c24: straight off the wire buffer (24-bit rows): no expansion pass, 3/4 of the bytes read
            const int64_t ldx = a->proj_c24 ? 3 * (int64_t)(din / 4) : din;      // (dwords per wire row)
            const float* xin = a->proj_c24 ? reinterpret_cast<const float*>(a->proj_c24) - a->proj_c24_row0 * ldx   // indexed by the LOCAL row id
                                           : a->x;
            return linear(xin, ldx, a->proj_rows, a->proj_off, T, a->proj_n, din, 2 * dp, a->w_qkv + (int64_t)dp * din, wstride, a->b_qkv + dp,
                          3 * dp, K, V, nullptr, dp, 0, ws_a, a->proj_c24 ? 2 : 0);
        }
        const bool own = (stage == 1);   // own rows only: one fused Q|K|V launch, exactly like the single-GPU layer
        if (own || NQ == N)
            return linear(a->x, din, own ? pr.rows_q : pr.rows_all, own ? pr.off_q : pr.off_all, T, own ? NQ : N, din, 3 * dp, a->w_qkv, wstride,
                          a->b_qkv, 3 * dp, Q, K, V, dp, 0, ws_qkv, 0, !fresh);
        // halo rows (>= NQ) only need K and V.  The split tiles of the full [Q|K|V] weight serve both launches:
        // Q = columns [0,dp) -> its own split; K|V = columns [dp,3dp)
        int rc = linear(a->x, din, pr.rows_q, pr.off_q, T, NQ, din, dp, a->w_qkv, wstride, a->b_qkv, 3 * dp, Q, nullptr, nullptr, dp, 0, ws_a);
        if (rc != HGT_OK) return rc;
        rc = linear(a->x, din, pr.rows_all, pr.off_all, T, N, din, 2 * dp, a->w_qkv + (int64_t)dp * din, wstride, a->b_qkv + dp, 3 * dp,
                    K, V, nullptr, dp, 0, wb + w.off_ws_qkv);      // (K|V-only tiles: workspace scratch)
        if (rc != HGT_OK || !(a->prepared && fresh && split)) return rc;
        // keep the prepared buffer complete: a later call may be a whole-graph or staged one
        return split_weights(a->w_qkv, wstride, T, din, 3 * dp, ws_qkv, stream);
    }

    // temporal tables: rte_k[t][p] = (emb[p] W_rte^T + b_rte) W_k[t]^T  (conv.py:91-92,298-299 hoisted off the edges)
    int temporal_tables() const {
        if (!a->use_rte || !fresh) return HGT_OK;
        float* rte_lin = (float*)(wb + w.off_rte_lin);
        int32_t* rrows = (int32_t*)(wb + w.off_rte_rows);
        int32_t* roff = (int32_t*)(wb + w.off_rte_off);
        k_rte_row_lists<<<(T * HGT_RTE_LEN + 255) / 256, 256, 0, stream>>>(T, rrows, roff);
        int rc = linear(a->rte_emb, din, rrows, roff, 1, HGT_RTE_LEN, din, din, a->rte_w, 0, a->rte_b, 0, rte_lin, nullptr, nullptr, din, 1,
                        wb + w.off_ws_rte);
        if (rc != HGT_OK) return rc;
        // K|V part of the weight, split again for this 2-output launch (tiny)
        return linear(rte_lin, din, rrows, roff, T, (int64_t)T * HGT_RTE_LEN, din, 2 * dp, a->w_qkv + (int64_t)dp * din, (int64_t)3 * dp * din,
                      nullptr, 0, rte_k, rte_v, nullptr, dp, 1, ws_a);
    }

    int edge_logits() const {
        const int kside_lane = (a->flags & HGT_FLAG_KSIDE_LANE_GATHER) ? 8 : 0;      // bit 3 of `frag_f16` of hgt_edge_logits_kside
        if (r.logits == LOGITS_KSIDE) {      // (route() checked the coverage; an answer of "unsupported" still takes the other kernels)
            const int rc = hgt_edge_logits_kside(a->plan, N, E, T, R, H, dkp, Q, K, rte_k, att_t, att_k_buf, fmode | kside_lane, logits, stream);
            if (rc != HGT_ERR_UNSUPPORTED) return rc;
            if (r.mfma_logits) return hgt_edge_logits_mfma(a->plan, N, E, T, R, H, dkp, Q, K, rte_k, att_t, att_f_buf, fmode, logits, stream);
        }
        switch (r.logits) {
            case LOGITS_RANGE:
                if (r.kside_range) {
                    const int rc = hgt_edge_logits_kside_items(a->plan, N, E, T, R, H, dkp, Q, K, rte_k, att_k_buf, logits, a->item_begin, a->item_end, kside_lane, stream);
                    if (rc != HGT_ERR_UNSUPPORTED) return rc;
                }
                return hgt_edge_logits_range(a->plan, N, E, T, R, H, dkp, Q, K, rte_k, att_t, r.mfma_logits ? att_f_buf : nullptr, fmode, logits,
                                             a->item_begin, a->item_end, stream);
            case LOGITS_SLICE: return hgt_edge_logits_slice(a->plan, N, E, T, R, H, dkp, Q, K, rte_k, att_t, logits, sl_lo, sl_hi, stream);
            case LOGITS_MFMA: return hgt_edge_logits_mfma(a->plan, N, E, T, R, H, dkp, Q, K, rte_k, att_t, att_f_buf, fmode, logits, stream);
            default: return hgt_edge_logits(a->plan, N, E, T, R, H, dkp, Q, K, rte_k, att_t, logits, stream);
        }
    }

    // the fused aggregation + update kernel (hgt_edge_aggregate_update) on the destination rows [q0, q1) (q1 = -1: all of them)
    int aggregate_update(int64_t q0, int64_t q1, int hub_det) const {
        return hgt_edge_aggregate_update_sel(a->plan, N, E, T, R, H, dkp, logits, V, rte_v, msg_p, msg_f, agg, NQ, hub_ws,
                                             (int32_t*)(wb + w.off_pending), a->node_type, ws_upd, a->b_a, a->x, din, a->skip, a->ln_w,
                                             a->ln_b, a->use_norm, dout, a->out, stream, q0, q1, f16 ? 1 : 0, hub_det);
    }

    // runs for E == 0 too: it writes the zero rows of isolated targets; HGTConv stores gelu(agg) (conv.py:119), DenseHGTConv agg
    int aggregate(AggForm form) const {
        void* zitems = wb + w.off_zitems;
        switch (form) {
            case AGG_FUSED:
                if (det_hubs && hub_ws && !msg_f)
                    return HGT_ERR_UNSUPPORTED;      // (vector-ALU aggregation: the unfused kernels carry the deterministic hub mode)
                return aggregate_update(0, (det_hubs && hub_ws) ? NQ : -1, (det_hubs && hub_ws) ? 1 : 0);
            case AGG_ITEMS_UPDATE:
                return hgt_edge_aggregate_items_update(a->plan, N, E, T, R, H, dkp, logits, V, rte_v, msg_f, fmode, NQ, zitems, w.zitems_bytes,
                                                       pr.rows_q, pr.off_q, T, ws_upd, a->b_a, a->x, din, a->skip, a->ln_w, a->ln_b,
                                                       a->use_norm, dout, a->out, stream);
            case AGG_ITEMS:
                return hgt_edge_aggregate_items(a->plan, N, E, T, R, H, dkp, logits, V, rte_v, msg_f, fmode, agg, NQ, dense ? 0 : 1, zitems,
                                                w.zitems_bytes, stream);
            case AGG_SLICE:   // (state + un-normalised rows stay in the workspace for the next slice)
                return hgt_edge_aggregate_slice_ex(a->plan, N, E, T, R, H, dkp, logits, V, rte_v, msg_p, msg_f, agg, NQ, 1, hub_ws, sl_lo,
                                                   sl_hi, (float*)(wb + w.off_state), sl_lo > 0, sl_more, det_hubs ? 1 : 0, stream);
            default:
                return hgt_edge_aggregate_ex(a->plan, N, E, T, R, H, dkp, logits, V, rte_v, msg_p, msg_f, (f16 && msg_f) ? 1 : 0, agg, NQ,
                                             dense ? 0 : 1, hub_ws, det_hubs ? 1 : 0, stream);
        }
    }

    // edge phase: logits, then softmax fused into the aggregation (online, per target sub-tile)
    int edge_phase(AggForm* used) const {
        int i = 0, rc = HGT_ERR_UNSUPPORTED;
        if (E > 0) {
            const int lrc = edge_logits();
            if (lrc != HGT_OK) return lrc;
        }
        mark(2);
        mark(3);
        for (; rc == HGT_ERR_UNSUPPORTED && i < r.n_agg; i++) {
            // (the two forms with the update inside read the image of W_a: a failed split ends the call, it is no fall-through)
            if ((r.agg[i] == AGG_FUSED || r.agg[i] == AGG_ITEMS_UPDATE) && (rc = wa_image()) != HGT_OK) return rc;
            rc = aggregate(r.agg[i]);
        }
        *used = r.agg[i - 1];
        return rc;
    }

    // self.att (conv.py:108): normalise the logits in place and un-sort them
    int export_att() const {
        if (!a->want_att || E == 0) return HGT_OK;
        int rc = hgt_edge_softmax(a->plan, N, E, T, R, H, logits, stream);
        if (rc != HGT_OK) return rc;
        return hgt_att_export(a->plan, N, E, T, R, H, logits, a->att_out, a->n_heads, stream);
    }

    // update: a_linear(gelu(agg)) -> gated skip -> LayerNorm (conv.py:119-133)
    int update(AggForm form) const {
        const UpdateForm u = (form == AGG_FUSED || form == AGG_ITEMS_UPDATE) ? UPDATE_IN_AGGREGATION : r.update;
        int rc = HGT_OK;
        if (u == UPDATE_LINEAR_FUSED && (rc = wa_image()) == HGT_OK)
            rc = (f16 ? hgt_linear_update_f16x3 : hgt_linear_update_bf16x3)(agg, dp, pr.rows_q, pr.off_q, T, NQ, dp, dout, ws_upd, a->b_a, dout, a->x, din, a->skip, a->ln_w,
                                          a->ln_b, (a->use_norm ? 1 : 0) | ((a->flags & HGT_FLAG_NO_TILE_GEMM) ? 2 : 0), a->out, stream);
        else if (u == UPDATE_LINEAR_NODE || u == UPDATE_DENSE)   // (n_hid = 400 ...: W_a's image is kept like the fused forms')
            rc = linear(agg, dp, pr.rows_q, pr.off_q, T, NQ, dp, dout, a->w_a, (int64_t)dout * dp, a->b_a, dout, trans, nullptr, nullptr, dout,
                        0, ws_upd, 0, !wa_written());
        if (rc != HGT_OK) return rc;
        mark(5);
        if (u == UPDATE_DENSE) return dense_layer();
        if (u == UPDATE_LINEAR_NODE)
            rc = hgt_node_update(trans, a->x, din, a->node_type, a->skip, a->ln_w, a->ln_b, a->use_norm, NQ, dout, T, a->out, stream);
        else if (form != AGG_FUSED && !no_unknown_rows)
            rc = hgt_zero_rows(pr.rows_q, pr.off_q + T, dout, a->out, stream);   // nodes of unknown type -> 0 (conv.py:120)
        mark(6);
        return rc;
    }

    // DenseHGTConv.update (conv.py:250-274) after a_linear: no gelu on the aggregate, plain residual, then the shared dense layer
    int dense_layer() const {
        // y1 = LN_t(a_linear(agg) + x), kept in `out`
        int rc = hgt_node_update_ex(trans, a->x, din, a->node_type, nullptr, a->ln_w, a->ln_b, a->use_norm, 0, NQ, dout, T, a->out, stream);
        if (rc != HGT_OK) return rc;
        int32_t* off2 = (int32_t*)(wb + w.off_off2);      // {0, off_q[T]}: all rows of a valid type as ONE group
        rc = hgt_single_group_offsets(pr.off_q, T, off2, stream);
        if (rc != HGT_OK) return rc;
        // mid = mid_linear(y1): [NQ][2*dout] in the (dead) Q|K region; gelu is applied where out_linear loads it
        float* mid = Q;
        if (w.off_k != w.off_q + (uint64_t)N * dp * 4 || 2 * dout > 2 * dp) return HGT_ERR_WORKSPACE;
        rc = linear(a->out, dout, pr.rows_q, off2, 1, NQ, dout, 2 * dout, a->mid_w, 0, a->mid_b, 0, mid, nullptr, nullptr, 2 * dout, 0, ws_a);
        if (rc != HGT_OK) return rc;
        rc = linear(mid, 2 * dout, pr.rows_q, off2, 1, NQ, 2 * dout, dout, a->out_w, 0, a->out_b, 0, trans, nullptr, nullptr, dout, 0, ws_a, 1);
        if (rc != HGT_OK) return rc;
        // out = out_norm(out_linear(...) + y1), in place over y1
        rc = hgt_node_update_ex(trans, a->out, dout, a->node_type, nullptr, a->out_ln_w, a->out_ln_b, 1, 1, NQ, dout, T, a->out, stream);
        mark(6);
        return rc;
    }

    // stage 5: edge phase + fused update of ONE target block (multi-GPU path: the block's in-edges only reference source rows of
    // the halo chunks that have arrived); every block is the single-GPU kernel pair on a range of destination tiles
    int block_pair() const {
        if (a->q_begin == a->q_end) return HGT_OK;
        int rc;
        if (E > 0 && a->item_end > a->item_begin && (rc = edge_logits()) != HGT_OK) return rc;
        mark(2);
        mark(3);
        if ((rc = wa_image()) != HGT_OK) return rc;
        rc = aggregate_update(a->q_begin, a->q_end, det_hubs ? 1 : 0);     // (f16 is 0 here: stage 5)
        mark(4);
        mark(5);
        mark(6);
        return rc;
    }
};

}  // namespace

extern "C" const char* hgt_strerror(int code) {
    switch (code) {
        case HGT_OK: return "ok";
        case HGT_ERR_INVALID_ARG: return "invalid argument";
        case HGT_ERR_UNSUPPORTED: return "unsupported shape (need d % n_heads == 0, n_heads <= 16, padded row width <= 1024)";
        case HGT_ERR_WORKSPACE: return "workspace too small";
        case HGT_ERR_TOO_LARGE: return "problem exceeds 32-bit plan indices";
        case HGT_ERR_LAUNCH: return "HIP launch/runtime error";
        default: return "unknown error";
    }
}

extern "C" int hgt_abi_version(void) { return HGT_ABI_VERSION; }
extern "C" int hgt_build_features(void) { return HGT_FEATURE_DETERMINISTIC_TRAINING; }

extern "C" int hgt_layout_for(int32_t d_out, int32_t n_heads, hgt_layout* out) {
    if (!out) return HGT_ERR_INVALID_ARG;
    int rc = hgt_layout_compute(d_out, n_heads, out);
    if (rc != HGT_OK) return rc;
    // rows of up to 1024 padded columns (vec 16: n_hid 768 / 1024; the edge kernels split them into head groups of <= 256 or 512
    // columns per wavefront), at least 4 lanes per head (n_heads <= 16)
    if (out->vec > 16 || 64 / out->heads < 4) return HGT_ERR_UNSUPPORTED;
    return HGT_OK;
}

extern "C" int hgt_conv_workspace_bytes(int64_t n_nodes, int64_t n_edges, int32_t in_dim, int32_t out_dim, int32_t n_types,
                                        int32_t n_relations, int32_t n_heads, int32_t use_rte, uint64_t* out) {
    return hgt_conv_workspace_bytes_ex(n_nodes, n_edges, in_dim, out_dim, n_types, n_relations, n_heads, use_rte, 1, out);
}

// ABI 6: the same without the scratch of the item-parallel aggregation (up to 1 GiB on graphs below 65536 nodes) for callers that
// know the call cannot take it: exact fp32 precision, HGT_FLAG_NO_ITEM_AGGREGATE, staged multi-GPU calls.  hgt_conv_forward
// accepts either size (a workspace without the scratch simply rules the item-parallel kernel out).
extern "C" int hgt_conv_workspace_bytes_ex(int64_t n_nodes, int64_t n_edges, int32_t in_dim, int32_t out_dim, int32_t n_types,
                                           int32_t n_relations, int32_t n_heads, int32_t use_rte, int32_t options, uint64_t* out) {
    if (!out || n_nodes < 0 || n_edges < 0 || in_dim <= 0) return HGT_ERR_INVALID_ARG;
    hgt_layout lay;
    int rc = hgt_layout_for(out_dim, n_heads, &lay);
    if (rc != HGT_OK) return rc;
    *out = conv_workspace(n_nodes, n_nodes, n_edges, in_dim, out_dim, n_types, n_relations, n_heads, use_rte, lay, (options & 1) != 0, (options & 2) != 0).total;
    return HGT_OK;
}

extern "C" int hgt_conv_prepared_bytes(int32_t in_dim, int32_t out_dim, int32_t n_types, int32_t n_relations, int32_t n_heads,
                                       int32_t use_rte, uint64_t* out) {
    if (!out || in_dim <= 0 || n_types <= 0 || n_relations <= 0) return HGT_ERR_INVALID_ARG;
    hgt_layout lay;
    int rc = hgt_layout_for(out_dim, n_heads, &lay);
    if (rc != HGT_OK) return rc;
    *out = prepared_layout(in_dim, out_dim, n_types, n_relations, n_heads, use_rte, lay).total;
    return HGT_OK;
}

// stages (include/hgt_hip.h) as compositions of the steps of Conv
extern "C" int hgt_conv_forward(const hgt_conv_args* a, void* stream) {
    Conv c;
    int rc = c.check(a);
    if (rc != HGT_OK || c.N == 0) return rc;
    c.setup((hipStream_t)stream);
    c.route();
    if (c.stage == 0 || c.stage == 1) c.mark(0);
    if ((rc = hgt_plan_row_lists(a->plan, c.N, c.E, c.T, c.R, &c.pr)) != HGT_OK) return rc;
    if (c.stage == 2) return c.project();
    if (c.stage == 0 || c.stage == 1) {
        if ((rc = c.relation_images()) != HGT_OK || (rc = c.project()) != HGT_OK || (rc = c.temporal_tables()) != HGT_OK) return rc;
        if (c.stage == 1) return c.wa_image(true);
    }
    c.mark(1);
    if (c.stage == 5) return c.block_pair();
    AggForm form;
    if ((rc = c.edge_phase(&form)) != HGT_OK) return rc;
    if (form == AGG_SLICE && c.sl_more) return HGT_OK;
    if ((rc = c.export_att()) != HGT_OK) return rc;
    c.mark(4);
    return c.update(form);
}
