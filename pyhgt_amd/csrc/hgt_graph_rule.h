// The entry rule of the resident-graph services (hgt_graph_view.hip, hgt_neighbourhood.hip): which CSR entry of a meta triple becomes
// an edge, and with which edge_time.  The numpy statement is pyhgt_amd.view._np_kept / _np_time_diff.
//   kept        stored time <= max_time (a TIME_NONE entry takes the target's time under the same test, and is kept where there are
//               no node times) and neither leave-out flag is set.
//   edge_time   tgt_time - src_time + 120; the reference's RTE table has HGT_RTE_LEN rows, so a value outside [0, 240) is an error --
//               what becomes of it (saturate, write as it is, which flag word) is the caller's.
// `Tri` is hgt_view_triple or hgt_nb_triple: their first seven pointer fields carry the same names.
#pragma once
#include "hgt_common.h"

#define HGT_TIME_NONE HGT_SAMPLER_TIME_NONE   // an entry (or a node) without a time of its own
#define HGT_RTE_SELF 120                      // data.py:250 for an edge between nodes of one time

// entry p of row `row` of triple `tr`, whose source is sl = tr.src[p]
template <class Tri, class Pos>
__device__ __forceinline__ bool entry_kept(const Tri& tr, int32_t row, Pos p, int32_t sl, int32_t has_max_time, int32_t max_time) {
    bool k = true;
    if (has_max_time) {
        const int32_t st = tr.time ? tr.time[p] : HGT_TIME_NONE;
        if (st == HGT_TIME_NONE) {                                      // data.py:125: the neighbour inherits the target's time
            if (tr.tgt_time) k = tr.tgt_time[row] <= max_time;
        } else {
            k = st <= max_time;
        }
    }
    if (tr.tgt_flags && tr.tgt_flags[row]) k = false;
    if (tr.src_flags && tr.src_flags[sl]) k = false;
    return k;
}

// (tr.tgt_time and tr.src_time are set: the caller has node times)
template <class Tri>
__device__ __forceinline__ int64_t entry_time_diff(const Tri& tr, int32_t row, int32_t sl) {
    return (int64_t)tr.tgt_time[row] - (int64_t)tr.src_time[sl] + HGT_RTE_SELF;
}
