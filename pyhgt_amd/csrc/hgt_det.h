// What the deterministic (`_det`) forms of the backward steps share (hgt_bwd_update.hip, hgt_bwd_wgrad.hip, hgt_bwd_outer.hip;
// include/hgt_hip.h, "Bit-reproducible training"): the optional workspace argument of a step's one host
// function, the workspace arithmetic and the slot-order reduction.  Slot counts are pure functions of the arguments of the
// *_det_bytes calls.  DET_FLOOR: what every workspace may take on a small problem; large problems get a fraction of the bytes of
// the operands they read (which the caller holds anyway: the saved Q|K|V of the layer bounds them).
#pragma once
#include "hgt_common.h"

constexpr uint64_t DET_FLOOR = 32ull << 20;
// many slots are summed in two passes (segments of DET_SEG slots into a scratch array, then the segments): k_det_reduce
constexpr int DET_SEG = 64, DET_TWO_PASS = 128;

// The workspace of a `_det` entry point.  Every step with a reduction has ONE host function that takes a `const HgtDetWs*`:
// NULL = the atomic form (+= into the caller's zeroed buffers), otherwise the atomic-free form (partials into the workspace, the
// outputs overwritten with their slot-order sums).
struct HgtDetWs {
    void* ptr;
    uint64_t bytes;
};

static inline unsigned nblk(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

// floats of a workspace of n_slots partials of n_elems floats, + the segment sums of the two-pass reduce
static inline uint64_t det_ws_floats(int64_t n_slots, uint64_t n_elems) {
    return (uint64_t)n_slots * n_elems + (n_slots > DET_TWO_PASS ? (uint64_t)((n_slots + DET_SEG - 1) / DET_SEG) * n_elems : 0);
}
// the largest slot count <= want whose workspace fits `budget` bytes (at least 1)
static inline int64_t det_fit_slots(int64_t want, uint64_t n_elems, uint64_t budget) {
    const uint64_t per = n_elems * 4;
    int64_t s = (int64_t)(budget / (per ? per : 1));
    if (s > DET_TWO_PASS) s = (int64_t)(budget / (per + per / DET_SEG + 1));      // the segment sums come on top
    if (s > want) s = want;
    return s < 1 ? 1 : s;
}

static inline bool det_ws_bad(const void* ws, uint64_t need) { return need > 0 && (!ws || ((uintptr_t)ws & 15) != 0); }
// can `ws` take the `need` bytes of a *_det_bytes call?
static inline int det_ws_check(const HgtDetWs& ws, uint64_t need) {
    if (det_ws_bad(ws.ptr, need)) return HGT_ERR_INVALID_ARG;
    return ws.bytes < need ? HGT_ERR_WORKSPACE : HGT_OK;
}

// out[(i / per) * ogs + i % per] = sum over the n_slots partials ([slot][slot_stride] floats, the first n_elems of each) in slot order;
// scratch: the segment sums (after the partials; only read when n_slots > DET_TWO_PASS).  Defined next to k_det_reduce
// (hgt_bwd_update.hip).
void det_reduce(const float* part, int64_t n_slots, int64_t slot_stride, int64_t n_elems, float* scratch, float* out, int64_t per,
                int64_t ogs, hipStream_t stream);
