"""Host behaviour of the backward entry points that have an atomic and a `_det` form (csrc/hgt_bwd_update.hip, hgt_bwd_wgrad.hip,
hgt_bwd_outer.hip), pinned down on the CPU: the exact return code of every argument error, and the exact byte count of every
`_det_bytes` function.  Nothing here launches: every row returns before the first HIP call, so the pointers are made-up addresses that
are never read.  Where the atomic and the det form have always answered differently to the same bad input, both answers are
recorded (RECORDED below) and kept.  The byte counts were recorded from the library before the host code was unified; they change
only with the slot formulas of DESIGN.md section 10, never by regenerating them from the code under test."""
import ctypes as C

import pytest

from pyhgt_amd import _lib

OK, INVALID, UNSUPPORTED, WORKSPACE, TOO_LARGE = 0, -1, -2, -3, -4
P = 0x10000          # an aligned, never dereferenced address
MISALIGNED = P + 8
BIG = 1 << 40        # "enough" workspace bytes

NUB_HEAD = ["grad_out", "trans", "x", "ldx", "node_type", "skip", "ln_w", "use_norm"]
NUB_TAIL = ["drop_mask", "n_rows", "d", "n_types", "d_trans", "dx", "ld_dx", "d_alpha", "d_ln_w", "d_ln_b"]
WGRAD = ["A", "lda", "B", "ldb", "rows", "group_off", "n_groups", "n_rows", "m", "n_cols", "out", "out_group_stride"]
COLSUM = ["A", "lda", "rows", "group_off", "n_groups", "n_rows", "m", "out", "out_group_stride"]
OUTER = ["plan", "N", "E", "T", "R", "H", "dk_pad", "weights", "a_src", "rte_a", "b_dst", "out"]
WS = ["ws", "ws_bytes"]

# entry point -> (argument names in order, its _det_bytes function and that function's arguments by name)
ENTRY = {
    "hgt_node_update_bwd": (NUB_HEAD + NUB_TAIL + ["stream"], None),
    "hgt_node_update_bwd_ex": (NUB_HEAD + ["shared_norm"] + NUB_TAIL + ["stream"], None),
    "hgt_node_update_bwd_det": (NUB_HEAD + ["shared_norm"] + NUB_TAIL + WS + ["stream"], ["n_rows", "d", "n_types"]),
    "hgt_typed_wgrad": (WGRAD + ["stream"], None),
    "hgt_typed_wgrad_det": (WGRAD + WS + ["stream"], ["n_groups", "n_rows", "m", "n_cols"]),
    "hgt_typed_wgrad_bf16x3": (WGRAD + ["colsum", "colsum_group_stride", "stream"], None),
    "hgt_typed_wgrad_bf16x3_det": (WGRAD + ["colsum", "colsum_group_stride"] + WS + ["stream"], ["n_groups", "n_rows", "m", "n_cols"]),
    "hgt_typed_colsum": (COLSUM + ["stream"], None),
    "hgt_typed_colsum_det": (COLSUM + WS + ["stream"], ["n_groups", "n_rows", "m"]),
    "hgt_relation_outer": (OUTER + ["stream"], None),
    "hgt_relation_outer_det": (OUTER + WS + ["stream"], ["N", "E", "T", "R", "H", "dk_pad"]),
    "hgt_relation_outer_wide": (OUTER + ["stream"], None),
    "hgt_relation_outer_wide_det": (OUTER + WS + ["stream"], ["N", "E", "T", "R", "H", "dk_pad"]),
}
NUB_FORMS = ["hgt_node_update_bwd", "hgt_node_update_bwd_ex", "hgt_node_update_bwd_det"]
WGRAD_FORMS = ["hgt_typed_wgrad", "hgt_typed_wgrad_det", "hgt_typed_wgrad_bf16x3", "hgt_typed_wgrad_bf16x3_det"]
COLSUM_FORMS = ["hgt_typed_colsum", "hgt_typed_colsum_det"]
NARROW_FORMS = ["hgt_relation_outer", "hgt_relation_outer_det"]
WIDE_FORMS = ["hgt_relation_outer_wide", "hgt_relation_outer_wide_det"]

# a valid call of every family, with sizes at which the det forms need a workspace (more than one row chunk / slot)
GOOD = {
    "nub": dict(grad_out=P, trans=P, x=P, ldx=64, node_type=P, skip=P, ln_w=P, use_norm=1, shared_norm=0, drop_mask=None, n_rows=4096, d=64,
                n_types=4, d_trans=P, dx=P, ld_dx=64, d_alpha=P, d_ln_w=P, d_ln_b=P, ws=P, ws_bytes=BIG, stream=None),
    "wgrad": dict(A=P, lda=64, B=P, ldb=64, rows=P, group_off=P, n_groups=4, n_rows=300000, m=64, n_cols=64, out=P, out_group_stride=64 * 64,
                  colsum=P, colsum_group_stride=64, ws=P, ws_bytes=BIG, stream=None),
    "colsum": dict(A=P, lda=64, rows=P, group_off=P, n_groups=4, n_rows=300000, m=64, out=P, out_group_stride=64, ws=P, ws_bytes=BIG,
                   stream=None),
    "narrow": dict(plan=P, N=4000, E=40000, T=4, R=7, H=8, dk_pad=32, weights=P, a_src=P, rte_a=None, b_dst=P, out=P, ws=P, ws_bytes=BIG,
                   stream=None),
    "wide": dict(plan=P, N=4000, E=40000, T=4, R=7, H=2, dk_pad=128, weights=P, a_src=P, rte_a=None, b_dst=P, out=P, ws=P, ws_bytes=BIG,
                 stream=None),
}
FAMILY = {**{n: "nub" for n in NUB_FORMS}, **{n: "wgrad" for n in WGRAD_FORMS}, **{n: "colsum" for n in COLSUM_FORMS},
          **{n: "narrow" for n in NARROW_FORMS}, **{n: "wide" for n in WIDE_FORMS}}


def _need(name, args):
    nb = C.c_uint64()
    assert getattr(_lib.load(), name + "_bytes")(*[args[k] for k in ENTRY[name][1]], C.byref(nb)) == OK
    return int(nb.value)


def _call(name, **changes):
    args = dict(GOOD[FAMILY[name]], **changes)
    if ENTRY[name][1] and isinstance(args["ws_bytes"], str):      # "need" / "need-1": relative to what the _bytes call asks for
        args["ws_bytes"] = _need(name, args) - (args["ws_bytes"] == "need-1")
    return getattr(_lib.load(), name)(*[args[k] for k in ENTRY[name][0]])


def _rows():
    rows = []

    def add(names, code, **changes):
        rows.extend((n, changes, code) for n in names)

    det = [n for n in ENTRY if n.endswith("_det")]
    # -- a null or misaligned workspace, one byte too few (every det form; the GOOD sizes need a workspace)
    add(det, INVALID, ws=None)
    add(det, INVALID, ws=MISALIGNED)
    add(det, WORKSPACE, ws_bytes="need-1")
    add(det, WORKSPACE, ws_bytes=0)

    # -- node update
    for p in ("grad_out", "trans", "x", "node_type", "d_trans", "dx", "d_alpha", "ln_w", "d_ln_w", "d_ln_b"):
        add(NUB_FORMS, INVALID, **{p: None})       # (d_alpha: skip is given; ln_*: use_norm = 1)
    add(["hgt_node_update_bwd"], INVALID, skip=None)      # the gate is optional in the _ex and det forms only
    add(["hgt_node_update_bwd_ex"], OK, skip=None, d_alpha=None, n_rows=0)
    for ch in (dict(n_rows=-1), dict(d=0), dict(d=-64), dict(d=1025)):
        add(NUB_FORMS, INVALID, **ch)
    add(["hgt_node_update_bwd", "hgt_node_update_bwd_ex"], OK, n_rows=0)
    add(NUB_FORMS, INVALID, n_rows=0, d=1025)

    # -- typed weight gradients and column sums
    for p in ("A", "B", "rows", "group_off", "out"):
        add(WGRAD_FORMS, INVALID, **{p: None})
    for p in ("A", "rows", "group_off", "out"):
        add(COLSUM_FORMS, INVALID, **{p: None})
    for ch in (dict(n_groups=0), dict(n_groups=-1), dict(m=0), dict(n_rows=-1)):
        add(WGRAD_FORMS + COLSUM_FORMS, INVALID, **ch)
    add(WGRAD_FORMS, INVALID, n_cols=0)
    add(["hgt_typed_wgrad", "hgt_typed_wgrad_bf16x3", "hgt_typed_colsum"], OK, n_rows=0)
    add(["hgt_typed_wgrad_det", "hgt_typed_wgrad_bf16x3_det"], INVALID, out_group_stride=64 * 64 - 1)
    add(["hgt_typed_colsum_det"], INVALID, out_group_stride=63)
    add(["hgt_typed_wgrad_bf16x3_det"], INVALID, colsum_group_stride=63)
    add(["hgt_typed_wgrad_det", "hgt_typed_wgrad_bf16x3_det"], TOO_LARGE, n_groups=65536)
    add(["hgt_typed_wgrad_bf16x3"], TOO_LARGE, n_groups=65536)        # row chunks + groups pass the grid's y extent
    add(["hgt_typed_wgrad_bf16x3"], TOO_LARGE, n_rows=4096 * 65535)

    # -- relation outer products
    for p in ("plan", "a_src", "b_dst", "out", "weights"):
        add(NARROW_FORMS + WIDE_FORMS, INVALID, **{p: None})
    for ch in (dict(H=0), dict(H=-8), dict(dk_pad=0), dict(dk_pad=-32)):
        add(NARROW_FORMS + WIDE_FORMS, INVALID, **ch)
    add(NARROW_FORMS, INVALID, H=3)                       # 64 % H != 0
    add(NARROW_FORMS, INVALID, H=8, dk_pad=36)            # dk_pad is no multiple of the 64 / H lanes of a head
    add(NARROW_FORMS, UNSUPPORTED, H=1, dk_pad=128, ws_bytes="need")      # a head wider than the narrow kernels take: no layout
    for dk in (64, 512, 32, 192):
        add(WIDE_FORMS, UNSUPPORTED, dk_pad=dk)
    add(WIDE_FORMS, INVALID, a_src=MISALIGNED)
    add(WIDE_FORMS, INVALID, b_dst=MISALIGNED)
    add(WIDE_FORMS, INVALID, rte_a=MISALIGNED)
    add(WIDE_FORMS, INVALID, R=0)
    add(WIDE_FORMS, TOO_LARGE, H=65536)
    add(WIDE_FORMS, TOO_LARGE, R=65536)
    add(["hgt_relation_outer", "hgt_relation_outer_wide"], OK, E=0)
    add(["hgt_relation_outer", "hgt_relation_outer_wide"], OK, E=0, weights=None)
    add(["hgt_relation_outer_det", "hgt_relation_outer_wide_det"], INVALID, N=-1)
    add(["hgt_relation_outer_det", "hgt_relation_outer_wide_det"], INVALID, E=-1, weights=None)
    add(["hgt_relation_outer_det", "hgt_relation_outer_wide_det"], INVALID, T=0)
    return rows


# The same bad input, two answers: what each twin has always returned (the atomic forms skip a check where they need nothing of the
# value, or return at an empty problem before they reach it).  (entry point, changes, code) like the rows above.
RECORDED = [
    # n_types is looked at by the det form alone (it sizes its slots with it)
    ("hgt_node_update_bwd", dict(n_types=0, n_rows=0), OK),
    ("hgt_node_update_bwd_ex", dict(n_types=0, n_rows=0), OK),
    ("hgt_node_update_bwd_det", dict(n_types=0, n_rows=0), INVALID),
    ("hgt_node_update_bwd_det", dict(n_types=0), INVALID),
    # the output strides are looked at by the det forms alone (they overwrite their outputs)
    ("hgt_typed_wgrad", dict(out_group_stride=1, n_rows=0), OK),
    ("hgt_typed_wgrad_det", dict(out_group_stride=1, n_rows=0), INVALID),
    ("hgt_typed_wgrad_bf16x3", dict(out_group_stride=1, colsum_group_stride=1, n_rows=0), OK),
    ("hgt_typed_wgrad_bf16x3_det", dict(out_group_stride=1, n_rows=0), INVALID),
    ("hgt_typed_wgrad_bf16x3_det", dict(colsum_group_stride=1, n_rows=0), INVALID),
    ("hgt_typed_colsum", dict(out_group_stride=1, n_rows=0), OK),
    ("hgt_typed_colsum_det", dict(out_group_stride=1, n_rows=0), INVALID),
    # more groups than a grid extent: refused by the det forms (and their _bytes) whatever the row count, by the atomic bf16 x3 form
    # once it has rows, never by the atomic fp32 form
    ("hgt_typed_wgrad", dict(n_groups=65536, n_rows=0), OK),
    ("hgt_typed_wgrad_bf16x3", dict(n_groups=65536, n_rows=0), OK),
    ("hgt_typed_wgrad_det", dict(n_groups=65536, n_rows=0), TOO_LARGE),
    ("hgt_typed_wgrad_bf16x3_det", dict(n_groups=65536, n_rows=0), TOO_LARGE),
    # hgt_relation_outer returns HGT_OK on an empty graph before it looks at dk_pad % (64 / H); its det form checks first
    ("hgt_relation_outer", dict(E=0, dk_pad=36), OK),
    ("hgt_relation_outer_det", dict(E=0, dk_pad=36), INVALID),
    ("hgt_relation_outer", dict(E=0, H=3), INVALID),
    # hgt_relation_outer never looks at n_relations, n_nodes or n_types; the other three forms refuse n_relations <= 0, the det forms
    # (through their _bytes) n_nodes < 0 and n_types <= 0 as well
    ("hgt_relation_outer", dict(E=0, R=0), OK),
    ("hgt_relation_outer_det", dict(E=0, R=0), INVALID),
    ("hgt_relation_outer_det", dict(R=0), INVALID),
    ("hgt_relation_outer", dict(E=0, N=-1, T=0), OK),
    ("hgt_relation_outer_wide", dict(E=0, N=-1, T=0), OK),
    ("hgt_relation_outer_det", dict(E=0, N=-1), INVALID),
    ("hgt_relation_outer_wide_det", dict(E=0, T=0), INVALID),
]


def _id(row):
    return "%s-%s" % (row[0], ",".join("%s=%s" % kv for kv in row[1].items()))


@pytest.mark.parametrize("row", _rows(), ids=_id)
def test_argument_errors(row):
    name, changes, code = row
    assert _call(name, **changes) == code


@pytest.mark.parametrize("row", RECORDED, ids=_id)
def test_recorded_codes_of_the_twins(row):
    name, changes, code = row
    assert _call(name, **changes) == code


def _bytes(name, *args, out=True):
    nb = C.c_uint64(12345)
    rc = getattr(_lib.load(), name)(*args, C.byref(nb) if out else None)
    return rc, int(nb.value)


BYTES_ERRORS = [
    ("hgt_node_update_bwd_det_bytes", (4096, 64, 4), None, INVALID),          # (arguments, index to change / None: out = NULL, code)
    ("hgt_node_update_bwd_det_bytes", (-1, 64, 4), 0, INVALID),
    ("hgt_node_update_bwd_det_bytes", (4096, 0, 4), 0, INVALID),
    ("hgt_node_update_bwd_det_bytes", (4096, 1025, 4), 0, INVALID),
    ("hgt_node_update_bwd_det_bytes", (4096, 64, 0), 0, INVALID),
    ("hgt_typed_wgrad_det_bytes", (4, 4096, 64, 64), None, INVALID),
    ("hgt_typed_wgrad_det_bytes", (0, 4096, 64, 64), 0, INVALID),
    ("hgt_typed_wgrad_det_bytes", (4, -1, 64, 64), 0, INVALID),
    ("hgt_typed_wgrad_det_bytes", (4, 4096, 0, 64), 0, INVALID),
    ("hgt_typed_wgrad_det_bytes", (4, 4096, 64, 0), 0, INVALID),
    ("hgt_typed_wgrad_det_bytes", (65536, 4096, 64, 64), 0, TOO_LARGE),
    ("hgt_typed_wgrad_bf16x3_det_bytes", (4, 4096, 64, 64), None, INVALID),
    ("hgt_typed_wgrad_bf16x3_det_bytes", (0, 4096, 64, 64), 0, INVALID),
    ("hgt_typed_wgrad_bf16x3_det_bytes", (4, -1, 64, 64), 0, INVALID),
    ("hgt_typed_wgrad_bf16x3_det_bytes", (4, 4096, 0, 64), 0, INVALID),
    ("hgt_typed_wgrad_bf16x3_det_bytes", (4, 4096, 64, 0), 0, INVALID),
    ("hgt_typed_wgrad_bf16x3_det_bytes", (65536, 4096, 64, 64), 0, TOO_LARGE),
    ("hgt_typed_colsum_det_bytes", (4, 4096, 64), None, INVALID),
    ("hgt_typed_colsum_det_bytes", (0, 4096, 64), 0, INVALID),
    ("hgt_typed_colsum_det_bytes", (4, -1, 64), 0, INVALID),
    ("hgt_typed_colsum_det_bytes", (4, 4096, 0), 0, INVALID),
    ("hgt_relation_outer_det_bytes", (4000, 40000, 4, 7, 8, 32), None, INVALID),
    ("hgt_relation_outer_det_bytes", (-1, 40000, 4, 7, 8, 32), 0, INVALID),
    ("hgt_relation_outer_det_bytes", (4000, -1, 4, 7, 8, 32), 0, INVALID),
    ("hgt_relation_outer_det_bytes", (4000, 40000, 0, 7, 8, 32), 0, INVALID),
    ("hgt_relation_outer_det_bytes", (4000, 40000, 4, 0, 8, 32), 0, INVALID),
    ("hgt_relation_outer_det_bytes", (4000, 40000, 4, 7, 0, 32), 0, INVALID),
    ("hgt_relation_outer_det_bytes", (4000, 40000, 4, 7, 3, 32), 0, INVALID),
    ("hgt_relation_outer_det_bytes", (4000, 40000, 4, 7, 8, 0), 0, INVALID),
    ("hgt_relation_outer_det_bytes", (4000, 40000, 4, 7, 8, 36), 0, INVALID),
    ("hgt_relation_outer_det_bytes", (4000, 0, 4, 7, 8, 36), 0, INVALID),
    ("hgt_relation_outer_wide_det_bytes", (4000, 40000, 4, 7, 2, 128), None, INVALID),
    ("hgt_relation_outer_wide_det_bytes", (-1, 40000, 4, 7, 2, 128), 0, INVALID),
    ("hgt_relation_outer_wide_det_bytes", (4000, 40000, 0, 7, 2, 128), 0, INVALID),
    ("hgt_relation_outer_wide_det_bytes", (4000, 40000, 4, 0, 2, 128), 0, INVALID),
    ("hgt_relation_outer_wide_det_bytes", (4000, 40000, 4, 7, 0, 128), 0, INVALID),
    ("hgt_relation_outer_wide_det_bytes", (4000, 40000, 4, 7, 2, 64), 0, UNSUPPORTED),
    ("hgt_relation_outer_wide_det_bytes", (4000, 40000, 4, 7, 2, 512), 0, UNSUPPORTED),
    ("hgt_relation_outer_wide_det_bytes", (4000, 0, 4, 7, 2, 64), 0, UNSUPPORTED),
]


@pytest.mark.parametrize("name,args,_,code", BYTES_ERRORS, ids=lambda v: str(v).replace(" ", ""))
def test_bytes_functions_argument_errors(name, args, _, code):
    rc, nb = _bytes(name, *args, out=_ is not None)
    assert rc == code
    assert nb == 12345, "an error must leave *out alone"


# Exact workspace bytes, recorded from the library as it was before the twins shared their host code.
WORKSPACE_BYTES = [
    # node update (rows, d, n_types): no rows, fewer rows than a wavefront takes, one-pass and two-pass reduces (128 / 129 slots), the
    # 4096-slot cap, and 4096 slots of [8][256] partials cut down to DET_FLOOR
    ("hgt_node_update_bwd_det_bytes", (0, 64, 4), 0),
    ("hgt_node_update_bwd_det_bytes", (3, 64, 4), 2064),
    ("hgt_node_update_bwd_det_bytes", (300, 64, 4), 154800),
    ("hgt_node_update_bwd_det_bytes", (512, 64, 4), 264192),
    ("hgt_node_update_bwd_det_bytes", (516, 64, 4), 272448),
    ("hgt_node_update_bwd_det_bytes", (4096, 64, 4), 2146560),
    ("hgt_node_update_bwd_det_bytes", (300000, 64, 4), 8501616),
    ("hgt_node_update_bwd_det_bytes", (300000, 256, 8), 33357312),
    ("hgt_node_update_bwd_det_bytes", (300000, 1024, 8), 33505248),
    # typed weight gradients (n_groups, rows, m, n_cols): one chunk (no workspace), 128 / 129 chunks, the budget (1/16 of A and B)
    # below the wanted chunk count, more groups than chunks fit beside
    ("hgt_typed_wgrad_det_bytes", (4, 0, 64, 64), 0),
    ("hgt_typed_wgrad_det_bytes", (4, 3, 64, 64), 0),
    ("hgt_typed_wgrad_det_bytes", (4, 4096, 64, 64), 131072),
    ("hgt_typed_wgrad_det_bytes", (4, 300000, 64, 64), 9830400),
    ("hgt_typed_wgrad_det_bytes", (1, 262144, 64, 64), 2097152),
    ("hgt_typed_wgrad_det_bytes", (1, 262145, 64, 64), 2162688),
    ("hgt_typed_wgrad_det_bytes", (4, 300000, 768, 256), 75497472),
    ("hgt_typed_wgrad_det_bytes", (1, 300000, 512, 256), 57147392),
    ("hgt_typed_wgrad_det_bytes", (1000, 300000, 16, 16), 32768000),
    ("hgt_typed_wgrad_bf16x3_det_bytes", (4, 0, 64, 64), 0),
    ("hgt_typed_wgrad_bf16x3_det_bytes", (4, 3, 64, 64), 0),
    ("hgt_typed_wgrad_bf16x3_det_bytes", (4, 4096, 64, 64), 0),
    ("hgt_typed_wgrad_bf16x3_det_bytes", (4, 300000, 64, 64), 4925440),
    ("hgt_typed_wgrad_bf16x3_det_bytes", (1, 524288, 64, 64), 2129920),
    ("hgt_typed_wgrad_bf16x3_det_bytes", (1, 524289, 64, 64), 2196480),
    ("hgt_typed_wgrad_bf16x3_det_bytes", (4, 300000, 768, 256), 75792384),
    ("hgt_typed_wgrad_bf16x3_det_bytes", (1, 300000, 512, 256), 38948864),
    ("hgt_typed_wgrad_bf16x3_det_bytes", (1000, 300000, 16, 16), 32640000),
    # column sums (n_groups, rows, m): the same, budget DET_FLOOR / 2; no limit on the group count
    ("hgt_typed_colsum_det_bytes", (4, 0, 64), 0),
    ("hgt_typed_colsum_det_bytes", (4, 3, 64), 0),
    ("hgt_typed_colsum_det_bytes", (4, 4096, 64), 16384),
    ("hgt_typed_colsum_det_bytes", (4, 300000, 64), 1064960),
    ("hgt_typed_colsum_det_bytes", (1, 32768, 64), 32768),
    ("hgt_typed_colsum_det_bytes", (1, 32769, 64), 33792),
    ("hgt_typed_colsum_det_bytes", (4, 300000, 3072), 16809984),
    ("hgt_typed_colsum_det_bytes", (65536, 300000, 64), 0),
    # relation outer products (N, E, T, R, H, dk_pad): sampled-batch and full-graph item counts, no edges, a budget-limited case
    ("hgt_relation_outer_det_bytes", (4000, 40000, 4, 7, 8, 32), 32800768),
    ("hgt_relation_outer_det_bytes", (4000, 0, 4, 7, 8, 32), 0),
    ("hgt_relation_outer_det_bytes", (1000000, 10000000, 4, 7, 8, 32), 93356032),
    ("hgt_relation_outer_det_bytes", (4000, 40000, 4, 7, 4, 16), 4902912),
    ("hgt_relation_outer_det_bytes", (100, 300, 2, 1, 1, 64), 131072),
    ("hgt_relation_outer_det_bytes", (300000, 3000000, 4, 60, 16, 64), 880803840),
    ("hgt_relation_outer_det_bytes", (4000, 40000, 4, 7, 1, 128), 33030144),
    ("hgt_relation_outer_wide_det_bytes", (4000, 40000, 4, 7, 2, 128), 33030144),
    ("hgt_relation_outer_wide_det_bytes", (4000, 40000, 4, 7, 1, 256), 33030144),
    ("hgt_relation_outer_wide_det_bytes", (4000, 0, 4, 7, 2, 128), 0),
    ("hgt_relation_outer_wide_det_bytes", (1000000, 10000000, 4, 7, 8, 128), 33030144),
    ("hgt_relation_outer_wide_det_bytes", (1000000, 10000000, 4, 7, 4, 256), 29360128),
    ("hgt_relation_outer_wide_det_bytes", (4000, 40000, 4, 7, 3, 128), 33030144),
]


@pytest.mark.parametrize("name,args,expected", WORKSPACE_BYTES, ids=lambda v: str(v).replace(" ", ""))
def test_workspace_bytes(name, args, expected):
    assert isinstance(expected, int)
    assert _bytes(name, *args) == (OK, expected)
