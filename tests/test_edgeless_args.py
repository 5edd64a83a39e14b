"""Host behaviour of the per-edge entry points of the training step on an edgeless graph (csrc/hgt_edge_logits.hip,
csrc/hgt_bwd_update.hip), pinned down on the CPU like tests/test_backward_args.py: at E == 0 the per-edge arrays may be NULL (an
empty tensor has no address) and nothing is launched; at E > 0 a NULL per-edge array is still an argument error, and every other
argument error answers as before.  Every row returns before the first HIP call: the pointers are made-up addresses, never read."""
import pytest

from pyhgt_amd import _lib

OK, INVALID = 0, -1
P = 0x10000          # an aligned, never dereferenced address

GRAPH = ["plan", "N", "E", "T", "R", "H"]
ENTRY = {
    "hgt_edge_logits": GRAPH + ["dk_pad", "Q", "K", "rte_k", "att_t", "logits", "stream"],
    "hgt_edge_logits_mfma": GRAPH + ["dk_pad", "Q", "K", "rte_k", "att_t", "att_frag", "frag_f16", "logits", "stream"],
    "hgt_edge_softmax": GRAPH + ["logits_att", "stream"],
    "hgt_att_export": GRAPH + ["att_sorted", "att_out", "H_out", "stream"],
    "hgt_edge_softmax_bwd": GRAPH + ["att", "d_att", "rho", "ld_rho", "d_logits", "stream"],
    "hgt_edge_gather_sorted": GRAPH + ["by_edge_id", "sorted", "stream"],
}
# a valid call of every entry point on a graph WITH edges (never made: it would launch)
GOOD = dict(plan=P, N=5, E=7, T=3, R=4, H=4, dk_pad=16, Q=P, K=P, rte_k=None, att_t=P, att_frag=P, frag_f16=0, logits=P, logits_att=P,
            att_sorted=P, att_out=P, H_out=4, att=P, d_att=P, rho=P, ld_rho=4, d_logits=P, by_edge_id=P, sorted=P, stream=None)
# the per-edge arrays of every entry point: [E, H] floats
PER_EDGE = {
    "hgt_edge_logits": ["logits"],
    "hgt_edge_logits_mfma": ["logits"],
    "hgt_edge_softmax": ["logits_att"],
    "hgt_att_export": ["att_sorted", "att_out"],
    "hgt_edge_softmax_bwd": ["att", "d_att", "d_logits"],
    "hgt_edge_gather_sorted": ["by_edge_id", "sorted"],
}


def _call(name, **changes):
    args = dict(GOOD, **changes)
    return getattr(_lib.load(), name)(*[args[k] for k in ENTRY[name]])


def _rows():
    rows = []
    for name, arrays in PER_EDGE.items():
        none = {a: None for a in arrays}
        rows.append((name, dict(E=0), OK))                          # an empty graph with addresses: as before
        rows.append((name, dict(E=0, **none), OK))                  # ... and without: what a zero-element tensor hands over
        rows.append((name, dict(none), INVALID))                    # E > 0: still an argument error
        for a in arrays if len(arrays) > 1 else []:                 # ... each array on its own
            rows.append((name, dict(E=0, **{a: None}), OK))
            rows.append((name, {a: None}, INVALID))
        # every other argument error, with and without edges, with and without the per-edge arrays
        for base in (dict(), dict(E=0), dict(E=0, **none)):
            rows.append((name, dict(base, plan=None), INVALID))
            rows.append((name, dict(base, H=0), INVALID))
            rows.append((name, dict(base, H=-4), INVALID))
    for name in ("hgt_edge_logits", "hgt_edge_logits_mfma"):
        for base in (dict(), dict(E=0, logits=None)):
            for ch in (dict(Q=None), dict(K=None), dict(att_t=None), dict(H=3), dict(dk_pad=0), dict(dk_pad=-16)):
                rows.append((name, dict(base, **ch), INVALID))
        rows.append((name, dict(dk_pad=18), INVALID))                # no multiple of the 64 / H lanes of a head (looked at after E == 0)
        rows.append((name, dict(E=0, logits=None, dk_pad=18), OK))
    for base in (dict(), dict(E=0, logits=None)):
        rows.append(("hgt_edge_logits_mfma", dict(base, att_frag=None), INVALID))
        rows.append(("hgt_att_export", dict(base, H_out=0), INVALID))
        rows.append(("hgt_att_export", dict(base, H_out=5), INVALID))
        rows.append(("hgt_edge_softmax_bwd", dict(base, rho=None), INVALID))      # rho is per node: required with or without edges
    rows.append(("hgt_edge_softmax_bwd", dict(E=0, att=None, d_att=None, d_logits=None, rho=None), INVALID))
    rows.append(("hgt_edge_softmax", dict(N=0), OK))                # no rows: nothing to do (as before)
    return rows


def _id(row):
    return "%s-%s" % (row[0], ",".join("%s=%s" % kv for kv in row[1].items()) or "good_but_one")


@pytest.mark.parametrize("row", _rows(), ids=_id)
def test_edgeless_argument_contract(row):
    name, changes, code = row
    assert _call(name, **changes) == code
