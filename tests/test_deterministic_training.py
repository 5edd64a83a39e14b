"""CPU tests of the bit-reproducible training mode (deterministic=True): the C ABI of the atomic-free `_det` entry points, their
workspace sizes against the cap of the issue, the Python switch, and the gfx950 assembly of the new kernels (no float atomics,
no scratch).  The GPU side is tests/test_deterministic_training_gpu.py."""
import ctypes as C
import os
import pickle
import re
import shutil
import subprocess

import pytest
import torch

import pyhgt_amd
from pyhgt_amd import _lib, HGTConv, DenseHGTConv, GNN, Classifier, Matcher
from pyhgt_amd.autograd import takes_det_route, training_supported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DET_ENTRY_POINTS = ["hgt_node_update_bwd_det", "hgt_typed_wgrad_det", "hgt_typed_wgrad_bf16x3_det", "hgt_typed_colsum_det",
                    "hgt_relation_outer_det", "hgt_relation_outer_wide_det", "hgt_edge_spmm_det"]

# the shapes of tests/test_training_limits.py
WIDE = [(256, 2, 128), (512, 4, 128), (400, 4, 128), (768, 8, 128), (1024, 8, 128), (512, 2, 256), (768, 4, 256), (256, 1, 256)]
NARROW = [(64, 4), (256, 8), (200, 4), (32, 2), (16, 1), (96, 3), (128, 4), (256, 4), (400, 8), (512, 8)]
SIZES = [(4000, 40000), (1000000, 10000000)]
T, R = 4, 7
MIB = 1 << 20


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "hgt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(hgt_[a-z_0-9]+)\s*\(", text)), text


def test_abi_declares_exports_and_binds_the_det_entry_points():
    names, text = _header_symbols()
    lib = C.CDLL(_lib.LIB_PATH)
    for n in DET_ENTRY_POINTS:
        for sym in (n, n + "_bytes"):
            assert sym in names, "include/hgt_hip.h does not declare %s" % sym
            assert hasattr(lib, sym), "libhgt_hip.so lacks %s" % sym
            assert sym in _lib.SIGNATURES, "_lib.SIGNATURES lacks %s" % sym
        # the ctypes table has one argument per parameter of the declaration
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[n][1]) == len([a for a in decl.split(",") if a.strip()]), n
    assert re.search(r"#define\s+HGT_ABI_VERSION\s+8\b", text)
    assert _lib.ABI_VERSION == 8 and _lib.load().hgt_abi_version() == 8


def test_feature_bit():
    assert _lib.HGT_FEATURE_DETERMINISTIC_TRAINING == 2
    assert _lib.load().hgt_build_features() & _lib.HGT_FEATURE_DETERMINISTIC_TRAINING


def _bytes(name, *args):
    nb = C.c_uint64(12345)
    rc = getattr(_lib.load(), name)(*args, C.byref(nb))
    return rc, int(nb.value)


def _layer_workspaces(N, E, d, H):
    """{call: bytes} of every deterministic workspace one layer's backward asks for (HGTConv and DenseHGTConv, both GEMM routes)."""
    lay = _lib.layout_for(d, H)
    dp, dkp, Hl = lay.d_pad, lay.dk_pad, lay.heads
    outer = "hgt_relation_outer_det_bytes" if dkp <= 64 else "hgt_relation_outer_wide_det_bytes"
    calls = {
        "node_update": ("hgt_node_update_bwd_det_bytes", N, d, T),
        "outer": (outer, N, E, T, R, Hl, dkp),
        "spmm": ("hgt_edge_spmm_det_bytes", E, Hl, dkp, R),
        "colsum_qkv": ("hgt_typed_colsum_det_bytes", T, N, 3 * dp),
        "colsum_mid": ("hgt_typed_colsum_det_bytes", 1, N, 2 * d),
    }
    for kind in ("hgt_typed_wgrad_det_bytes", "hgt_typed_wgrad_bf16x3_det_bytes"):
        calls[kind + ":qkv"] = (kind, T, N, 3 * dp, d)
        calls[kind + ":a"] = (kind, T, N, d, dp)
        calls[kind + ":mid"] = (kind, 1, N, 2 * d, d)
        calls[kind + ":out"] = (kind, 1, N, d, 2 * d)
    out = {}
    for k, (name, *args) in calls.items():
        rc, nb = _bytes(name, *args)
        assert rc == 0, (k, rc)
        rc2, nb2 = _bytes(name, *args)
        assert (rc2, nb2) == (rc, nb), "%s is not a function of its arguments alone" % name
        out[k] = nb
    return out, 3 * N * dp * 4


@pytest.mark.parametrize("N,E", SIZES)
@pytest.mark.parametrize("d,H", [(d, H) for d, H, _ in WIDE] + NARROW)
def test_workspace_sizes_within_the_cap(d, H, N, E):
    """No deterministic workspace of a layer's backward exceeds max(64 MiB, bytes of the layer's saved Q|K|V) (one workspace is live
    at a time: each call allocates its own and releases it)."""
    sizes, qkv_bytes = _layer_workspaces(N, E, d, H)
    cap = max(64 * MIB, qkv_bytes)
    for k, nb in sizes.items():
        assert nb <= cap, "%s: %d bytes > cap %d (N=%d d=%d H=%d)" % (k, nb, cap, N, d, H)


def test_bytes_functions_refuse_bad_arguments():
    INVALID = -1
    nb = C.c_uint64()
    lib = _lib.load()
    assert lib.hgt_node_update_bwd_det_bytes(100, 0, 4, C.byref(nb)) == INVALID
    assert lib.hgt_node_update_bwd_det_bytes(100, 2048, 4, C.byref(nb)) == INVALID
    assert lib.hgt_node_update_bwd_det_bytes(-1, 64, 4, C.byref(nb)) == INVALID
    assert lib.hgt_node_update_bwd_det_bytes(100, 64, 4, None) == INVALID
    assert lib.hgt_typed_wgrad_det_bytes(0, 100, 64, 64, C.byref(nb)) == INVALID
    assert lib.hgt_typed_wgrad_bf16x3_det_bytes(4, -1, 64, 64, C.byref(nb)) == INVALID
    assert lib.hgt_typed_colsum_det_bytes(4, 100, 0, C.byref(nb)) == INVALID
    assert lib.hgt_relation_outer_det_bytes(100, 1000, 4, 7, 3, 32, C.byref(nb)) == INVALID          # 64 % heads != 0
    assert lib.hgt_relation_outer_wide_det_bytes(100, 1000, 4, 7, 8, 64, C.byref(nb)) == -2           # not a wide head: unsupported
    assert lib.hgt_edge_spmm_det_bytes(1000, 8, 32, 0, C.byref(nb)) == INVALID


def test_entry_points_refuse_bad_arguments_and_small_workspaces_without_a_launch():
    """Host-side argument checks come first: NULL tensors -> HGT_ERR_INVALID_ARG, a workspace smaller than *_det_bytes ->
    HGT_ERR_WORKSPACE (the pointers are never dereferenced on the host and nothing is launched: this runs without a GPU)."""
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -3
    buf = (C.c_char * 4096)()
    p = (C.addressof(buf) + 255) // 256 * 256       # a 16-byte aligned non-NULL stand-in
    N, d, m, n = 1000000, 256, 768, 256
    rc, need = _bytes("hgt_typed_wgrad_bf16x3_det_bytes", T, N, m, n)
    assert rc == 0 and need > 0
    args = (p, m, p, n, p, p, T, N, m, n, p, m * n, p, m)
    assert lib.hgt_typed_wgrad_bf16x3_det(*args, p, need - 1, None) == WORKSPACE
    assert lib.hgt_typed_wgrad_bf16x3_det(*args, None, need, None) == INVALID
    assert lib.hgt_typed_wgrad_bf16x3_det(None, *args[1:], p, need, None) == INVALID
    rc, need = _bytes("hgt_typed_wgrad_det_bytes", T, N, m, n)
    assert need > 0 and lib.hgt_typed_wgrad_det(*args[:12], p, need - 1, None) == WORKSPACE
    assert lib.hgt_typed_wgrad_det(*args[:10], None, m * n, p, need, None) == INVALID
    rc, need = _bytes("hgt_typed_colsum_det_bytes", T, N, m)
    assert need > 0 and lib.hgt_typed_colsum_det(p, m, p, p, T, N, m, p, m, p, need - 1, None) == WORKSPACE
    rc, need = _bytes("hgt_node_update_bwd_det_bytes", N, d, T)
    nub = (p, p, p, d, p, p, p, 1, 0, None, N, d, T, p, p, d, p, p, p)
    assert need > 0 and lib.hgt_node_update_bwd_det(*nub, p, need - 1, None) == WORKSPACE
    assert lib.hgt_node_update_bwd_det(*nub[:12], 0, *nub[13:], p, need, None) == INVALID            # no node types
    for name, dkp in (("hgt_relation_outer_det", 32), ("hgt_relation_outer_wide_det", 128)):
        rc, need = _bytes(name + "_bytes", N, 10 * N, T, R, 8, dkp)
        assert rc == 0 and need > 0
        og = (p, N, 10 * N, T, R, 8, dkp, p, p, None, p, p)
        assert getattr(lib, name)(*og, p, need - 1, None) == WORKSPACE
        assert getattr(lib, name)(*og[:11], None, p, need, None) == INVALID
    rc, need = _bytes("hgt_edge_spmm_det_bytes", 10 * N, 8, 32, R)
    sp = (p, N, 10 * N, T, R, 8, 32, p, p, None, p, p, p, 256, N)
    assert lib.hgt_edge_spmm_det(*sp, p, need - 1, None) == WORKSPACE
    assert lib.hgt_edge_spmm_det(*sp, None, need, None) == INVALID


def _ref_modules():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "ref", "ref_modules.json")) as f:
        return json.load(f)


def test_state_dict_names_do_not_move():
    """deterministic=True adds no parameter or buffer: the names, order and shapes are the reference's own (recorded from the live
    reference in tests/golden/ref/ref_modules.json with the constructor arguments used below, as in tests/test_capi.py)."""
    ref = _ref_modules()
    built = [
        ("hgt_conv_norm_rte", HGTConv(32, 32, 2, 3, 4, 0.2, True, True, deterministic=True)),
        ("hgt_conv_plain", HGTConv(32, 32, 2, 3, 4, 0.2, False, False, deterministic=True)),
        ("dense_hgt_conv", DenseHGTConv(32, 32, 2, 3, 4, 0.2, True, True, deterministic=True)),
        ("gnn", GNN(32, 64, 3, 4, 4, 2, prev_norm=True, last_norm=False, use_RTE=True, deterministic=True)),
        ("classifier", Classifier(32, 7, deterministic=True)),
        ("matcher", Matcher(32, deterministic=True)),
    ]
    for name, ours in built:
        rec = ref[name]
        sd = ours.state_dict()
        assert sorted(sd.keys()) == sorted(rec["keys"]), name
        shapes = dict(zip(rec["keys"], rec["shapes"]))
        assert all(list(sd[k].shape) == list(shapes[k]) for k in sd), name
        assert takes_det_route(ours)
        if "repr" in rec and name != "gnn":
            assert repr(ours) == rec["repr"], name
    assert not takes_det_route(HGTConv(32, 32, 2, 3, 4)) and HGTConv(32, 32, 2, 3, 4).deterministic is False


def test_deterministic_ors_the_hub_flag_for_inference():
    a = HGTConv(32, 32, 3, 4, 2, deterministic=True)
    assert a._flags() & _lib.HGT_FLAG_DETERMINISTIC_HUBS
    assert a.kernel_flags == 0
    assert HGTConv(32, 32, 3, 4, 2)._flags() == 0


def test_set_deterministic_reaches_every_module():
    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.gnn = GNN(16, 32, 3, 4, 2, 2, conv_name="hgt")
            self.dense = GNN(16, 32, 3, 4, 2, 2, conv_name="dense_hgt")
            self.cls = Classifier(32, 5)
            self.match = Matcher(32)

    m = Model()
    mods = [m.gnn, m.dense, m.cls, m.match] + [gc.base_conv for g in (m.gnn, m.dense) for gc in g.gcs]
    assert len(mods) == 8 and not any(takes_det_route(x) for x in mods)
    assert pyhgt_amd.set_deterministic(m, True) is m
    assert all(takes_det_route(x) for x in mods)
    pyhgt_amd.set_deterministic(m, False)
    assert not any(takes_det_route(x) for x in mods)
    g = GNN(16, 32, 3, 4, 2, 2, deterministic=True)
    assert takes_det_route(g) and all(takes_det_route(gc.base_conv) for gc in g.gcs)


def test_torch_switch_does_not_move_the_route():
    layer = HGTConv(32, 32, 3, 4, 2)
    torch.use_deterministic_algorithms(True)
    try:
        assert not takes_det_route(layer) and layer._flags() == 0
    finally:
        torch.use_deterministic_algorithms(False)


def test_module_unpickled_without_the_attribute_is_a_default_one():
    layer = HGTConv(32, 32, 3, 4, 2, deterministic=True)
    again = pickle.loads(pickle.dumps(layer))
    assert again.deterministic is True                      # the attribute travels with a pickle of this class
    st = layer.__getstate__()
    st.pop("deterministic")                                 # what the reference class's pickle looks like
    bare = HGTConv.__new__(HGTConv)
    bare.__setstate__(st)
    assert bare.deterministic is False and not takes_det_route(bare) and bare._flags() == 0
    for mod in (GNN(16, 32, 3, 4, 2, 1), Classifier(32, 5), Matcher(32)):
        st = dict(mod.__dict__)
        st.pop("deterministic")
        bare = type(mod).__new__(type(mod))
        bare.__setstate__(st)
        assert not takes_det_route(bare)


def test_unsupported_layout_is_still_refused_by_name():
    ok, reason = training_supported(512, 1)
    assert not ok and "backward pass supports heads" in reason


# -- the assembly of the new kernels -----------------------------------------------------------------------------------------
def _makefile_flags():
    text = open(os.path.join(ROOT, "pyhgt_amd", "csrc", "Makefile")).read()
    line = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, flags=re.M).group(1)
    return [f for f in line.replace("$(EXTRA)", "").replace("$(LABFLAGS)", "").replace("$(ARCH)", "gfx950").split() if f]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.isfile(c):
            return c
    return None


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is absent")
def test_no_float_atomics_and_no_scratch_in_the_det_kernels(tmp_path):
    """csrc/hgt_bwd_{update,wgrad,outer}.hip -> gfx950 assembly with the Makefile's flags (as tools/lab/isa.sh does), taken together;
    every kernel whose name carries k_det_ must be free of global / flat / buffer atomics and of scratch."""
    csrc = os.path.join(ROOT, "pyhgt_amd", "csrc")
    asm = ""
    for part in ("hgt_bwd_update", "hgt_bwd_wgrad", "hgt_bwd_outer"):
        out = tmp_path / (part + ".s")
        subprocess.run([_hipcc()] + _makefile_flags() + ["-S", "--cuda-device-only", part + ".hip", "-o", str(out)], cwd=csrc, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        asm += out.read_text()
    # kernel bodies: "<symbol>:" ... ".Lfunc_end"; resources: the .amdhsa_kernel blocks / metadata
    bodies = dict(re.findall(r"^(_Z\w*k_det_\w+):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.S | re.M))
    expected = ["k_det_node_update_bwd", "k_det_node_update_bwd_wide", "k_det_reduce", "k_det_typed_wgrad", "k_det_typed_wgrad_x3",
                "k_det_typed_colsum", "k_det_relation_outer", "k_det_relation_outer_mfma", "k_det_relation_outer_wide"]
    for name in expected:
        assert any(re.search(r"\d%s(I|E)" % name, sym) for sym in bodies), "no kernel %s in the assembly" % name
    assert len(bodies) >= 20      # the outer products come in many (VEC, LPH, RTE) instantiations
    for sym, body in bodies.items():
        bad = re.findall(r"^\s*((?:global|flat|buffer)_atomic\w*)", body, flags=re.M)
        assert not bad, "%s executes %s" % (sym, sorted(set(bad)))
        assert not re.search(r"^\s*scratch_(load|store)", body, flags=re.M), "%s touches scratch" % sym
        desc = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(sym), asm, flags=re.S).group(1)
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), "%s has a private segment" % sym
    # the yardstick bites: the atomic forms in the same files do execute float atomics
    atomic_bodies = dict(re.findall(r"^(_Z\w*k_typed_wgrad\w*):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.S | re.M))
    assert atomic_bodies and all(re.search(r"global_atomic_add_f32|global_atomic_pk_add", b) for b in atomic_bodies.values())
    # budgets of the wide outer product: 112 / 100 VGPRs, 40 KiB of LDS, like the kernel it mirrors
    for sym in bodies:
        if "k_det_relation_outer_wide" in sym:
            desc = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(sym), asm, flags=re.S).group(1)
            assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1)) == 40960
            vg = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1))
            assert vg <= 112, (sym, vg)
