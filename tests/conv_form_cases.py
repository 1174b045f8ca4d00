"""Shared by tests/test_conv_forms_cpu.py and tests/test_gpu_conv_forms.py: one table of fp32 graph-convolution layers, each
built to make the library take a particular form of its kernels (fgc_conv_forms, include/fgc.h), with the graphs, the inputs
and the float64 / float32 oracle (oracle/model_ref.custom_conv2d through autograd) of every case.

A case is a dict:
  name, graph (recipe of klist()), n, c0, c1, shift, cout, act, bias_mask, seed
  mode     "dx" (input gradient wanted), "nodx" (io.dx0 == NULL), "acc0" / "acc1" / "acc01" (accumulate into a pre-filled dx0 /
           dx1 / both), "pool" (pool_y + pool_dy: the backward of the fused activation + 4:1 max pooling, two tied rows in
           some groups)
  options  per-descriptor option overrides (_lib.option_overrides); never process-level options
  off      byte offsets of x0 / dy / y / ds / r from 16-byte alignment
  expect   the fgc_conv_forms keys the case exists to reach
Default-form cases (no options) come first."""
import numpy as np
import torch

ALPHA = 0.1
K = 23
TIE_GROUPS = (2, 9, 17)          # mode "pool": rows 4g and 4g + 1 of these groups are tied (same input row, same neighbours)


# ---------------------------------------------------------------------------------------------
# graphs: 23-slot one-based K-lists, slot 0 = the node itself, zeros trailing
# ---------------------------------------------------------------------------------------------
_KLISTS = {}


def klist(recipe, n):
    """recipe: '+'-joined words.
    reg   every seventh row self-only, the others 0..15 neighbours out of a pool of 15 offsets within +-40: degrees AND
          in-degrees stay <= 16
    long  ... plus rows with 17..23 entries
    hub   ... plus one node listed by 62 rows and one by 30 (in-edge lists of three and of two chunks of 24)
    tail  the last 5 rows all zero (fake nodes of degree 0 that nobody lists)
    tie   rows 4g + 1 repeat the neighbours of rows 4g for g in TIE_GROUPS"""
    key = (recipe, n)
    if key in _KLISTS:
        return _KLISTS[key]
    words = recipe.split("+")
    rs = np.random.RandomState(1000 + n)
    real = n - 5 if "tail" in words else n
    span = np.concatenate([np.arange(-40, 0), np.arange(1, 41)])
    pool = rs.choice(span, size=15, replace=False)
    adj = np.zeros((n, K), dtype=np.int32)
    for i in range(real):
        adj[i, 0] = i + 1
        if i % 7 == 3:
            continue
        js = i + rs.permutation(pool)[:rs.randint(0, 16)]
        js = js[(js >= 0) & (js < real)]
        adj[i, 1:1 + len(js)] = js + 1
    deg = lambda i: int((adj[i] != 0).sum())
    if "long" in words:
        for i in range(1, real, 5):
            if i % 7 == 3:
                continue
            want = rs.randint(17, 24)
            while deg(i) < want:
                adj[i, deg(i)] = rs.randint(max(0, i - 40), min(real, i + 41)) + 1
    if "hub" in words:
        for hub, count, slot in ((real // 2, 62, 15), (real // 3, 30, 14)):
            rows = [i for i in rs.permutation(real) if i % 7 != 3 and i != hub and not (adj[i] == hub + 1).any()]
            have = int((adj == hub + 1).sum())
            for i in rows[:count - have]:
                adj[i, min(deg(i), slot)] = hub + 1
    if "tie" in words:
        for g in TIE_GROUPS:
            adj[4 * g + 1, 1:] = adj[4 * g, 1:]
    for i in range(n):      # zeros trailing
        nz = adj[i][adj[i] != 0]
        assert (adj[i, :len(nz)] == nz).all()
    _KLISTS[key] = adj
    return adj


# ---------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------
CASES = []


def _case(name, graph, n, cin, cout, shift=0, act=1, bias_mask=1, mode="dx", options=None, off=None, expect=None, seed=0):
    c0, c1 = cin if isinstance(cin, tuple) else (cin, 0)
    if mode == "pool" and "tie" not in graph:
        graph += "+tie"
    assert not any(c["name"] == name for c in CASES), name
    CASES.append(dict(name=name, graph=graph, n=n, c0=c0, c1=c1, shift=shift, cout=cout, act=act, bias_mask=bias_mask, mode=mode,
                      options=dict(options or {}), off=dict(off or {}), expect=dict(expect or {}), seed=seed))


def _w(cin, cout):
    return "%s_%d" % ("+".join(map(str, cin)) if isinstance(cin, tuple) else cin, cout)


W8F16 = dict(fwd="w8", fwd_fast="1", fwd_slots="16", fwd_nt="16")
W8F32 = dict(fwd="w8", fwd_fast="1", fwd_slots="16", fwd_nt="32")
K2F32 = dict(k2="w8", k2_fast="1", k2_slots="16", k2_nt="32")
DEEP = dict(k1="deep", k1_long="0", k1_half="1", k1_aglobal="0")

# ---- default options -------------------------------------------------------------------------
# plain widths, regular graph
_case("plain_32_32", "reg", 404, 32, 32, expect=dict(W8F16, **K2F32, **DEEP, k1_split="1", k1_okg="2", ds="fused", k3="stream2", proj="stream"))
_case("plain_64_32", "reg", 404, 64, 32, expect=dict(W8F16, **K2F32, **DEEP, k1_split="1", k1_okg="2", ds="fused", k3="stream4"))
_case("plain_32_64", "reg", 404, 32, 64, expect=dict(W8F16, **K2F32, **DEEP, k1_split="0", k1_okg="4", ds="fused", k3="stream2"))
_case("plain_64_64", "reg", 404, 64, 64, expect=dict(W8F16, **K2F32, **DEEP, k1_okg="4", ds="fused", k3="stream4"))
_case("plain_128_64", "reg", 404, 128, 64, expect=dict(W8F16, **K2F32, **DEEP, k1_okg="4", ds="fused", k3="stream4", proj="stream"))
_case("plain_64_128", "reg", 404, 64, 128, expect=dict(W8F32, **K2F32, **DEEP, k1_okg="8", ds="fused", k3="stream4"))
_case("plain_128_128", "reg", 404, 128, 128, expect=dict(W8F32, **K2F32, **DEEP, k1_okg="8", ds="fused", k3="stream4"))
# concatenated sources
_case("concat_32+32_32", "reg", 404, (32, 32), 32, expect=dict(W8F16, **DEEP, k1_split="1", ds="fused", k3="stream4", proj="stream"))
_case("concat_64+64_64", "reg", 404, (64, 64), 64, expect=dict(W8F16, **DEEP, k1_okg="4", ds="fused", proj="stream"))
_case("concat_32+64_64", "reg", 404, (32, 64), 64, expect=dict(W8F16, **DEEP, k1_okg="4", proj="block"))
_case("concat_48+16_32", "reg", 404, (48, 16), 32, expect=dict(fwd="w8", fwd_fast="0", fwd_slots="24", fwd_nt="32", k1="mfma", k1_vec4="1",
                                                               ds="vec", k2="w8", k2_fast="1"))
# 4x-upsampled source, no pair graph
_case("up_64_32", "reg", 404, 64, 32, shift=2, expect=dict(W8F16, **DEEP, k1_split="1", k3="stream4"))
_case("up_128_64", "reg", 404, 128, 64, shift=2, expect=dict(W8F16, **DEEP, k1_okg="4"))
# odd widths
_case("odd_32_96", "reg", 404, 32, 96, expect=dict(fwd="tiled", fwd_vec4="1", k1="deep", k1_okg="0", ds="scalar", k2="w8", k2_fast="1"))
_case("odd_32_48", "reg", 404, 32, 48, expect=dict(fwd="tiled", fwd_vec4="1", k1="deep", k1_okg="0", ds="scalar", k2="w8", k2_fast="0"))
_case("odd_30_20", "reg", 404, 30, 20, expect=dict(fwd="w8", fwd_fast="0", fwd_vec4="0", k1="mfma", k1_vec4="0", ds="scalar", k2="w8", k2_fast="0",
                                                   k3="plain", proj="block"))
_case("odd_5_7", "reg", 404, 5, 7, expect=dict(fwd="tiled", fwd_vec4="0", k1="mfma", k1_vec4="0", ds="scalar", k2="tiled", k2_vec4="0", k3="plain"))
# narrow first layer, with and without an input gradient
_case("narrow_6_32", "reg", 404, 6, 32, expect=dict(fwd="narrow", fwd_mma="1", proj="narrow", k1="mfma", k2="w8", k2_fast="1"))
_case("narrow_6_32_nodx", "reg", 404, 6, 32, mode="nodx", expect=dict(fwd="narrow", k1="narrow", k1_mma="1", ds="narrow-fused", k2="none", k3="narrow"))
_case("narrow_6_64", "reg", 404, 6, 64, expect=dict(fwd="narrow", fwd_mma="0", k1="mfma"))
_case("narrow_6_64_nodx", "reg", 404, 6, 64, mode="nodx", expect=dict(fwd="narrow", k1="narrow", k1_mma="0", ds="vec", k2="none", k3="narrow"))
# degrees 17..23
LONG = dict(fwd="w8", fwd_fast="1", fwd_slots="24", fwd_nt="32", k1="deep", k1_long="1", k1_half="0", k1_split="0", k2="w8", k2_slots="24")
_case("long_32_32", "long", 404, 32, 32, expect=dict(LONG, k1_okg="2", k1_aglobal="0", ds="fused"))
_case("long_128_64", "long", 404, 128, 64, expect=dict(LONG, k1_okg="4", k1_aglobal="1", ds="vec"))
_case("long_64_128", "long", 404, 64, 128, expect=dict(LONG, k1_okg="0", k1_aglobal="1", ds="vec"))
_case("long_64_64", "long", 404, 64, 64, expect=dict(LONG, k1_okg="4", k1_aglobal="1", ds="vec"))
_case("long_30_20", "long", 404, 30, 20, expect=dict(fwd="w8", fwd_fast="0", fwd_slots="24", k1="mfma", k1_long="1"))
# in-edge lists of three chunks
HUB = dict(k2="tiled", k2_vec4="1", k2_chunks="3")
_case("hub_32_32", "hub", 404, 32, 32, expect=dict(W8F16, **HUB))
_case("hub_128_64", "hub", 404, 128, 64, expect=dict(W8F16, **HUB))
_case("hub_64_128", "hub", 404, 64, 128, expect=dict(W8F32, **HUB))
_case("hub_64_32_n100", "hub", 100, 64, 32, expect=dict(HUB))
_case("hub_30_20", "hub", 404, 30, 20, expect=dict(HUB))
_case("hub_5_7", "hub", 404, 5, 7, expect=dict(k2="tiled", k2_vec4="0", k2_chunks="3"))
# fake nodes of degree 0 behind the real ones, with and without the bias mask
_case("tail_32_32_nomask", "reg+tail", 404, 32, 32, bias_mask=0, expect=dict(W8F16, ds="fused"))
_case("tail_128_64_nomask", "reg+tail", 404, 128, 64, bias_mask=0, expect=dict(W8F16, ds="fused"))
_case("tail_64_128_n37", "reg+tail", 37, 64, 128, expect=dict(W8F32, k1_okg="8"))
_case("tail_32_96_nomask", "reg+tail", 404, 32, 96, bias_mask=0, expect=dict(fwd="tiled", ds="scalar"))
# node counts: 37 (ragged for 16- and 32-node tiles, one slab), 100 (one slab), 1101 / 1100 (eight slabs, the last ragged)
_case("n37_32_32", "reg", 37, 32, 32, expect=dict(W8F16, k1_nodes="16", n_dc="3", k3_slabs="1"))
_case("n37_128_128", "reg", 37, 128, 128, expect=dict(W8F32, k3_slabs="1"))
_case("n37_30_20", "reg", 37, 30, 20, expect=dict(fwd="w8", fwd_fast="0", k1_nodes="32", n_dc="2"))
_case("n37_6_32_nodx", "reg", 37, 6, 32, mode="nodx", expect=dict(k1="narrow"))
_case("n100_64_64", "reg", 100, 64, 64, expect=dict(W8F16, k3_slabs="1", k3_rows="100"))
_case("n100_up_64_32", "reg", 100, 64, 32, shift=2, expect=dict(W8F16, k3_slabs="1"))
_case("n1101_32_32", "reg", 1101, 32, 32, expect=dict(W8F16, k3="stream2", k3_slabs="8", k3_rows="140"))
_case("n1101_64_128", "reg", 1101, 64, 128, expect=dict(W8F32, k3="stream4", k3_slabs="8", k3_rows="140"))
_case("n1100_128_64", "reg", 1100, 128, 64, expect=dict(W8F16, k3_slabs="8", k3_rows="140"))
_case("n1100_up_128_64", "reg", 1100, 128, 64, shift=2, expect=dict(W8F16, k3_slabs="8"))
_case("n1101_5_7", "reg", 1101, 5, 7, expect=dict(k3="plain", k3_slabs="8"))
# no activation
_case("noact_32_32", "reg", 404, 32, 32, act=0, expect=dict(ds="fused"))
_case("noact_128_64", "reg", 404, 128, 64, act=0, expect=dict(ds="fused"))
_case("noact_64_128", "reg", 404, 64, 128, act=0, expect=dict(ds="fused", k1_okg="8"))
_case("noact_32_48", "reg", 404, 32, 48, act=0, expect=dict(ds="scalar"))
# call modes
_case("nodx_64_64", "reg", 404, 64, 64, mode="nodx", expect=dict(k1="deep", k2="w8"))
_case("nodx_128_64", "reg", 404, 128, 64, mode="nodx", expect=dict(k1="deep", k2="w8"))
_case("nodx_hub_64_64", "hub", 404, 64, 64, mode="nodx", expect=dict(HUB))
_case("acc0_32_32", "reg", 404, 32, 32, mode="acc0", expect=dict(K2F32))
_case("acc01_concat_64+64_64", "reg", 404, (64, 64), 64, mode="acc01", expect=dict(K2F32))
_case("acc1_concat_32+32_32", "reg", 404, (32, 32), 32, mode="acc1", expect=dict(K2F32))
_case("acc0_up_64_32", "reg", 404, 64, 32, shift=2, mode="acc0", expect=dict(K2F32))
_case("acc0_hub_64_64", "hub", 404, 64, 64, mode="acc0", expect=dict(HUB))
_case("acc01_concat_48+16_32", "reg", 404, (48, 16), 32, mode="acc01", expect=dict(k2="w8"))
_case("pool_32_32", "reg", 404, 32, 32, mode="pool", expect=dict(ds="fused", k1_okg="2"))
_case("pool_128_64", "reg", 404, 128, 64, mode="pool", expect=dict(ds="fused", k1_okg="4"))
_case("pool_64_128", "reg", 404, 64, 128, mode="pool", expect=dict(ds="fused", k1_okg="8"))
_case("pool_32_96", "reg", 404, 32, 96, mode="pool", expect=dict(ds="scalar"))
_case("pool_concat_48+16_32", "reg", 404, (48, 16), 32, mode="pool", expect=dict(ds="vec"))
_case("pool_6_32_nodx", "reg", 404, 6, 32, mode="nodx+pool", expect=dict(ds="narrow-fused"))
# alignment: x0 at +4 / +8 bytes, dy / y / ds at +4, r at +4
for cin, cout in ((32, 32), (128, 64), (64, 128)):
    w = _w(cin, cout)
    _case("x0p4_" + w, "reg", 404, cin, cout, off=dict(x0=4), expect=dict(fwd="tiled", fwd_vec4="0", proj="block", k1="mfma", k1_vec4="0", k3="plain"))
    _case("x0p8_" + w, "reg", 404, cin, cout, off=dict(x0=8), expect=dict(fwd="w8", fwd_vec4="0", proj="block", k1="mfma", k1_vec4="0", k3="plain"))
    # (32 outputs: the split d-logits operand needs a 16-byte aligned ds; a call that packs its own operands takes the fp32 layout)
    _case("dyp4_" + w, "reg", 404, cin, cout, off=dict(dy=4, y=4, ds=4),
          expect=dict(ds="scalar", k1="deep", k1_half="1", k1_split="0", k1_okg="0", k2="tiled", k2_vec4="0"))
    _case("rp4_" + w, "reg", 404, cin, cout, off=dict(r=4), expect=dict(k2="w8", k3="plain"))
_case("rp4_hub_64_64", "hub", 404, 64, 64, off=dict(r=4), expect=dict(k2="tiled", k2_vec4="0", k3="plain"))

# ---- one option flipped (per-descriptor overrides), on 32->32, 128->64 and 64->128 wherever the option changes a form ---
N_DEFAULT = len(CASES)
for cin, cout in ((32, 32), (128, 64), (64, 128)):
    w = _w(cin, cout)
    half_k2 = cout != 64          # (the data-gradient kernel of a layer with 128 inputs has no half tiles)
    _case("NO_W8_" + w, "reg", 404, cin, cout, options=dict(NO_W8=1), expect=dict(fwd="tiled", fwd_vec4="1", k2="tiled", k2_vec4="1", k2_chunks="1"))
    _case("NO_W8FAST_" + w, "reg", 404, cin, cout, options=dict(NO_W8FAST=1),
          expect=dict(fwd="w8", fwd_fast="0", fwd_slots="24", fwd_nt="32", k2="w8", k2_fast="0", k2_slots="24"))
    if cout != 128:
        _case("W8_NT16=0_" + w, "reg", 404, cin, cout, options=dict(W8_NT16=0), expect=dict(W8F32))
    if half_k2:
        _case("W8_NT16=2_" + w, "reg", 404, cin, cout, options=dict(W8_NT16=2), expect=dict(k2="w8", k2_fast="1", k2_slots="16", k2_nt="16"))
    _case("NO_K1M_" + w, "reg", 404, cin, cout, options=dict(NO_K1M=1), expect=dict(k1="valu", k1_vec4="1", ds="vec"))
    _case("NO_K1DEEP_" + w, "reg", 404, cin, cout, options=dict(NO_K1DEEP=1), expect=dict(k1="mfma", k1_vec4="1", ds="vec"))
    _case("K1_NT16=0_" + w, "reg", 404, cin, cout, options=dict(K1_NT16=0),
          expect=dict(k1="deep", k1_half="0", k1_long="0", k1_split="0", k1_nodes="32", ds="vec" if cout == 128 else "fused"))
    _case("NO_FUSED_DS_" + w, "reg", 404, cin, cout, options=dict(NO_FUSED_DS=1), expect=dict(ds="vec", k1="deep", k1_okg="0" if cout == 128 else str(cout // 16)))
    _case("NO_TNSTREAM_" + w, "reg", 404, cin, cout, options=dict(NO_TNSTREAM=1), expect=dict(k3="plain_v4"))
    _case("NO_PROJ_STREAM_" + w, "reg", 404, cin, cout, options=dict(NO_PROJ_STREAM=1), expect=dict(proj="block", fwd_vec4="1"))
_case("NO_K1_SPLIT_32_32", "reg", 404, 32, 32, options=dict(NO_K1_SPLIT=1), expect=dict(DEEP, k1_split="0", k1_okg="2"))
_case("NO_K1_SPLIT_64_32", "reg", 404, 64, 32, options=dict(NO_K1_SPLIT=1), expect=dict(DEEP, k1_split="0", k1_okg="2"))
_case("NO_FUSED_DS128_64_128", "reg", 404, 64, 128, options=dict(NO_FUSED_DS128=1), expect=dict(ds="vec", k1="deep", k1_half="1", k1_okg="0"))
_case("NO_FUSED_DS128_128_128", "reg", 404, 128, 128, options=dict(NO_FUSED_DS128=1), expect=dict(ds="vec", k1_okg="0"))
_case("NO_DS_VEC_long_128_64", "long", 404, 128, 64, options=dict(NO_DS_VEC=1), expect=dict(ds="scalar"))
_case("NO_DS_VEC_long_64_128", "long", 404, 64, 128, options=dict(NO_DS_VEC=1), expect=dict(ds="scalar"))
_case("NO_DS_VEC_concat_48+16_32", "reg", 404, (48, 16), 32, options=dict(NO_DS_VEC=1), expect=dict(ds="scalar"))
_case("NO_K1M_long_30_20", "long", 404, 30, 20, options=dict(NO_K1M=1), expect=dict(k1="valu", k1_vec4="0", k1_long="1"))
_case("K1_NT16=0_pool_64_128", "reg", 404, 64, 128, mode="pool", options=dict(K1_NT16=0), expect=dict(ds="vec", k1_half="0"))
_case("NO_FUSED_DS_pool_32_32", "reg", 404, 32, 32, mode="pool", options=dict(NO_FUSED_DS=1), expect=dict(ds="vec"))
_case("NO_W8_hub_32_32", "hub", 404, 32, 32, options=dict(NO_W8=1), expect=dict(fwd="tiled", k2="tiled", k2_chunks="3"))
_case("NO_W8_long_64_64", "long", 404, 64, 64, options=dict(NO_W8=1), expect=dict(fwd="tiled", k2="tiled", k2_chunks="1"))
_case("NO_W8FAST_long_32_32", "long", 404, 32, 32, options=dict(NO_W8FAST=1), expect=dict(fwd_fast="0", k2_fast="0"))
_case("NO_TNSTREAM_n1101_32_32", "reg", 1101, 32, 32, options=dict(NO_TNSTREAM=1), expect=dict(k3="plain_v4", k3_slabs="8", k3_rows="140"))
_case("TN_SLOTS=8_n1101_32_32", "reg", 1101, 32, 32, options=dict(TN_SLOTS=8), expect=dict(k3="stream2", k3_slabs="8"))
_case("TN_SLOTS=256_n1101_32_32", "reg", 1101, 32, 32, options=dict(TN_SLOTS=256), expect=dict(k3="stream2", k3_slabs="8"))
_case("NO_NARROW_6_32_nodx", "reg", 404, 6, 32, mode="nodx", options=dict(NO_NARROW=1), expect=dict(fwd="w8", fwd_fast="0", k1="mfma", k2="w8"))
_case("NO_NARROW_MMA_6_32_nodx", "reg", 404, 6, 32, mode="nodx", options=dict(NO_NARROW_MMA=1),
      expect=dict(fwd="narrow", fwd_mma="0", k1="narrow", k1_mma="0", ds="vec"))
_case("NO_NARROW_FUSED_DS_6_32_nodx", "reg", 404, 6, 32, mode="nodx", options=dict(NO_NARROW_FUSED_DS=1),
      expect=dict(fwd="narrow", k1="narrow", k1_mma="1", ds="vec"))

NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


def default_sibling(case):
    """The case with the same layer, inputs and pointers on default options (None if the table has none)."""
    if not case["options"]:
        return None
    same = lambda a, b: all(a[k] == b[k] for k in ("graph", "n", "c0", "c1", "shift", "cout", "act", "bias_mask", "mode", "seed", "off"))
    return next((c for c in CASES if not c["options"] and same(c, case)), None)


# ---------------------------------------------------------------------------------------------
# inputs and the oracle
# ---------------------------------------------------------------------------------------------
def _numeric_key(case):
    return tuple(case[k] for k in ("graph", "n", "c0", "c1", "shift", "cout", "act", "bias_mask", "mode", "seed"))


_INPUTS = {}


def inputs(case):
    """CPU float32 tensors of the case: x0, x1 (or None), dy, params [W0, b, u, c, v], pool_dy (mode pool), dx0_fill /
    dx1_fill (accumulate modes).  A function of the numeric fields alone: option and offset variants share them."""
    from oracle import model_ref as R
    key = _numeric_key(case)
    if key in _INPUTS:
        return _INPUTS[key]
    n, c0, c1, cout, mode = case["n"], case["c0"], case["c1"], case["cout"], case["mode"]
    rows = n >> case["shift"]
    rs = np.random.RandomState(77 + case["seed"])
    t = lambda *shape: torch.tensor(rs.normal(size=shape).astype(np.float32))
    d = dict(x0=t(rows, c0), x1=t(rows, c1) if c1 else None, dy=t(n, cout), params=R.conv_params(c0 + c1, cout, 21 + case["seed"]))
    if "pool" in mode:
        d["pool_dy"] = t(n // 4, cout)
        for g in TIE_GROUPS:
            for x in (d["x0"], d["x1"]):
                if x is not None:
                    x[4 * g + 1] = x[4 * g]
    if "acc0" in mode or "acc01" in mode:
        d["dx0_fill"] = t(rows, c0)
    if "acc1" in mode or "acc01" in mode:
        d["dx1_fill"] = t(rows, c1)
    _INPUTS[key] = d
    return d


_PRE = {}


def preactivation(case, dtype):
    """The layer's output before the activation, by the oracle in `dtype` (cached)."""
    from oracle import model_ref as R
    key = (_numeric_key(case), dtype)
    if key not in _PRE:
        d = inputs(case)
        with torch.no_grad():
            xin = torch.cat([x.to(dtype) for x in (d["x0"], d["x1"]) if x is not None], 1)[None]
            if case["shift"]:
                xin = R.custom_upsampling(xin, 2)
            adj = torch.tensor(klist(case["graph"], case["n"])[None])
            _PRE[key] = R.custom_conv2d(xin, adj, [p.to(dtype) for p in d["params"]], biasMask=bool(case["bias_mask"]))[0]
    return _PRE[key]


_GRADS = {}


def oracle_grads(case, dtype, slope):
    """Gradients of sum(y * dy) (+ sum(pool(y) * pool_dy)) by autograd through the oracle in `dtype`, y = pre * slope with
    the given leaky-ReLU slopes (a [n, cout] tensor of 1 / ALPHA; None without activation).  Returns a dict dx0, dx1, dW0, db,
    du, dc, dv; the accumulate modes add the pre-fill.  Cached per (inputs, dtype, slopes)."""
    from oracle import model_ref as R
    key = (_numeric_key(case), dtype, None if slope is None else slope.numpy().tobytes())
    if key in _GRADS:
        return _GRADS[key]
    d = inputs(case)
    xs = [x.to(dtype).requires_grad_(True) for x in (d["x0"], d["x1"]) if x is not None]
    ps = [p.to(dtype).requires_grad_(True) for p in d["params"]]
    xin = torch.cat(xs, 1)[None]
    if case["shift"]:
        xin = R.custom_upsampling(xin, 2)
    adj = torch.tensor(klist(case["graph"], case["n"])[None])
    y = R.custom_conv2d(xin, adj, ps, biasMask=bool(case["bias_mask"]))
    if slope is not None:
        y = y * slope.to(dtype)[None]
    loss = (y[0] * d["dy"].to(dtype)).sum()
    if "pool" in case["mode"]:
        loss = loss + (R.custom_binary_tree_pooling(y, 2)[0] * d["pool_dy"].to(dtype)).sum()
    loss.backward()
    out = dict(zip(["dW0", "db", "du", "dc", "dv"], [p.grad for p in ps]))
    out["dx0"] = xs[0].grad + (d["dx0_fill"].to(dtype) if "dx0_fill" in d else 0)
    if len(xs) > 1:
        out["dx1"] = xs[1].grad + (d["dx1_fill"].to(dtype) if "dx1_fill" in d else 0)
    _GRADS[key] = out
    return out


def slopes_of(y):
    """lrelu'(pre) as the backward kernels read it from the stored y."""
    return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, ALPHA))


def sign_flips(y, pre64):
    """Elements where the sign of a float32 y differs from the sign of the float64 pre-activation: (count, largest |pre64|)."""
    bad = torch.sign(y.double()) != torch.sign(pre64)
    return int(bad.sum()), float(pre64[bad].abs().max()) if bad.any() else 0.0
