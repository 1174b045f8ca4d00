"""Shared by tests/test_conv_forms_bf16_cpu.py and tests/test_gpu_conv_forms_bf16.py: one table of graph-convolution layers in
bf16 storage (FGC_CONV_BF16) and in the pair form of the up-convolutions (fp32 and bf16), each built to make the library take a
particular form of its kernels (fgc_conv_forms, include/fgc.h), with the inputs, the float64 / float32 oracle
(oracle/model_ref.custom_conv2d through autograd) and the float64 STORAGE REFERENCE of every case.  The companion of
tests/conv_form_cases.py (fp32, fine form), whose graphs and helpers it reuses.

A case is a dict with the fields of conv_form_cases.py -
  name, graph, n, c0, c1, shift, cout, act, bias_mask, mode, options, off, expect, seed
- and
  storage  "bf16" | "fp32"
  pairs    the layer (shift == 2, one source, n % 4 == 0) is described with its pair graph (FacetGraph.pairs)
  r_ld     0 (the call derives the stride of r) | "pad" (fgc_conv_r_ld(cout, 1, bf16), stated in io.r_ld)
  refused  None, or the entry point that must return FGC_EINVAL for the case ("fgc_conv_fwd" / "fgc_conv_bwd")
`off` counts BYTES from 16-byte alignment.  Default-option cases come first.

Inputs: x, dy, pool_dy and every pre-fill are bf16-rounded normal draws, W0 is rounded to bf16 and kept as float (packing it
as a bf16 MFMA operand is exact), so both storages and every reference see the same numbers.

The table is a little larger than its 60..90 guideline: every pair-form layer runs in both storages."""
import numpy as np
import torch

from conv_form_cases import klist, K, ALPHA, TIE_GROUPS, slopes_of, sign_flips      # noqa: F401 (re-exported to the tests)

FLOOR_BF16 = 2.0 ** -9            # half a bf16 ulp at a tensor's largest entry
CAPS = {"y": 4e-3, "y_pool": 4e-3, "dx0": 5e-3, "dx1": 5e-3, "dW0": 3e-3, "db": 1e-5, "du": 6e-3, "dv": 6e-3, "dc": 1e-2}
GRAD_NAMES = ["dx0", "dx1", "dW0", "db", "du", "dc", "dv"]

CASES = []

# Seeds, per layer (graph, n, c0, c1, shift, cout, act, bias_mask, mode); 0 where a layer is not listed.  Rounding to bf16 costs
# between 2^-9 and 2^-8 of a tensor's largest entry, depending on where that entry lies in its binade and on how the elements
# near it happen to round: each seed is the first for which the storage reference of the layer uses at most half of every cap
# (test_conv_forms_bf16_cpu.py::test_the_storage_reference_stays_inside_the_caps) and the float32 oracle keeps float64's
# signs.  Found by a search over the inputs and the float64 references alone - no kernel result enters it.
# The layers that run in the bf16 pair form meet a second condition of the same kind: the float64 emulation of the pair form's
# own storage points (pair_storage_errors) uses at most PAIR_STORE_ROOM of the caps of y and dW0.
_SEEDS = {
    ('reg', 404, 32, 0, 0, 32, 1, 1, 'dx'): 13,
    ('reg', 404, 64, 0, 0, 32, 1, 1, 'dx'): 1,
    ('reg', 404, 32, 0, 0, 64, 1, 1, 'dx'): 14,
    ('reg', 404, 64, 0, 0, 64, 1, 1, 'dx'): 11,
    ('reg', 404, 128, 0, 0, 64, 1, 1, 'dx'): 4,
    ('reg', 404, 64, 0, 0, 128, 1, 1, 'dx'): 55,
    ('reg', 404, 128, 0, 0, 128, 1, 1, 'dx'): 1,
    ('reg', 404, 32, 32, 0, 32, 1, 1, 'dx'): 2,
    ('reg', 404, 64, 64, 0, 64, 1, 1, 'dx'): 49,
    ('reg', 404, 64, 0, 2, 32, 1, 1, 'dx'): 12,
    ('reg', 404, 128, 0, 2, 64, 1, 1, 'dx'): 4,
    ('long', 404, 32, 0, 0, 32, 1, 1, 'dx'): 24,
    ('long', 404, 128, 0, 0, 64, 1, 1, 'dx'): 4,
    ('long', 404, 64, 0, 0, 128, 1, 1, 'dx'): 8,
    ('reg+tail', 404, 32, 0, 0, 32, 1, 0, 'dx'): 13,
    ('reg+tail', 404, 128, 0, 0, 64, 1, 0, 'dx'): 4,
    ('reg', 404, 32, 0, 0, 32, 0, 1, 'dx'): 23,
    ('reg', 404, 64, 0, 0, 128, 0, 1, 'dx'): 55,
    ('reg', 404, 6, 0, 0, 32, 1, 1, 'nodx'): 9,
    ('reg', 404, 6, 0, 0, 64, 1, 1, 'nodx'): 17,
    ('reg', 37, 32, 0, 0, 32, 1, 1, 'dx'): 5,
    ('reg', 1101, 64, 0, 0, 128, 1, 1, 'dx'): 160,
    ('reg', 1100, 128, 0, 0, 64, 1, 1, 'dx'): 4,
    ('reg', 404, 32, 0, 0, 32, 1, 1, 'acc0'): 24,
    ('reg', 404, 32, 32, 0, 32, 1, 1, 'acc1'): 1,
    ('reg', 404, 64, 0, 2, 32, 1, 1, 'acc0'): 2,
    # (mode pool: dy + the pooled share is no bf16 value, so every s of a group's maximum rounds - the storage reference of dW0
    #  sits at 1.4e-3 .. 2.6e-3 against 0.8e-3 without pooling, and few seeds stay below half the cap of 3e-3)
    ('reg+tie', 404, 32, 0, 0, 32, 1, 1, 'pool'): 289,
    ('reg+tie', 404, 128, 0, 0, 64, 1, 1, 'pool'): 587,
    ('reg+tie', 404, 64, 0, 0, 128, 1, 1, 'pool'): 3633,
    ('reg', 404, 6, 0, 0, 32, 1, 1, 'nodx+pool'): 9,
    ('reg', 404, 32, 0, 2, 64, 1, 1, 'dx'): 29,
    ('reg', 404, 128, 0, 2, 32, 1, 1, 'dx'): 12,
    ('long', 404, 64, 0, 2, 32, 1, 1, 'dx'): 4,
    ('long', 404, 128, 0, 2, 64, 1, 1, 'dx'): 17,
    ('long', 404, 32, 0, 2, 64, 1, 1, 'dx'): 53,
    ('long', 404, 128, 0, 2, 32, 1, 1, 'dx'): 12,
    ('reg+tail', 404, 64, 0, 2, 32, 1, 0, 'dx'): 10,
    ('reg', 148, 128, 0, 2, 64, 1, 1, 'dx'): 41,
    ('reg', 100, 64, 0, 2, 32, 0, 1, 'dx'): 1,
    ('reg', 1100, 64, 0, 2, 32, 1, 1, 'acc0'): 3,
    ('hub', 404, 64, 0, 2, 32, 1, 1, 'dx'): 2,
}


def _case(name, graph, n, cin, cout, storage="bf16", pairs=False, shift=0, act=1, bias_mask=1, mode="dx", options=None, off=None,
          expect=None, seed=None, r_ld=0, refused=None):
    c0, c1 = cin if isinstance(cin, tuple) else (cin, 0)
    if mode == "pool" and "tie" not in graph:
        graph += "+tie"
    if seed is None:
        seed = _SEEDS.get((graph, n, c0, c1, shift, cout, act, bias_mask, mode), 0)
    assert not any(c["name"] == name for c in CASES), name
    assert storage in ("bf16", "fp32") and r_ld in (0, "pad")
    assert not pairs or (shift == 2 and c1 == 0 and n % 4 == 0)
    CASES.append(dict(name=name, graph=graph, n=n, c0=c0, c1=c1, shift=shift, cout=cout, act=act, bias_mask=bias_mask, mode=mode,
                      options=dict(options or {}), off=dict(off or {}), expect=dict(expect or {}), seed=seed, storage=storage,
                      pairs=bool(pairs), r_ld=r_ld, refused=refused))


def _w(cin, cout):
    return "%s_%d" % ("+".join(map(str, cin)) if isinstance(cin, tuple) else cin, cout)


# ---- bf16 storage, fine form, default options ----------------------------------------------------------------------------
FWD16 = dict(fwd="w8", fwd_slots="16", fwd_bfm="1", fwd_nt="16", proj="bf16")
FWD32 = dict(fwd="w8", fwd_slots="16", fwd_bfm="1", fwd_nt="32", proj="bf16")
K1H = dict(ds="fused", k1="bf16", k1_long="0", k1_half="1", k1_nodes="16")
K2M = dict(k2="w8", k2_slots="16", k2_bfm="1", k2_nt="32")
FINE = dict(FWD16, **K1H, **K2M)
_case("bf_plain_32_32", "reg", 404, 32, 32, expect=dict(FINE, k3="bf16_2"))
_case("bf_plain_64_32", "reg", 404, 64, 32, expect=dict(FINE, k3="bf16_4"))
_case("bf_plain_32_64", "reg", 404, 32, 64, expect=dict(FINE, k3="bf16_2"))
_case("bf_plain_64_64", "reg", 404, 64, 64, expect=dict(FINE, k3="bf16_4"))
_case("bf_plain_128_64", "reg", 404, 128, 64, expect=dict(FINE, k3="bf16_4"))
_case("bf_plain_64_128", "reg", 404, 64, 128, expect=dict(FWD32, **K1H, **K2M, k1_okg="8", k3="bf16_4"))
_case("bf_plain_128_128", "reg", 404, 128, 128, expect=dict(FWD32, **K1H, **K2M, k1_okg="8", k3="bf16_4"))
# concatenated sources; 4x-upsampled source without a pair graph
_case("bf_concat_32+32_32", "reg", 404, (32, 32), 32, expect=dict(FINE, k3="bf16_4"))
_case("bf_concat_64+64_64", "reg", 404, (64, 64), 64, expect=dict(FINE, k3="bf16_4"))
_case("bf_up_64_32", "reg", 404, 64, 32, shift=2, expect=dict(FINE, k3="bf16_4"))
_case("bf_up_128_64", "reg", 404, 128, 64, shift=2, expect=dict(FINE, k3="bf16_4"))
# degrees 17..23: 24 edge slots, the vector form of both eight-wave kernels, the long d-logits kernel
LONG = dict(fwd="w8", fwd_slots="24", fwd_bfm="0", fwd_nt="32", k1="bf16", k1_long="1", k1_half="0", k1_nodes="32", k2="w8",
            k2_slots="24", k2_bfm="0", k2_nt="32")
_case("bf_long_32_32", "long", 404, 32, 32, expect=dict(LONG, ds="fused", k3="bf16_2"))
_case("bf_long_64_64", "long", 404, 64, 64, expect=dict(LONG, ds="fused", k3="bf16_4"))
_case("bf_long_128_64", "long", 404, 128, 64, expect=dict(LONG, ds="fused", k3="bf16_4"))
_case("bf_long_64_128", "long", 404, 64, 128, expect=dict(LONG, ds="fused", k3="bf16_4"))
# fake nodes of degree 0 behind the real ones, no bias mask
_case("bf_tail_32_32_nomask", "reg+tail", 404, 32, 32, bias_mask=0, expect=dict(FINE))
_case("bf_tail_128_64_nomask", "reg+tail", 404, 128, 64, bias_mask=0, expect=dict(FINE))
# no activation (32 -> 32 with a padded stride of r)
_case("bf_noact_32_32_rpad", "reg", 404, 32, 32, act=0, r_ld="pad", expect=dict(FINE))
_case("bf_noact_64_128", "reg", 404, 64, 128, act=0, expect=dict(FWD32, **K1H, k1_okg="8"))
# narrow first layer: fp32 x0 and ds, bf16 y / y_pool / dy.  With an input gradient fgc_conv_forms names the general bf16 kernels
# (stream2_bf among them), but fgc_conv_bwd refuses the call: the bf16 d-logits kernel needs 32-channel passes
NARROW = dict(fwd="narrow", proj="narrow", k1="narrow", k2="none", k3="narrow")
NARROW_DX = dict(fwd="narrow", ds="vec", k1="bf16", k1_half="0", k2="w8", k2_bfm="0", k3="stream2_bf")
_case("bf_narrow_6_32_nodx", "reg", 404, 6, 32, mode="nodx", expect=dict(NARROW, ds="narrow-fused"))
_case("bf_narrow_6_64_nodx", "reg", 404, 6, 64, mode="nodx", expect=dict(NARROW))
_case("bf_narrow_6_32_dx", "reg", 404, 6, 32, expect=dict(NARROW_DX), refused="fgc_conv_bwd")
_case("bf_narrow_6_64_dx", "reg", 404, 6, 64, expect=dict(NARROW_DX), refused="fgc_conv_bwd")
# node counts: 37 / 100 (no full tile, one slab), 16 (one half tile), 1101 (five slabs of 224 rows, the last ragged: 205), 1100 (5 x 220)
_case("bf_n37_32_32", "reg", 37, 32, 32, expect=dict(FINE, k3_slabs="1"))
_case("bf_n100_64_64", "reg", 100, 64, 64, expect=dict(FINE, k3_slabs="1"))
_case("bf_n16_32_64", "reg", 16, 32, 64, expect=dict(FINE, k3_slabs="1"))
_case("bf_n1101_64_128", "reg", 1101, 64, 128, expect=dict(FWD32, k3="bf16_4", k3_slabs="5", k3_rows="224"))
_case("bf_n1100_128_64", "reg", 1100, 128, 64, expect=dict(FWD16, k3="bf16_4", k3_slabs="5", k3_rows="220"))
# call modes (64 -> 64 without dx: a padded stride of r)
_case("bf_nodx_64_64_rpad", "reg", 404, 64, 64, mode="nodx", r_ld="pad", expect=dict(FINE))
_case("bf_acc0_32_32", "reg", 404, 32, 32, mode="acc0", expect=dict(K2M))
_case("bf_acc1_concat_32+32_32", "reg", 404, (32, 32), 32, mode="acc1", expect=dict(K2M))
_case("bf_acc01_concat_64+64_64", "reg", 404, (64, 64), 64, mode="acc01", expect=dict(K2M))
_case("bf_acc0_up_64_32", "reg", 404, 64, 32, shift=2, mode="acc0", expect=dict(K2M))
_case("bf_pool_32_32", "reg", 404, 32, 32, mode="pool", expect=dict(FINE))
_case("bf_pool_128_64", "reg", 404, 128, 64, mode="pool", expect=dict(FINE))
_case("bf_pool_64_128", "reg", 404, 64, 128, mode="pool", expect=dict(FWD32, **K1H, k1_okg="8"))
_case("bf_pool_6_32_nodx", "reg", 404, 6, 32, mode="nodx+pool", expect=dict(NARROW, ds="narrow-fused"))

# ---- pair form of the up-convolutions, default options: every layer in fp32 and in bf16 -----------------------------------
# (the d-logits kernel of the pair form takes 32 blocks = 128 nodes per workgroup at 32 outputs, 16 blocks = 64 nodes at 64)
PAIR = dict(fwd="pair", proj="pair", ds="pair", k1="pair", k1_long="0", k2="w8", k2_slots="16")
PAIR_LONG = dict(fwd="pair", proj="pair", ds="pair", k1="pair", k1_long="1", k2="w8", k2_slots="24", k2_bfm="0")


def _pair_case(name, graph, n, cin, cout, expect=None, slabs=None, **kw):
    for storage, tag in (("fp32", "f32"), ("bf16", "bf")):
        e = dict(expect if expect is not None else PAIR, k1_nodes="128" if cout == 32 else "64")
        if storage == "fp32":
            e.update(k2_bfm="0", k3="stream2" if cin == 32 else "stream4")
        else:
            e.update(k2_bfm=e.get("k2_bfm", "1"), k3="bf16_2" if cin == 32 else "bf16_4")
        if slabs:
            e.update(k3_slabs=slabs[storage][0], k3_rows=slabs[storage][1])
        _case("pair_%s_%s" % (tag, name), graph, n, cin, cout, storage=storage, pairs=True, shift=2, expect=e, **kw)


for cin, cout in ((64, 32), (128, 64), (32, 64), (128, 32)):
    _pair_case(_w(cin, cout), "reg", 404, cin, cout)
for cin, cout in ((64, 32), (128, 64), (32, 64), (128, 32)):
    _pair_case("long_" + _w(cin, cout), "long", 404, cin, cout, expect=PAIR_LONG)
_pair_case("tail_64_32_nomask", "reg+tail", 404, 64, 32, bias_mask=0)       # fake rows, no bias mask
_pair_case("n100_64_32_noact", "reg", 100, 64, 32, act=0)                   # blocks that do not fill the last workgroup
_pair_case("n148_128_64_rpad", "reg", 148, 128, 64, r_ld="pad")
# 275 coarse rows: three slabs of 92 (fp32) and two of 140 (bf16), the last ragged; accumulating into a pre-filled dx0
_pair_case("n1100_acc0_64_32", "reg", 1100, 64, 32, mode="acc0", slabs=dict(fp32=("3", "92"), bf16=("2", "140")))
# a coarse row with more than 24 in-pairs: not a pair-form layer (fgc_conv_uses_pairs == 0), the fine form runs.  fp32 only
_case("pair_f32_hub_64_32", "hub", 404, 64, 32, storage="fp32", pairs=True, shift=2,
      expect=dict(fwd="w8", k1="deep", k2="tiled", k2_chunks="3", k3="stream4"))

# ---- refusals: argument checks that return FGC_EINVAL before any launch -------------------------------------------------------
_case("bf_refused_hub_32_32", "hub", 404, 32, 32, expect=dict(k2_slots="24", k2_chunks="3"), refused="fgc_conv_bwd")
_case("bf_refused_32_96", "reg", 404, 32, 96, expect=dict(fwd="w8"), refused="fgc_conv_fwd")
_case("bf_refused_x0p8_32_32", "reg", 404, 32, 32, off=dict(x0=8), expect=dict(fwd="w8"), refused="fgc_conv_fwd")
_case("bf_refused_concat_48+16_32", "reg", 404, (48, 16), 32, expect=dict(fwd="w8"), refused="fgc_conv_fwd")

# ---- one option flipped (per-descriptor overrides) ---------------------------------------------------------------------------
N_DEFAULT = len(CASES)
for cin, cout in ((32, 32), (128, 64), (64, 128)):
    w = _w(cin, cout)
    k3s = "stream2_bf" if cin == 32 else "stream4_bf"
    _case("bf_NO_BFM_" + w, "reg", 404, cin, cout, options=dict(NO_BFM=1), expect=dict(fwd="w8", fwd_bfm="0", k2="w8", k2_bfm="0"))
    if cout != 64:           # (the data-gradient kernel of a layer with 128 inputs has no half tiles)
        _case("bf_W8_NT16=2_" + w, "reg", 404, cin, cout, options=dict(W8_NT16=2), expect=dict(k2="w8", k2_bfm="1", k2_nt="16"))
        _case("bf_NO_BFM_W8_NT16=2_" + w, "reg", 404, cin, cout, options=dict(NO_BFM=1, W8_NT16=2),
              expect=dict(fwd_bfm="0", k2="w8", k2_bfm="0", k2_nt="16"))
    if cout != 128:
        _case("bf_W8_NT16=0_" + w, "reg", 404, cin, cout, options=dict(W8_NT16=0), expect=dict(fwd="w8", fwd_bfm="1", fwd_nt="32"))
    _case("bf_K1_NT16=0_" + w, "reg", 404, cin, cout, options=dict(K1_NT16=0), expect=dict(k1="bf16", k1_long="0", k1_half="0", k1_nodes="32"))
    _case("bf_NO_FUSED_DS_BF16_" + w, "reg", 404, cin, cout, options=dict(NO_FUSED_DS_BF16=1), expect=dict(ds="vec", k1="bf16", k1_half="1"))
    _case("bf_NO_TNBF16_" + w, "reg", 404, cin, cout, options=dict(NO_TNBF16=1), expect=dict(k3=k3s, k3_slabs="4", k3_rows="104"))
_case("bf_NO_TNBF16_n1101_64_128", "reg", 1101, 64, 128, options=dict(NO_TNBF16=1), expect=dict(k3="stream4_bf"))
_case("bf_TNB_WGS=4_n1101_64_128", "reg", 1101, 64, 128, options=dict(TNB_WGS=4), expect=dict(k3="bf16_4", k3_slabs="1"))
_case("bf_TNB_WGS=12_n1101_64_128", "reg", 1101, 64, 128, options=dict(TNB_WGS=12), expect=dict(k3="bf16_4", k3_slabs="3", k3_rows="368"))
_case("bf_NO_BFM_pool_32_32", "reg", 404, 32, 32, mode="pool", options=dict(NO_BFM=1), expect=dict(fwd_bfm="0", k2_bfm="0", ds="fused"))
_case("bf_NO_BFM_acc0_32_32", "reg", 404, 32, 32, mode="acc0", options=dict(NO_BFM=1), expect=dict(fwd_bfm="0", k2_bfm="0"))
# pair form: the vector form of the bf16 data kernel; the fine form of the same layer
_case("pair_bf_NO_BFM_64_32", "reg", 404, 64, 32, pairs=True, shift=2, options=dict(NO_BFM=1), expect=dict(PAIR, k2_bfm="0", k3="bf16_4"))
# ... and its half tiles (by default only from 81 920 rows): the EROW instances of conv_bfm_kernel<DATA, 16> and of
# conv_w8_kernel<DATA, FAST, 16, BF, 16> in bf16, of the latter in fp32
_case("pair_bf_W8_NT16=2_64_32", "reg", 404, 64, 32, pairs=True, shift=2, options=dict(W8_NT16=2),
      expect=dict(PAIR, k2_bfm="1", k2_nt="16", k3="bf16_4"))
_case("pair_bf_NO_BFM_W8_NT16=2_64_32", "reg", 404, 64, 32, pairs=True, shift=2, options=dict(NO_BFM=1, W8_NT16=2),
      expect=dict(PAIR, k2_bfm="0", k2_nt="16", k3="bf16_4"))
_case("pair_f32_W8_NT16=2_64_32", "reg", 404, 64, 32, storage="fp32", pairs=True, shift=2, options=dict(W8_NT16=2),
      expect=dict(PAIR, k2_bfm="0", k2_nt="16", k3="stream4"))
_case("pair_f32_NO_PAIRS_64_32", "reg", 404, 64, 32, storage="fp32", pairs=True, shift=2, options=dict(NO_PAIRS=1),
      expect=dict(fwd="w8", k1="deep", ds="fused", k3="stream4"))
_case("pair_bf_NO_PAIRS_64_32", "reg", 404, 64, 32, pairs=True, shift=2, options=dict(NO_PAIRS=1),
      expect=dict(fwd="w8", fwd_bfm="1", k1="bf16", ds="fused", k2_bfm="1", k3="bf16_4"))

NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
RUN_NAMES = [c["name"] for c in CASES if not c["refused"]]
REFUSED_NAMES = [c["name"] for c in CASES if c["refused"]]


def default_sibling(case):
    """The case with the same layer, storage, inputs and pointers on default options (None if the table has none)."""
    if not case["options"]:
        return None
    keys = ("graph", "n", "c0", "c1", "shift", "cout", "act", "bias_mask", "mode", "seed", "off", "storage", "pairs", "r_ld")
    return next((c for c in CASES if not c["options"] and all(c[k] == case[k] for k in keys)), None)


def uses_pairs(case):
    """What fgc_conv_uses_pairs must answer for the case."""
    return int(case["pairs"] and "hub" not in case["graph"] and not case["options"].get("NO_PAIRS"))


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _numeric_key(case):
    return tuple(case[k] for k in ("graph", "n", "c0", "c1", "shift", "cout", "act", "bias_mask", "mode", "seed"))


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


_INPUTS = {}


def inputs(case):
    """CPU float32 tensors holding bf16 values: x0, x1 (or None), dy, params [W0 (bf16 values), b, u, c, v], pool_dy (mode
    pool), dx0_fill / dx1_fill (accumulate modes).  A function of the numeric fields alone: the storages, the two forms of an
    up-convolution and every option variant share them."""
    from oracle import model_ref as R
    key = _numeric_key(case)
    if key in _INPUTS:
        return _INPUTS[key]
    n, c0, c1, cout, mode = case["n"], case["c0"], case["c1"], case["cout"], case["mode"]
    rows = n >> case["shift"]
    rs = np.random.RandomState(177 + case["seed"])
    t = lambda *shape: bf16_round(torch.tensor(rs.normal(size=shape).astype(np.float32)))
    params = R.conv_params(c0 + c1, cout, 21 + case["seed"])
    params[0] = bf16_round(params[0])
    d = dict(x0=t(rows, c0), x1=t(rows, c1) if c1 else None, dy=t(n, cout), params=params)
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


def degrees(case):
    return torch.tensor((klist(case["graph"], case["n"]) != 0).sum(1))


# ---------------------------------------------------------------------------------------------
# the oracle and the storage reference
# ---------------------------------------------------------------------------------------------
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


def output_gradient(case, y, dtype):
    """d loss / d pre-activation of loss = sum(y dy) + sum(pool(y) pool_dy), with the kinks resolved by a STORED y as the
    backward kernels resolve them: lrelu' = where(y > 0, 1, alpha), and the pooled gradient goes to the rows of a group of four
    that equal its maximum, in equal shares (tf.reduce_max; include/fgc.h, fgc_conv_bwd_io.pool_dy)."""
    d = inputs(case)
    y = y.to(dtype)
    g = d["dy"].to(dtype)
    if "pool" in case["mode"]:
        y4 = y.reshape(-1, 4, y.shape[1])
        hit = (y4 == y4.amax(1, keepdim=True)).to(dtype)
        g = g + (hit / hit.sum(1, keepdim=True) * d["pool_dy"].to(dtype)[:, None]).reshape(y.shape)
    return g * slopes_of(y) if case["act"] else g


def _backward(case, dtype, gpre):
    """Gradients for a given d loss / d pre-activation, by autograd through the oracle in `dtype`: dict dx0, dx1, dW0, db, du,
    dc, dv (without the pre-fill of the accumulate modes)."""
    from oracle import model_ref as R
    d = inputs(case)
    # (copies: .to() of a tensor that already has the type returns the cached input itself)
    xs = [x.detach().to(dtype).clone().requires_grad_(True) for x in (d["x0"], d["x1"]) if x is not None]
    ps = [p.detach().to(dtype).clone().requires_grad_(True) for p in d["params"]]
    xin = torch.cat(xs, 1)[None]
    if case["shift"]:
        xin = R.custom_upsampling(xin, 2)
    adj = torch.tensor(klist(case["graph"], case["n"])[None])
    pre = R.custom_conv2d(xin, adj, ps, biasMask=bool(case["bias_mask"]))
    pre[0].backward(gpre.detach().to(dtype))
    out = dict(zip(["dW0", "db", "du", "dc", "dv"], [p.grad for p in ps]))
    out["dx0"] = xs[0].grad
    if len(xs) > 1:
        out["dx1"] = xs[1].grad
    return out


def _with_fill(case, grads, dtype, rounded):
    d = inputs(case)
    out = dict(grads)
    for k in ("dx0", "dx1"):
        if k in out:
            if k + "_fill" in d:
                out[k] = out[k] + d[k + "_fill"].to(dtype)
            if rounded:
                out[k] = bf16_round(out[k])
    return out


_GRADS = {}


def oracle_grads(case, dtype, y):
    """The oracle's gradients in `dtype` with the kinks resolved by the stored output `y` (the accumulate modes add the
    pre-fill).  Cached per (inputs, dtype, y)."""
    key = (_numeric_key(case), dtype, y.to(torch.float32).numpy().tobytes())
    if key not in _GRADS:
        _GRADS[key] = _with_fill(case, _backward(case, dtype, output_gradient(case, y, dtype)), dtype, False)
    return _GRADS[key]


_STORE = {}


def storage_reference(case):
    """What a layer that computes in float64 and STORES as bf16 gives: bf16 rounding at the storage points include/fgc.h names
    and autograd can reach, nowhere else -
      y      bf16(lrelu(pre64));  y_pool = max of the rounded y
      s      bf16(dloss/dpre / deg): the oracle is given the effective output gradient bf16(s) deg (rows of degree 0: as is)
      dx0/1  bf16(pre-fill + gradient)
    Not emulated: r, hc and dt of the pair form, and db, which the kernels sum in fp32 from unrounded terms (db is taken from
    the unrounded run).  Returns (y, y_pool or None, grads, ref64) with ref64 = oracle_grads(case, float64, y): the kinks of
    both are resolved by this y, so that e_store measures the roundings alone."""
    from oracle import model_ref as R
    key = _numeric_key(case)
    if key in _STORE:
        return _STORE[key]
    f64 = torch.float64
    pre = preactivation(case, f64)
    y = bf16_round(R.lrelu(pre, ALPHA) if case["act"] else pre)
    y_pool = y.reshape(-1, 4, y.shape[1]).amax(1) if "pool" in case["mode"] else None
    g = output_gradient(case, y, f64)
    deg = degrees(case).to(f64)[:, None]
    s = bf16_round(g / deg.clamp(min=1))
    g_eff = torch.where(deg > 0, s * deg, g)
    grads = _backward(case, f64, g_eff)
    ref = oracle_grads(case, f64, y)
    grads["db"] = ref["db"]
    _STORE[key] = (y, y_pool, _with_fill(case, grads, f64, True), ref)
    return _STORE[key]


def rel_err(got, ref):
    """e = max|got - ref| / max|ref| (the absolute error where the reference is all zero), and the scale."""
    ref = ref.double()
    scale = ref.abs().max().item()
    err = (got.double().reshape(ref.shape) - ref).abs().max().item()
    return (err / scale if scale > 0 else err), scale


def e_store(case):
    """{tensor: e of the storage reference against float64} - the yardstick of bound (b), never measured on the kernels."""
    from oracle import model_ref as R
    y, y_pool, grads, ref = storage_reference(case)
    pre = preactivation(case, torch.float64)
    y64 = R.lrelu(pre, ALPHA) if case["act"] else pre
    out = {"y": rel_err(y, y64)[0]}
    if y_pool is not None:
        out["y_pool"] = rel_err(y_pool, y64.reshape(-1, 4, y64.shape[1]).amax(1))[0]
    for k in GRAD_NAMES:
        if k in grads and not ("nodx" in case["mode"] and k.startswith("dx")):
            out[k] = rel_err(grads[k], ref[k])[0]
    return out


PAIR_STORE_ROOM = 0.9       # share of a cap the pair form's own storage roundings may use (pair_storage_errors)
_PAIR_STORE = {}


def pair_storage_errors(case):
    """{y, dW0: e against float64} of a float64 computation that rounds to bf16 exactly where the bf16 PAIR form stores
    (include/fgc.h): hc = W0 x_P per coarse row and y in the forward; dt_pP = sum over the children of block p of mult_iP s_i per
    pair and r_P = sum_p q_pP dt_pP per coarse row in the backward (dW0 = sum_P r_P x_P).  storage_reference leaves hc, dt and r
    out (it is the yardstick of bound (b) for both forms); this one says how much of cap (a) the pair form's declared storage
    uses up before any kernel computes anything: rounding ONE sum over a block's children costs up to twice what rounding the
    children's terms one by one and adding them in fp32 costs, so the pair form's dW0 sits 1.3 .. 2 times above the fine
    form's at the same inputs.  CPU only."""
    from oracle import model_ref as R
    key = _numeric_key(case)
    if key in _PAIR_STORE:
        return _PAIR_STORE[key]
    assert case["shift"] == 2 and not case["c1"]
    f64 = torch.float64
    d = inputs(case)
    adj = klist(case["graph"], case["n"])
    n, nc, cout = case["n"], case["n"] // 4, case["cout"]
    W0, b, u, c, v = [p.to(f64) for p in d["params"]]
    M = W0.shape[0]
    xc = d["x0"].to(f64)
    q = R.get_weight_assignments(R.custom_upsampling(xc[None], 2), torch.tensor(adj[None]), u, v, c)[0]      # [n, K, M]
    I, Kk = np.nonzero(adj)
    J = adj[I, Kk] - 1
    It, Pt = torch.tensor(I).long(), torch.tensor(J >> 2).long()
    q_e = q[It, torch.tensor(Kk)]                                                   # [E, M]
    deg = degrees(case).to(f64)[:, None]
    # forward: y_i = (1 / deg_i) sum_e q_e . hc_P(e) + b
    hc = bf16_round(xc @ W0.reshape(M * cout, -1).t()).reshape(nc, M, cout)
    pre = torch.zeros(n, cout, dtype=f64).index_add_(0, It, (q_e[:, :, None] * hc[Pt]).sum(1)) / deg.clamp(min=1)
    pre = pre + (b if not case["bias_mask"] else torch.where(deg > 0, b[None, :], torch.zeros_like(pre)))
    pre64 = preactivation(case, f64)
    y64 = R.lrelu(pre64, ALPHA) if case["act"] else pre64
    y = bf16_round(R.lrelu(pre, ALPHA) if case["act"] else pre)
    # backward: the kinks resolved by the storage reference's y, as in e_store
    ys, _, _, ref = storage_reference(case)
    s = output_gradient(case, ys, f64) / deg.clamp(min=1)
    _, inv = np.unique((I >> 2).astype(np.int64) * nc + (J >> 2), return_inverse=True)
    inv = torch.tensor(inv)
    npairs = int(inv.max()) + 1
    dt = bf16_round(torch.zeros(npairs, cout, dtype=f64).index_add_(0, inv, s[It]))
    q_p = torch.zeros(npairs, M, dtype=f64)
    q_p[inv] = q_e                                                                   # (the same for every edge of a pair)
    P_p = torch.zeros(npairs, dtype=torch.long)
    P_p[inv] = Pt
    r = bf16_round(torch.zeros(nc, M, cout, dtype=f64).index_add_(0, P_p, q_p[:, :, None] * dt[:, None, :]))
    dW0 = torch.einsum("pmo,pc->moc", r, xc)
    _PAIR_STORE[key] = {"y": rel_err(y, y64)[0], "dW0": rel_err(dW0, ref["dW0"])[0]}
    return _PAIR_STORE[key]
