"""Shared by tests/test_mlp_forms_cpu.py and tests/test_gpu_mlp_forms.py: one table of calls of the per-facet MLP head
cin -> hidden -> cout, each built to make the library take a particular form of its kernels (fgc_mlp_forms, include/fgc.h), with
the inputs and the float64 / float32 reference (plain torch through autograd, relu(h) - alpha relu(-h)) of every case.

A case is a dict:
  name, n, cin, hidden, cout, alpha, dtype ("f32" | "bf16": the storage type of x / dx), seed
  options  process-level library options (_lib.options) in force for the whole case; the MLP has no per-call overrides
  off      byte offsets from 16-byte alignment of x / dx / b1 / ws (ws: both workspaces)
  packed   the operands are also packed ahead by fgc_conv_pack and handed over with FGC_MLP_PACKED | FGC_MLP_LAYOUT(id): the
           bits of the self-packed call
  inputs   "plain" | "zeros" (8 all-zero rows of x, 16 entries of b1 exactly +-0.0: 128 pre-activations exactly zero in every
           form and precision) | "scaled" (row i of x times 2^((i % 25) - 12))
  expect   the fgc_mlp_forms keys the case exists to reach; fwd / bwd = "none": the entry point refuses the call (-22)
Rows: 1, 33 (a second 32-row backward tile of one row; four walkers of which two stay idle in the split and bf16 forms), 65 (a
second 64-row forward tile of one row), 4097 (129 backward tiles: the first size at which a walker - 128 at most in every form -
takes a second tile, of one row).  Seeds: 0 unless a case of up to 65 rows had a pre-activation within 1e-6 of zero with it
(tests/test_mlp_forms_cpu.py holds every seed to that).  Default-option cases come first."""
import numpy as np
import torch

CASES = []
ZERO_ROWS = (0, 15, 16, 31, 32, 47, 63, 64)
ZERO_COLS = (0, 15, 16, 17, 31, 63, 64, 100, 127, 128, 129, 191, 192, 200, 254, 255)     # odd positions of the list: -0.0


def _case(name, n, cin, hidden, cout, alpha=0.1, dtype="f32", options=None, off=None, packed=False, seed=0, inputs="plain", expect=None):
    assert not any(c["name"] == name for c in CASES), name
    assert n in (1, 33, 65, 4097) and alpha in (0.0, 0.1, 1.0) and expect
    CASES.append(dict(name=name, n=n, cin=cin, hidden=hidden, cout=cout, alpha=alpha, dtype=dtype, options=dict(options or {}),
                      off=dict(off or {}), packed=packed, seed=seed, inputs=inputs, expect={k: str(v) for k, v in expect.items()}))


def F32F(ks, co, **kw):
    return dict(fwd="f32", fwd_ks=ks, fwd_co=co, **kw)


def F32B(mt, co, **kw):
    return dict(bwd="f32", bwd_mt=mt, bwd_ctw=8 // mt, bwd_co=co, bwd_dx_gx=0, **kw)


def SPLF(ks, co, **kw):
    return dict(fwd="split", fwd_ks=ks, fwd_co=co, **kw)


def BF16F(ks, co, **kw):
    return dict(fwd="bf16", fwd_ks=ks, fwd_co=co, **kw)


SPLB = dict(bwd="split", bwd_mt=2, bwd_co=3, bwd_dx_slabs=0)
NOB = dict(bwd="none")


def BF16B(mt, **kw):
    return dict(bwd="bf16", bwd_mt=mt, bwd_co=3, bwd_dx_slabs=0, **kw)


# ---- default options ---------------------------------------------------------------------------------------------------------
# fp32-MFMA forward alone: hidden = 64 / 192 (one and three column tiles per wave; the backward wants a multiple of 256)
_case("f32_1_64_3_n65", 65, 1, 64, 3, expect=dict(F32F(1, 3, fwd_kpad=16, fwd_gx=2), **NOB))
_case("f32_5_64_1_n65", 65, 5, 64, 1, alpha=0.0, expect=dict(F32F(1, 3), **NOB))
_case("f32_16_192_4_n65", 65, 16, 192, 4, expect=dict(F32F(1, 4), **NOB))
_case("f32_17_192_2_n33", 33, 17, 192, 2, alpha=1.0, expect=dict(F32F(2, 3, fwd_kpad=32, fwd_gx=1), **NOB))
_case("f32_32_64_4_n65", 65, 32, 64, 4, expect=dict(F32F(2, 4), fwd_shape="f32", **NOB))
_case("f32_33_192_4_n65", 65, 33, 192, 4, alpha=0.0, expect=dict(F32F(0, 4, fwd_kpad=48), **NOB))
_case("f32_48_64_3_n33", 33, 48, 64, 3, expect=dict(F32F(0, 3), **NOB))
_case("f32_64_192_3_n65", 65, 64, 192, 3, expect=dict(F32F(0, 3, fwd_kpad=64), fwd_shape="f32", **NOB))
_case("f32_100_192_1_n65", 65, 100, 192, 1, alpha=1.0, expect=dict(F32F(0, 3, fwd_kpad=112), **NOB))
_case("f32_128_64_4_n1", 1, 128, 64, 4, expect=dict(F32F(0, 4, fwd_kpad=128, fwd_gx=1), **NOB))
# fp32 MFMA both ways: hidden = 256, 512, 768 (gy = hidden / (64 ctw))
_case("f32_1_256_3_n33", 33, 1, 256, 3, expect=dict(F32F(1, 3), **F32B(2, 3, bwd_slabs=2, bwd_gx=2, bwd_gy=1, bwd_dx_slabs=1)))
_case("f32_5_256_1_n33", 33, 5, 256, 1, alpha=1.0, expect=dict(F32F(1, 3), **F32B(2, 3)))
_case("f32_16_768_2_n65", 65, 16, 768, 2, expect=dict(F32F(1, 3), **F32B(2, 3, bwd_slabs=3, bwd_gy=3, bwd_dx_slabs=3)))
_case("f32_17_512_4_n65", 65, 17, 512, 4, alpha=0.0, expect=dict(F32F(2, 4), **F32B(2, 4, bwd_gy=2)))
_case("f32_17_256_3_n1", 1, 17, 256, 3, expect=dict(F32F(2, 3), **F32B(2, 3, bwd_slabs=1)))
_case("f32_33_256_2_n65", 65, 33, 256, 2, expect=dict(F32F(0, 3), **F32B(4, 3, bwd_gy=2)))
_case("f32_48_256_4_n33", 33, 48, 256, 4, expect=dict(F32F(0, 4), **F32B(4, 4, bwd_gy=2)))
_case("f32_48_768_1_n65", 65, 48, 768, 1, alpha=0.0, expect=dict(F32F(0, 3), **F32B(4, 3, bwd_gy=6, bwd_dx_slabs=6)))
_case("f32_100_256_3_n33", 33, 100, 256, 3, expect=dict(F32F(0, 3), **F32B(8, 3, bwd_gy=4)))
_case("f32_100_512_1_n65", 65, 100, 512, 1, alpha=1.0, expect=dict(F32F(0, 3), **F32B(8, 3, bwd_gy=8)))
_case("f32_128_256_4_n33", 33, 128, 256, 4, alpha=0.0, expect=dict(F32F(0, 4), **F32B(8, 4)))
_case("f32_128_768_2_n1", 1, 128, 768, 2, expect=dict(F32F(0, 3), **F32B(8, 3, bwd_gy=12)))
# split forward (cin = 32, 64), split backward (cin = 32, cout <= 3), fp32-MFMA backward for the rest
_case("split_32_256_3_n33", 33, 32, 256, 3, expect=dict(SPLF(1, 3), **SPLB, bwd_slabs=4, bwd_gx=4, bwd_gy=1, bwd_dx_gx=1))
_case("split_32_256_1_n33", 33, 32, 256, 1, alpha=0.0, expect=dict(SPLF(1, 3), **SPLB))
_case("split_32_512_2_n65", 65, 32, 512, 2, alpha=1.0, expect=dict(SPLF(1, 3), **SPLB, bwd_gy=2))
_case("split_32_768_3_n65", 65, 32, 768, 3, expect=dict(SPLF(1, 3), **SPLB, bwd_gy=3, bwd_slabs=4))
_case("split_32_256_2_n1", 1, 32, 256, 2, expect=dict(SPLF(1, 3), **SPLB, bwd_slabs=4))
_case("split_32_256_4_n33", 33, 32, 256, 4, expect=dict(SPLF(1, 4), **F32B(2, 4), bwd_shape="f32"))
_case("split_64_256_3_n33", 33, 64, 256, 3, expect=dict(SPLF(2, 3), **F32B(4, 3), bwd_shape="f32"))
_case("split_64_512_4_n65", 65, 64, 512, 4, alpha=0.0, expect=dict(SPLF(2, 4), **F32B(4, 4, bwd_gy=4)))
_case("split_64_768_1_n65", 65, 64, 768, 1, alpha=1.0, expect=dict(SPLF(2, 3), **F32B(4, 3, bwd_gy=6)))
# bf16 storage; the backward has no kernel for cin = 128 or cout = 4
_case("bf16_32_256_3_n33", 33, 32, 256, 3, dtype="bf16", expect=dict(BF16F(1, 3), **BF16B(2, bwd_slabs=4, bwd_gx=1, bwd_gy=4, bwd_dx_gx=1)))
_case("bf16_32_512_1_n65", 65, 32, 512, 1, alpha=0.0, dtype="bf16", expect=dict(BF16F(1, 3), **BF16B(2, bwd_gy=8)))
_case("bf16_32_768_2_n1", 1, 32, 768, 2, dtype="bf16", expect=dict(BF16F(1, 3), **BF16B(2, bwd_gy=12)))
_case("bf16_64_256_2_n33", 33, 64, 256, 2, alpha=1.0, dtype="bf16", expect=dict(BF16F(2, 3), **BF16B(4)))
_case("bf16_64_768_3_n65", 65, 64, 768, 3, dtype="bf16", expect=dict(BF16F(2, 3), **BF16B(4, bwd_gy=12)))
_case("bf16_128_256_3_n33_bwd_refused", 33, 128, 256, 3, dtype="bf16", expect=dict(BF16F(4, 3), **NOB))
_case("bf16_32_256_4_n33_bwd_refused", 33, 32, 256, 4, dtype="bf16", expect=dict(BF16F(1, 4), **NOB))
_case("bf16_64_512_4_n65_bwd_refused", 65, 64, 512, 4, alpha=1.0, dtype="bf16", expect=dict(BF16F(2, 4), **NOB))
_case("bf16_128_512_4_n65_bwd_refused", 65, 128, 512, 4, alpha=0.0, dtype="bf16", expect=dict(BF16F(4, 4), **NOB))
# 4097 rows, no kink (alpha = 1): tiles, walkers, tails and slabs against float64 with nothing excluded
BIG = dict(fwd_gx=65, bwd_slabs=128)
_case("f32_17_256_3_n4097_a1", 4097, 17, 256, 3, alpha=1.0, expect=dict(F32F(2, 3), **F32B(2, 3, bwd_gx=128), **BIG))
_case("f32_48_256_4_n4097_a1", 4097, 48, 256, 4, alpha=1.0, expect=dict(F32F(0, 4), **F32B(4, 4, bwd_gx=128), **BIG))
_case("f32_128_1024_3_n4097_a1", 4097, 128, 1024, 3, alpha=1.0, expect=dict(F32F(0, 3), **F32B(8, 3, bwd_gy=16), **BIG))
_case("split_32_256_3_n4097_a1", 4097, 32, 256, 3, alpha=1.0, expect=dict(SPLF(1, 3), **SPLB, bwd_gx=128, bwd_dx_gx=33, **BIG))
_case("split_32_1024_2_n4097_a1", 4097, 32, 1024, 2, alpha=1.0, expect=dict(SPLF(1, 3), **SPLB, bwd_gy=4, **BIG))
_case("split_64_256_4_n4097_a1", 4097, 64, 256, 4, alpha=1.0, expect=dict(SPLF(2, 4), **F32B(4, 4), **BIG))
_case("bf16_32_256_3_n4097_a1", 4097, 32, 256, 3, alpha=1.0, dtype="bf16", expect=dict(BF16F(1, 3), **BF16B(2, bwd_gx=32, bwd_dx_gx=33), **BIG))
_case("bf16_64_1024_1_n4097_a1", 4097, 64, 1024, 1, alpha=1.0, dtype="bf16", expect=dict(BF16F(2, 3), **BF16B(4, bwd_gy=16), **BIG))
_case("bf16_128_256_4_n4097_a1_bwd_refused", 4097, 128, 256, 4, alpha=1.0, dtype="bf16", expect=dict(BF16F(4, 4), fwd_gx=65, **NOB))
# ... and one per backward form with the kink, through the ambiguity helper (tests/mlp_kink.py)
_case("f32_48_256_3_n4097", 4097, 48, 256, 3, expect=dict(F32F(0, 3), **F32B(4, 3), **BIG))
_case("split_32_1024_3_n4097", 4097, 32, 1024, 3, expect=dict(SPLF(1, 3), **SPLB, **BIG))
_case("bf16_32_256_3_n4097", 4097, 32, 256, 3, dtype="bf16", expect=dict(BF16F(1, 3), **BF16B(2), **BIG))
# alignment (fp32 storage, cin = 32): misaligned rows, dx or b1 take the fp32 MFMA; a misaligned workspace is refused (every
# form reads its packed W1 in 16-byte pieces)
_case("xp4_32_256_3_n33", 33, 32, 256, 3, off=dict(x=4), expect=dict(F32F(2, 3), **F32B(2, 3), fwd_shape="split", bwd_shape="split"))
_case("xp8_32_256_3_n33", 33, 32, 256, 3, off=dict(x=8), expect=dict(F32F(2, 3), **F32B(2, 3), fwd_shape="split", bwd_shape="split"))
_case("dxp4_32_256_3_n33", 33, 32, 256, 3, off=dict(dx=4), expect=dict(SPLF(1, 3), **F32B(2, 3), bwd_shape="split"))
_case("b1p4_32_256_3_n33", 33, 32, 256, 3, off=dict(b1=4), expect=dict(SPLF(1, 3), **F32B(2, 3), bwd_shape="split"))
_case("wsp4_32_256_3_n33_refused", 33, 32, 256, 3, off=dict(ws=4), expect=dict(fwd="none", bwd="none", fwd_shape="split", bwd_shape="split"))
_case("xp4_32_512_2_n65", 65, 32, 512, 2, alpha=1.0, off=dict(x=4), expect=dict(F32F(2, 3), **F32B(2, 3, bwd_gy=2)))
# operands packed ahead by fgc_conv_pack, one per form (fp32 forward at cout = 4)
_case("packed_f32_17_256_4_n33", 33, 17, 256, 4, packed=True, expect=dict(F32F(2, 4), **F32B(2, 4), layout=1))
_case("packed_split_32_256_3_n33", 33, 32, 256, 3, packed=True, expect=dict(SPLF(1, 3), **SPLB, layout=7))
_case("packed_split_64_256_4_n65", 65, 64, 256, 4, packed=True, expect=dict(SPLF(2, 4), **F32B(4, 4), layout=3))
_case("packed_bf16_64_256_3_n33", 33, 64, 256, 3, dtype="bf16", packed=True, seed=1, expect=dict(BF16F(2, 3), **BF16B(4), layout=9))
_case("packed_bf16_128_256_4_n65_bwd_refused", 65, 128, 256, 4, dtype="bf16", packed=True, expect=dict(BF16F(4, 4), **NOB, layout=9))
# pre-activations that are exactly zero: slope 0, as relu(h) - alpha relu(-h) has it
for a, tag in ((0.1, ""), (1.0, "_a1")):
    _case("zeros_f32_17_256_3_n65" + tag, 65, 17, 256, 3, alpha=a, inputs="zeros", expect=dict(F32F(2, 3), **F32B(2, 3)))
    _case("zeros_split_32_256_3_n65" + tag, 65, 32, 256, 3, alpha=a, inputs="zeros", expect=dict(SPLF(1, 3), **SPLB))
    _case("zeros_bf16_32_256_3_n65" + tag, 65, 32, 256, 3, alpha=a, dtype="bf16", inputs="zeros", expect=dict(BF16F(1, 3), **BF16B(2)))
# rows of x over 25 binades: y and dx judged row by row
_case("scaled_f32_17_256_3_n65", 65, 17, 256, 3, inputs="scaled", seed=6, expect=dict(F32F(2, 3), **F32B(2, 3)))
_case("scaled_split_32_256_3_n65", 65, 32, 256, 3, inputs="scaled", seed=1, expect=dict(SPLF(1, 3), **SPLB))
_case("scaled_split_64_256_4_n65", 65, 64, 256, 4, inputs="scaled", seed=1, expect=dict(SPLF(2, 4), **F32B(4, 4)))

# ---- one option flipped --------------------------------------------------------------------------------------------------------
N_DEFAULT = len(CASES)
_case("NO_MLP_SPLIT_32_256_3_n33", 33, 32, 256, 3, options=dict(NO_MLP_SPLIT=1), expect=dict(F32F(2, 3), **F32B(2, 3), fwd_shape="f32", bwd_shape="f32", layout=1))
_case("NO_MLP_BWD_SPLIT_32_256_3_n33", 33, 32, 256, 3, options=dict(NO_MLP_BWD_SPLIT=1), expect=dict(SPLF(1, 3), **F32B(2, 3), bwd_shape="f32", layout=3))
_case("NO_MLP_SPLIT_64_256_3_n33", 33, 64, 256, 3, options=dict(NO_MLP_SPLIT=1), expect=dict(F32F(0, 3), **F32B(4, 3), fwd_shape="f32"))
_case("NO_MLP_SPLIT_32_512_2_n65", 65, 32, 512, 2, alpha=1.0, options=dict(NO_MLP_SPLIT=1), expect=dict(F32F(2, 3), **F32B(2, 3, bwd_gy=2)))
_case("NO_MLP_BWD_SPLIT_32_1024_3_n4097", 4097, 32, 1024, 3, options=dict(NO_MLP_BWD_SPLIT=1), expect=dict(SPLF(1, 3), **F32B(2, 3, bwd_gy=4), **BIG))
_case("NO_MLP_SPLIT_packed_32_256_3_n33", 33, 32, 256, 3, packed=True, options=dict(NO_MLP_SPLIT=1), expect=dict(F32F(2, 3), **F32B(2, 3), layout=1))

NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


def default_sibling(case):
    """The case with the same shape, inputs and pointers on default options (None if the table has none)."""
    if not case["options"]:
        return None
    same = lambda a, b: all(a[k] == b[k] for k in ("n", "cin", "hidden", "cout", "alpha", "dtype", "seed", "inputs", "off", "packed"))
    return next((c for c in CASES if not c["options"] and same(c, case)), None)


# ---------------------------------------------------------------------------------------------
# inputs and the reference
# ---------------------------------------------------------------------------------------------
def _numeric_key(case):
    return tuple(case[k] for k in ("n", "cin", "hidden", "cout", "alpha", "dtype", "seed", "inputs"))


_INPUTS = {}


def inputs(case):
    """CPU float32 tensors x, W1, b1, W2, b2, dy as tests/test_gpu_ops.py draws them: x ~ N(0, 1), W ~ N(0, 0.05), b ~ N(0, 0.01),
    dy ~ N(0, 1) from RandomState(seed).  bf16 storage: x and W1 hold bf16-representable values (what the kernels and the
    reference are both fed).  A function of the numeric fields alone: option, offset and packed variants share them."""
    key = _numeric_key(case)
    if key in _INPUTS:
        return _INPUTS[key]
    n, cin, hidden, cout = case["n"], case["cin"], case["hidden"], case["cout"]
    rs = np.random.RandomState(case["seed"])
    t = lambda *a: torch.from_numpy(rs.normal(*a).astype(np.float32))
    d = dict(x=t(0, 1, (n, cin)), W1=t(0, 0.05, (cin, hidden)), b1=t(0, 0.01, hidden), W2=t(0, 0.05, (hidden, cout)), b2=t(0, 0.01, cout),
             dy=t(0, 1, (n, cout)))
    if case["inputs"] == "zeros":
        assert n > max(ZERO_ROWS) and hidden > max(ZERO_COLS)
        d["x"][list(ZERO_ROWS)] = 0.0
        d["b1"][list(ZERO_COLS)] = torch.tensor([0.0, -0.0] * (len(ZERO_COLS) // 2))
    elif case["inputs"] == "scaled":
        d["x"] *= torch.tensor([2.0 ** ((i % 25) - 12) for i in range(n)])[:, None]
    if case["dtype"] == "bf16":
        d["x"], d["W1"] = d["x"].bfloat16().float(), d["W1"].bfloat16().float()
    _INPUTS[key] = d
    return d


_REFS = {}


def reference(case, dtype):
    """y, dx, dW1, db1, dW2, db2 of the case by plain torch in `dtype` through autograd, the activation written as
    relu(h) - alpha relu(-h) (slope 0 at h == 0); float64 also keeps the pre-activations h.  Cached; never modified."""
    key = (_numeric_key(case), dtype)
    if key in _REFS:
        return _REFS[key]
    d = inputs(case)
    x, W1, b1, W2, b2 = (d[k].to(dtype).requires_grad_(True) for k in ("x", "W1", "b1", "W2", "b2"))
    h = x @ W1 + b1
    y = (torch.relu(h) - case["alpha"] * torch.relu(-h)) @ W2 + b2
    y.backward(d["dy"].to(dtype))
    out = dict(y=y.detach(), dx=x.grad, dW1=W1.grad, db1=b1.grad, dW2=W2.grad, db2=b2.grad)
    if dtype == torch.float64:
        out["h"] = h.detach()
    _REFS[key] = out
    return out


def ambiguous(case):
    """The units of the case at the leaky ReLU's kink (tests/mlp_kink.py); none where the layer has no kink (alpha == 1)."""
    import mlp_kink
    if case["alpha"] == 1.0:
        return []
    return mlp_kink.ambiguous_units(reference(case, torch.float64)["h"], skip_exact_zeros=True)
