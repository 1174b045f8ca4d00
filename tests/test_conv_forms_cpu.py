"""Which kernel form every case of tests/conv_form_cases.py makes the library take, asked of fgc_conv_forms on the host
(include/fgc.h): descriptors and ios with fake addresses that carry the case's byte offsets - nothing is launched and no
pointer is followed.  The GPU test (tests/test_gpu_conv_forms.py) asserts the same expectations on the real pointers and
then holds each case to float64; this file proves that the table as a whole reaches every form of the fp32 kernels, and that
the seeds keep the leaky-ReLU kink out of the comparison."""
import ctypes as C

import pytest
import torch

import conv_form_cases as T
from facet_graph_convolution_amd import _lib

FAKE = 1 << 20      # 16-byte aligned, never dereferenced


def fake_desc_io(case):
    """(descriptor, io, keep-alive) of a case with fake addresses at the case's offsets."""
    from facet_graph_convolution_amd.graph import FacetGraph
    g = FacetGraph(T.klist(case["graph"], case["n"]), "cpu")
    off = case["off"]
    d = _lib.ConvDesc()
    d.n, d.nnz, d.rowptr, d.col = g.n, g.nnz, FAKE, FAKE
    d.x0, d.x1 = FAKE + off.get("x0", 0), (FAKE if case["c1"] else None)
    d.c0, d.c1, d.shift, d.cout = case["c0"], case["c1"], case["shift"], case["cout"]
    d.W0 = d.b = d.u = d.c = d.v = FAKE
    d.bias_mask, d.act, d.alpha, d.max_deg = case["bias_mask"], case["act"], T.ALPHA, g.max_deg
    over = _lib.option_overrides(**case["options"]) if case["options"] else None
    if over is not None:
        d.options, d.n_options = C.addressof(over), len(over)
    io = _lib.ConvBwdIO()
    io.trowptr = io.tcol = io.tedge = io.ag = io.dl = io.dag = FAKE
    io.dW0 = io.db = io.du = io.dc = io.dv = FAKE
    io.max_in_deg = g.max_in_deg
    io.y, io.dy, io.ds, io.r = (FAKE + off.get(k, 0) for k in ("y", "dy", "ds", "r"))
    mode = case["mode"]
    io.dx0 = None if "nodx" in mode else FAKE
    io.dx1 = FAKE if (case["c1"] and "nodx" not in mode) else None
    io.accumulate0, io.accumulate1 = int("acc0" in mode), int("acc1" in mode or "acc01" in mode)
    if "pool" in mode:
        io.pool_y = io.pool_dy = FAKE
    return d, io, over


def test_the_table_has_the_agreed_shape():
    assert 80 <= len(T.CASES) <= 130 and len(set(T.NAMES)) == len(T.NAMES)
    assert all(not c["options"] for c in T.CASES[:T.N_DEFAULT]) and all(c["options"] for c in T.CASES[T.N_DEFAULT:])
    assert all(c["expect"] for c in T.CASES)
    # the graphs are what their recipes promise
    import numpy as np
    reg, lng, hub, tail = (T.klist(r, 404) for r in ("reg", "long", "hub", "reg+tail"))
    indeg = lambda a: np.bincount(a[a != 0] - 1, minlength=len(a))
    deg = lambda a: (a != 0).sum(1)
    assert deg(reg).max() <= 16 and indeg(reg).max() <= 16 and deg(reg).min() == 1 and (deg(reg)[3::7] == 1).all()
    assert 17 <= deg(lng).max() <= 23
    top = np.sort(indeg(hub))[::-1]
    assert 49 <= top[0] <= 72 and 25 <= top[1] <= 48 and top[2] <= 24 and deg(hub).max() <= 16
    assert (tail[-5:] == 0).all() and tail.max() <= 399
    assert 49 <= indeg(T.klist("hub", 100)).max() <= 72


@pytest.mark.parametrize("name", T.NAMES)
def test_each_case_takes_the_form_it_exists_for(name):
    case = T.BY_NAME[name]
    d, io, keep = fake_desc_io(case)
    forms = _lib.conv_forms(d, io)
    missed = {k: (v, forms.get(k)) for k, v in case["expect"].items() if forms.get(k) != v}
    assert not missed, "%s: (expected, got) %s in %s" % (name, missed, forms)
    sib = T.default_sibling(case)
    if case["options"]:      # an option that changes no form tests nothing: the table holds none
        assert sib is not None, "no default-option sibling"
        ds, ios, _ = fake_desc_io(sib)
        if not name.startswith("TN_SLOTS"):     # (at 1101 rows the slab count is capped by rows / 128 whatever the slots)
            assert _lib.conv_forms(ds, ios) != forms
    # forward-only form: the same forward keys, and what the plan alone decides
    fwd_only = _lib.conv_forms(d)
    narrow = forms["k1"] == "narrow"      # (chosen per call: the plan alone names the tiled kernel and its GEMM's slabs)
    per_call = ("k1", "k3_slabs", "k3_rows") if narrow else ("k1_split", "layout_id") if case["off"].get("ds") else ()
    assert all(forms[k] == v for k, v in fwd_only.items() if k not in per_call)


def test_the_table_reaches_every_form():
    forms = []
    for case in T.CASES:
        d, io, keep = fake_desc_io(case)
        forms.append(_lib.conv_forms(d, io))
    has = lambda **kv: any(all(f.get(k) == str(v) for k, v in kv.items()) for f in forms)
    for lng, half in ((0, 0), (0, 1), (1, 0)):
        assert has(k1="deep", k1_long=lng, k1_half=half), (lng, half)
    for split in (0, 1):
        assert has(k1="deep", k1_split=split)
    for okg in (0, 2, 4, 8):
        assert has(k1="deep", k1_okg=okg), okg
    for ag in (0, 1):
        assert has(k1="deep", k1_aglobal=ag)
    for v4 in (0, 1):
        assert has(k1="mfma", k1_vec4=v4)
    assert has(k1="valu") and has(k1="narrow")
    for ds in ("fused", "vec", "scalar", "narrow-fused"):
        assert has(ds=ds), ds
    for pre in ("fwd", "k2"):
        kv = lambda **d: {pre if k == "kind" else "%s_%s" % (pre, k): v for k, v in d.items()}
        assert has(**kv(kind="w8", fast=1, slots=16, nt=16)), pre
        assert has(**kv(kind="w8", fast=1, slots=16, nt=32)), pre
        assert has(**kv(kind="w8", fast=1, slots=24)), pre
        assert has(**kv(kind="w8", fast=0)), pre
        assert has(**kv(kind="tiled", vec4=1)), pre
        assert has(**kv(kind="tiled", vec4=0)), pre
    assert any(f["k2"] == "tiled" and int(f["k2_chunks"]) >= 3 for f in forms)
    for variant in ("stream2", "stream4", "plain_v4", "plain"):
        assert has(k3=variant), variant
    assert has(k3_slabs=1)
    ragged = [c["name"] for c, f in zip(T.CASES, forms) if f["k3"] != "narrow" and int(f["k3_slabs"]) > 1 and
              (c["n"] % int(f["k3_rows"])) != 0]
    assert ragged
    assert has(proj="stream") and has(proj="block")


def test_the_form_string_follows_a_descriptors_own_overrides():
    case = T.BY_NAME["plain_32_32"]
    d, io, _ = fake_desc_io(case)
    base = _lib.conv_forms(d, io)
    over = _lib.option_overrides(NO_W8=1, NO_K1DEEP=1, NO_TNSTREAM=1)
    before = {k: _lib.get_option(k) for k in ("NO_W8", "NO_K1DEEP", "NO_TNSTREAM")}
    d.options, d.n_options = C.addressof(over), len(over)
    mine = _lib.conv_forms(d, io)
    assert (base["fwd"], base["k1"], base["k3"]) == ("w8", "deep", "stream2")
    assert (mine["fwd"], mine["k1"], mine["k3"]) == ("tiled", "mfma", "plain_v4")
    assert {k: _lib.get_option(k) for k in before} == before == dict(NO_W8=0, NO_K1DEEP=0, NO_TNSTREAM=0)
    d.options, d.n_options = None, 0
    assert _lib.conv_forms(d, io) == base
    # ... and the process-level table still rules a descriptor without a list
    with _lib.options(NO_W8=1):
        assert _lib.conv_forms(d, io)["fwd"] == "tiled"
    # a ds that is not 16-byte aligned: a call that packs its own operands leaves the split layout (whose kernel needs the
    # alignment), a call on operands packed ahead cannot (the launch refuses it)
    d4, io4, _ = fake_desc_io(T.BY_NAME["dyp4_32_32"])
    assert _lib.conv_forms(d4)["k1_split"] == "1" and _lib.conv_forms(d4, io4)["k1_split"] == "0"
    io4.flags = _lib.CONV_PACKED
    assert _lib.conv_forms(d4, io4)["k1_split"] == "1"
    # errors: a null descriptor, a buffer too small
    L = _lib.lib()
    buf = C.create_string_buffer(16)
    assert L.fgc_conv_forms(None, None, buf, 16) == -22
    assert L.fgc_conv_forms(C.byref(d), C.byref(io), buf, 16) == -22 and b"too small" in L.fgc_last_error()


def test_the_seeds_keep_the_leaky_relu_kink_out_of_the_comparison():
    """The backward reads lrelu' from the stored y, and the GPU test gives the oracle the kernel's own slopes.  That is only
    a fair comparison while a sign that differs from float64's belongs to a pre-activation at rounding distance from 0:
    the torch float32 oracle on the CPU meets the condition the GPU test asserts of the kernels."""
    seen = set()
    for case in T.CASES:
        key = T._numeric_key(case)
        if key in seen or not case["act"]:
            continue
        seen.add(key)
        pre64, pre32 = T.preactivation(case, torch.float64), T.preactivation(case, torch.float32)
        count, worst = T.sign_flips(pre32, pre64)
        assert count <= 4 and worst < 1e-6, (case["name"], count, worst)
