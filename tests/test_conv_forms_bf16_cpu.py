"""Which kernel form every case of tests/conv_form_cases_bf16.py makes the library take, asked of fgc_conv_forms on the host
(include/fgc.h) with fake addresses that carry the case's byte offsets - nothing is launched and no pointer is followed.  The
GPU test (tests/test_gpu_conv_forms_bf16.py) asserts the same expectations on the real pointers and then holds each case to
float64; this file proves that the table as a whole reaches every form of the bf16 and of the pair-form kernels, that the
graphs are what the cases assume, that the storage reference behind bound (b) stays well inside the caps of bound (a), and
that the seeds keep the leaky-ReLU kink out of the comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_form_cases_bf16 as T
from facet_graph_convolution_amd import _lib
from test_conv_forms_cpu import FAKE, fake_desc_io as _fp32_fake_desc_io

_CPU_GRAPHS = {}


def cpu_graph(case):
    from facet_graph_convolution_amd.graph import FacetGraph
    key = (case["graph"], case["n"])
    if key not in _CPU_GRAPHS:
        _CPU_GRAPHS[key] = FacetGraph(T.klist(*key), "cpu")
    return _CPU_GRAPHS[key]


def fake_desc_io(case):
    """(descriptor, io, keep-alive) of a case with fake addresses: fake_desc_io of the fp32 table, extended for the storage
    flag, the pair graph (its counts are the real ones), tpair_* / dt, r_ld and offsets counted in bytes."""
    d, io, over = _fp32_fake_desc_io(case)
    bf16 = case["storage"] == "bf16"
    if bf16:
        d.flags = _lib.CONV_BF16
    d.src_rows = case["n"] >> case["shift"]
    if case["pairs"]:
        pg = cpu_graph(case).pairs()
        d.pair_rowptr = d.pair_col = d.pair_mul = d.hc = FAKE
        d.n_pairs, d.max_pair_deg, d.max_pair_in_deg = pg.n_pairs, pg.max_deg, pg.max_in_deg
        io.tpair_rowptr = io.tpair_col = io.tpair_edge = io.dt = FAKE
    if case["r_ld"] == "pad":
        io.r_ld = _lib.lib().fgc_conv_r_ld(case["cout"], 1, int(bf16))
    return d, io, over


def forms_of(case):
    d, io, keep = fake_desc_io(case)
    return _lib.conv_forms(d, io)


def test_the_table_has_the_agreed_shape():
    assert 60 <= len(T.CASES) <= 95 and len(set(T.NAMES)) == len(T.NAMES)
    assert all(not c["options"] for c in T.CASES[:T.N_DEFAULT]) and all(c["options"] for c in T.CASES[T.N_DEFAULT:])
    assert all(c["expect"] for c in T.CASES)
    assert all(c["n"] == 404 or any(w in c["name"] for w in ("_n16_", "_n37_", "_n100_", "_n148_", "_n1100_", "_n1101_")) for c in T.CASES)
    # every pair-form layer on default options runs in both storages
    f32 = {c["name"].replace("pair_f32_", "") for c in T.CASES if c["pairs"] and c["storage"] == "fp32" and not c["options"]}
    bf = {c["name"].replace("pair_bf_", "") for c in T.CASES if c["pairs"] and c["storage"] == "bf16" and not c["options"]}
    assert f32 - bf == {"hub_64_32"} and not bf - f32
    assert sorted(c["refused"] for c in T.CASES if c["refused"]) == ["fgc_conv_bwd"] * 3 + ["fgc_conv_fwd"] * 3


def test_the_graphs_are_what_the_cases_assume():
    from facet_graph_convolution_amd.graph import FacetGraph
    indeg = lambda a: np.bincount(a[a != 0] - 1, minlength=len(a))
    deg = lambda a: (a != 0).sum(1)
    reg, lng, hub, tail = (T.klist(r, 404) for r in ("reg", "long", "hub", "reg+tail"))
    assert deg(reg).max() <= 16 and indeg(reg).max() <= 16 and deg(reg).min() == 1
    assert 17 <= deg(lng).max() <= 23 and indeg(lng).max() <= 24
    assert indeg(hub).max() > 24 and deg(hub).max() <= 16
    assert (tail[-5:] == 0).all() and tail.max() <= 399
    for n in (16, 37, 100, 148, 1100, 1101):
        assert deg(T.klist("reg", n)).max() <= 16 and indeg(T.klist("reg", n)).max() <= 16
    pairs = lambda recipe, n: FacetGraph(T.klist(recipe, n), "cpu").pairs()
    pr, pl, ph, pt = pairs("reg", 404), pairs("long", 404), pairs("hub", 404), pairs("reg+tail", 404)
    assert (pr.n_pairs, pr.max_deg, pr.max_in_deg) == (1342, 16, 16)
    assert (pl.n_pairs, pl.max_deg, pl.max_in_deg) == (1555, 20, 20) and 17 <= pl.max_in_deg <= 24
    assert ph.max_in_deg > 24 and pt.max_in_deg <= 16
    for n in (100, 148, 1100):
        assert 0 < pairs("reg", n).max_in_deg <= 16
    assert pairs("reg", 100).max_deg > 16        # (a block with more than 16 pairs: the pair kernels walk it in chunks)
    # the blocks of 100 and 148 nodes do not fill the last workgroup of the pair d-logits kernel (32 blocks = 128 nodes)
    assert (100 // 4) % 32 and (148 // 4) % 32


@pytest.mark.parametrize("name", T.NAMES)
def test_each_case_takes_the_form_it_exists_for(name):
    case = T.BY_NAME[name]
    d, io, keep = fake_desc_io(case)
    forms = _lib.conv_forms(d, io)
    missed = {k: (v, forms.get(k)) for k, v in case["expect"].items() if forms.get(k) != v}
    assert not missed, "%s: (expected, got) %s in %s" % (name, missed, forms)
    assert _lib.lib().fgc_conv_uses_pairs(C.byref(d)) == T.uses_pairs(case)
    if case["options"]:      # an option that changes no form tests nothing: the table holds none
        sib = T.default_sibling(case)
        assert sib is not None, "no default-option sibling"
        assert forms_of(sib) != forms
    # forward-only form: the same forward keys, and what the plan alone decides
    fwd_only = _lib.conv_forms(d)
    per_call = ("k1", "k3_slabs", "k3_rows") if forms["k1"] == "narrow" else ()
    assert all(forms[k] == v for k, v in fwd_only.items() if k not in per_call)


def test_the_table_reaches_every_form():
    cases = [c for c in T.CASES if not c["refused"]]
    forms = [forms_of(c) for c in cases]
    bf = [f for c, f in zip(cases, forms) if c["storage"] == "bf16"]
    has = lambda fs, **kv: any(all(f.get(k) == str(v) for k, v in kv.items()) for f in fs)
    for bfm in (0, 1):
        for nt in (16, 32):
            assert has(bf, fwd="w8", fwd_bfm=bfm, fwd_nt=nt), ("fwd", bfm, nt)
            assert has(bf, fwd="w8", k2="w8", k2_bfm=bfm, k2_nt=nt), ("k2", bfm, nt)
    assert has(bf, fwd="w8", fwd_slots=24) and has(bf, fwd="w8", k2_slots=24)
    for lng, half in ((0, 0), (0, 1), (1, 0)):
        assert has(bf, k1="bf16", k1_long=lng, k1_half=half), (lng, half)
    for lng in (0, 1):
        assert has(bf, k1="pair", k1_long=lng) and has(forms, k1="pair", k1_long=lng, k3="stream4")
    for ds in ("fused", "vec", "narrow-fused", "pair"):
        assert has(bf, ds=ds), ds
    # the data kernel of the pair form (the EROW instances): matrix pipe and vector form, 16 and 24 slots, both storages
    for bfm in (0, 1):
        for nt in (16, 32):
            assert has(bf, fwd="pair", k2_bfm=bfm, k2_slots=16, k2_nt=nt), ("pair k2", bfm, nt)
    assert has(bf, fwd="pair", k2_bfm=0, k2_slots=24, k2_nt=32)
    f32 = [f for c, f in zip(cases, forms) if c["storage"] == "fp32"]
    for nt in (16, 32):
        assert has(f32, fwd="pair", k2_slots=16, k2_nt=nt), ("fp32 pair k2", nt)
    assert has(f32, fwd="pair", k2_slots=24, k2_nt=32)
    for variant in ("bf16_2", "bf16_4", "stream2_bf", "stream4_bf"):
        assert has(bf, k3=variant), variant
    assert has(bf, k3_slabs=1)
    for variant in ("bf16_2", "bf16_4", "stream2_bf", "stream4_bf"):      # (404 rows: 2 x 204 or 4 x 104, the last slab short)
        ragged = [c["name"] for c, f in zip(cases, forms) if f["k3"] == variant and int(f["k3_slabs"]) > 1 and
                  ((c["n"] >> (2 if f["fwd"] == "pair" else 0)) % int(f["k3_rows"])) != 0]
        assert ragged, variant
    # the slab count follows TNB_WGS
    slabs = {forms_of(T.BY_NAME[n])["k3_slabs"] for n in ("bf_n1101_64_128", "bf_TNB_WGS=4_n1101_64_128", "bf_TNB_WGS=12_n1101_64_128")}
    assert len(slabs) == 3, slabs


def test_the_storage_reference_stays_inside_the_caps():
    """Bound (b) of the GPU test allows 8 max(e_store, 2^-9), bound (a) the project's caps.  (b) only says something while the
    storage reference itself - float64 arithmetic, bf16 at the storage points - uses at most half of each cap: a case that
    fails this needs another seed or size, never another cap."""
    seen, worst = set(), {}
    for case in T.CASES:
        key = T._numeric_key(case)
        if key in seen or case["refused"]:
            continue
        seen.add(key)
        for k, e in T.e_store(case).items():
            assert e <= 0.5 * T.CAPS[k], (case["name"], k, e)
            worst[k] = max(worst.get(k, 0.0), e)
    print("largest e_store per tensor:", " ".join("%s %.2e" % kv for kv in sorted(worst.items())))


def test_the_pair_forms_own_storage_stays_inside_the_caps():
    """The bf16 pair form stores hc, y, dt and r as bf16 (include/fgc.h); the storage reference leaves hc, dt and r out.
    A float64 computation that rounds at exactly those points lands within 1e-5 of what the kernels give for y and dW0 (the
    kernels add nothing of their own there), and for dW0 1.3 .. 2 times above the fine form's storage: one sum over a block's
    children is rounded once, at its larger size.  With free seeds the long graph sits at 3.1e-3 .. 3.6e-3 against the cap of
    3e-3.  So that cap (a) measures the kernels and not the draw, every layer that runs in the bf16 pair form leaves a tenth
    of the caps of y and dW0 free (fp32 summation order, a slope that differs at a rounded zero) - by its seed, never by the
    cap.  The price: for these layers cap (a) on y and dW0 holds by selection of the draw, not on arbitrary inputs."""
    seen = set()
    for case in T.CASES:
        key = T._numeric_key(case)
        if key in seen or case["storage"] != "bf16" or not T.uses_pairs(case):
            continue
        seen.add(key)
        for k, e in T.pair_storage_errors(case).items():
            assert e <= T.PAIR_STORE_ROOM * T.CAPS[k], (case["name"], k, e)
    assert len(seen) == 12


def test_the_seeds_keep_the_leaky_relu_kink_out_of_the_comparison():
    """The condition of the fp32 table on the same kind of inputs: the torch float32 oracle's signs differ from float64's in at
    most 4 elements per case, each with |pre64| < 1e-6."""
    seen = set()
    for case in T.CASES:
        key = T._numeric_key(case)
        if key in seen or not case["act"] or case["refused"]:
            continue
        seen.add(key)
        pre64, pre32 = T.preactivation(case, torch.float64), T.preactivation(case, torch.float32)
        count, worst = T.sign_flips(pre32, pre64)
        assert count <= 4 and worst < 1e-6, (case["name"], count, worst)
