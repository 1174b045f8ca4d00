"""Which kernel form every case of tests/mlp_form_cases.py makes the MLP head take, asked of fgc_mlp_forms on the host
(include/fgc.h) with fake addresses that carry the case's byte offsets - nothing is launched and no pointer is followed.  The
GPU test (tests/test_gpu_mlp_forms.py) asserts the same expectations on the real pointers and then holds each case to float64;
this file proves that the table as a whole reaches every template instance behind plan_mlp_fwd / plan_mlp_bwd, and that the
seeds keep the leaky-ReLU kink out of the comparison."""
import ctypes as C

import pytest
import torch

import mlp_form_cases as T
from facet_graph_convolution_amd import _lib

FAKE = 1 << 20      # 16-byte aligned, never dereferenced


def fake_forms(case):
    """fgc_mlp_forms of a case with fake addresses at the case's offsets, under the case's options."""
    off = case["off"]
    with _lib.options(**case["options"]):
        return _lib.mlp_forms(case["n"], case["cin"], case["hidden"], case["cout"], case["dtype"] == "bf16",
                              x=FAKE + off.get("x", 0), dx=FAKE + off.get("dx", 0), b1=FAKE + off.get("b1", 0),
                              fwd_ws=FAKE + off.get("ws", 0), bwd_ws=FAKE + off.get("ws", 0))


def test_the_table_has_the_agreed_shape():
    assert 60 <= len(T.CASES) <= 100 and len(set(T.NAMES)) == len(T.NAMES)
    assert all(not c["options"] for c in T.CASES[:T.N_DEFAULT]) and all(c["options"] for c in T.CASES[T.N_DEFAULT:])
    assert all("fwd" in c["expect"] and "bwd" in c["expect"] for c in T.CASES)
    assert {c["n"] for c in T.CASES} == {1, 33, 65, 4097} and {c["alpha"] for c in T.CASES} == {0.0, 0.1, 1.0}
    assert {c["cout"] for c in T.CASES} == {1, 2, 3, 4}
    assert {c["hidden"] for c in T.CASES} == {64, 192, 256, 512, 768, 1024}
    # hidden = 1024 belongs to the existing tests: here only where 4097 rows want it
    assert all(c["n"] == 4097 for c in T.CASES if c["hidden"] == 1024)
    # every 4097-row backward exists without a kink; the zero cases run with and without one, in every form
    for c in T.CASES:
        if c["n"] == 4097 and c["alpha"] != 1.0 and not c["options"]:
            assert any(d["n"] == 4097 and d["alpha"] == 1.0 and d["expect"]["bwd"] == c["expect"]["bwd"] for d in T.CASES), c["name"]
    for form in ("f32", "split", "bf16"):
        assert {c["alpha"] for c in T.CASES if c["inputs"] == "zeros" and c["expect"]["bwd"] == form} == {0.1, 1.0}
    assert {c["expect"]["bwd"] for c in T.CASES if c["inputs"] == "scaled"} >= {"f32", "split"}
    assert {tuple(sorted(c["off"].items())) for c in T.CASES if c["off"]} == {(("x", 4),), (("x", 8),), (("dx", 4),), (("b1", 4),), (("ws", 4),)}
    assert all(c["dtype"] == "f32" and c["cin"] == 32 and not c["packed"] for c in T.CASES if c["off"])
    assert {c["expect"]["fwd"] for c in T.CASES if c["packed"]} == {"f32", "split", "bf16"}


@pytest.mark.parametrize("name", T.NAMES)
def test_each_case_takes_the_form_it_exists_for(name):
    case = T.BY_NAME[name]
    forms = fake_forms(case)
    missed = {k: (v, forms.get(k)) for k, v in case["expect"].items() if forms.get(k) != v}
    assert not missed, "%s: (expected, got) %s in %s" % (name, missed, forms)
    if case["options"]:      # an option that changes no form tests nothing: the table holds none
        sib = T.default_sibling(case)
        assert sib is not None, "no default-option sibling"
        theirs = fake_forms(sib)
        changed = {k for k in forms if forms[k] != theirs[k]}
        assert changed & set(case["expect"]), (changed, case["expect"])
    # NULL pointers stand for aligned ones
    if not case["off"]:
        with _lib.options(**case["options"]):
            assert _lib.mlp_forms(case["n"], case["cin"], case["hidden"], case["cout"], case["dtype"] == "bf16") == forms


def test_the_table_reaches_every_instance_behind_the_plan():
    """Every arm of the four dispatch switches (launch_mlp_fwd_f32, launch_mlp_bwd_f32, launch_mlp_fwd_split,
    launch_mlp_fwd_bf16), the two launches of the split backward and the arrangements of the bf16 backward, each as the
    EXPECTED form of at least one case: a later edit of the table cannot quietly drop an instance."""
    ex = [dict(c["expect"], n=str(c["n"]), dtype=c["dtype"], cin=str(c["cin"]), cout=str(c["cout"])) for c in T.CASES]
    has = lambda **kv: any(all(e.get(k) == str(v) for k, v in kv.items()) for e in ex)
    missing = []
    for co in (3, 4):
        for ks in (1, 2, 0):
            missing += [] if has(fwd="f32", fwd_ks=ks, fwd_co=co) else [("mlp_fwd_kernel", ks, co)]
        for mt in (2, 4, 8):
            missing += [] if has(bwd="f32", bwd_mt=mt, bwd_co=co) else [("mlp_bwd_kernel", mt, co)]
        for ks in (1, 2):
            missing += [] if has(fwd="split", fwd_ks=ks, fwd_co=co) else [("mlp_fwd_split_kernel", ks, co)]
        for ks in (1, 2, 4):
            missing += [] if has(fwd="bf16", fwd_ks=ks, fwd_co=co) else [("mlp_fwd_bf16_kernel", ks, co)]
    # the split backward (dx kernel + parameter kernel) and the bf16 backward (MT = 2, 4), each with idle walkers (33 rows: four
    # walkers, two tiles) and with a walker that takes a second tile (4097 rows); the bf16 refusals
    for n in (1, 33, 65, 4097):
        missing += [] if has(bwd="split", bwd_mt=2, n=n) else [("mlp_bwd_*_split_kernel", n)]
    for mt in (2, 4):
        for n in (33, 4097):
            missing += [] if has(bwd="bf16", bwd_mt=mt, n=n) else [("mlp_bwd_*_bf16_kernel", mt, n)]
    missing += [] if has(bwd="none", dtype="bf16", cin=128) else ["bf16 backward refuses cin = 128"]
    missing += [] if has(bwd="none", dtype="bf16", cout=4, cin=32) else ["bf16 backward refuses cout = 4"]
    missing += [] if has(bwd="f32", bwd_co=4, fwd="split", cin=32) else ["split backward leaves cout = 4 to the fp32 MFMA"]
    for mt in (2, 4, 8):
        missing += [] if has(bwd="f32", bwd_mt=mt, n=4097) else [("mlp_bwd_kernel second tile", mt)]
    assert not missing, missing
    # ... and the expectations are what the library answers (test_each_case_takes_the_form_it_exists_for), so the instances are real
    for gy in (1, 2, 3):
        assert has(bwd="split", bwd_gy=gy) and has(bwd="f32", bwd_mt=2, bwd_gy=gy), gy


def test_the_seeds_keep_the_leaky_relu_kink_out_of_the_comparison():
    """A unit whose float64 pre-activation lies within 1e-6 of zero (and is not exactly zero) may take either slope in fp32.
    Cases of up to 65 rows have none; the 4097-row cases with a kink have a few, which the GPU test resolves one by one
    (tests/mlp_kink.py): at most 40, at most 6 per hidden column.  Float64 reference only."""
    seen = set()
    for case in T.CASES:
        key = T._numeric_key(case)
        if key in seen:
            continue
        seen.add(key)
        amb = T.ambiguous(case)
        if case["n"] <= 133:
            assert not amb, (case["name"], amb)
        else:
            per_col = {}
            for i, k in amb:
                per_col[k] = per_col.get(k, 0) + 1
            assert len(amb) <= 40 and max(per_col.values(), default=0) <= 6, (case["name"], len(amb))
        if case["inputs"] == "zeros":
            h = T.reference(case, torch.float64)["h"]
            assert int((h == 0).sum()) == len(T.ZERO_ROWS) * len(T.ZERO_COLS)
            assert bool((h[list(T.ZERO_ROWS)][:, list(T.ZERO_COLS)] == 0).all())


def test_the_form_string_and_its_buffer():
    L = _lib.lib()
    args = (33, 32, 256, 3, 0, None, None, None, None, None)
    big = C.create_string_buffer(1024)
    full = L.fgc_mlp_forms(*args, big, len(big))
    assert full > 0 and big.value.decode() == " ".join("%s=%s" % kv for kv in _lib.mlp_forms(33, 32, 256, 3).items())
    assert len(big.value) == full < 512
    text = big.value
    assert L.fgc_mlp_forms(*args, None, 1024) == -22 and b"no buffer" in L.fgc_last_error()
    assert L.fgc_mlp_forms(*args, big, 0) == -22
    GUARD = 32
    for length in range(1, full + 2):
        buf = C.create_string_buffer(b"\xAB" * (length + GUARD), length + GUARD)
        rc = L.fgc_mlp_forms(*args, buf, length)
        assert buf.raw[length:] == b"\xAB" * GUARD, "wrote behind a buffer of %d bytes" % length
        if length <= full:
            assert rc == -22 and b"too small" in L.fgc_last_error(), length
            assert b"\0" in buf.raw[:length] and text.startswith(buf.value)     # (whole pairs only, terminated)
        else:
            assert rc == full and buf.value == text
    # the line follows the options and the pointers of the moment, and shapes without a kernel read `none`
    base = _lib.mlp_forms(33, 32, 256, 3)
    assert (base["fwd"], base["bwd"], base["layout"]) == ("split", "split", "7")
    with _lib.options(NO_MLP_BWD_SPLIT=1):
        f = _lib.mlp_forms(33, 32, 256, 3)
        assert (f["fwd"], f["bwd"], f["bwd_shape"], f["layout"]) == ("split", "f32", "f32", "3")
    assert _lib.mlp_forms(33, 32, 256, 3) == base
    f = _lib.mlp_forms(33, 32, 256, 3, x=FAKE + 4)
    assert (f["fwd"], f["bwd"], f["fwd_shape"], f["bwd_shape"]) == ("f32", "f32", "split", "split")
    f = _lib.mlp_forms(33, 32, 256, 3, bwd_ws=FAKE + 8)
    assert (f["fwd"], f["bwd"]) == ("split", "none")
    assert _lib.mlp_forms(33, 32, 256, 3, bf16=True, x=FAKE + 8)["fwd"] == "none"
    for shape in ((0, 32, 256, 3), (33, 129, 256, 3), (33, 0, 256, 3), (33, 32, 256, 5), (33, 32, 256, 0), (33, 32, 0, 3)):
        f = _lib.mlp_forms(*shape)
        assert (f["fwd"], f["bwd"]) == ("none", "none"), shape
    f = _lib.mlp_forms(33, 48, 320, 3)
    assert (f["fwd"], f["bwd"]) == ("f32", "none")


@pytest.mark.parametrize("option", ["default", "NO_MLP_SPLIT", "NO_MLP_BWD_SPLIT"])
def test_the_form_string_agrees_with_the_layout_id_and_the_recorded_workspace_sizes(option):
    """fgc_mlp_forms, fgc_mlp_layout_id and the size queries read one plan: the layout the line names is the id, and the
    forward operand of the form it names fills the recorded workspace (tests/test_abi_cpu.py) - of the fp32 entry point, the
    larger of the two forms it may take."""
    import test_abi_cpu as A
    L = _lib.lib()
    up = lambda b: (b + 255) // 256 * 256
    with _lib.options(**({} if option == "default" else {option: 1})):
        for (cin, hidden), recorded in A._MLP_FWD_BYTES.items():
            for cout in (1, 3):
                f = _lib.mlp_forms(33, cin, hidden, cout)
                assert int(f["layout"]) == L.fgc_mlp_layout_id(cin, hidden, cout, 0) == A._MLP_IDS[option].get(cin, 1)
                assert int(f["layout"]) == 1 | (2 if f["fwd_shape"] == "split" else 0) | (4 if f["bwd_shape"] == "split" else 0)
                kpad = int(_lib.mlp_forms(33, cin, hidden, cout, x=FAKE + 4)["fwd_kpad"])      # (the fp32 MFMA's operand)
                assert kpad == (cin + 15) // 16 * 16
                assert recorded == max(up(kpad * hidden * 4), up(3 * cin * hidden * 2))
                want = dict(A._MLP_BWD_BYTES)
                want.update({} if option == "default" else A._MLP_BWD_BYTES_NO_SPLIT)
                assert L.fgc_mlp_bwd_workspace_bytes(33, cin, hidden, cout) == want[(cin, hidden)][A._MLP_NS.index(33)]
                # the dx slabs of the fp32 MFMA are what makes its workspace grow with n: hidden / (64 ctw) slabs of n x cin floats
                g = _lib.mlp_forms(33, cin, hidden, cout, x=FAKE + 4)
                assert int(g["bwd_dx_slabs"]) == hidden // (64 * int(g["bwd_ctw"])) and g["bwd"] == "f32"
        for (cin, hidden), recorded in A._MLP_BF16_FWD_BYTES.items():
            f = _lib.mlp_forms(33, cin, hidden, 3, bf16=True)
            assert int(f["layout"]) == L.fgc_mlp_layout_id(cin, hidden, 3, 1) == 9
            assert (f["fwd"], f["fwd_ks"]) == ("bf16", str(cin // 32)) and recorded == up(cin * hidden * 2)
