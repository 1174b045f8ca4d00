"""Every kernel form of the per-facet MLP head, one call pair at a time, against float64 - and proof of which form ran.

tests/mlp_form_cases.py lists ~80 calls (widths, hidden sizes, output counts, slopes, row counts, pointer alignments, operands
packed ahead, one developer option flipped).  For each, one helper drives the C ABI directly: it asks fgc_mlp_forms (with the
REAL pointers) which form the two entry points will take and asserts the keys the case exists to reach, runs fgc_mlp_fwd +
fgc_mlp_bwd (or their _bf16 forms; a form of `none` must be refused with -22 and leave its outputs alone), and compares with
plain torch in float64 through autograd, the activation written relu(h) - alpha relu(-h).

Bounds, fp32 storage:
 (a) the project's kernel tolerances (tests/test_gpu_ops.py): |y - y64| < 3e-6 max(1, max|y64|), every gradient within
     5e-6 max(1, max|g64|).
 (b) no floor of 1: e = max|g - g64| / max|g64| <= 8 max(e32, 2^-22), where e32 is the same measure of plain torch float32 on
     the same inputs (margin and floor as in tests/test_gpu_conv_forms.py: a different summation order earns that and no
     more); y likewise.  The "scaled" cases judge y and dx row by row: the error over that row's largest reference entry.
 Every forward partial sum of |y| against the float64 sum over its own 64 rows, relative 1e-4.
Bounds, bf16 storage (the reference is fed the same bf16-rounded x and W1): those of test_bf16_mlp_kernels_against_torch - y
1e-5; dx, dW1, db1 1.5e-2, dW2 4e-3, db2 1e-5 of the largest entry.  They cannot see a lost row, so every bf16 backward of 33
rows and more (and every 4097-row fp32 case) is also run as two calls on rows [0, k) and [k, n), k = 32 and 4096: the parameter
gradients of the whole call equal the sum of the parts within (a), and each part's rows of y and dx equal the whole call's bit
for bit (a row's result does not depend on where its tile sits).
The kink: cases of up to 65 rows have no pre-activation within 1e-6 of zero (tests/test_mlp_forms_cpu.py); the 4097-row cases
with alpha != 1 have a few, resolved one by one (tests/mlp_kink.py; at most 40, 6 per column).  Pre-activations that are
EXACTLY zero ("zeros" cases) are no such matter: slope 0, as the reference has it - held by the comparison and, sharply, by a
call on the zero rows alone whose db1 must be exactly zero in the zero-bias columns.
Parameters, dy and the outputs lie between NaN-filled surroundings that must come back untouched: a read past W2's last row
(cout < 4) would show even where it is multiplied by zero.  Measured e / e32 per form: DESIGN.md section 3.8."""
import ctypes as C

import pytest
import torch

import mlp_form_cases as T
import mlp_kink
from test_gpu_conv_forms import _Slices

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -22
MARGIN = 8.0
UNTOUCHED = 768.0          # (exact in bf16)
GRADS = ["dx", "dW1", "db1", "dW2", "db2"]
BF16_TOL = dict(dx=1.5e-2, dW1=1.5e-2, db1=1.5e-2, dW2=4e-3, db2=1e-5)


def _workspace(nbytes, off, dev):
    base = torch.empty(nbytes + 512, dtype=torch.uint8, device=dev)
    view = base[256 + off:256 + off + nbytes]
    assert view.data_ptr() % 16 == off % 16
    return view


def _mlp_fwd_bwd(case, dev, rows=None, x=None, dy=None, check_expect=True):
    """One MLP call pair straight through the C ABI, on rows [rows[0], rows[1]) of the case's x / dy (or on the x / dy given).
    Returns dict(forms, y, partials, dx, dW1, db1, dW2, db2); y / the gradients are None where the entry point refused."""
    from facet_graph_convolution_amd import _lib
    from facet_graph_convolution_amd._lib import ptr, stream_ptr, check
    L = _lib.lib()
    inp, off, bf = T.inputs(case), case["off"], case["dtype"] == "bf16"
    x = inp["x"] if x is None else x
    dy = inp["dy"] if dy is None else dy
    if rows is not None:
        x, dy = x[rows[0]:rows[1]], dy[rows[0]:rows[1]]
    n, cin, hidden, cout, alpha = x.shape[0], case["cin"], case["hidden"], case["cout"], case["alpha"]
    S = _Slices(dev, fill=float("nan"))
    xd = x.bfloat16().to(dev).contiguous() if bf else S.copy(x, off.get("x", 0), padded=True)
    W1, W2, b2, dyd = (S.copy(t, padded=True) for t in (inp["W1"], inp["W2"], inp["b2"], dy))
    b1 = S.copy(inp["b1"], off.get("b1", 0), padded=True)
    y = S.empty((n, cout), padded=True).fill_(UNTOUCHED)
    partials = torch.empty(L.fgc_mlp_num_partials(n), dtype=torch.float32, device=dev)
    dx = torch.empty(n, cin, dtype=torch.bfloat16, device=dev) if bf else S.empty((n, cin), off.get("dx", 0), padded=True)
    dx.fill_(UNTOUCHED)
    grads = [S.empty(tuple(t.shape), padded=True).fill_(UNTOUCHED) for t in (W1, b1, W2, b2)]
    fwd_bytes = (L.fgc_mlp_bf16_workspace_bytes if bf else L.fgc_mlp_workspace_bytes)(cin, hidden, cout)
    bwd_bytes = (L.fgc_mlp_bwd_bf16_workspace_bytes if bf else L.fgc_mlp_bwd_workspace_bytes)(n, cin, hidden, cout)
    fwd_entry, bwd_entry = (L.fgc_mlp_fwd_bf16, L.fgc_mlp_bwd_bf16) if bf else (L.fgc_mlp_fwd, L.fgc_mlp_bwd)
    st = stream_ptr()

    def call(flags, wsf, wsb):
        rc_f = fwd_entry(ptr(xd), n, cin, hidden, cout, ptr(W1), ptr(b1), ptr(W2), ptr(b2), alpha, ptr(y), ptr(partials), flags,
                         ptr(wsf), wsf.numel(), st)
        rc_b = bwd_entry(ptr(xd), ptr(dyd), n, cin, hidden, cout, ptr(W1), ptr(b1), ptr(W2), alpha, ptr(dx), ptr(grads[0]),
                         ptr(grads[1]), ptr(grads[2]), ptr(grads[3]), flags, ptr(wsb), wsb.numel(), st)
        torch.cuda.synchronize()
        return rc_f, rc_b

    wsf, wsb = _workspace(fwd_bytes, off.get("ws", 0), dev), _workspace(bwd_bytes, off.get("ws", 0), dev)
    # which form will run: asked with the pointers the launches get
    forms = _lib.mlp_forms(n, cin, hidden, cout, bf, x=xd.data_ptr(), dx=dx.data_ptr(), b1=b1.data_ptr(), fwd_ws=wsf.data_ptr(),
                           bwd_ws=wsb.data_ptr())
    if check_expect:
        missed = {k: (v, forms.get(k)) for k, v in case["expect"].items() if forms.get(k) != v}
        assert not missed, "%s: (expected, got) %s in %s" % (case["name"], missed, forms)
    rc_f, rc_b = call(0, wsf, wsb)
    out = dict(forms=forms, partials=partials.cpu())
    if forms["fwd"] == "none":
        assert rc_f == -22, rc_f
        assert bool((y == UNTOUCHED).all()), "a refused forward call wrote y"
        out["y"] = None
    else:
        check(rc_f, "fgc_mlp_fwd")
        out["y"] = y.cpu()
    if forms["bwd"] == "none":
        assert rc_b == -22, rc_b
        assert all(bool((t == UNTOUCHED).all()) for t in [dx] + grads), "a refused backward call wrote a gradient"
        out.update({k: None for k in GRADS})
    else:
        check(rc_b, "fgc_mlp_bwd")
        out.update({k: t.float().cpu() for k, t in zip(GRADS, [dx] + grads)})
    if case["packed"]:
        # the same two calls on operands packed ahead by fgc_conv_pack, the layout id in the flags: bit for bit
        lid = L.fgc_mlp_layout_id(cin, hidden, cout, int(bf))
        assert int(forms["layout"]) == lid
        pf, pb = _workspace(fwd_bytes, 0, dev), _workspace(bwd_bytes, 0, dev)
        ex = _lib.PackExtra(mlp_bf16=int(bf), mlp_W1=ptr(W1), mlp_W2=ptr(W2), mlp_n=n, mlp_cin=cin, mlp_hidden=hidden, mlp_cout=cout,
                            mlp_fwd_ws=ptr(pf) if forms["fwd"] != "none" else None, mlp_bwd_ws=ptr(pb) if forms["bwd"] != "none" else None)
        check(L.fgc_conv_pack(None, None, None, None, 0, C.byref(ex), st), "fgc_conv_pack")
        for t in [y, dx] + grads:
            t.fill_(UNTOUCHED)
        rc_f, rc_b = call(_lib.MLP_PACKED | _lib.mlp_layout(lid), pf, pb)
        assert rc_f == (-22 if forms["fwd"] == "none" else 0) and rc_b == (-22 if forms["bwd"] == "none" else 0), (rc_f, rc_b)
        if out["y"] is not None:
            assert torch.equal(y.cpu(), out["y"]), "packed forward differs from self-packed"
        if out["dx"] is not None:
            for k, t in zip(GRADS, [dx] + grads):
                assert torch.equal(t.float().cpu(), out[k]), "packed backward differs from self-packed in " + k
    S.check()
    return out


def _rel(got, ref, by_row=False):
    """max|got - ref| / max|ref| (by_row: the largest such ratio of a row), and the scale"""
    err = (got.double() - ref).abs()
    if by_row:
        return (err.amax(1) / ref.abs().amax(1)).max().item(), ref.abs().max().item()
    scale = ref.abs().max().item()
    return err.max().item() / scale if scale > 0 else err.max().item(), scale


def _kink_resolved(case, got, amb):
    """A copy of the float64 gradients moved to the slopes `got` took at the ambiguous units."""
    r64, inp = T.reference(case, torch.float64), T.inputs(case)
    ref = {k: r64[k].clone() for k in GRADS}
    if amb:
        h, alpha = r64["h"], case["alpha"]
        slope = torch.where(h > 0, torch.ones_like(h), torch.full_like(h, alpha))
        g = inp["dy"].double() @ inp["W2"].double().t()
        moved = mlp_kink.resolve(ref, {k: got[k].double() for k in GRADS}, amb, g, slope, inp["x"].double(), inp["W1"].double(),
                                 alpha=alpha, max_units=40, max_per_col=6)
        print("%s: %d pre-activations within 1e-6 of zero, moved %s" % (case["name"], len(amb), moved))
    return ref


@pytest.mark.parametrize("name", T.NAMES)
def test_mlp_form_against_float64(name):
    from facet_graph_convolution_amd import _lib
    case = T.BY_NAME[name]
    dev = torch.device("cuda:0")
    bf, n = case["dtype"] == "bf16", case["n"]
    with _lib.options(**case["options"]):
        out = _mlp_fwd_bwd(case, dev)
        forms = out["forms"]
        print("%s: %s" % (name, " ".join("%s=%s" % kv for kv in forms.items())))
        r64, r32 = T.reference(case, torch.float64), T.reference(case, torch.float32)
        by_row = case["inputs"] == "scaled"
        failed = []

        def judge(k, got, ref, got32, rows=False):
            e, scale = _rel(got, ref, rows)
            e32, _ = _rel(got32, ref, rows)
            print("MLP_E %s %s e %.3e e32 %.3e scale %.3e" % (name, k, e, e32, scale))
            if bf:
                tol = 1e-5 / scale if k == "y" else BF16_TOL[k]        # (y: 1e-5 absolute)
                if not e < tol:
                    failed.append(("bf16", k, e, tol))
                return
            if not rows and not e * scale < (3e-6 if k == "y" else 5e-6) * max(1.0, scale):
                failed.append(("a", k, e * scale, scale))
            if not e <= MARGIN * max(e32, FLOOR):
                failed.append(("b", k, e, e32))

        if out["y"] is not None:
            judge("y", out["y"], r64["y"], r32["y"], by_row)
            if by_row:
                judge("y", out["y"], r64["y"], r32["y"])
            want = r64["y"].abs().sum(1).split(64)
            assert len(want) == out["partials"].numel()
            for i, w in enumerate(want):
                assert abs(out["partials"][i].item() - w.sum().item()) < 1e-4 * w.sum().item(), ("partial", i)
        if out["dx"] is not None:
            amb = T.ambiguous(case)
            assert n > 133 or not amb
            ref = _kink_resolved(case, out, amb)
            ref32 = _kink_resolved(case, r32, amb) if amb else ref       # (torch float32 at the kink: its own decisions)
            for k in GRADS:
                g32 = r32[k].double() - (ref32[k] - ref[k])              # float32's distance to ITS resolved reference
                judge(k, out[k], ref[k], g32, by_row and k == "dx")
                if by_row and k == "dx":
                    judge(k, out[k], ref[k], g32)
            if case["inputs"] == "zeros":
                # the zero rows alone: every one of their zero-bias units has slope 0, so db1 there is exactly zero (and dW1 is
                # zero everywhere: x is); their dx as in the whole call's reference
                rows = list(T.ZERO_ROWS)
                z = _mlp_fwd_bwd(case, dev, x=T.inputs(case)["x"][rows], dy=T.inputs(case)["dy"][rows], check_expect=False)
                assert bool((z["db1"][list(T.ZERO_COLS)] == 0).all()), ("slope at an exact zero", z["db1"][list(T.ZERO_COLS)])
                assert bool((z["dW1"] == 0).all())
                e, _ = _rel(z["dx"], r64["dx"][rows])
                assert e < (BF16_TOL["dx"] if bf else 5e-6), ("dx of the zero rows", e)
                e, _ = _rel(out["dx"][rows], r64["dx"][rows])
                assert e < (BF16_TOL["dx"] if bf else 5e-6), ("dx of the zero rows in the whole call", e)
        # the call in two parts: no row lost, none counted twice, none that depends on its tile's place
        if out["dx"] is not None and ((bf and n >= 33) or n == 4097) and not case["off"]:
            for k in (32, 4096):
                if k >= n:
                    continue
                parts = [_mlp_fwd_bwd(case, dev, rows=r, check_expect=False) for r in ((0, k), (k, n))]
                assert torch.equal(torch.cat([p["y"] for p in parts]), out["y"]), ("y rows depend on the tile's place", k)
                assert torch.equal(torch.cat([p["dx"] for p in parts]), out["dx"]), ("dx rows depend on the tile's place", k)
                for g in GRADS[1:]:
                    whole, total = out[g].double(), parts[0][g].double() + parts[1][g].double()
                    err, scale = (whole - total).abs().max().item(), whole.abs().max().item()
                    print("MLP_PARTS %s %s k %d |whole - parts| %.3e scale %.3e" % (name, g, k, err, scale))
                    if not err < 5e-6 * max(1.0, scale):
                        failed.append(("parts", g, k, err, scale))
        assert not failed, (name, failed)
