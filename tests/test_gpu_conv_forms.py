"""Every fp32 form of the graph-convolution kernels, one layer at a time, against float64 - and proof of which form ran.

tests/conv_form_cases.py lists ~125 layers (widths, graphs, node counts, call modes, pointer alignments, one developer option
flipped per descriptor).  For each, one helper drives the C ABI directly: it asks fgc_conv_forms (with the REAL pointers) which
kernel form every launch will take and asserts the keys the case exists to reach, runs fgc_conv_fwd + fgc_conv_bwd, and
compares with oracle/model_ref.custom_conv2d in float64 through autograd (concat / upsampling / pooling materialised;
accumulate modes add the reference gradient to the pre-fill).

Bounds:
 (a) the project's kernel tolerances (tests/test_gpu_conv.py): |y - y64| < 2e-6 max(1, max|y64|), every gradient within
     5e-6 max(1, max|g64|).
 (b) no floor of 1: e = max|g - g64| / max|g64| <= 8 max(e32, 2^-22), where e32 is the same measure of the torch float32
     oracle on the same inputs (a different summation order over up to 24 edges x 1100 nodes earns a factor of 8 and no more;
     2^-22 = four ulps of the largest entry, for where the float32 oracle happens to land exactly).
The leaky-ReLU kink: the backward reads lrelu' from the stored y, so the oracle is given the kernel's own slopes
where(y_gpu > 0, 1, alpha); y itself is checked against lrelu(pre64), and every element whose sign differs from float64's
must have |pre64| < 1e-6, at most 4 per case.  Offset tensors are slices of larger pre-filled tensors whose surroundings
must come back unchanged.  Measured e / e32 per form: DESIGN.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_form_cases as T

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
PAD = 64                # floats in front of and behind an offset tensor
FLOOR = 2.0 ** -22
MARGIN = 8.0
GRAD_NAMES = ["dx0", "dx1", "dW0", "db", "du", "dc", "dv"]

_GRAPHS = {}
RESULTS = {}            # case name -> {tensor name: CPU tensor}: an option-flipped case prints its distance to the default form


def _graph(case, dev):
    from facet_graph_convolution_amd.graph import FacetGraph
    key = (case["graph"], case["n"])
    if key not in _GRAPHS:
        _GRAPHS[key] = FacetGraph(T.klist(*key), dev)
        _GRAPHS[key].transposed()
    return _GRAPHS[key]


class _Slices:
    """Device tensors at a byte offset from 16-byte alignment: slices of larger tensors filled with a sentinel (`fill`; NaN makes
    a value read from the surroundings show in whatever it is multiplied into, zero included).  padded: surroundings even at
    offset 0.  dtype: the element type (bf16 tensors of FGC_CONV_BF16 storage; PAD counts elements, the fill is rounded to the
    type).  (Shared with tests/test_gpu_mlp_forms.py and tests/test_gpu_conv_forms_bf16.py.)"""

    def __init__(self, dev, fill=SENTINEL):
        self.dev, self.made, self.fill = dev, [], fill

    def empty(self, shape, off_bytes=0, padded=False, dtype=torch.float32):
        if not off_bytes and not padded:
            return torch.empty(*shape, dtype=dtype, device=self.dev)
        numel = int(np.prod(shape))
        base = torch.empty(numel + 2 * PAD, dtype=dtype, device=self.dev)
        base.fill_(self.fill)
        start = PAD + off_bytes // base.element_size()
        view = base[start:start + numel].view(*shape)
        assert view.data_ptr() % 16 == off_bytes % 16
        self.made.append((base, start, numel))
        return view

    def copy(self, t, off_bytes=0, padded=False, dtype=torch.float32):
        return self.empty(tuple(t.shape), off_bytes, padded, dtype).copy_(t)

    def check(self):
        same = lambda t: bool((t == torch.tensor(self.fill, dtype=t.dtype, device=t.device)).all())
        untouched = (lambda t: bool(torch.isnan(t).all())) if self.fill != self.fill else same
        for base, start, numel in self.made:
            assert untouched(base[:start]) and untouched(base[start + numel:]), "the surroundings of an offset tensor were written"


def _fp32_conv_fwd_bwd(case, dev):
    """One fp32 conv layer straight through the C ABI.  Returns (forms, y, y_pool, {gradient name: tensor})."""
    from facet_graph_convolution_amd import _lib, ops
    from facet_graph_convolution_amd._lib import ConvBwdIO, AG_LD, DL_LD, FGC_M, ptr, stream_ptr, check
    L = _lib.lib()
    g = _graph(case, dev)
    inp, off, mode = T.inputs(case), case["off"], case["mode"]
    n, cout, c1 = case["n"], case["cout"], case["c1"]
    S = _Slices(dev)
    x0 = S.copy(inp["x0"], off.get("x0", 0))
    x1 = S.copy(inp["x1"]) if c1 else None
    params = [S.copy(p) for p in inp["params"]]
    dy = S.copy(inp["dy"], off.get("dy", 0))
    d = ops.make_conv_desc(g, x0, x1, case["shift"], params, case["bias_mask"], case["act"], T.ALPHA)
    over = None
    if case["options"]:          # per-descriptor library options (fgc_conv_desc.options): this layer only
        over = _lib.option_overrides(**case["options"])
        d.options, d.n_options = C.addressof(over), len(over)
    ag = torch.empty(x0.shape[0], AG_LD, dtype=torch.float32, device=dev)
    y = S.empty((n, cout), off.get("y", 0))
    pool = "pool" in mode
    y_pool = torch.empty(n // 4, cout, dtype=torch.float32, device=dev) if pool else None
    trow, tcol, tedge = g.transposed()
    io = ConvBwdIO()
    io.trowptr, io.tcol, io.tedge = trow.data_ptr(), tcol.data_ptr(), tedge.data_ptr()
    io.max_in_deg = g.max_in_deg
    ds = S.empty((n, cout), off.get("ds", 0))
    dl = torch.empty(max(g.nnz, 1), DL_LD, dtype=torch.float32, device=dev)
    dag = torch.empty(n, AG_LD, dtype=torch.float32, device=dev)
    r = S.empty((n, FGC_M * cout + 24), off.get("r", 0))
    grads = [torch.empty_like(p) for p in params]
    want_dx = "nodx" not in mode
    dx0 = (S.copy(inp["dx0_fill"]) if "dx0_fill" in inp else torch.empty_like(x0)) if want_dx else None
    dx1 = (S.copy(inp["dx1_fill"]) if "dx1_fill" in inp else torch.empty_like(x1)) if (want_dx and c1) else None
    io.ag, io.y, io.dy = ag.data_ptr(), y.data_ptr(), dy.data_ptr()
    io.ds, io.dl, io.dag, io.r = ds.data_ptr(), dl.data_ptr(), dag.data_ptr(), r.data_ptr()
    io.dx0, io.dx1 = (dx0.data_ptr() if dx0 is not None else None), (dx1.data_ptr() if dx1 is not None else None)
    io.accumulate0, io.accumulate1 = int("dx0_fill" in inp), int("dx1_fill" in inp)
    io.dW0, io.db, io.du, io.dc, io.dv = [t.data_ptr() for t in grads]
    if pool:
        pool_dy = S.copy(inp["pool_dy"])
        io.pool_y, io.pool_dy = y_pool.data_ptr(), pool_dy.data_ptr()
    # which form will run: asked with the pointers the launches get
    forms = _lib.conv_forms(d, io)
    missed = {k: (v, forms.get(k)) for k, v in case["expect"].items() if forms.get(k) != v}
    assert not missed, "%s: (expected, got) %s in %s" % (case["name"], missed, forms)
    ws = torch.empty(L.fgc_conv_workspace_bytes(C.byref(d)) + 256, dtype=torch.uint8, device=dev)
    check(L.fgc_conv_fwd(C.byref(d), ptr(ag), ptr(y), ptr(y_pool), ptr(ws), ws.numel(), stream_ptr()), "fgc_conv_fwd")
    wsb = torch.empty(L.fgc_conv_bwd_workspace_bytes(C.byref(d)) + 256, dtype=torch.uint8, device=dev)
    check(L.fgc_conv_bwd(C.byref(d), C.byref(io), ptr(wsb), wsb.numel(), stream_ptr()), "fgc_conv_bwd")
    torch.cuda.synchronize()
    S.check()
    out = dict(zip(["dW0", "db", "du", "dc", "dv"], grads))
    if dx0 is not None:
        out["dx0"] = dx0
    if dx1 is not None:
        out["dx1"] = dx1
    return forms, y, y_pool, out


@pytest.mark.parametrize("name", T.NAMES)
def test_conv_form_against_float64(name):
    from oracle import model_ref as R
    case = T.BY_NAME[name]
    dev = torch.device("cuda:0")
    forms, y, y_pool, grads = _fp32_conv_fwd_bwd(case, dev)
    y = y.cpu()
    pre64 = T.preactivation(case, torch.float64)
    y64 = R.lrelu(pre64, T.ALPHA) if case["act"] else pre64
    err_y = (y.double() - y64).abs().max().item()
    print("%s: %s" % (name, " ".join("%s=%s" % kv for kv in forms.items())))
    print("%s: y |gpu-f64| %.2e (max|y64| %.2f)" % (name, err_y, y64.abs().max().item()))
    assert err_y < 2e-6 * max(1.0, y64.abs().max().item())
    if y_pool is not None:
        yp64 = R.custom_binary_tree_pooling(y64[None], 2)[0]
        assert (y_pool.cpu().double() - yp64).abs().max().item() < 2e-6 * max(1.0, yp64.abs().max().item())
    slope = None
    if case["act"]:
        count, worst = T.sign_flips(y, pre64)
        print("%s: %d signs differ from float64, largest |pre64| there %.2e" % (name, count, worst))
        assert count <= 4 and worst < 1e-6
        slope = T.slopes_of(y)
    g64, g32 = T.oracle_grads(case, torch.float64, slope), T.oracle_grads(case, torch.float32, slope)
    got = {k: v.cpu() for k, v in grads.items()}
    RESULTS[name] = dict(got, y=y)
    sib = T.default_sibling(case)
    failed = []
    for k in GRAD_NAMES:
        if k not in got:
            continue
        ref = g64[k].reshape(got[k].shape)
        scale = ref.abs().max().item()
        err = (got[k].double() - ref).abs().max().item()
        err32 = (g32[k].reshape(got[k].shape).double() - ref).abs().max().item()
        e, e32 = (err / scale, err32 / scale) if scale > 0 else (err, err32)
        line = "FORM_E %s %s e %.3e e32 %.3e scale %.3e" % (name, k, e, e32, scale)
        if sib is not None and sib["name"] in RESULTS:
            line += " |this-default| %.3e" % (got[k] - RESULTS[sib["name"]][k]).abs().max().item()
        print(line)
        if not err < 5e-6 * max(1.0, scale):
            failed.append(("a", k, err, scale))
        if not e <= MARGIN * max(e32, FLOOR):
            failed.append(("b", k, e, e32))
    assert not failed, (name, failed)
