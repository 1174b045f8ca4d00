"""The streaming weight-gradient GEMM (csrc/fgc_gemm_tn.hip: gemm_tn_stream_kernel<2> / <4> and their grouped forms) against
the plain form of the same GEMM, bit for bit, and against float64.

Every layer of CASES runs twice through fgc_conv_fwd + fgc_conv_bwd on the same inputs and pointers: on its own options
(fgc_conv_forms must say k3 = stream2 / stream4) and with the per-descriptor override NO_TNSTREAM = 1 (k3 = plain_v4).  The
two forms multiply the same products and add them in the same order - within a wave, across the four waves of a workgroup
and across slabs -, so dW0, du and dv must be EQUAL (torch.equal), and both are held to the float64 oracle at the bounds of
tests/test_gpu_conv_forms.py: (a) |g - g64| < 5e-6 max(1, max|g64|), (b) max|g - g64| / max|g64| <= 8 max(e32, 2^-22) with
e32 the same measure of the torch float32 oracle.  (Run once on the kernels as they were before the streaming body took its
operands through buffer descriptors: every case was equal there too, so every case keeps its equality half.)

What the cases are for:
  32->32 (two columns per lane, P = 312), 64->32, 128->64 (P = 600: ten row tiles of the product, the last one partial);
  64+32->48 (two sources, P = 456, the second column tile ends inside the tile) and 32+64->64 (the concat boundary in the
  middle of a column tile: its two halves come from different tensors); 48+16->32 (a boundary that no 32-column half can
  follow: the workgroups fall back to the clamped-pointer body inside the same kernel); a 4x-upsampled source (shift = 2);
  37 nodes (one slab, shorter than one unrolled pass of a wave: three of the four operand sets start past the end), 404,
  1101 = 4 * 275 + 1 (the last k-step holds one valid row, the last slab is short);
  r 16 bytes into a sentinel-filled tensor (the rows past the end of the last slab ARE the sentinel: a descriptor that ends
  late multiplies it into the sums; the surroundings must also come back untouched);
  TN_SLOTS = 8 at 1101 nodes.
One more test sends two layers of different shapes through the GROUPED launch (FGC_CONV_DEFER_DW + fgc_conv_bwd_reduce) and
compares with the same layers launched on their own."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_form_cases as T

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
PAD = 64
FLOOR = 2.0 ** -22
MARGIN = 8.0
TN_GRADS = ("dW0", "du", "dv")


def _layer(name, n, cin, cout, shift=0, options=None, off=None, k3="stream4", seed=0):
    c0, c1 = cin if isinstance(cin, tuple) else (cin, 0)
    return dict(name=name, graph="reg", n=n, c0=c0, c1=c1, shift=shift, cout=cout, act=1, bias_mask=1, mode="dx",
                options=dict(options or {}), off=dict(off or {}), expect=dict(k3=k3), seed=seed)


CASES = [
    _layer("w32_32", 404, 32, 32, k3="stream2"),
    _layer("w64_32", 404, 64, 32),
    _layer("w128_64", 404, 128, 64),
    _layer("concat_64+32_48", 404, (64, 32), 48),
    _layer("concat_32+64_64", 404, (32, 64), 64),
    _layer("concat_48+16_32", 404, (48, 16), 32),
    _layer("up_64_32", 404, 64, 32, shift=2),
    _layer("n37_32_32", 37, 32, 32, k3="stream2"),
    _layer("n37_64_32", 37, 64, 32),
    _layer("n1101_32_32", 1101, 32, 32, k3="stream2"),
    _layer("n1101_128_64_r16", 1101, 128, 64, off=dict(r=16)),
    _layer("r16_64_32", 404, 64, 32, off=dict(r=16)),
    _layer("r16_32_32", 404, 32, 32, off=dict(r=16), k3="stream2"),
    _layer("slots8_n1101_32_32", 1101, 32, 32, options=dict(TN_SLOTS=8), k3="stream2"),
    _layer("slots8_n1101_64_32", 1101, 64, 32, options=dict(TN_SLOTS=8)),
]
BY_NAME = {c["name"]: c for c in CASES}

_GRAPHS = {}


def _graph(case, dev):
    from facet_graph_convolution_amd.graph import FacetGraph
    key = (case["graph"], case["n"])
    if key not in _GRAPHS:
        _GRAPHS[key] = FacetGraph(T.klist(*key), dev)
        _GRAPHS[key].transposed()
    return _GRAPHS[key]


class _Layer:
    """One fp32 conv layer bound to device tensors, as tests/test_gpu_conv_forms.py binds it; r (and whatever else the case
    offsets) is a slice of a sentinel-filled tensor.  run(flags) = fgc_conv_fwd + fgc_conv_bwd."""

    def __init__(self, case, dev, options):
        from facet_graph_convolution_amd import _lib, ops
        from facet_graph_convolution_amd._lib import ConvBwdIO, AG_LD, DL_LD, FGC_M
        self.case, self.L, self.made = case, _lib.lib(), []
        g = _graph(case, dev)
        inp, off = T.inputs(case), case["off"]
        n, cout, c1 = case["n"], case["cout"], case["c1"]
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        self.x0 = inp["x0"].to(dev)
        self.x1 = inp["x1"].to(dev) if c1 else None
        self.params = [p.to(dev) for p in inp["params"]]
        self.dy = inp["dy"].to(dev)
        self.d = d = ops.make_conv_desc(g, self.x0, self.x1, case["shift"], self.params, case["bias_mask"], case["act"], T.ALPHA)
        self.over = None
        if options:
            self.over = _lib.option_overrides(**options)
            d.options, d.n_options = C.addressof(self.over), len(self.over)
        self.ag, self.y = f(self.x0.shape[0], AG_LD), f(n, cout)
        trow, tcol, tedge = g.transposed()
        self.io = io = ConvBwdIO()
        io.trowptr, io.tcol, io.tedge = trow.data_ptr(), tcol.data_ptr(), tedge.data_ptr()
        io.max_in_deg = g.max_in_deg
        self.ds, self.dl, self.dag = f(n, cout), f(max(g.nnz, 1), DL_LD), f(n, AG_LD)
        self.r = self._slice((n, FGC_M * cout + 24), off.get("r", 0), dev)
        self.grads = [torch.zeros_like(p) for p in self.params]
        self.dx0 = torch.empty_like(self.x0)
        self.dx1 = torch.empty_like(self.x1) if c1 else None
        io.ag, io.y, io.dy = self.ag.data_ptr(), self.y.data_ptr(), self.dy.data_ptr()
        io.ds, io.dl, io.dag, io.r = self.ds.data_ptr(), self.dl.data_ptr(), self.dag.data_ptr(), self.r.data_ptr()
        io.dx0, io.dx1 = self.dx0.data_ptr(), (self.dx1.data_ptr() if c1 else None)
        io.dW0, io.db, io.du, io.dc, io.dv = [t.data_ptr() for t in self.grads]
        self.forms = _lib.conv_forms(d, io)
        self.ws = torch.empty(self.L.fgc_conv_workspace_bytes(C.byref(d)) + 256, dtype=torch.uint8, device=dev)
        self.wsb = torch.empty(self.L.fgc_conv_bwd_workspace_bytes(C.byref(d)) + 256, dtype=torch.uint8, device=dev)

    def _slice(self, shape, off_bytes, dev):
        numel = int(np.prod(shape))
        base = torch.full((numel + 2 * PAD,), SENTINEL, dtype=torch.float32, device=dev)
        start = PAD + off_bytes // 4
        view = base[start:start + numel].view(*shape)
        assert view.data_ptr() % 16 == off_bytes % 16
        self.made.append((base, start, numel))
        return view

    def run(self, flags=0):
        from facet_graph_convolution_amd._lib import ptr, stream_ptr, check
        L, d = self.L, self.d
        check(L.fgc_conv_fwd(C.byref(d), ptr(self.ag), ptr(self.y), None, ptr(self.ws), self.ws.numel(), stream_ptr()), "fgc_conv_fwd")
        self.io.flags = flags
        check(L.fgc_conv_bwd(C.byref(d), C.byref(self.io), ptr(self.wsb), self.wsb.numel(), stream_ptr()), "fgc_conv_bwd")
        return self

    def results(self):
        torch.cuda.synchronize()
        for base, start, numel in self.made:
            assert bool((base[:start] == SENTINEL).all()) and bool((base[start + numel:] == SENTINEL).all()), \
                "the surroundings of r were written"
        out = {k: v.cpu() for k, v in zip(["dW0", "db", "du", "dc", "dv"], self.grads)}
        out["y"] = self.y.cpu()
        return out


def _hold_to_float64(name, case, got):
    slope = T.slopes_of(got["y"])
    g64, g32 = T.oracle_grads(case, torch.float64, slope), T.oracle_grads(case, torch.float32, slope)
    failed = []
    for k in TN_GRADS:
        ref = g64[k].reshape(got[k].shape)
        scale = ref.abs().max().item()
        err = (got[k].double() - ref).abs().max().item()
        err32 = (g32[k].reshape(got[k].shape).double() - ref).abs().max().item()
        e, e32 = (err / scale, err32 / scale) if scale > 0 else (err, err32)
        print("TN_E %s %s e %.3e e32 %.3e scale %.3e" % (name, k, e, e32, scale))
        if not err < 5e-6 * max(1.0, scale):
            failed.append(("a", k, err, scale))
        if not e <= MARGIN * max(e32, FLOOR):
            failed.append(("b", k, e, e32))
    assert not failed, (name, failed)


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_stream_form_equals_the_plain_form_bit_for_bit(name):
    case = BY_NAME[name]
    dev = torch.device("cuda:0")
    stream = _Layer(case, dev, case["options"])
    assert stream.forms["k3"] == case["expect"]["k3"], stream.forms
    plain = _Layer(case, dev, dict(case["options"], NO_TNSTREAM=1))
    assert plain.forms["k3"] == "plain_v4", plain.forms
    assert (stream.forms["k3_slabs"], stream.forms["k3_rows"]) == (plain.forms["k3_slabs"], plain.forms["k3_rows"])
    print("%s: k3 %s, %s slabs of %s rows" % (name, stream.forms["k3"], stream.forms["k3_slabs"], stream.forms["k3_rows"]))
    a, b = stream.run().results(), plain.run().results()
    assert torch.equal(a["y"], b["y"])
    unequal = {k: (a[k] - b[k]).abs().max().item() for k in TN_GRADS if not torch.equal(a[k], b[k])}
    _hold_to_float64(name + "/stream", case, a)
    _hold_to_float64(name + "/plain", case, b)
    assert not unequal, "%s: stream and plain forms differ (max |difference|): %s" % (name, unequal)


def test_grouped_launch_equals_the_per_layer_launches_bit_for_bit():
    """Two stream4 layers of different shapes and one stream2 layer: with FGC_CONV_DEFER_REDUCE | FGC_CONV_DEFER_DW stage 8
    launches no GEMM, and fgc_conv_bwd_reduce runs the deferred GEMMs as jobs of one launch per kernel form (each layer keeps
    its own r until then)."""
    from facet_graph_convolution_amd import _lib
    from facet_graph_convolution_amd._lib import ConvDesc, ConvBwdIO, stream_ptr, check
    dev = torch.device("cuda:0")
    names = ["w64_32", "n1101_128_64_r16", "concat_32+64_64", "n1101_32_32", "n37_32_32"]
    alone = [_Layer(BY_NAME[k], dev, None).run().results() for k in names]
    layers = [_Layer(BY_NAME[k], dev, None) for k in names]
    assert [l.forms["k3"] for l in layers] == ["stream4", "stream4", "stream4", "stream2", "stream2"]
    for l in layers:
        l.run(_lib.CONV_DEFER_REDUCE | _lib.CONV_DEFER_DW)
    nl = len(layers)
    descs = (C.POINTER(ConvDesc) * nl)(*[C.pointer(l.d) for l in layers])
    ios = (C.POINTER(ConvBwdIO) * nl)(*[C.pointer(l.io) for l in layers])
    wsb = (C.c_void_p * nl)(*[l.wsb.data_ptr() for l in layers])
    check(_lib.lib().fgc_conv_bwd_reduce(descs, ios, wsb, nl, stream_ptr()), "fgc_conv_bwd_reduce")
    for k, l, ref in zip(names, layers, alone):
        got = l.results()
        for g in ("dW0", "db", "du", "dc", "dv"):
            assert torch.equal(got[g], ref[g]), (k, g, (got[g] - ref[g]).abs().max().item())
        assert got["dW0"].abs().max().item() > 0
