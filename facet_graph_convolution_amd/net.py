"""FacetDenoiser: the reference's 3-level graph U-Net + per-facet MLP, hand-scheduled on libfgc.

Replaces, for one mesh / patch (batch size is 1 in the reference, train.py:405):
  * ``get_model_reg_multi_scale``  (model.py:837-946)        -> ``forward``
  * ``normalizeTensor``            (utils.py:1700-1715)      -> fused after the MLP
  * the training objective         (train.py:439-451,503-520) -> ``loss_and_grad`` / ``train_step``
  * the inference epilogue         (train.py:115-121,136)    -> ``infer_normals``

Design (MI355X-first, nothing traced or compiled at run time):
  * every activation, gradient and scratch buffer of a mesh lives in HBM for the whole run and is
    allocated ONCE per mesh size (a 100k-facet mesh needs ~0.7 GB of 288 GB);
  * parameters, gradients and Adam moments are three flat fp32 buffers (16-byte aligned views per
    variable, creation order of the reference), so Adam is one kernel and a data-parallel
    all-reduce is one RCCL call;
  * pooling, upsampling, concat and leaky-ReLU never exist as tensors of their own: they are
    address modes / epilogues of the conv kernels (see include/fgc.h);
  * the backward pass is scheduled by hand in a fixed order (no autograd tape, no float atomics):
    results are bitwise reproducible;
  * the whole forward+backward enqueue is capturable into a hipGraph (``capture=True``).
"""
import collections
import ctypes as C
import hashlib
import os
import types

import numpy as np
import torch

from . import _lib, ops, require_graph_replay_safe, schedule, shard, synth
from ._lib import ConvDesc, ConvBwdIO, AG_LD, DL_LD, FGC_M
from .graph import FacetGraph, as_graph
from .synth import NoiseSpec, SynthState
from .utils import direction_key

LRELU_ALPHA = 0.1      # model.py:846
STD_W, STD_B = 0.05, 0.01  # model.py:17-18
HIDDEN = 1024          # model.py:936
COST_SAMPLES = 4000    # train.py:411
POINT_SAMPLES = 500    # SAMP_NUM of trainAccuracyNet (train.py:653)
POINT_LOSS_THRESHOLD = 5000.0   # accuracyThreshold / compThreshold of fullLoss (train.py:1375-1376)
VERTEX_ITERS = (80, 20, 20)     # update_position_MS in trainAccuracyNet (train.py:776)


def param_spec(multi_scale=False, in_channels=6):
    """(kind, shape) per variable in the reference's creation order (model.py:430-433,447,767-768,855-941)."""
    M = FGC_M

    def conv(cin, cout):
        return [("weight", (M, cout, cin)), ("bias", (cout,)), ("assignment", (M, cin)), ("assignment", (M,)),
                ("assignment", (M, cin))]

    def lin(cin, cout):
        return [("weight", (cin, cout)), ("bias", (cout,))]

    spec = conv(in_channels, 32) + conv(32, 64) + conv(64, 128) + conv(128, 128)
    if multi_scale:
        spec += lin(128, HIDDEN) + lin(HIDDEN, 3)
    spec += conv(128, 64) + conv(128, 64)
    if multi_scale:
        spec += lin(64, HIDDEN) + lin(HIDDEN, 3)
    spec += conv(64, 32) + conv(64, 32) + lin(32, HIDDEN) + lin(HIDDEN, 3)
    return spec


class FlatParams:
    """All variables as 16-byte aligned views into one flat fp32 buffer (plus grad / Adam moment twins)."""

    def __init__(self, spec, device):
        self.spec = spec
        self.offsets = []
        off = 0
        for _, shape in spec:
            self.offsets.append(off)
            off += (int(np.prod(shape)) + 3) // 4 * 4
        self.total = off
        self.device = torch.device(device)
        self.theta = torch.zeros(off, dtype=torch.float32, device=self.device)
        # the gradient buffer has a 4-float tail: a facet-sharded step puts its loss sum there, so that one all-reduce
        # carries the gradient and the loss
        self.grad_ext = torch.zeros(off + 4, dtype=torch.float32, device=self.device)
        self.grad = self.grad_ext[:off]
        self.m = torch.zeros_like(self.theta)
        self.v = torch.zeros_like(self.theta)
        self.step = 0

    def _views(self, flat):
        return [flat[o:o + int(np.prod(s))].view(*s) for o, (_, s) in zip(self.offsets, self.spec)]

    @property
    def values(self):
        return self._views(self.theta)

    @property
    def grads(self):
        return self._views(self.grad)

    def init_random(self, seed=0):
        """N(0, 0.05^2) weights/assignments, N(0, 0.01^2) biases from RandomState(seed) in creation order."""
        rs = np.random.RandomState(seed)
        host = np.zeros(self.total, dtype=np.float32)
        for o, (kind, shape) in zip(self.offsets, self.spec):
            std = STD_B if kind == "bias" else STD_W
            host[o:o + int(np.prod(shape))] = rs.normal(0.0, std, size=shape).astype(np.float32).reshape(-1)
        self.theta.copy_(torch.from_numpy(host))

    def load(self, tensors):
        assert len(tensors) == len(self.spec)
        for view, t in zip(self.values, tensors):
            view.copy_(torch.as_tensor(t, dtype=torch.float32).reshape(view.shape))

    def num_parameters(self):
        return sum(int(np.prod(s)) for _, s in self.spec)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# One conv of the trunk (in forward order, model.py:858-931): level, inputs, 4x upsampling shift, output, pooled output,
# activation, width, and (per network) its first parameter slot
_ConvLayer = collections.namedtuple("_ConvLayer", "name level x0 x1 shift y pool act cout pidx", defaults=(None,))
TRUNK = (
    _ConvLayer("conv1", 0, "xr", None, 0, "h1", "p1", 1, 32),
    _ConvLayer("conv2", 1, "p1", None, 0, "h2", "p2", 1, 64),
    _ConvLayer("conv3", 2, "p2", None, 0, "h3", None, 1, 128),
    _ConvLayer("dconv3", 2, "h3", None, 0, "d3", None, 1, 128),
    _ConvLayer("upconv2", 1, "d3", None, 2, "u2", None, 0, 64),
    _ConvLayer("dconv2", 1, "u2", "h2", 0, "d2", None, 1, 64),
    _ConvLayer("upconv1", 0, "d2", None, 2, "u1", None, 0, 32),
    _ConvLayer("dconv1", 0, "u1", "h1", 0, "d1", None, 1, 32),
)
# What a layer's output feeds on OTHER ranks, as (level, tensor, parent rows) of schedule.rows: sent in one grouped exchange
# right behind the layer; the consumer - the next layer - waits for it between its interior and its boundary tiles
SEND_AFTER = {"conv1": ((0, "h1", False), (1, "p1", False)), "conv2": ((1, "h2", False), (2, "p2", False)),
              "conv3": ((2, "h3", False),), "dconv3": ((1, "d3", True),), "upconv2": ((1, "u2", False),),
              "dconv2": ((0, "d2", True),), "upconv1": ((0, "u1", False),)}


def r_ld(cout, r_pad, bf16):
    """Elements per row of a layer's backward aggregate r (include/fgc.h: FGC_CONV_R_PAD)."""
    return _lib.lib().fgc_conv_r_ld(cout, 1 if r_pad else 0, 1 if bf16 else 0)


def plan_grouped_dw(ns, dtype, pairs, mode, max_r_bytes, windowed, training, r_pad=True):
    """The layers (in forward order) whose weight-gradient GEMM waits for the grouped launch at the end of the backward
    pass (FGC_CONV_DEFER_DW); all but the first keep an `r` of their own until then.  ns: the level sizes [N0, N1, N2];
    mode "0" / "1": none / all, otherwise the layers whose `r` is at most max_r_bytes; windowed: a facet-sharded mesh with
    the weight-gradient stages in the next layer's exchange window (FacetDenoiser.dw_in_window).  Allocates nothing."""
    if mode == "0" or not training:
        return ()
    # (the first layer has no r to keep apart: its GEMM reads the saved aggregates and ds.)  Facet-sharded: a layer's GEMM
    # is what the NEXT layer's backward exchange hides behind, worth a collective's latency per layer - more than the ramp
    # and tail a grouped launch saves; only the first layer, which has no exchange, still waits for the grouped launch
    grouped = [TRUNK[0].name]
    for lay in ([] if windowed else TRUNK[1:]):
        cnt = ns[lay.level] * r_ld(lay.cout, r_pad, dtype == "bf16")
        # (a layer over a 4x-upsampled tensor runs on its n / 4 coarse rows - the pair form - unless refused)
        used = cnt // 4 if (lay.shift == 2 and pairs) else cnt
        if mode == "1" or used * (2 if dtype == "bf16" else 4) <= max_r_bytes:
            grouped.append(lay.name)
    return tuple(grouped)


class FacetDenoiser:
    def __init__(self, device="cuda", multi_scale=False, in_channels=6, seed=0, dtype="f32", options=None):
        if not torch.cuda.is_available():
            raise RuntimeError("FacetDenoiser needs an MI355X (no CPU fallback)")
        if dtype not in ("f32", "bf16"):
            raise ValueError("dtype must be 'f32' or 'bf16' (storage of the activations; weights stay fp32)")
        self.dtype = dtype
        self.L = _lib.lib()
        # entry points that differ between the fp32 and the bf16-storage network
        self._mlp_fwd, self._mlp_bwd, self._pool4_bwd = (getattr(self.L, name + ("_bf16" if dtype == "bf16" else ""))
                                                         for name in ("fgc_mlp_fwd", "fgc_mlp_bwd", "fgc_pool4_bwd"))
        # options: {name: value} of library options (fgc_option_name) that hold for THIS network's conv layers only - they
        # travel in every layer's descriptor (fgc_conv_desc.options), the process-level table (fgc_set_option) is not touched:
        # two networks in one process can run different kernel forms.  (The MLP entry points take no descriptor: their
        # options stay process-level.)
        self.option_overrides = _lib.option_overrides(**options) if options else None
        self.device = torch.device(device)
        self.multi_scale = multi_scale
        self.in_channels = in_channels
        self.params = FlatParams(param_spec(multi_scale, in_channels), self.device)
        self.params.init_random(seed)
        # the bound mesh's state - buffers, descriptors, the grouped-dw set, captured steps - and the states bind_cached keeps
        self._mesh = None
        self._mesh_cache = {}
        self.profile = False   # when True every enqueue is labelled for fgc_profile_collect
        self.comm = None       # exchange back end of a facet-sharded run (shard.DistComm)
        self.segment_nodes = []     # the node count of every schedule segment captured so far (_capture_segments)
        # facet-sharded runs: compute the interior tiles of a layer while its halo rows travel (FGC_NO_OVERLAP=1: the
        # whole layer after a blocking exchange, for A/B timing)
        self.overlap = os.environ.get("FGC_NO_OVERLAP", "0") != "1"
        # ... only where the interior is big enough to hide an exchange and to fill the GPU on its own: a layer of a
        # coarse level has a few hundred tiles in all, splitting it costs more than the exchange it would cover
        self.split_min_tiles = int(os.environ.get("FGC_SPLIT_MIN_TILES", "1024"))
        # ... and a layer's weight-gradient stage runs inside the NEXT layer's backward exchange window (_loss_backward_gen)
        self.dw_in_window = os.environ.get("FGC_NO_DW_IN_WINDOW", "0") != "1"
        # one launch packs the weight operands of all layers, one pair sums all parameter gradients (each small launch
        # costs ~5 us on an idle MI355X, and there were 37 of them per step); FGC_NO_BATCHED=1 = per-layer housekeeping
        self.batched = os.environ.get("FGC_NO_BATCHED", "0") != "1"
        self.step_prologue = os.environ.get("FGC_NO_STEP_PROLOGUE", "0") != "1"
        # The weight-gradient GEMMs of several layers in ONE launch per kernel form at the end of the backward pass
        # (FGC_CONV_DEFER_DW; a deferring layer keeps an `r` of its own until then).  bf16 storage: all layers - a layer's GEMM is
        # mostly ramp and tail there (100k facets: 1.095 -> 1.070 ms per step, 50k: 0.726 -> 0.705).  fp32: the GEMMs are
        # matrix-bound and grouping ALL of them loses the shared `r` whose lines stay in the Infinity Cache (1.761 -> 1.773 ms
        # at 100k facets), so a layer defers only if its `r` is small (grouped_dw_max_r_bytes, plan_grouped_dw decides per
        # mesh and layer): on a 100k-facet mesh the level-2 layers and the up-convolutions' coarse rows, on a mesh of 25k
        # facets or a shard of a strong-scaling run every layer - where a step is its launches, not its FLOPs.
        # FGC_GROUPED_DW=0 / 1: none / all (also on a facet-sharded mesh, which otherwise groups the first layer only).
        self.grouped_dw_mode = os.environ.get("FGC_GROUPED_DW", "1" if dtype == "bf16" else "auto") if self.batched else "0"
        self.grouped_dw_forced = "FGC_GROUPED_DW" in os.environ
        self.grouped_dw_max_r_bytes = int(os.environ.get("FGC_GROUPED_DW_MAX_R_MB", "40")) << 20
        self.save_z = os.environ.get("FGC_NO_SAVE_Z", "0") != "1"
        # rows of the backward aggregate r padded to whole 128-byte lines (include/fgc.h: FGC_CONV_R_PAD); FGC_NO_R_PAD=1: the
        # packed rows of M*cout + 24 elements
        self.r_pad = 0 if os.environ.get("FGC_NO_R_PAD", "0") == "1" else _lib.CONV_R_PAD
        # the gradient of the 4:1 max pooling behind conv1 / conv2 is a term of those layers' backward stage 1
        self.fused_pool = os.environ.get("FGC_NO_FUSED_POOL", "0") != "1"
        # the loss end of an unsharded training step (normalise, rotate the ground truth, sampled loss, both gradients) in
        # two launches instead of seven (fgc_loss_step); FGC_NO_FUSED_LOSS=1: the separate entry points
        self.fused_loss = os.environ.get("FGC_NO_FUSED_LOSS", "0") != "1"
        # the two up-convolutions on their coarse source rows (pair form, include/fgc.h); library option NO_PAIRS = 1
        # (fgc_set_option; initial value from FGC_NO_PAIRS): the fine form
        self.pairs = self._option("NO_PAIRS") != 1
        # parameter slots
        k = 0
        self.slot = {}
        for name in ["conv1", "conv2", "conv3", "dconv3"]:
            self.slot[name] = k
            k += 5
        if multi_scale:
            self.slot["head2"] = k
            k += 4
        for name in ["upconv2", "dconv2"]:
            self.slot[name] = k
            k += 5
        if multi_scale:
            self.slot["head1"] = k
            k += 4
        for name in ["upconv1", "dconv1"]:
            self.slot[name] = k
            k += 5
        self.slot["head0"] = k
        self.layers = [lay._replace(pidx=self.slot[lay.name]) for lay in TRUNK]

    # ------------------------------------------------------------------------------------------
    # mesh binding: graphs + every buffer, once
    # ------------------------------------------------------------------------------------------
    def bind_mesh(self, x, adjs, gt=None, plan=None, comm=None):
        """x: [1,N0,C] / [N0,C] features (float64 numpy as in in_list, or tensor); adjs: 3 K-lists or FacetGraphs;
        gt: [1,N0,3] ground-truth normals (training only).  Casts once (float64->float32, int64->int32 as the
        TF feed does, train.py:409-427).

        plan / comm (facet sharding, shard.py): x, adjs, gt are still the WHOLE mesh; this rank keeps only its
        shard ([owned rows | halo rows] per level) and exchanges halos through `comm` between the layers."""
        M = self._bind_inputs(x, adjs, plan, gt is not None)
        B = M["B"]
        B.update(self._bind_activations(M))
        scratch, M["grouped_dw_layers"] = self._bind_backward_scratch(M)
        B.update(scratch)
        B.update(self._bind_ground_truth(M, gt))
        layer_bufs, M["descs"], M["ios"], M["layer_flags"] = self._bind_layers(M)
        B.update(layer_bufs)
        self._bind_backward_wiring(M)
        mlp_bufs, M["arrays"] = self._bind_mlp_and_arrays(M)
        B.update(mlp_bufs)
        self._mesh = M
        self.comm = comm
        return self

    def _bind_inputs(self, x, adjs, plan, training):
        """A new mesh state: the graphs, the level sizes, the input rows and the per-step inputs."""
        dev = self.device
        xt = torch.as_tensor(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32))
        xt = xt.reshape(-1, xt.shape[-1]).contiguous()
        if xt.shape[1] != self.in_channels:
            raise ValueError("expected %d input channels" % self.in_channels)
        if plan is None:
            graphs = [as_graph(a, dev) for a in adjs]
            if len(graphs) != 3:
                raise ValueError("the network needs exactly 3 adjacency levels (model.py:858-931)")
            nh, nhp, n_total, own_lo = [0, 0, 0], [0, 0], [g.n for g in graphs], 0
        else:
            graphs = [shard.LocalGraph(P, dev) for P in plan.levels]
            nh = [g.n_halo for g in graphs]
            # tail rows of the coarse tensors read 4x-upsampled by the level above: one per UNIQUE parent of that level's
            # halo nodes (shard.ShardPlan)
            nhp = [graphs[0].pair.n_halo, graphs[1].pair.n_halo]
            n_total = list(plan.n_total)
            own_lo = plan.levels[0].lo
            xt = xt[torch.from_numpy(plan.local_rows(0))]
        n0, n1, n2 = ns = [g.n for g in graphs]
        if n0 != 4 * n1 or n1 != 4 * n2 or xt.shape[0] != n0 + nh[0]:
            raise ValueError("level sizes must be N0 = 4 N1 = 16 N2 and match x (got %d, %d, %d, x %d)" %
                             (n0, n1, n2, xt.shape[0]))
        B = {"x": xt.contiguous().to(dev)}
        B["xr"] = torch.empty_like(B["x"])
        self._alloc_step_inputs(B, COST_SAMPLES)
        # (captured: the mesh's captured steps by form - "angular", "points", "double" -, each (graph or segments, rotate);
        #  mode: what the mesh is bound for, written by the bind methods, read by the steps and the _require_* checks - clean:
        #  a synthesis state M["synth"]; verts: a vertex state M["verts"]; gt_normals: the double loss's ground truth in it;
        #  synth_points: the point sets come from fgc_point_sets_prepare)
        mode = types.SimpleNamespace(clean=False, verts=False, gt_normals=False, synth_points=False)
        return dict(graphs=graphs, B=B, ns=ns, nh=nh, nhp=nhp, has_gt=training, plan=plan, n_total=n_total,
                    own_lo=own_lo, captured={}, mode=mode)

    def _bind_activations(self, M):
        """Every activation and its gradient twin, the aggregate tables, and the heads' output and loss buffers."""
        (n0, n1, n2), nh, nhp = M["ns"], M["nh"], M["nhp"]
        f = dict(dtype=torch.float32, device=self.device)
        # rows: owned + the halo rows a consumer gathers (d3 / d2 are read 4x-upsampled by the level above, their tail
        # rows hold the parents of THAT level's halo nodes)
        shapes = {"h1": (n0 + nh[0], 32), "p1": (n1 + nh[1], 32), "h2": (n1 + nh[1], 64), "p2": (n2 + nh[2], 64),
                  "h3": (n2 + nh[2], 128), "d3": (n2 + nhp[1], 128), "u2": (n1 + nh[1], 64), "d2": (n1 + nhp[0], 64),
                  "u1": (n0 + nh[0], 32), "d1": (n0, 32), "y0": (n0, 3), "nconv": (n0, 3)}
        # dtype "bf16": every activation that crosses a layer boundary (and its gradient) is STORED as bf16; the network
        # input, the 3-channel outputs, logit tables, per-edge d-logits and all parameters stay fp32 (include/fgc.h:
        # FGC_CONV_BF16)
        act = dict(dtype=torch.bfloat16, device=self.device) if self.dtype == "bf16" else f
        B = {}
        for k, sh in shapes.items():
            kw = f if k in ("y0", "nconv") else act
            B[k] = torch.zeros(*sh, **kw)
            B["g_" + k] = torch.zeros(*sh, **kw)   # gradient twin
        rows = dict({k: sh[0] for k, sh in shapes.items()}, xr=M["B"]["xr"].shape[0])
        for lay in self.layers:
            B["ag_" + lay.name] = torch.empty(rows[lay.x0], AG_LD, **f)
        if self.multi_scale:
            for k, nk in (("1", n1), ("2", n2)):
                B["y" + k] = torch.empty(nk, 3, **f)
                B["nconv" + k] = torch.empty(nk, 3, **f)
                B["abs_part" + k] = torch.empty(self.L.fgc_mlp_num_partials(nk), **f)
                B["norm_scratch" + k] = torch.zeros(2 + self.L.fgc_norm_num_partials(nk), **f)
                if M["has_gt"] and M["plan"] is None:
                    B["g_y" + k] = torch.zeros(nk, 3, **f)
                    B["g_nconv" + k] = torch.zeros(nk, 3, **f)
                    B["loss" + k] = torch.zeros(2, **f)
        B["abs_part"] = torch.empty(self.L.fgc_mlp_num_partials(n0), **f)
        B["norm_scratch"] = torch.zeros(2 + self.L.fgc_norm_num_partials(n0), **f)
        B["loss"] = torch.zeros(2, **f)
        B["loss_gacc"] = torch.zeros(n0, 3, **f)     # scatter accumulator of the fused loss end (zero between steps)
        return B

    def _bind_backward_scratch(self, M):
        """The shared backward scratch and the own `r` of each deferring layer (plan_grouped_dw): (buffers, grouped set)."""
        ns, nh, graphs = M["ns"], M["nh"], M["graphs"]
        bf16, f = self.dtype == "bf16", dict(dtype=torch.float32, device=self.device)
        max_ds = max((ns[l.level] + nh[l.level]) * l.cout for l in self.layers)
        max_r = max(ns[l.level] * r_ld(l.cout, self.r_pad, bf16) for l in self.layers)
        if bf16:
            max_r = (max_r + 1) // 2           # (B["r"] is allocated in fp32 words)
        max_dl = max(max(g.nnz + getattr(g, "n_cross_in", 0) for g in graphs),
                     max((g.pair.n_pairs + g.pair.n_cross_in for g in graphs[:2] if getattr(g, "pair", None) is not None), default=0))
        B = {"ds": torch.zeros(max_ds, **f), "dl": torch.zeros(max(max_dl, 1) * DL_LD, **f),
             "dag": torch.empty(max(ns) * AG_LD, **f), "r": torch.empty(max_r, **f)}
        windowed = M["plan"] is not None and self.dw_in_window and not self.grouped_dw_forced
        grouped = plan_grouped_dw(ns, self.dtype, self.pairs, self.grouped_dw_mode, self.grouped_dw_max_r_bytes, windowed,
                                  M["has_gt"], self.r_pad)
        for lay in self.layers[1:]:
            if lay.name in grouped:
                cnt = ns[lay.level] * r_ld(lay.cout, self.r_pad, bf16)
                B["r_" + lay.name] = torch.empty((cnt + 1) // 2 if bf16 else cnt, **f)
        return B, frozenset(grouped)

    def _bind_ground_truth(self, M, gt):
        """A training mesh's ground-truth normals (facet-sharded: this rank's rows), the flags of the real rows of the whole
        mesh (facet-sharded) or the pooled ground truth of the coarse heads (multi-scale)."""
        if gt is None:
            return {}
        dev, plan = self.device, M["plan"]
        gtt = torch.as_tensor(np.asarray(gt.cpu() if isinstance(gt, torch.Tensor) else gt, dtype=np.float32))
        gtt = gtt.reshape(-1, 3).contiguous()
        B = {"gt": gtt.to(dev) if plan is None else gtt[plan.levels[0].lo:plan.levels[0].hi].contiguous().to(dev)}
        B["gtr"] = torch.empty_like(B["gt"])
        if plan is not None:
            # which rows of the WHOLE mesh count in the loss (train.py:1283-1292): every rank can then count the
            # real rows among a step's samples without asking the others
            B["real_flag"] = (gtt.abs().sum(1) > 1e-3).to(torch.float32).to(dev)
        elif self.multi_scale:
            # ground truth of the coarse heads (build extension, see train_step): the fine normals pooled with
            # "average ignoring zero rows" (model.py:792-814) and renormalised; rows of fake nodes only stay zero
            g = B["gt"]
            for k in ("1", "2"):
                g = ops.pool4_avg_iz(g)
                nrm = g.norm(dim=1, keepdim=True)
                g = torch.where(nrm > 0, g / nrm.clamp_min(1e-20), torch.zeros_like(g)).contiguous()
                B["gt" + k] = g
                B["gtr" + k] = torch.empty_like(g)
        return B

    def _bind_layers(self, M):
        """Per layer: descriptor, backward io, workspaces and pair-form tables.  Returns (buffers, descs, ios, layer_flags)."""
        dev, plan, graphs, training = self.device, M["plan"], M["graphs"], M["has_gt"]
        bf16 = self.dtype == "bf16"
        act = dict(dtype=torch.bfloat16 if bf16 else torch.float32, device=dev)
        A = M["B"]          # (the buffers bound so far)
        vals, grads = self.params.values, self.params.grads
        descs, ios, layer_flags, B = {}, {}, {}, {}
        pair_ios = []
        for lay in self.layers:
            g = graphs[lay.level]
            W0, b, u, c, v = vals[lay.pidx:lay.pidx + 5]
            d = ConvDesc()
            d.n, d.nnz = g.n, g.nnz
            col = g.col_up if (plan is not None and lay.shift) else g.col
            d.rowptr, d.col = g.rowptr.data_ptr(), col.data_ptr()
            d.x0 = A[lay.x0].data_ptr()
            d.x1 = A[lay.x1].data_ptr() if lay.x1 else None
            d.c0 = A[lay.x0].shape[1]
            d.c1 = A[lay.x1].shape[1] if lay.x1 else 0
            d.shift, d.cout = lay.shift, W0.shape[1]
            d.W0, d.b, d.u, d.c, d.v = (t.data_ptr() for t in (W0, b, u, c, v))
            d.bias_mask, d.act, d.alpha = 1, lay.act, LRELU_ALPHA
            d.src_rows = A[lay.x0].shape[0]
            d.max_deg = g.max_deg
            # a narrow first layer leaves its aggregates in the forward workspace for the backward pass (training only;
            # _bind_backward_wiring drops the flag where the library does not take that path)
            d.flags = _lib.CONV_SAVE_Z if (training and lay.name == "conv1" and self.save_z) else 0
            if bf16:
                d.flags |= _lib.CONV_BF16
            layer_flags[lay.name] = d.flags
            if self.option_overrides is not None:
                d.options, d.n_options = C.addressof(self.option_overrides), len(self.option_overrides)
            descs[lay.name] = d
            # a layer over a 4x-upsampled input (the two up-convolutions) runs on its COARSE source rows: the pair graph
            # of its level + the table of transformed coarse rows (include/fgc.h: fgc_conv_desc.pair_rowptr)
            pg = None
            use_pairs = lay.shift == 2 and self.pairs
            if use_pairs and plan is not None:
                # facet-sharded: the graph-dependent limits of the pair form on the GLOBAL pair graph - a rank-local test
                # lets ranks disagree (one shard with a coarse row of 25 in-pairs), and the two forms exchange different
                # tensors in the backward pass
                use_pairs = shard.pair_form_allowed(g.pair, W0.shape[1])
            if use_pairs:
                # (facet-sharded: the level's LOCAL pair graph, whose columns address [owned coarse rows | unique halo parents])
                pg = g.pairs() if plan is None else g.pair
                hc = torch.empty(A[lay.x0].shape[0], FGC_M * d.cout, **act)      # (bf16 storage: a bf16 table)
                d.pair_rowptr, d.pair_col, d.pair_mul = pg.prow.data_ptr(), pg.pcol.data_ptr(), pg.pmul.data_ptr()
                d.n_pairs, d.max_pair_deg, d.max_pair_in_deg = pg.n_pairs, pg.max_deg, pg.max_in_deg
                d.hc = hc.data_ptr()
                if self.L.fgc_conv_uses_pairs(C.byref(d)):
                    B["hc_" + lay.name] = hc
                elif plan is not None and not any(self._option(k) == 1 for k in ("NO_PAIRS", "NO_W8", "NO_W8FAST")):
                    # the job-wide test passed and the switches are on: a rank that still refuses would leave the others
                    # waiting for messages of the pair form
                    raise RuntimeError("layer %s: the pair form is allowed job-wide but refused on this rank (n_pairs=%d, "
                                       "max in-degree %d)" % (lay.name, pg.n_pairs, pg.max_in_deg))
                else:
                    d.pair_rowptr = d.pair_col = d.pair_mul = d.hc = None
                    d.n_pairs = d.max_pair_deg = d.max_pair_in_deg = 0
                    pg = None
            # a workspace of its own per layer: packed operands and partial sums stay put for the step
            B["wsf_" + lay.name] = torch.empty(self.L.fgc_conv_workspace_bytes(C.byref(d)) + 256, dtype=torch.uint8,
                                               device=dev)
            if training:
                B["wsb_" + lay.name] = torch.empty(self.L.fgc_conv_bwd_workspace_bytes(C.byref(d)) + 256,
                                                   dtype=torch.uint8, device=dev)
            trow, tcol, tedge = g.transposed()
            io = ConvBwdIO()
            io.trowptr, io.tcol, io.tedge = trow.data_ptr(), tcol.data_ptr(), tedge.data_ptr()
            io.max_in_deg = g.max_in_deg
            io.stages = 0
            io.ag, io.y, io.dy = A["ag_" + lay.name].data_ptr(), A[lay.y].data_ptr(), A["g_" + lay.y].data_ptr()
            io.ds, io.dl, io.dag = (A[k].data_ptr() for k in ("ds", "dl", "dag"))
            io.r = A.get("r_" + lay.name, A["r"]).data_ptr()
            # the stride of r belongs to the buffer: stated once here, not re-derived from every staged call's flags
            io.r_ld = r_ld(lay.cout, self.r_pad, bf16)
            gW0, gb, gu, gc, gv = grads[lay.pidx:lay.pidx + 5]
            io.dW0, io.db, io.du, io.dc, io.dv = (t.data_ptr() for t in (gW0, gb, gu, gc, gv))
            if pg is not None:
                io.tpair_rowptr, io.tpair_col, io.tpair_edge = pg.trow.data_ptr(), pg.tcol.data_ptr(), pg.tedge.data_ptr()
                if training:
                    # (one row per owned pair, then the incoming cross-shard pairs of a facet-sharded rank)
                    need = max(pg.n_pairs + getattr(pg, "n_cross_in", 0), 1) * d.cout
                    if "dt" not in B or B["dt"].numel() < need:
                        B["dt"] = torch.empty(need, **act)
                pair_ios.append(io)
            ios[lay.name] = io
        for io in pair_ios:
            io.dt = B["dt"].data_ptr() if "dt" in B else None
        return B, descs, ios, layer_flags

    def _bind_backward_wiring(self, M):
        """Where each layer's backward pass writes (dx, accumulate, pool fusion) and whether conv1 keeps its aggregates."""
        B, descs, ios, layer_flags, training = M["B"], M["descs"], M["ios"], M["layer_flags"], M["has_gt"]
        # who writes each activation gradient first (write) / second (accumulate): fixed backward order
        #   g_h1: dconv1 (x1, write) then pool1 backward (accumulate);  g_h2: dconv2 (x1) then pool2 backward
        for lay in self.layers[1:]:
            io = ios[lay.name]
            io.dx0 = B["g_" + lay.x0].data_ptr()
            io.dx1 = B["g_" + lay.x1].data_ptr() if lay.x1 else None
            io.accumulate0, io.accumulate1 = 0, 0
        ios["conv1"].dx0 = ios["conv1"].dx1 = None       # (the network input has no gradient)
        if self.fused_pool and training:
            ios["conv1"].pool_y, ios["conv1"].pool_dy = B["p1"].data_ptr(), B["g_p1"].data_ptr()
            ios["conv2"].pool_y, ios["conv2"].pool_dy = B["p2"].data_ptr(), B["g_p2"].data_ptr()
        if self.multi_scale and training and M["plan"] is None:
            # training the three heads: the coarse heads write their input gradients into g_d3 / g_d2 first, the
            # up-convolutions then add theirs
            ios["upconv2"].accumulate0 = 1
            ios["upconv1"].accumulate0 = 1
        if (layer_flags["conv1"] & _lib.CONV_SAVE_Z) and not self.L.fgc_conv_bwd_needs_exchange(
                C.byref(descs["conv1"]), C.byref(ios["conv1"])):
            ios["conv1"].z_saved = B["wsf_conv1"].data_ptr()      # (the library took the narrow path: see FGC_CONV_SAVE_Z)
        else:
            layer_flags["conv1"] = descs["conv1"].flags = layer_flags["conv1"] & ~_lib.CONV_SAVE_Z
        # a deferring layer's r must outlive the layers behind it: one of its own (the first layer has none)
        if any(ios[n].r == B["r"].data_ptr() for n in M["grouped_dw_layers"] if n != "conv1"):
            raise RuntimeError("a layer that defers its weight-gradient GEMM shares the backward scratch r")

    def _bind_mlp_and_arrays(self, M):
        """The MLP heads' workspaces and the layer arrays of fgc_conv_pack / fgc_conv_bwd_reduce: (buffers, arrays)."""
        L, B, (n0, n1, n2) = self.L, M["B"], M["ns"]
        u8 = dict(dtype=torch.uint8, device=self.device)
        ws_b = L.fgc_mlp_bwd_workspace_bytes(n0, 32, HIDDEN, 3)
        if self.multi_scale:
            ws_b = max(ws_b, L.fgc_mlp_bwd_workspace_bytes(n1, 64, HIDDEN, 3), L.fgc_mlp_bwd_workspace_bytes(n2, 128, HIDDEN, 3))
        if self.dtype == "bf16":
            ws_b = max(ws_b, L.fgc_mlp_bwd_bf16_workspace_bytes(n0, 32, HIDDEN, 3))
        bufs = {"ws": torch.empty(max(L.fgc_mlp_workspace_bytes(128, HIDDEN, 3), ws_b) + 256, **u8)}     # the MLP heads
        # the last head's forward operands have a workspace of their own: the step's first launch (fgc_conv_pack with an
        # fgc_pack_extra) packs them and the backward operands (at the start of B["ws"]) beside the conv operands
        bufs["ws_mlp_f"] = torch.empty(max(L.fgc_mlp_workspace_bytes(32, HIDDEN, 3),
                                           L.fgc_mlp_bf16_workspace_bytes(32, HIDDEN, 3)) + 256, **u8)
        names = [lay.name for lay in self.layers]
        nl = len(names)
        arrays = dict(
            descs=(C.POINTER(ConvDesc) * nl)(*[C.pointer(M["descs"][k]) for k in names]),
            ios=(C.POINTER(ConvBwdIO) * nl)(*[C.pointer(M["ios"][k]) for k in names]),
            wsf=(C.c_void_p * nl)(*[B["wsf_" + k].data_ptr() for k in names]),
            wsb=(C.c_void_p * nl)(*[B["wsb_" + k].data_ptr() for k in names]) if M["has_gt"] else None, count=nl)
        return bufs, arrays

    def _alloc_step_inputs(self, B, ns):
        """The per-step inputs - sample indices (train.py:561) and the rotation (train.py:563-565) - live in ONE device
        buffer [ns ints | 9 floats | 3 noise words]: a step refreshes them with a single device-to-device copy
        (set_step_inputs_packed).  The noise words (build extension, bind_clean / set_noise: step low, step high, sigma
        word of fgc_synth_noise) are zero - synthesis off - unless set_noise or a packed row fills them."""
        B["step_in"] = B["step_in_own"] = torch.zeros(ns + 12, dtype=torch.int32, device=self.device)
        B["loss_scratch"] = torch.zeros(self.L.fgc_loss_step_scratch_floats(ns), dtype=torch.float32, device=self.device)
        # facet-sharded steps: [0] the all-reduced sum of |y|, [4:] the all-reduced per-256-samples partial table
        B["loss_sums"] = torch.zeros(self.L.fgc_loss_shard_floats(ns), dtype=torch.float32, device=self.device)
        self._bind_step_inputs(B, B["step_in"])
        B["R"].copy_(torch.eye(3, dtype=torch.float32).reshape(9))

    @staticmethod
    def _bind_step_inputs(B, row):
        ns = row.numel() - 12
        B["step_in"] = row
        B["sample_ind"] = row[:ns]
        B["R"] = row[ns:ns + 9].view(torch.float32)
        B["noise"] = row[ns + 9:ns + 12]

    def _own_step_inputs(self):
        """The step inputs back in the network's own buffer (set_step_inputs_packed may have let the steps read a caller's
        row in place): before anything writes them, and before a hipGraph records their address."""
        B = self._mesh["B"]
        own = B["step_in_own"]
        if B["step_in"] is not own:
            own.copy_(B["step_in"])
            self._bind_step_inputs(B, own)

    def _cached(self, key, bind, max_bytes=64 << 30):
        """Bind the mesh state kept under `key`, or bind() a new one and keep it while all fit in max_bytes."""
        cache = self._mesh_cache
        if key in cache:
            self._mesh = cache[key]
            return self._mesh
        bind()
        used = sum(sum(t.numel() * t.element_size() for t in m["B"].values()) for m in cache.values())
        mine = sum(t.numel() * t.element_size() for t in self._mesh["B"].values())
        if used + mine <= max_bytes:
            cache[key] = self._mesh
        return self._mesh

    def bind_cached(self, key, x, adjs, gt=None, max_bytes=64 << 30):
        """bind_mesh with the bound state (graphs, buffers, descriptors, captured steps: ~7 KB per facet) kept in HBM under
        `key`: a training loop that alternates between meshes (train.py:556 draws one per iteration) switches between them
        without re-uploading, re-allocating or re-capturing anything.  States are kept while they fit in max_bytes."""
        self._cached(key, lambda: self.bind_mesh(x, adjs, gt=gt), max_bytes)
        return self

    # ------------------------------------------------------------------------------------------
    # training from clean meshes (BUILD EXTENSION): per-step noise synthesis on the GPU
    # ------------------------------------------------------------------------------------------
    def bind_clean(self, key, x, adjs, gt, verts, faces_rows, edge_len, seed=0, stream=0, direction="random", lf=None,
                   sensor=None):
        """Build extension: bind a CLEAN mesh whose input rows every step rebuilds from freshly displaced vertices
        (include/fgc.h: fgc_synth_noise, fgc_face_features_rows).  bind_cached(key, x, adjs, gt=gt) plus a synthesis
        state kept with the mesh: the clean vertices verts [V,3], faces_rows int [N0,3] (the faces in node order, -1 rows
        = fake nodes: TrainingSet.addCleanMesh's clean_faces_rows), the mean edge length edge_len (a noise level is a
        multiple of it), the Philox key `seed` and `stream` id (training 0, validation mesh i 1 + i) and the
        direction - "random", "normal": along the clean mesh's area-weighted vertex normals, or a [V,3] array of unit rows
        (finite, every norm within 1e-3 of 1), e.g. the viewing rays of utils.view_rays for the noise of a depth scan: the
        white noise goes along them; binds are compared by a digest of the rows.  x: the clean mesh's own
        rows (what the steps read until set_noise switches the synthesis on); gt: the clean normals.  Unsharded only.
        lf = (width_rel, bumps) (None: white noise only): low-frequency noise on top (include/fgc.h: fgc_synth_noise_lf),
        a field of `bumps` Gaussian bumps (None: ceil(real faces / 6), the count of the reference's addLFGaussianNoise
        stub) of width width_rel mean edge lengths along the clean vertex normals (whatever the white direction, a table of
        rays included), switched on per step by
        set_noise(step, level, lf_level).  Centres are uniform over the vertices, distances Euclidean.
        sensor = utils.sensor_model(...) (None: plain noise): the depth-sensor model (include/fgc.h: fgc_synth_noise_sensor) -
        `direction` must be the table of viewing rays from the model's camera (refused otherwise, and together with lf=); a
        level of set_noise is then the sigma at the model's reference range, growing with range^power, and a model with q > 0
        quantises every range: noisy_vertices() returns the quantised vertices.  The model is fixed per bound mesh and part of
        what two binds of one key are compared by."""
        self._bind_synth(key, NoiseSpec(seed, stream, direction, lf, sensor), (x, verts, faces_rows, edge_len), False,
                         lambda: self._cached(key, lambda: self.bind_mesh(x, adjs, gt=gt)))
        return self

    def _bind_synth(self, key, spec, mesh_args, points, bind):
        """What bind_clean and bind_clean_vertices (points=True) share: the refusals, the mesh cached under `key` (a training
        loop rebinds its meshes every iteration: a lookup, as in bind_cached), otherwise the synthesis state (synth.py:
        SynthState) of the NoiseSpec `spec` and mesh_args = (x, verts, faces_rows, edge_len) on the mesh bind() returns.
        Returns (mesh, newly bound)."""
        if self.comm is not None or (self._mesh is not None and self.sharded):
            raise NotImplementedError("noise synthesis runs on an unsharded network")
        if points:
            self._require_vertex_network()
        M = self._mesh_cache.get(key)
        if M is not None and (M["mode"].clean or (points and M["mode"].verts)):
            if points and not M["mode"].synth_points:
                raise ValueError("mesh %r is bound under this key without synthesised point sets" % (key,))
            M["synth"].same_setting(spec, key)
            self._mesh = M
            return M, False
        S = SynthState(spec, *mesh_args, self.device)
        M = bind()
        M["synth"] = S
        M["mode"].clean = True
        # (a step captured while the mesh was bound without the synthesis under this key has no synthesis nodes: record it again)
        M["captured"].clear()
        return M, True

    def _require_synth(self):
        if self._mesh is None or not self._mesh["mode"].clean:
            raise RuntimeError("bind_clean(...) or bind_clean_vertices(...) is required for noise synthesis")
        return self._mesh["synth"]

    def _enqueue_rows(self, M, ctl, have_bbox, what):
        """fgc_face_features_rows of the mesh's displaced vertices into its input rows (ctl None: whatever the noise words)."""
        S = M["synth"]
        _lib.check(self.L.fgc_face_features_rows(_p(S.v_out), S.plan.nv, _p(S.faces), M["ns"][0], _p(ctl), have_bbox,
                                                 _p(M["B"]["x"]), _p(S.scratch), S.scratch.numel(), self._st()), what)

    def _enqueue_synth(self):
        """Two launches: noise (+ per-workgroup bounding boxes), then the input rows (each workgroup reduces the boxes).
        Both read the step's noise words from device memory and return at once while they are zero.  A mesh bound with
        lf=: three launches, the bump table and field + displacement of fgc_synth_noise_lf in the place of the first; with
        sensor=: fgc_synth_noise_sensor in the place of the first (synth.enqueue: the plan's entry point)."""
        M = self._mesh
        S, noise = M["synth"], M["B"]["noise"]
        self._tag("fwd:synth")
        synth.enqueue(S.plan, S.v, S.v_out, S.scratch, noise, S.lf_ctl, self._st())
        self._enqueue_rows(M, noise, 1, "synth features")

    def noisy_vertices(self):
        """The displaced vertices [V,3] of the last step that synthesised noise (device tensor, overwritten by the next)."""
        return self._require_synth().v_out

    def bind_clean_vertices(self, key, x, adjs, verts, faces_rows, v_faces, edge_len, gt_normals=None, iters=VERTEX_ITERS,
                            seed=0, stream=0, direction="random", lf=None, ray_update=False, sensor=None,
                            surface_loss=False):
        """Build extension: bind a CLEAN mesh for the point-set and double-loss steps on noise synthesised per step -
        bind_vertices plus bind_clean's synthesis state, kept with the mesh under `key`.  verts [V,3]: the RAW clean
        vertices (TrainingSet.addCleanMeshWithVertices' clean_vertices), which are also the ground-truth vertices;
        faces_rows int [N0,3]: the faces in node order (-1 rows = fake nodes), v_faces [V,K], edge_len, seed, stream,
        direction, lf, sensor as in bind_clean; gt_normals: the clean face normals [N0,3] in node order, for the double loss.
        Every step then runs three launches in front (four with lf=: the two of fgc_synth_noise_lf in the place of the
        first): fgc_synth_noise, fgc_face_features_rows (the input rows) and fgc_point_sets_prepare, which normalises the displaced and the clean vertices by the diagonal of their union box
        and rotates both, straight into the buffers the vertex update and fgc_point_loss read - in the place of the two
        fgc_rotate_rows launches of a mesh bound by bind_vertices.  The last launch has no control word: while the noise
        words are zero (right after binding, or set_noise(step, None)) a step runs on the vertices the last
        synthesising step left; right after binding these are the clean ones.
        ray_update: the vertex update of every step is the ray-constrained one (bind_vertices(depth_dir=)) along the table
        of rays the noise goes along - `direction`, built from the clean vertices - so the network is trained on what a depth
        scan asks of it; refused unless `direction` is such a table.
        surface_loss: the clean mesh's own faces_rows are the ground-truth faces (bind_vertices(gt_faces=)): the steps
        measure to surfaces.  With or without for good."""
        if ray_update and isinstance(direction, str):
            raise ValueError("ray_update moves the vertices along the noise's rays: direction must be a [V,3] table of rays")

        def bind():
            # (the plain vertex state holds the clean mesh normalised by its own box; the steps read xr / gtr instead)
            from .utils import normalizePointSets
            vx = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
            vn = normalizePointSets(vx, vx)[0]
            self.bind_vertices(key, x, adjs, vn, faces_rows, v_faces, vn, iters=iters,
                               depth_dir=direction if ray_update else None,
                               gt_faces=np.asarray(faces_rows).reshape(-1, 3).astype(np.int32) if surface_loss else None)
            return self._mesh
        spec = NoiseSpec(seed, stream, direction, lf, sensor, bool(ray_update))
        M, fresh = self._bind_synth(key, spec, (x, verts, faces_rows, edge_len), True, bind)
        if spec.ray_update != (M["verts"]["dirs"] is not None):      # (the direction itself: compared by _bind_synth)
            raise ValueError("mesh %r is bound %s ray_update" % (key, "without" if ray_update else "with"))
        if bool(surface_loss) != (M["verts"]["gt_faces"] is not None):
            raise ValueError("mesh %r is bound %s surface_loss" % (key, "without" if surface_loss else "with"))
        if fresh:
            S = M["synth"]
            S.gt_box = torch.cat([S.v.min(0).values, S.v.max(0).values])
            # the boxes of the clean vertices (and the clean input rows once more): what a step without noise words runs on
            self._enqueue_rows(M, None, 0, "clean features")
            M["mode"].synth_points = True
        self._attach_gt_normals(M, gt_normals)
        return self

    # ------------------------------------------------------------------------------------------
    # enqueue helpers (no allocation, no sync).  The schedules are GENERATORS: they yield an exchange request
    # wherever a facet-sharded run must talk to its peers; an unsharded run just drains them.  The requests - Xchg, Wait,
    # Sum, Call - and what serves, captures and replays them: schedule.py; a step's 17 collectives: shard.py.
    # ------------------------------------------------------------------------------------------
    def _option(self, name):
        """The value a library option has for THIS network: its own override (options=...) or the process-level value."""
        if self.option_overrides is not None:
            names = _lib.option_names()
            for o in self.option_overrides:
                if names[o.index] == name:
                    return int(o.value)
        return _lib.get_option(name)

    def _st(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _tag(self, name):
        if self.profile:
            self.L.fgc_profile_tag(name.encode())

    def _conv_fwd(self, d, args, label, part=None):
        """One fgc_conv_fwd call with the arguments `args` of the layer of descriptor d.  part = (tile_list, n_tiles, proj_row0,
        proj_rows, flags): a PARTIAL call (include/fgc.h: partial forward calls) - the fields are set for this call and put
        back to those of a full call behind it.  Nothing else writes them during a step: one left behind would make the
        layer run a partial call in the next step."""
        if part is None:
            _lib.check(self.L.fgc_conv_fwd(*args), label)
            return
        full = d.flags
        d.tile_list, d.n_tiles, d.proj_row0, d.proj_rows, d.flags = part
        _lib.check(self.L.fgc_conv_fwd(*args), label)
        d.tile_list, d.n_tiles, d.proj_row0, d.proj_rows, d.flags = None, 0, 0, 0, full

    def _conv_bwd(self, d, io, lws, st, label, stages, flags, tiles=None, flags_after=None):
        """One fgc_conv_bwd call of `stages` (0: all of them) under `flags`.  tiles = (tile list, count): the data kernel on
        these tiles only; the list is taken back behind the call.  flags_after: what io.flags is left at - the grouped
        reduction reads it - where that is not `flags`.  Nothing else writes these fields of an io during a step, but the
        loop in front of fgc_conv_bwd_reduce."""
        io.stages, io.flags = stages, flags
        if tiles is not None:
            io.data_tile_list, io.n_data_tiles = tiles[0].data_ptr(), tiles[1]
        _lib.check(self.L.fgc_conv_bwd(C.byref(d), C.byref(io), _p(lws), lws.numel(), st), label)
        if tiles is not None:
            io.data_tile_list, io.n_data_tiles = None, 0
        if flags_after is not None:
            io.flags = flags_after

    def _mlp_head_fwd(self, head, vals, xin, rows, out, partials, packed, ws, st):
        """The MLP head `head` ("head0" / "head1" / "head2") on `rows` rows of xin: raw normals into `out`, the partial sums
        of |out| (normalizeTensor's mean) into `partials`.  vals: self.params.values; packed: 0 or the step's FGC_MLP_PACKED
        word, with the packed operands in `ws`."""
        W1, b1, W2, b2 = vals[self.slot[head]:self.slot[head] + 4]
        _lib.check(self._mlp_fwd(_p(xin), rows, xin.shape[1], HIDDEN, 3, _p(W1), _p(b1), _p(W2), _p(b2), LRELU_ALPHA,
                                 _p(out), _p(partials), packed, _p(ws), ws.numel(), st), head)

    def _mlp_head_bwd(self, head, vals, grads, xin, g_out, rows, g_in, packed, ws, st):
        """Backward of _mlp_head_fwd: g_out (the gradient of the head's raw output) -> the head's parameter gradients and
        g_in, the gradient of xin (written)."""
        s = self.slot[head]
        _lib.check(self._mlp_bwd(_p(xin), _p(g_out), rows, xin.shape[1], HIDDEN, 3, _p(vals[s]), _p(vals[s + 1]),
                                 _p(vals[s + 2]), LRELU_ALPHA, _p(g_in), _p(grads[s]), _p(grads[s + 1]), _p(grads[s + 2]),
                                 _p(grads[s + 3]), packed, _p(ws), ws.numel(), st), head + " bwd")

    def _angular_head(self, k, samp, st, rotate=False, gt=None, normalize=False, backward=False, between=None):
        """The angular loss of the head of level k ("" / "1" / "2": the buffers' suffix) on the sampled rows `samp`:
        normalise (normalize), rotate the ground truth, loss, then (backward) the loss's gradient and (normalize) that of
        normalizeTensor.  gt: ground-truth rows that ARE rotated already, instead of the level's own.  between(): run
        between the loss and its gradient."""
        B, L = self._mesh["B"], self.L
        nk = self._mesh["ns"][int(k or 0)]
        nc = B["nconv" + k]
        if normalize:
            self._drain(self._normalize_gen(k))
        if gt is None:
            gt = B["gt" + k]
            if rotate:
                _lib.check(L.fgc_rotate_rows(_p(gt), _p(B["gtr" + k]), nk, 1, _p(B["R"]), st), "rotate gt")
                gt = B["gtr" + k]
        if k:
            # a coarse head: the fine head's sampled rows modulo the level's size (kept alive until the kernels have run)
            samp = B["sample_ind" + k] = torch.remainder(samp, nk)
        _lib.check(L.fgc_angular_loss_fwd(_p(nc), _p(gt), _p(samp), samp.numel(), _p(B["loss" + k]), st), "loss")
        if between is not None:
            between()
        if backward:
            _lib.check(L.fgc_angular_loss_bwd(_p(nc), _p(gt), _p(samp), samp.numel(), nk, _p(B["loss" + k]), 1.0,
                                              _p(B["g_nconv" + k]), st), "loss bwd")
            if normalize:
                _lib.check(L.fgc_normalize_bwd(_p(B["y" + (k or "0")]), _p(B["g_nconv" + k]), nk, _p(B["g_y" + k]),
                                               _p(B["norm_scratch" + k]), st), "normalize bwd")

    def _normalize_gen(self, k):
        """normalizeTensor on the head of level k ("" / "1" / "2": the buffers' suffix), y -> nconv, as a schedule: the mean |y| is
        taken over the WHOLE tensor (utils.py:1705) - on a facet-sharded mesh by one scalar all-reduce, then the rows."""
        M, B, st, level = self._mesh, self._mesh["B"], self._st(), int(k or 0)
        y, part, sc, nc = B["y" + (k or "0")], B["abs_part" + k], B["norm_scratch" + k], B["nconv" + k]
        if not self.sharded:
            _lib.check(self.L.fgc_normalize_fwd(_p(y), M["ns"][level], _p(part), part.numel(), _p(nc), _p(sc), st), "normalize")
            return
        tot = part.sum().reshape(1)
        yield schedule.sum_(tot)
        sc[0:1] = tot / (3.0 * M["n_total"][level]) + 1e-5
        _lib.check(self.L.fgc_normalize_apply(_p(y), M["ns"][level], _p(sc), _p(nc), st), "normalize")

    @property
    def grouped_dw_layers(self):
        """The bound mesh's layers whose weight-gradient GEMM waits for the grouped launch (plan_grouped_dw)."""
        return self._mesh["grouped_dw_layers"] if self._mesh is not None else frozenset()

    @property
    def _graph_fb(self):
        """The bound mesh's captured angular-loss step: (hipGraph, rotate), or on a facet-sharded rank ((forward segments,
        backward segments), rotate) (_capture_segments); None until forward_backward(capture=True) has recorded it."""
        return self._mesh["captured"].get("angular") if self._mesh is not None else None

    @_graph_fb.setter
    def _graph_fb(self, step):
        self._mesh["captured"].pop("angular", None)
        if step is not None:
            self._mesh["captured"]["angular"] = step

    @property
    def sharded(self):
        return self._mesh["plan"] is not None

    def _forward_gen(self, rotate, defer_normalize=False):
        """defer_normalize: an unsharded TRAINING step leaves normalizeTensor to fgc_loss_step (which writes n_conv too)."""
        M, L, st = self._mesh, self.L, self._st()
        B, ws = M["B"], M["B"]["ws"]
        n0 = M["ns"][0]
        rows0 = B["x"].shape[0]
        vals = self.params.values
        # one housekeeping launch per step: conv operands, the rotation of the input rows, the MLP's operands
        # (FGC_NO_STEP_PROLOGUE=1: the rotation and the MLP packs as launches of their own)
        prologue = self.batched and self.step_prologue
        mlp_packed = _lib.MLP_PACKED if (prologue and not self.multi_scale) else 0
        M["mlp_packed"] = mlp_packed
        if M["mode"].clean:
            # a clean mesh (bind_clean): this step's noisy vertices and input rows, in front of everything that reads x;
            # inside a captured step these launches are nodes of its graph
            self._enqueue_synth()
        self._tag("fwd:input")
        if rotate and not prologue:
            _lib.check(L.fgc_rotate_rows(_p(B["x"]), _p(B["xr"]), rows0, self.in_channels // 3, _p(B["R"]), st),
                       "rotate")
        elif not rotate:
            B["xr"].copy_(B["x"])
        split = self.sharded and self.overlap
        # A layer's output exchange is begun under a key only if its consumer launches something before it waits (interior
        # tiles, the transform of the owned coarse rows, a multi-scale head); otherwise it is served as ONE blocking call - a
        # synchronous collective runs on the compute stream itself, without the two cross-stream dependencies of an
        # asynchronous one (20 - 25 us per call on this platform: tools/rccl_call_cost_probe.py)
        in_flight = set()

        def consumer_overlaps(nxt):
            return nxt is not None and split and (L.fgc_conv_uses_pairs(C.byref(M["descs"][nxt.name])) or
                                                  M["graphs"][nxt.level].tiles["tiles_int"][1] >= self.split_min_tiles)
        packed = 0
        table_done = False      # the first layer's logit table came with the housekeeping launch
        if self.batched:
            A = M["arrays"]
            self._tag("fwd:pack")
            ex = None
            if prologue:
                ex = _lib.PackExtra()
                if rotate:
                    ex.rot_x, ex.rot_y, ex.rot_R = _p(B["x"]), _p(B["xr"]), _p(B["R"])
                    ex.rot_rows, ex.rot_vecs = rows0, self.in_channels // 3
                    d1 = M["descs"]["conv1"]
                    if self.in_channels <= 6 and (d1.src_rows or d1.n) == rows0:
                        # ... and the first layer's logit table of the rotated rows in the same pass
                        s1 = self.slot["conv1"]
                        ex.rot_ag = _p(B["ag_conv1"])
                        ex.rot_u, ex.rot_c, ex.rot_v = _p(vals[s1 + 2]), _p(vals[s1 + 3]), _p(vals[s1 + 4])
                        table_done = True
                if mlp_packed:
                    s0 = self.slot["head0"]
                    ex.mlp_bf16 = 1 if self.dtype == "bf16" else 0
                    ex.mlp_W1, ex.mlp_W2 = _p(vals[s0]), _p(vals[s0 + 2])
                    ex.mlp_n, ex.mlp_cin, ex.mlp_hidden, ex.mlp_cout = n0, 32, HIDDEN, 3
                    ex.mlp_fwd_ws = _p(B["ws_mlp_f"])
                    ex.mlp_bwd_ws = _p(ws) if M["has_gt"] else None
            _lib.check(L.fgc_conv_pack(A["descs"], A["ios"], A["wsf"], A["wsb"], A["count"],
                                       C.byref(ex) if ex is not None else None, st), "pack")
            packed = _lib.CONV_PACKED
            # the operands carry the identity of their layout: a library option that moves between this launch and a layer's
            # FGC_CONV_PACKED / FGC_MLP_PACKED calls is then an error, not a product with the wrong operand
            for dd in M["descs"].values():
                dd.packed_layout = L.fgc_conv_layout_id(C.byref(dd))
            if mlp_packed:
                mlp_packed = M["mlp_packed"] = _lib.MLP_PACKED | _lib.mlp_layout(
                    L.fgc_mlp_layout_id(32, HIDDEN, 3, 1 if self.dtype == "bf16" else 0))
        for li, lay in enumerate(self.layers):
            d = M["descs"][lay.name]
            lws = B["wsf_" + lay.name]
            lflags = M["layer_flags"][lay.name]
            d.flags = packed | lflags
            args = (C.byref(d), _p(B["ag_" + lay.name]), _p(B[lay.y]), _p(B[lay.pool]) if lay.pool else None, _p(lws),
                    lws.numel(), st)
            # a layer waits for the layer before it - if that one's exchange is in flight: after a blocking call the halo
            # rows are there
            need = self.layers[li - 1].name if li else None
            if need not in in_flight:
                need = None
            pair = need is not None and L.fgc_conv_uses_pairs(C.byref(d))
            if split and need and (pair or M["graphs"][lay.level].tiles["tiles_int"][1] >= self.split_min_tiles):
                # the interior tiles (they gather owned rows only) and the logit rows of the owned sources run while the halo
                # rows travel, then the rest.  Pair form: the owned coarse rows are transformed while the halo parents travel,
                # then the tail rows and every block (include/fgc.h: partial forward calls)
                ti, tb = M["graphs"][lay.level].tiles["tiles_int"], M["graphs"][lay.level].tiles["tiles_bnd"]
                interior, boundary = (((ti[0].data_ptr(), 0), (None, 0)) if pair else
                                      ((ti[0].data_ptr(), ti[1]), (tb[0].data_ptr(), tb[1])))
                own_src = d.n >> d.shift
                self._tag("fwd:" + lay.name)
                self._conv_fwd(d, args, lay.name, interior + (0, own_src, packed | lflags))
                yield schedule.wait(need)
                self._conv_fwd(d, args, lay.name, boundary + (own_src, (d.src_rows - own_src) or -1,
                                                              _lib.CONV_PACKED | lflags))
            else:
                # (the unpack behind a pair-form layer's wait has always been counted under that layer's tag)
                if pair:
                    self._tag("fwd:" + lay.name)
                if need:
                    yield schedule.wait(need)
                if not pair:
                    self._tag("fwd:" + lay.name)
                # (conv1's logit table may have come with the housekeeping launch: no projection then)
                self._conv_fwd(d, args, lay.name,
                               (None, 0, 0, -1, packed | lflags) if lay.name == "conv1" and table_done else None)
            if self.sharded and lay.name in SEND_AFTER:
                items = [schedule.rows(lv, B[t], par) for lv, t, par in SEND_AFTER[lay.name]]
                nxt = self.layers[li + 1] if li + 1 < len(self.layers) else None
                if consumer_overlaps(nxt) or (self.multi_scale and lay.name in ("dconv3", "dconv2")):
                    in_flight.add(lay.name)
                    yield schedule.xchg(items, lay.name)
                else:
                    yield schedule.xchg(items)
            if self.multi_scale and lay.name in ("dconv3", "dconv2"):
                k = "2" if lay.name == "dconv3" else "1"
                self._mlp_head_fwd("head" + k, vals, B[lay.y], M["ns"][lay.level], B["y" + k], B["abs_part" + k], 0, ws, st)
        self._tag("fwd:mlp")
        self._mlp_head_fwd("head0", vals, B["d1"], n0, B["y0"], B["abs_part"], mlp_packed, B["ws_mlp_f"], st)
        self._tag("fwd:normalize")
        if defer_normalize and self.sharded:
            # training: the global mean |y| (utils.py:1705 takes it over the whole tensor) is all that is needed here -
            # one launch sums this rank's partials, one scalar all-reduce; the rows are normalised by fgc_loss_shard_rows
            LS = B["loss_sums"]
            _lib.check(L.fgc_loss_shard_abs_sum(_p(B["abs_part"]), B["abs_part"].numel(), _p(LS), st), "abs sum")
            yield schedule.sum_(LS[0:1])
        elif not defer_normalize:
            yield from self._normalize_gen("")

    def _loss_backward_gen(self, rotate):
        M, L, st = self._mesh, self.L, self._st()
        B, n0 = M["B"], M["ns"][0]
        gt = B["gt"]
        self._tag("bwd:loss")
        fused = self.fused_loss
        if rotate and not fused:
            _lib.check(L.fgc_rotate_rows(_p(B["gt"]), _p(B["gtr"]), n0, 1, _p(B["R"]), st), "rotate gt")
            gt = B["gtr"]

        def shard_loss_sum():
            # loss = sum over ranks of (sum of angles) / (real rows among ALL samples).  The count is known to every
            # rank (flags of the whole mesh were kept at bind time), so the backward pass can start at once; the sum
            # of angles rides in the tail of the gradient all-reduce at the end of the step
            ext = self.params.grad_ext
            ext[-4:-3] = torch.nan_to_num(B["loss"][0:1] * B["loss"][1:2])
            B["loss"][1:2] = B["real_flag"][B["sample_ind"].long()].sum().reshape(1)

        def loss_rows():
            samp = B["sample_ind_local"] if self.sharded else B["sample_ind"]
            between = shard_loss_sum if self.sharded else None
            if samp.numel():
                self._angular_head("", samp, self._st(), gt=gt, backward=True, between=between)
            else:
                B["loss"].zero_()
                if between is not None:
                    between()
                B["g_nconv"].zero_()

        if fused and self.sharded:
            # the same in three launches with the step's second scalar all-reduce (the partial table {sum of angles, real
            # samples, sum(d xs . y)} per 256 samples) between them; every rank leaves with the loss of the whole step
            LS = B["loss_sums"]
            ns_total = B["sample_ind"].numel()
            count = 3.0 * M["n_total"][0]

            def shard_samples():
                samp = B["sample_ind_local"]
                _lib.check(L.fgc_loss_shard_samples(_p(B["y0"]), count, _p(B["gt"]), _p(B["R"]) if rotate else None,
                                                    _p(samp) if samp.numel() else None, samp.numel(), ns_total,
                                                    _p(B["loss_gacc"]), _p(LS), self._st()), "loss samples")
            # (a rank's own samples are a list of another length - and another tensor - every step: a request of its own,
            #  served by an eager call also when the schedule is replayed from hipGraphs)
            yield schedule.call(shard_samples)
            yield schedule.sum_(LS[4:])
            _lib.check(L.fgc_loss_shard_rows(_p(B["y0"]), n0, count, ns_total, _p(LS), _p(B["loss_gacc"]), _p(B["nconv"]),
                                             _p(B["g_y0"]), _p(B["loss"]), st), "loss rows")
        elif fused:
            # normalise + rotate the sampled ground-truth rows + loss + both gradients: two launches (loss_gacc is the
            # zero-on-entry / zero-on-exit scratch of fgc_loss_step: a buffer of its own, never the g_nconv that the
            # separate-launch path fills with real gradients)
            samp = B["sample_ind"]
            _lib.check(L.fgc_loss_step(_p(B["y0"]), n0, _p(B["abs_part"]), B["abs_part"].numel(), _p(B["gt"]),
                                       _p(B["R"]) if rotate else None, _p(samp), samp.numel(), _p(B["loss_gacc"]),
                                       _p(B["nconv"]), _p(B["g_y0"]), _p(B["loss"]), _p(B["loss_scratch"]), st), "loss step")
        elif self.sharded:
            # a rank's own samples are a list of another length (and another tensor) every step: these few launches are
            # a request of their own, served by an eager call also when the schedule is replayed from hipGraphs
            yield schedule.call(loss_rows)
            sc = B["norm_scratch"]
            _lib.check(L.fgc_normalize_bwd_partial(_p(B["y0"]), _p(B["g_nconv"]), n0, _p(sc), _p(B["g_y0"]),
                                                   C.c_void_p(sc.data_ptr() + 8), st), "normalize bwd 1")
            tot = sc[2:].sum().reshape(1)
            yield schedule.sum_(tot)
            sc[1:2] = -tot / (sc[0:1] * sc[0:1])
            _lib.check(L.fgc_normalize_bwd_apply(_p(B["y0"]), n0, 3.0 * M["n_total"][0], _p(sc), _p(B["g_y0"]), st),
                       "normalize bwd 2")
        else:
            loss_rows()
            _lib.check(L.fgc_normalize_bwd(_p(B["y0"]), _p(B["g_nconv"]), n0, _p(B["g_y0"]), _p(B["norm_scratch"]),
                                           st), "normalize bwd")
        if self.multi_scale:
            if self.sharded or self.dtype != "f32":
                raise NotImplementedError("training the multi-scale heads: unsharded fp32 network only")
            # Build extension: the reference trains the coarse heads through a point-set loss on the vertex update
            # (trainAccuracyNet: pointset_step below).  Here every head gets the angular loss of the fine head
            # (train.py:1272-1294) against the pooled ground truth, on the same sampled rows modulo the level's size.
            for k in ("2", "1"):
                self._tag("bwd:head" + k)
                self._angular_head(k, B["sample_ind"], st, rotate=rotate, normalize=True, backward=True)
                self._coarse_head_bwd(k)
        yield from self._params_backward_gen(fused)

    def _coarse_head_bwd(self, k):
        """g_y<k> (the gradient of coarse head k's raw output) -> the head's parameter gradients and g_d3 / g_d2 (written:
        the up-convolution adds its own later).  (The coarse heads train on the fp32 network only.)"""
        B = self._mesh["B"]
        y = {"2": "d3", "1": "d2"}[k]
        self._mlp_head_bwd("head" + k, self.params.values, self.params.grads, B[y], B["g_y" + k], self._mesh["ns"][int(k)],
                           B["g_" + y], 0, B["ws"], self._st())

    def _params_backward_gen(self, fused):
        """g_y0 (and, multi-scale, the coarse heads' contributions to g_d3 / g_d2, already written) -> every parameter
        gradient: the fine head's backward, the trunk's backward, the batched reduction (sharded: the flat all-reduce).
        Shared by the angular-loss step and the point-set step."""
        M, L, st = self._mesh, self.L, self._st()
        B, ws, ns = M["B"], M["B"]["ws"], M["ns"]
        n0 = ns[0]
        self._tag("bwd:mlp")
        self._mlp_head_bwd("head0", self.params.values, self.params.grads, B["d1"], B["g_y0"], n0, B["g_d1"],
                           M.get("mlp_packed", 0), ws, st)
        # (the stride of r - padded to whole 128-byte lines unless FGC_NO_R_PAD=1 - is stated in every io's r_ld at bind time:
        #  the staged calls below may reset io.flags freely)
        # Facet-sharded: a layer's weight-gradient stage (8: the GEMM over its r rows and inputs, the partial sums) depends on
        # nothing that follows it, and r stays intact until the NEXT layer's data kernel writes it.  So it is launched inside
        # the next layer's exchange window - between the begin of that layer's exchange (s + d-logit rows, or dt + d-logit
        # rows) and its wait - where it hides 20 - 55 us of a collective's latency that nothing else in a strictly sequential
        # backward pass can hide (tools/shard_latency_probe.py; FGC_NO_DW_IN_WINDOW=1: right behind its own data kernel).
        # Same launches, same arithmetic, another order.
        pending_dw = []      # (at most one weight-gradient stage: (layer, descriptor, io, workspace, flags))

        def flush_dw():
            if pending_dw:
                name, d, io, lws, flags = pending_dw.pop()
                self._tag("bwd:" + name)
                self._conv_bwd(d, io, lws, st, name + " bwd/weights", 8, flags, flags_after=0)

        for lay in reversed(self.layers):
            name = lay.name
            self._tag("bwd:" + name)
            # (g_h2 += d pool2 and g_h1 += d pool1 are folded into stage 1 of conv2 / conv1: fgc_conv_bwd_io.pool_y / pool_dy;
            #  FGC_NO_FUSED_POOL=1: by launches of their own)
            if lay.pool and not self.fused_pool:
                _lib.check(self._pool4_bwd(_p(B[lay.y]), _p(B[lay.pool]), _p(B["g_" + lay.pool]), _p(B["g_" + lay.y]),
                                           ns[lay.level + 1], lay.cout, 1, st), "pool" + lay.pool[1:] + " bwd")
            d, io = M["descs"][name], M["ios"][name]
            lws = B["wsb_" + name]
            base = (_lib.CONV_PACKED | _lib.CONV_DEFER_REDUCE) if self.batched else 0
            if self.batched and name in M["grouped_dw_layers"]:
                base |= _lib.CONV_DEFER_DW
            if not self.sharded:
                self._conv_bwd(d, io, lws, st, name + " bwd", 0, base)
                continue
            cout = d.cout
            nloc = ns[lay.level] + M["nh"][lay.level]
            g = M["graphs"][lay.level]
            if not L.fgc_conv_bwd_needs_exchange(C.byref(d), C.byref(io)):
                # first layer over a narrow input: its parameter gradients are sums over owned nodes, nothing to
                # exchange (the flat-gradient all-reduce adds the ranks)
                flush_dw()
                self._tag("bwd:" + name)
                self._conv_bwd(d, io, lws, st, name + " bwd/params", 1 | 2 | 8, base)
                continue
            pair = L.fgc_conv_uses_pairs(C.byref(d))
            self._conv_bwd(d, io, lws, st, name + (" bwd/pair logits" if pair else " bwd/logits"), 1 | 2, base)
            packed_base = base | _lib.CONV_PACKED      # (the logits call packed the operands of the data and weight stages)
            if pair:
                # pair form: dt and the d-logits of the owned pairs; the rows of the pairs whose parent a peer owns travel to it
                # (ONE grouped exchange, no rows of s), then the data kernel over the owned coarse rows and the weight gradients
                pg = g.pair
                npl = pg.n_pairs + pg.n_cross_in
                items = [schedule.pedges(lay.level, B["dt"][:npl * cout].view(npl, cout)),
                         schedule.pedges(lay.level, B["dl"][:npl * DL_LD].view(npl, DL_LD))]
                tiles, what = pg.tiles, name + " bwd/pair data"
            else:
                # s = dy * lrelu'(y) / deg on owned rows and the d-logits of owned edges came in one call (the deep d-logits
                # kernel computes s in its prologue; packs the operands of stages 2 and 4 when the network did not).  ONE
                # grouped exchange per layer: the halo rows of s (their owners') and the d-logits of incoming cross-shard
                # edges, both first read by the data kernel
                ds_rows = (B["ds"].view(torch.bfloat16) if self.dtype == "bf16" else B["ds"])[:nloc * cout].view(nloc, cout)
                items = [schedule.rows(lay.level, ds_rows), schedule.edges(lay.level)]
                tiles, what = g.tiles, name + " bwd/data"
            # The split threshold of a pair-form layer's backward exchange counts 32-row tiles of its COARSE rows: the same
            # NUMBER as for the other layers, i.e. four times stricter in rows.  Its boundary launch - a handful of workgroups
            # of the data kernel - costs that kernel's single-workgroup latency (~20 us at level 0 of a 100k-facet shard,
            # measured: tools/shard_latency_probe.py), so the split pays only where a collective's latency is well above that;
            # at the default threshold no pair layer of a 100k-facet shard splits (782 coarse tiles), at bench.py's tuning
            # candidates 256 / 64 they do.
            if self.overlap and tiles["ttiles_int"][1] >= self.split_min_tiles:
                # ... it travels under the data kernel of the interior tiles (all in-edges from owned rows; pair form: all
                # in-pairs with owned parents); the boundary tiles and the weight gradients follow (round 6: the pair layers'
                # backward exchange used to block - tools/shard_latency_probe.py)
                yield schedule.xchg(items, "bwd")
                flush_dw()
                self._tag("bwd:" + name)
                self._conv_bwd(d, io, lws, st, what + "/interior", 4, packed_base, tiles["ttiles_int"])
                yield schedule.wait("bwd")
                self._conv_bwd(d, io, lws, st, what + "/boundary", 4, packed_base, tiles["ttiles_bnd"], flags_after=0)
            else:
                # (nothing to put under it - no weight-gradient stage pending -: ONE blocking call, a synchronous collective on
                #  the compute stream, without the cross-stream dependencies of an asynchronous one)
                key = "bwd" if pending_dw else None
                yield schedule.xchg(items, key)
                flush_dw()
                if key:
                    yield schedule.wait(key)
                self._tag("bwd:" + name)
                self._conv_bwd(d, io, lws, st, what, 4, packed_base, flags_after=0)
            pending_dw.append((name, d, io, lws, packed_base))
            if not self.dw_in_window:
                flush_dw()
        flush_dw()
        if self.batched:
            A = M["arrays"]
            for lname in M["grouped_dw_layers"]:      # (the staged calls of a sharded step leave other flags behind)
                M["ios"][lname].flags = _lib.CONV_PACKED | _lib.CONV_DEFER_REDUCE | _lib.CONV_DEFER_DW
            self._tag("bwd:reduce")
            _lib.check(L.fgc_conv_bwd_reduce(A["descs"], A["ios"], A["wsb"], A["count"], st), "reduce")
        if self.sharded:
            # every rank summed its own facets: one flat all-reduce (gradient + the loss sum in the tail)
            yield schedule.sum_(self.params.grad_ext)
            if not fused:
                B["loss"][0:1] = self.params.grad_ext[-4:-3] / B["loss"][1:2]

    def _packed(self, req):
        """The PackedExchange of a schedule.Xchg request; built at its first use, the same every step."""
        cache = self._mesh.setdefault("packed", {})
        key = tuple(tuple((f.data_ptr(), tuple(f.shape)) if isinstance(f, torch.Tensor) else f for f in it) for it in req.items)
        px = cache.get(key)
        if px is None:
            world = len(self._mesh["graphs"][0].send_counts)
            px = cache[key] = shard.PackedExchange([shard.exchange_block(self._mesh, it) for it in req.items], world)
        return px

    def _drain(self, gen):
        """Run a schedule on this rank: nothing to serve when unsharded, collectives through self.comm otherwise."""
        schedule.drain(gen, self.comm, self._packed)

    def _capture_segments(self, make_gen):
        """The schedule make_gen() as hipGraph segments (schedule.capture_segments); their node counts join segment_nodes."""
        segs, counts = schedule.capture_segments(make_gen)
        self.segment_nodes += counts
        return segs

    def _replay_segments(self, segs):
        self._drain(schedule.replay(segs))

    def _capture_angular_segments(self, rotate):
        """The angular step of a facet-sharded mesh as hipGraph segments, kept as captured["angular"] = ((forward segments,
        backward segments), rotate).  Run one step eagerly first: lazy one-time set-up inside the library must not happen
        under capture."""
        self._own_step_inputs()
        self._graph_fb = ((self._capture_segments(lambda: self._forward_gen(rotate, self.fused_loss)),
                           self._capture_segments(lambda: self._loss_backward_gen(rotate))), rotate)

    # ------------------------------------------------------------------------------------------
    # public API
    # ------------------------------------------------------------------------------------------
    def _upload(self, dst, host_array):
        """Stream-ordered host -> device update of a small per-step input.  The source is a fresh PINNED tensor and
        the copy is non_blocking: it is a DMA enqueued on the current stream (so it cannot overtake kernels of the
        previous step that still read `dst`), and torch's caching host allocator keeps the pinned block alive until
        the copy has run.  A plain pageable copy is not ordered against in-flight work on ROCm: with several steps
        queued it changed the inputs of steps that had not executed yet."""
        t = torch.from_numpy(np.ascontiguousarray(host_array)).pin_memory()
        dst.copy_(t, non_blocking=True)

    def set_rotation(self, R):
        """R [3,3] (train.py:563-565); identity = no augmentation."""
        self._own_step_inputs()
        self._upload(self._mesh["B"]["R"], np.asarray(R, dtype=np.float32).reshape(9))

    def set_noise(self, step, level, lf_level=None):
        """Build extension (bind_clean, bind_clean_vertices): the next steps draw the noise of counter `step` (64-bit) at
        `level` x the bound clean mesh's mean edge length; level 0 rebuilds the clean input, level None switches the
        synthesis off (the steps read x as the last synthesis left it).  Filled the way set_rotation fills R; the kernels
        read the words from device memory, so a captured step replays with the new values.
        lf_level (a mesh bound with lf=; None: bumps off, the white noise alone, bit for bit): the target RMS displacement
        of the low-frequency field in mean edge lengths; the amplitude is ops.lf_amplitude of it, the bound width, bump
        count and the clean mesh's area.  The bump words live in a buffer of their own, beside the packed step inputs: a
        packed row carries the white words only, and the last set_noise holds for the bumps."""
        S = self._require_synth()
        if lf_level is not None:
            if S.plan.lf is None:
                raise ValueError("lf_level needs a mesh bound with lf=(width, bumps)")
            if level is None:
                raise ValueError("lf_level needs a level (0 for bumps alone): level None switches the synthesis off")
            if not (np.isfinite(lf_level) and lf_level >= 0):
                raise ValueError("lf_level must be finite and >= 0 (got %r)" % (lf_level,))
        self._own_step_inputs()
        self._upload(self._mesh["B"]["noise"], S.plan.noise_words(step, level))
        if S.plan.lf is not None:
            self._upload(S.lf_ctl, S.plan.lf_words(lf_level))

    def set_samples(self, sample_ind):
        """Indices of the rows the loss is evaluated on (train.py:561), any of the N0 padded rows."""
        t = np.asarray(sample_ind).astype(np.int32)
        self._own_step_inputs()
        B = self._mesh["B"]
        if t.size != B["sample_ind"].numel():
            R, noise = B["R"].clone(), B["noise"].clone()
            self._alloc_step_inputs(B, t.size)
            B["R"].copy_(R)
            B["noise"].copy_(noise)
            self._mesh["captured"].clear()     # (every captured step of the mesh holds the old buffer's address)
        self._upload(B["sample_ind"], t)
        if self.sharded:
            lo = self._mesh["own_lo"]
            loc = t[(t >= lo) & (t < lo + self._mesh["ns"][0])] - lo
            buf = torch.empty(loc.size, dtype=torch.int32, device=self.device)
            if loc.size:
                self._upload(buf, loc.astype(np.int32))
            B["sample_ind_local"] = buf

    def set_step_inputs_device(self, sample_ind_dev, R_dev, sample_local_dev=None):
        """Per-step inputs that are ALREADY on the device (e.g. a window of steps uploaded in one go): device-to-device
        copies are kernels on the compute queue, ordered with hipGraph replays; host -> device DMAs between replays of a
        captured graph were observed to race on this stack when many steps are queued.  sample_local_dev: a facet-sharded
        rank's own part of the samples (local_samples_device), used in place as this step's list.  The noise words of a
        clean mesh (bind_clean) are not part of this call: the last set_noise, or the last packed row, still holds."""
        self._own_step_inputs()
        B = self._mesh["B"]
        B["sample_ind"].copy_(sample_ind_dev)
        B["R"].copy_(R_dev.reshape(9))
        if self.sharded:
            if sample_local_dev is None:
                raise ValueError("a sharded network needs the rank's local sample list (local_samples_device)")
            B["sample_ind_local"] = sample_local_dev

    @staticmethod
    def pack_step_inputs(sample_inds, rotations, device, noise=None):
        """[steps, ns + 12] int32 on the device: row k = the samples and the rotation (bit pattern of 9 floats) of step k,
        in the layout of the network's step-input buffer.  noise (build extension, bind_clean): one (step, sigma) pair per
        row - the noise counter and the ABSOLUTE standard deviation (level x the mesh's mean edge length) - or None per
        row / for all rows: the three noise words stay zero, synthesis off."""
        S = np.stack([np.asarray(s).astype(np.int32) for s in sample_inds])
        R = np.stack([np.asarray(r, dtype=np.float32).reshape(9) for r in rotations]).view(np.int32)
        out = np.zeros((S.shape[0], S.shape[1] + 12), dtype=np.int32)
        out[:, :S.shape[1]] = S
        out[:, S.shape[1]:S.shape[1] + 9] = R
        if noise is not None:
            if len(noise) != S.shape[0]:
                raise ValueError("one (step, sigma) pair (or None) per row")
            for k, pair in enumerate(noise):
                if pair is not None:
                    out[k, S.shape[1] + 9:] = ops.noise_words(pair[0], pair[1]).view(np.int32)
        return torch.from_numpy(out).to(device)

    def set_step_inputs_packed(self, packed_row, sample_local_dev=None, in_place=False):
        """Samples and rotation of the next step(s) = a row of pack_step_inputs, COPIED into the network's own buffer (one
        device-to-device copy; the caller may reuse the row at once).  in_place=True: with eager launches the step reads the
        row where it is - no copy launch, and the caller must keep the row alive and unchanged until every queued step that
        uses it has run (bench.py, whose rows are a window bound once); a mesh whose step is held by a hipGraph copies
        anyway, because the graph holds the address of the own buffer."""
        B = self._mesh["B"]
        if (in_place and not self._mesh["captured"] and packed_row.dtype == torch.int32 and packed_row.is_contiguous()
                and packed_row.numel() == B["step_in_own"].numel() and packed_row.device == B["step_in_own"].device
                and packed_row.data_ptr() % 4 == 0):
            self._bind_step_inputs(B, packed_row)
        else:
            if B["step_in"] is not B["step_in_own"]:
                self._bind_step_inputs(B, B["step_in_own"])
            B["step_in_own"].copy_(packed_row)
        if self.sharded:
            if sample_local_dev is None:
                raise ValueError("a sharded network needs the rank's local sample list (local_samples_device)")
            B["sample_ind_local"] = sample_local_dev

    def local_samples_device(self, sample_ind):
        """The samples (row ids of the WHOLE mesh, train.py:561) that fall into this rank's owned rows, as local row
        ids on the device; the unsharded network keeps them all."""
        t = np.asarray(sample_ind).astype(np.int32)
        if self.sharded:
            lo = self._mesh["own_lo"]
            t = t[(t >= lo) & (t < lo + self._mesh["ns"][0])] - lo
        return torch.from_numpy(np.ascontiguousarray(t.astype(np.int32))).to(self.device)

    def forward(self, rotate=False):
        """Normalised normals of the bound mesh: [N0,3] (padded, permuted order). Un-normalised output in buffers['y0']."""
        self._drain(self._forward_gen(rotate))
        return self._mesh["B"]["nconv"]

    def _forward_ms_gen(self, rotate):
        """The multi-scale forward as a schedule: the network, then normalizeTensor on the two coarse heads (on a
        facet-sharded run one scalar all-reduce each: utils.py:1705 takes the mean over the whole tensor)."""
        yield from self._forward_gen(rotate)
        for k in ("1", "2"):
            yield from self._normalize_gen(k)

    def _normalize_coarse_heads(self):
        """normalizeTensor on the coarse heads 1 and 2 of an unsharded mesh: y1 / y2 -> nconv1 / nconv2, one launch each."""
        for k in ("1", "2"):
            self._drain(self._normalize_gen(k))

    def forward_multi_scale(self, rotate=False):
        """The multi-scale denoising forward of inferNet (train.py:188-193): the three heads, each through
        normalizeTensor.  Returns (n_conv0 [N0,3], n_conv1 [N0/4,3], n_conv2 [N0/16,3]) in node order."""
        if not self.multi_scale:
            raise RuntimeError("the network was built without the multi-scale heads (multi_scale=True)")
        self._drain(self._forward_ms_gen(rotate))
        B = self._mesh["B"]
        return B["nconv"], B["nconv1"], B["nconv2"]

    def measure_exchanges(self, step_fn, steps=3):
        """Facet-sharded runs: what a step's exchanges cost when nothing overlaps them.  Runs `steps` steps with
        every collective made blocking and bracketed by device synchronises (host clock); returns the collectives per
        step, their summed time and bytes sent by this rank.  Diagnostic only: never inside a timed region."""
        import time
        comm = self.comm
        stats = {"n": 0, "s": 0.0, "bytes": 0, "each": []}

        class Timed:
            world, rank, host_staged = comm.world, comm.rank, comm.host_staged

            def _t(self, fn, nbytes, kind="all_to_all"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                stats["s"] += dt
                stats["n"] += 1
                stats["bytes"] += nbytes
                stats["each"].append((kind, nbytes, dt))

            def exchange(self, px):
                self._t(lambda: comm.exchange(px), px.send_buf.numel() * 4)

            def exchange_begin(self, px):
                self.exchange(px)
                return None

            def finish(self, h):
                pass

            def all_reduce_sum(self, t):
                self._t(lambda: comm.all_reduce_sum(t), t.numel() * t.element_size(), "all_reduce")

        self.comm = Timed()
        try:
            for _ in range(steps):
                step_fn()
            torch.cuda.synchronize()
        finally:
            self.comm = comm
        per = stats["n"] // steps
        # the step's collectives in schedule order (pack + collective + unpack, blocking), averaged over the steps
        each = [{"kind": stats["each"][i][0], "bytes_sent": stats["each"][i][1],
                 "ms": round(sum(stats["each"][i + k * per][2] for k in range(steps)) / steps * 1e3, 4)}
                for i in range(per)] if per * steps == stats["n"] else None
        return {"collectives_per_step": per, "blocking_ms_per_step": stats["s"] / steps * 1e3,
                "bytes_sent_per_step": stats["bytes"] // steps, "per_collective": each}

    def _angular_step(self, rotate):
        self._drain(self._forward_gen(rotate, defer_normalize=self.fused_loss))
        self._drain(self._loss_backward_gen(rotate))

    def _run_step(self, form, rotate, capture, enqueue):
        """The bound mesh's step `form` ("angular", "points", "double"): enqueue(), or capture=True: ONE hipGraph kept with
        the mesh, recorded (after a warm-up on a side stream) by the first call for this `rotate` value and replayed."""
        if not capture:
            return enqueue()
        require_graph_replay_safe()
        g = self._mesh["captured"].get(form)
        if g is None or g[1] != rotate:
            self._own_step_inputs()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                enqueue()
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with schedule._no_gc_while_capturing(), torch.cuda.graph(graph):
                enqueue()
            self._mesh["captured"][form] = g = (graph, rotate)
        g[0].replay()

    def forward_backward(self, rotate=True, capture=False):
        """One forward + backward (train.py:492-520 without the optimiser); loss in buffers['loss'][0]."""
        return self._forward_backward("angular", rotate, capture)

    def _angular_step_segments(self, rotate):
        """A facet-sharded captured step: one hipGraph per stretch of launches between two exchanges (17 collectives -> ~25
        graphs per step instead of ~110 launches); the recording call runs one step eagerly (lazy one-time set-up inside
        the library must not happen under capture), every later one replays."""
        require_graph_replay_safe()
        g = self._graph_fb
        if g is None or g[1] != rotate:
            self._own_step_inputs()
            self._angular_step(rotate)
            torch.cuda.synchronize()
            self._capture_angular_segments(rotate)
        else:
            for segs in g[0]:
                self._replay_segments(segs)

    def _require_gt(self, loss_only):
        if not self._mesh["has_gt"]:
            raise RuntimeError("bind_mesh(..., gt=...) is required for " + ("a loss" if loss_only else "training"))
        if loss_only and self.sharded:
            raise NotImplementedError("validation runs on an unsharded network")

    def _angular_loss(self, rotate):
        self._drain(self._forward_gen(rotate))
        self._angular_head("", self._mesh["B"]["sample_ind"], self._st(), rotate=rotate)

    def eval_loss(self, rotate=True):
        """Forward + sampled angular loss, no gradients: the validation pass of trainNet (train.py:588-617 runs
        customLoss alone on the validation feed).  Uses the bound rotation and samples; loss in buffers['loss'][0]."""
        return self._loss_only("angular", rotate)

    # ------------------------------------------------------------------------------------------
    # point-set training (trainAccuracyNet, train.py:636-916): network -> update_position_MS -> fullLoss
    # ------------------------------------------------------------------------------------------
    def bind_vertices(self, key, x, adjs, verts, faces, v_faces, gt_verts, iters=VERTEX_ITERS, gt_normals=None,
                      depth_dir=None, gt_faces=None):
        """Bind a mesh for the point-set step: its graph (bind_cached under `key`) together with its vertex data - the
        normalised vertices [V,3], the faces in node order [N0,3] (-1 rows = fake nodes), v_faces [V,K], the
        ground-truth vertices [Vgt,3] and the two inverse tables of the vertex-update adjoint (ops.vertex_ms_tables) -
        all cached with the graph, like bind_cached.  gt_normals: the ground-truth face normals [N0,3] in node order
        (gt_list), for the double-loss step; uploaded into the cached vertex state (the first time they are given).
        depth_dir (build extension): [V,3] or [1,3] viewing rays (utils.view_rays; used as given, rows longer than 1 can
        diverge), kept with the cached vertex state - the steps then run the ray-constrained update and its adjoint
        (include/fgc.h: fgc_vertex_update_ms_dir_traj / _bwd), with the rays rotated like the vertices.  A key is bound
        with its rays or without for good: a later bind that differs is refused.
        gt_faces (build extension): int [Fgt,3], the faces of the ground-truth mesh on gt_verts, of any topology, kept
        with the cached vertex state - the steps then measure to SURFACES (include/fgc.h: fgc_surface_loss on the refined
        mesh and the ground-truth mesh) in the place of fgc_point_loss.  With or without for good, like the rays."""
        self._require_vertex_network()
        if gt_faces is not None:
            gt_faces = np.asarray(gt_faces.cpu() if isinstance(gt_faces, torch.Tensor) else gt_faces)
            if gt_faces.ndim < 2 or gt_faces.shape[-1] != 3 or gt_faces.size == 0 or gt_faces.dtype.kind not in "iu":
                raise ValueError("gt_faces: an int [Fgt,3] table, got %s %r" % (gt_faces.dtype, gt_faces.shape))
            gt_faces = np.ascontiguousarray(gt_faces.reshape(-1, 3).astype(np.int32))
        if depth_dir is not None:      # (before anything is bound under the key)
            shape = tuple(depth_dir.shape) if hasattr(depth_dir, "shape") else np.shape(depth_dir)
            nv = np.asarray(verts).reshape(-1, 3).shape[0]
            if shape[-1:] != (3,) or int(np.prod(shape[:-1])) not in (1, nv):
                raise ValueError("depth_dir: [V,3] or [1,3] rows for %d vertices, got shape %r" % (nv, shape))

        def bind():
            # the backward buffers of the heads come with a ground truth; the point-set step never reads its values
            xa = np.asarray(x)
            self.bind_mesh(x, adjs, gt=np.zeros((1, xa.size // xa.shape[-1], 3), dtype=np.float32))
        M = self._cached(key, bind)      # (a training loop rebinds its meshes every iteration)
        if not M["mode"].verts:
            dev, n0 = self.device, M["ns"][0]
            vx = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
            fc = np.asarray(faces).reshape(-1, 3).astype(np.int32)
            vf = np.asarray(v_faces).reshape(vx.shape[0], -1).astype(np.int32)
            gv = np.asarray(gt_verts, dtype=np.float32).reshape(-1, 3)
            if fc.shape[0] != n0:
                raise ValueError("faces has %d rows, the graph %d nodes" % (fc.shape[0], n0))
            if gv.shape[0] == 0:
                raise ValueError("no ground-truth vertices")
            tabs = ops.vertex_ms_tables(fc, vf, vx.shape[0])
            it = [int(i) for i in iters]
            nv, T = vx.shape[0], sum(it)
            f = dict(dtype=torch.float32, device=dev)
            V = dict(x=torch.as_tensor(vx, device=dev), gt=torch.as_tensor(gv, device=dev),
                     faces=torch.as_tensor(fc, device=dev), v_faces=torch.as_tensor(vf, device=dev),
                     tables=[torch.as_tensor(t, device=dev) for t in tabs], iters=it)
            V["xr"], V["gtr"] = torch.empty_like(V["x"]), torch.empty_like(V["gt"])
            V["traj"] = torch.empty((T + 1) * nv * 3, **f)
            V["centres"] = torch.empty(3 * (n0 + n0 // 4 + n0 // 16), **f)
            V["g_p"], V["g_x"] = torch.zeros(nv, 3, **f), torch.zeros(nv, 3, **f)
            V["bwd_ws"] = torch.empty(self.L.fgc_vertex_update_ms_bwd_workspace_floats(nv, n0), **f)
            V["i0"], V["i1"] = (torch.zeros(POINT_SAMPLES, dtype=torch.int32, device=dev) for _ in range(2))
            V["loss"] = torch.zeros(1, **f)
            V["gt_faces"] = None if gt_faces is None else torch.as_tensor(gt_faces, device=dev)
            V["gt_faces_key"] = self._faces_key(gt_faces)
            V["loss_ws"] = torch.empty((self.L.fgc_point_loss_workspace_bytes(nv, gv.shape[0], POINT_SAMPLES, POINT_SAMPLES)
                                        if gt_faces is None else
                                        self.L.fgc_surface_loss_workspace_bytes(n0, gt_faces.shape[0], POINT_SAMPLES,
                                                                                POINT_SAMPLES)) + 256,
                                       dtype=torch.uint8, device=dev)
            V["threshold"] = POINT_LOSS_THRESHOLD
            V["dirs"] = None
            if depth_dir is not None:
                self._attach_rays(V, depth_dir, n0)
            M["verts"] = V
            M["mode"].verts = True
        elif not self._same_rays(M["verts"], depth_dir):
            raise ValueError("mesh %r is bound with other rays, or without (depth_dir)" % (key,))
        elif M["verts"]["gt_faces_key"] != self._faces_key(gt_faces):
            raise ValueError("mesh %r is bound with other ground-truth faces, or without (gt_faces)" % (key,))
        self._attach_gt_normals(M, gt_normals)
        return self

    @staticmethod
    def _faces_key(gt_faces):
        """What two binds compare the ground-truth faces by (None: without): the digest of the int32 rows."""
        return None if gt_faces is None else hashlib.sha1(gt_faces.tobytes()).hexdigest()

    def _attach_rays(self, V, depth_dir, n0):
        """The ray table of the constrained vertex update and its buffers into the vertex state V."""
        nv = V["x"].shape[0]
        rows = ops.ray_rows(depth_dir, nv, self.device, "depth_dir").detach().clone()      # (the state's own copy)
        d = rows.cpu().numpy()
        if not np.isfinite(d).all():
            raise ValueError("depth_dir: finite rows, one or one per vertex (%d), got %d" % (nv, d.shape[0]))
        f = dict(dtype=torch.float32, device=self.device)
        V["dirs"], V["dirs_key"] = rows, direction_key(d)
        V["dirs_r"] = torch.empty_like(V["dirs"])
        V["dir_scratch"] = torch.empty(self.L.fgc_vertex_update_ms_dir_scratch_floats(nv, n0), **f)
        V["dir_bwd_ws"] = torch.empty(self.L.fgc_vertex_update_ms_dir_bwd_workspace_floats(nv, n0), **f)

    @staticmethod
    def _same_rays(V, depth_dir):
        """Whether depth_dir is what the vertex state V was bound with (None: without rays): by the digest of the rows."""
        if depth_dir is None or V["dirs"] is None:
            return depth_dir is None and V["dirs"] is None
        if isinstance(depth_dir, torch.Tensor):
            depth_dir = depth_dir.detach().cpu().numpy()
        return direction_key(np.asarray(depth_dir, dtype=np.float32).reshape(-1, 3)) == V["dirs_key"]

    def _step_rays(self, rotate):
        """The ray table a step of the bound mesh runs along (None: the free update): rotated steps read the rotated copy."""
        V = self._mesh["verts"]
        if V["dirs"] is None:
            return None
        return V["dirs_r"] if rotate else V["dirs"]

    def _require_vertex_network(self):
        if not self.multi_scale or self.dtype != "f32":      # (bind_cached binds unsharded)
            raise NotImplementedError("point-set training: unsharded fp32 multi-scale network only")

    def _attach_gt_normals(self, M, gt_normals):
        """The ground-truth face normals and the double-loss step's buffers into the vertex state, the first time given."""
        if gt_normals is not None and not M["mode"].gt_normals:
            g = np.asarray(gt_normals.cpu() if isinstance(gt_normals, torch.Tensor) else gt_normals, dtype=np.float32)
            g = g.reshape(-1, 3)
            if g.shape[0] != M["ns"][0]:
                raise ValueError("gt_normals has %d rows, the graph %d nodes" % (g.shape[0], M["ns"][0]))
            V = M["verts"]
            V["gtn"] = torch.as_tensor(g, device=self.device)
            V["dl_out"] = torch.zeros(4, dtype=torch.float32, device=self.device)      # {total, points, normals, real rows}
            V["dl_scratch"] = torch.zeros(self.L.fgc_dense_normals_loss_scratch_floats(M["ns"][0]), dtype=torch.float32,
                                          device=self.device)
            M["mode"].gt_normals = True

    def set_point_samples(self, sample_ind0, sample_ind1):
        """The 500 + 500 sampled rows of fullLoss (train.py:810-811): rows of the vertices and of the ground truth."""
        V = self._mesh["verts"]
        for dst, src in ((V["i0"], sample_ind0), (V["i1"], sample_ind1)):
            a = np.asarray(src).astype(np.int32).reshape(-1)
            if a.shape[0] != dst.numel():
                raise ValueError("the point-set step samples %d rows per side" % dst.numel())
            self._upload(dst, a)

    def _vertex_heads(self, double):
        """(the three normal fields the vertex update reads, where its adjoint writes their gradients): head 0 normalised and
        the RAW coarse heads (train.py:767-773), or - double - all three normalised (train.py:1079-1081)."""
        B, names = self._mesh["B"], ("nconv", "nconv1", "nconv2") if double else ("nconv", "y1", "y2")
        return tuple(B[k] for k in names), tuple(B["g_" + k] for k in names)

    def _vertex_fwd(self, x, heads, rotate):
        """The multi-scale vertex update of x with its trajectory into V["traj"]: the free one, or - the bound mesh has rays
        (_step_rays) - the one along them."""
        M, L, st = self._mesh, self.L, self._st()
        V, rays = M["verts"], self._step_rays(rotate)
        fn, what, sc, ray_args, t_out = L.fgc_vertex_update_ms_traj, "vertex update", V["centres"], (), ()
        if rays is not None:
            # along rays: the rays turn with the vertices (fgc_point_sets_prepare scales uniformly: they stay valid there)
            if rotate:
                _lib.check(L.fgc_rotate_rows(_p(V["dirs"]), _p(rays), rays.shape[0], 1, _p(M["B"]["R"]), st), "rotate rays")
            fn, what, sc = L.fgc_vertex_update_ms_dir_traj, "vertex update along rays", V["dir_scratch"]
            ray_args, t_out = (_p(rays), rays.shape[0]), (None,)
        _lib.check(fn(_p(x), V["x"].shape[0], _p(V["faces"]), M["ns"][0], _p(V["v_faces"]), V["v_faces"].shape[1],
                      *(_p(h) for h in heads), (C.c_int32 * 3)(*V["iters"]), *ray_args, _p(V["traj"]), V["traj"].numel(),
                      *t_out, _p(sc), sc.numel(), st), what)

    def _vertex_bwd(self, heads, g_heads, rotate):
        """The adjoint of _vertex_fwd: V["g_p"] = dL/d refined vertices into V["g_x"] and the heads' gradients."""
        M, L, st = self._mesh, self.L, self._st()
        V, rays = M["verts"], self._step_rays(rotate)      # (rotated by the forward)
        fn, what, ws, ray_args = L.fgc_vertex_update_ms_bwd, "vertex update bwd", V["bwd_ws"], ()
        if rays is not None:
            fn, what, ws = L.fgc_vertex_update_ms_dir_bwd, "vertex update along rays bwd", V["dir_bwd_ws"]
            ray_args = (_p(rays), rays.shape[0])
        _lib.check(fn(_p(V["traj"]), V["traj"].numel(), V["x"].shape[0], _p(V["faces"]), M["ns"][0], _p(V["v_faces"]),
                      V["v_faces"].shape[1], *(_p(h) for h in heads), (C.c_int32 * 3)(*V["iters"]), *ray_args,
                      *(_p(t) for t in V["tables"]), _p(V["g_p"]), _p(V["g_x"]), *(_p(g) for g in g_heads), _p(ws),
                      ws.numel(), st), what)

    def _pointset_forward(self, rotate, want_grad, double=False):
        """Network (normalizeTensor on head 0 only, train.py:767-773), the rotated vertices moved by update_position_MS
        with its trajectory, fullLoss (and its gradient on the moved vertices).  double: trainDoubleLossNet's form
        (train.py:1075-1102) - normalizeTensor on all three heads, which feed the vertex update, fullLoss into
        dl_out[1] and the dense face-normal loss of head 0 into dl_out[2], their sum into dl_out[0]."""
        M, L, st = self._mesh, self.L, self._st()
        B, V = M["B"], M["verts"]
        n0, nv = M["ns"][0], V["x"].shape[0]
        self._drain(self._forward_gen(rotate))
        if double:
            self._tag("dl:normalize")
            self._normalize_coarse_heads()
        heads = self._vertex_heads(double)[0]
        x, gt = V["x"], V["gt"]
        if M["mode"].synth_points:
            # a clean mesh (bind_clean_vertices): the displaced and the clean vertices over the diagonal of their union
            # box, rotated - one launch behind the two of _enqueue_synth, whose boxes it reads
            self._tag("pts:prepare")
            S = M["synth"]
            sc = S.scratch
            _lib.check(L.fgc_point_sets_prepare(_p(S.v_out), nv, _p(S.v), nv, _p(S.gt_box),
                                                _p(B["R"]) if rotate else None, 1, _p(V["xr"]), _p(V["gtr"]), _p(sc),
                                                sc.numel(), st), "point sets")
            x, gt = V["xr"], V["gtr"]
        elif rotate:
            self._tag("pts:rotate")
            _lib.check(L.fgc_rotate_rows(_p(x), _p(V["xr"]), nv, 1, _p(B["R"]), st), "rotate vertices")
            _lib.check(L.fgc_rotate_rows(_p(gt), _p(V["gtr"]), gt.shape[0], 1, _p(B["R"]), st), "rotate gt vertices")
            x, gt = V["xr"], V["gtr"]
        self._tag("pts:vertex_fwd")
        self._vertex_fwd(x, heads, rotate)
        self._tag("pts:loss")
        T = sum(V["iters"])
        refined = C.c_void_p(V["traj"].data_ptr() + T * nv * 12)
        ws = V["loss_ws"]
        out = V["dl_out"] if double else None
        loss = C.c_void_p(out.data_ptr() + 4) if double else _p(V["loss"])
        samples = (_p(V["i0"]), V["i0"].numel(), _p(V["i1"]), V["i1"].numel(), V["threshold"], loss,
                   _p(V["g_p"]) if want_grad else None, _p(ws), ws.numel(), st)
        if V["gt_faces"] is None:
            _lib.check(L.fgc_point_loss(refined, nv, _p(gt), gt.shape[0], *samples), "point loss")
        else:      # to surfaces: the refined mesh on the bound faces, the ground-truth mesh on its own
            gf = V["gt_faces"]
            _lib.check(L.fgc_surface_loss(refined, nv, _p(V["faces"]), n0, _p(gt), gt.shape[0], _p(gf), gf.shape[0], *samples),
                       "surface loss")
        if double:
            self._tag("dl:loss")
            sc = V["dl_scratch"]
            _lib.check(L.fgc_dense_normals_loss_fwd(_p(B["nconv"]), _p(V["gtn"]), _p(B["R"]) if rotate else None, n0,
                                                    C.c_void_p(out.data_ptr() + 8), loss, _p(out), _p(sc), sc.numel(),
                                                    st), "dense normals loss")

    def _pointset_gen(self, rotate, double=False):
        self._pointset_forward(rotate, True, double)
        M, L, st = self._mesh, self.L, self._st()
        B, V = M["B"], M["verts"]
        n0 = M["ns"][0]
        self._tag("pts:vertex_bwd")
        # dL/d normals: head 0 into g_nconv (then through normalizeTensor), the raw coarse heads straight into g_y1 / g_y2
        # (double: the normalised coarse heads into g_nconv1 / g_nconv2, then through their own normalizeTensor)
        self._vertex_bwd(*self._vertex_heads(double), rotate)
        if double:
            self._tag("dl:bwd")      # (added to what the vertex adjoint has just written)
            sc = V["dl_scratch"]
            _lib.check(L.fgc_dense_normals_loss_bwd(_p(B["nconv"]), _p(V["gtn"]), _p(B["R"]) if rotate else None, n0,
                                                    _p(sc), sc.numel(), 1.0, _p(B["g_nconv"]), st), "dense normals bwd")
        self._tag("bwd:normalize")
        _lib.check(L.fgc_normalize_bwd(_p(B["y0"]), _p(B["g_nconv"]), n0, _p(B["g_y0"]), _p(B["norm_scratch"]), st),
                   "normalize bwd")
        for k in ("2", "1"):
            self._tag("bwd:head" + k)
            if double:
                _lib.check(L.fgc_normalize_bwd(_p(B["y" + k]), _p(B["g_nconv" + k]), M["ns"][int(k)], _p(B["g_y" + k]),
                                               _p(B["norm_scratch" + k]), st), "normalize bwd head" + k)
            self._coarse_head_bwd(k)
        yield from self._params_backward_gen(False)

    def _require_verts(self, double=False):
        if self._mesh is None or not self._mesh["mode"].verts:
            raise RuntimeError("bind_vertices(...) is required for the %s step" % ("double-loss" if double else "point-set"))
        if double and not self._mesh["mode"].gt_normals:
            raise RuntimeError("the double-loss step needs the ground-truth face normals: bind_vertices(..., gt_normals=...)")

    def pointset_forward_backward(self, rotate=True, capture=False):
        """One point-set step without the optimiser: loss in the returned device tensor [1], every parameter gradient
        in params.grads.  capture=True: the whole step as ONE hipGraph (recorded on the first call, replayed after)."""
        return self._forward_backward("points", rotate, capture)

    def pointset_loss(self, rotate=True):
        """The point-set loss alone (the validation pass of trainAccuracyNet, keep_prob 1): device tensor [1]."""
        return self._loss_only("points", rotate)

    def pointset_step(self, sample_ind0, sample_ind1, R, capture=False, noise=None):
        """One iteration of trainAccuracyNet's loop body (train.py:800-840): samples, rotation, forward, backward, Adam.
        noise = (step, level) or (step, level, lf_level) (build extension, a mesh bound by bind_clean_vertices):
        set_noise(*noise) first."""
        return self._step("points", (sample_ind0, sample_ind1), R, capture, noise)

    # double-loss training (trainDoubleLossNet, train.py:919-1268): the point-set loss + the dense face-normal loss
    def double_loss_forward_backward(self, rotate=True, capture=False):
        """One double-loss step without the optimiser (train.py:1079-1102): all three heads normalised, update_position_MS
        on them, fullLoss + faceNormalsLoss(head 0, the rotated ground-truth normals); the returned device tensor [3] =
        {total, points, normals}, every parameter gradient in params.grads.  capture=True: ONE hipGraph per mesh."""
        return self._forward_backward("double", rotate, capture)

    def double_loss(self, rotate=True):
        """The double loss alone (the validation pass of trainDoubleLossNet, keep_prob 1): device tensor [3] = {total,
        points, normals}."""
        return self._loss_only("double", rotate)

    def double_loss_step(self, sample_ind0, sample_ind1, R, capture=False, noise=None):
        """One iteration of trainDoubleLossNet's loop body (train.py:1160-1243): samples, rotation, step, Adam.
        noise = (step, level) or (step, level, lf_level) (build extension, bind_clean_vertices): set_noise(*noise) first."""
        return self._step("double", (sample_ind0, sample_ind1), R, capture, noise)

    # The step forms behind the *_step, *_forward_backward and loss-only entries: require(self, loss_only) raises unless the
    # bound mesh can run the form, set_samples(self, *samples), enqueue(self, rotate) the forward + backward launches,
    # enqueue_loss(self, rotate) the forward and the loss alone, result(mesh state) the loss tensor, trainer(self) trainer_form.
    _StepForm = collections.namedtuple("_StepForm", "require set_samples enqueue enqueue_loss result trainer")
    _TrainerForm = collections.namedtuple("_TrainerForm", "bind bind_clean set_samples step loss samples outputs gt_normals")
    _STEP_FORMS = {
        "angular": _StepForm(_require_gt, set_samples, _angular_step, _angular_loss, lambda M: M["B"]["loss"],
                             lambda self: self._TrainerForm(self.bind_cached, self.bind_clean, self.set_samples,
                                                            self.train_step, self.eval_loss, COST_SAMPLES, 1, False)),
        "points": _StepForm(lambda self, _: self._require_verts(), set_point_samples,
                            lambda self, rotate: self._drain(self._pointset_gen(rotate)),
                            lambda self, rotate: self._pointset_forward(rotate, False), lambda M: M["verts"]["loss"],
                            lambda self: self._TrainerForm(self.bind_vertices, self.bind_clean_vertices, self.set_point_samples,
                                                           self.pointset_step, self.pointset_loss, POINT_SAMPLES, 1, False)),
        "double": _StepForm(lambda self, _: self._require_verts(True), set_point_samples,
                            lambda self, rotate: self._drain(self._pointset_gen(rotate, True)),
                            lambda self, rotate: self._pointset_forward(rotate, False, True), lambda M: M["verts"]["dl_out"][:3],
                            lambda self: self._TrainerForm(self.bind_vertices, self.bind_clean_vertices, self.set_point_samples,
                                                           self.double_loss_step, self.double_loss, POINT_SAMPLES, 3, True)),
    }

    def trainer_form(self, form):
        """What a training loop (train.py) calls for `form`, as bound methods: bind a plain / a clean mesh, set the samples, one
        iteration, the loss alone; the rows per sample set, the loss's entries {total[, points, normals]}, binds take gt_normals."""
        return self._STEP_FORMS[form].trainer(self)

    def _loss_only(self, form, rotate):
        """Forward and the loss of `form`, no gradients: the validation passes."""
        F = self._STEP_FORMS[form]
        F.require(self, True)
        F.enqueue_loss(self, rotate)
        return F.result(self._mesh)

    def _forward_backward(self, form, rotate, capture):
        """One step of `form` without the optimiser: _run_step, or the segments of a facet-sharded captured (angular) step."""
        F = self._STEP_FORMS[form]
        F.require(self, False)
        if capture and self.sharded:
            if form != "angular":
                raise NotImplementedError("a facet-sharded captured step exists for the angular form only")
            self._angular_step_segments(rotate)
        else:
            self._run_step(form, rotate, capture, lambda: F.enqueue(self, rotate))
        return F.result(self._mesh)

    def _step(self, form, samples, R, capture, noise):
        """One training iteration of `form`: samples, rotation, the noise words when given, forward + backward, Adam."""
        self._STEP_FORMS[form].set_samples(self, *samples)
        self.set_rotation(R)
        if noise is not None:
            self.set_noise(*noise)
        out = self._forward_backward(form, True, capture)
        self.adam_step()
        return out

    def adam_step(self, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
        P = self.params
        P.step += 1
        self._tag("adam")
        _lib.check(self.L.fgc_adam_step(_p(P.theta), _p(P.grad), _p(P.m), _p(P.v), P.total, P.step, lr, b1, b2, eps,
                                        self._st()), "adam")

    def train_step(self, sample_ind=None, R=None, capture=False, noise=None):
        """One iteration of trainNet's loop body (train.py:558-575,619): returns the loss tensor (device, [2]).
        noise = (step, level) or (step, level, lf_level) (build extension, a mesh bound by bind_clean):
        set_noise(*noise) first."""
        if sample_ind is None:
            sample_ind = np.random.randint(self._mesh["ns"][0], size=COST_SAMPLES)
        if R is None:
            from .utils import rand_rotation_matrix
            R = rand_rotation_matrix()
        return self._step("angular", (sample_ind,), R, capture, noise)

    def infer_normals(self, permutations, num_faces):
        """Denoised unit normals in the ORIGINAL face order, [F,3] (train.py:115-121,136)."""
        n_conv = self.forward(rotate=False)
        perm = torch.as_tensor(np.asarray(permutations).astype(np.int32)).to(self.device)
        out = torch.empty(num_faces, 3, dtype=torch.float32, device=self.device)
        _lib.check(self.L.fgc_infer_epilogue(_p(n_conv), _p(perm), int(num_faces), _p(out), self._st()), "epilogue")
        return out

    @property
    def buffers(self):
        return self._mesh["B"]

    # ------------------------------------------------------------------------------------------
    # per-kernel timing through the library's hipEvent hooks
    # ------------------------------------------------------------------------------------------
    def profile_start(self):
        self.profile = True
        self.L.fgc_profile_enable(1)

    def profile_stop(self):
        """Returns {"tag/kernel": (launches, total_ms)}."""
        buf = C.create_string_buffer(1 << 16)
        n = self.L.fgc_profile_collect(buf, len(buf))
        self.L.fgc_profile_enable(0)
        self.profile = False
        out = {}
        if n > 0:
            for line in buf.value.decode().splitlines():
                name, cnt, ms = line.rsplit(" ", 2)
                out[name] = (int(cnt), float(ms))
        return out

    def layer_dims(self):
        """[(layer, n, nnz, cin, cout)] of the bound mesh, in forward order (for the roofline accounting)."""
        M = self._mesh
        out = []
        for lay in self.layers:
            g = M["graphs"][lay.level]
            d = M["descs"][lay.name]
            out.append((lay.name, g.n, g.nnz, d.c0 + d.c1, d.cout))
        return out

    def pair_dims(self):
        """{layer: (coarse rows, pairs)} of the layers that run in the pair form (include/fgc.h: fgc_conv_uses_pairs)."""
        M = self._mesh
        return {name: (d.n >> 2, d.n_pairs) for name, d in M["descs"].items() if self.L.fgc_conv_uses_pairs(C.byref(d))}
