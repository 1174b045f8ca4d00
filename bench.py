#!/usr/bin/env python3
"""Benchmark of the facet-graph-convolution hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W          (plain shell: N > 1 starts its own torchrun child)
    python bench.py ... --full                             (also every untimed extra listed below)
    python bench.py ... --dump-outputs DIR                 (what the last timed step computed, as DIR/<name>.npy)

One "step" = one full training iteration of the reference's loop body (train.py:558-575,619) on one
synthetic mesh: random rotation of inputs and ground truth, full 3-level graph U-Net + MLP forward,
normalisation, angular loss on 4000 sampled rows, full backward, TF1-Adam update.  fp32 by default
(--dtype bf16: activations stored as bf16, matrix products on the bf16 MFMA, fp32 accumulation and fp32
master weights - BASELINE config 3, never the headline).

Workloads (--config):
  c2 (default)  torus 250 x 200 quads = 100 000 facets per GPU, train step          [headline metric]
  c3            torus 250 x 100 = 50 000 facets, train step (meant for --dtype bf16)
  c4            torus 1000 x 500 = 1 000 000 facets, ONE mesh facet-sharded over the N GPUs (strong scaling)
  c5            torus 500 x 500 = 500 000 facets, multi-scale network (three heads), ONE mesh over the N GPUs;
                step = the reference's multi-scale denoising forward (inferNet, train.py:188-193: three normal
                fields, each through normalizeTensor); its training objective is a point-set loss (out of scope)
--nu/--nv override the torus, --multi-scale the network, --scaling weak|strong the decomposition.

N > 1: one process per GPU.  Default (--mode shard): ONE mesh is facet-sharded over the N GPUs (shard.py): each
rank owns a contiguous range of the coarsest graph level and everything under it, halo rows are exchanged by
RCCL all-to-all before every conv (and s = dy/deg rows plus cross-edge d-logits in backward), the flat fp32
gradient is all-reduced once per step.  With c2 the mesh has N x 100 000 facets: per-GPU work is fixed as N
grows ("weak" scaling).  --mode replicas: each rank trains on its own mesh, gradient all-reduce only.
FGC_BENCH_BACKEND=gloo rehearses N > 1 with N processes on ONE GPU (host-staged exchange).

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps and prints it: `value` and `ms_per_step`
come from those K steps alone.  With --full the line also carries what takes runs of its own, all measured outside the
timed region:
  roofline      the dominant kernel FAMILY (summed time per step) through its launch with the most algorithmic work:
                achieved TFLOP/s from hipEvent timings taken live in this process; `families` has the top three
  cpu_baseline  the oracle (reference-shaped torch CPU restatement) timed on this host on a bounded sample
  extras        repeat blocks of K steps, the eager / hipGraph comparison, the forward-only rate, the bf16 runs (`also`),
                a sharded run's blocking exchange costs (`exchange`) and its strong-scaling reading (`strong`)
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time
import faulthandler

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # see facet_graph_convolution_amd/__init__.py

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

PEAK_F32_MFMA_TFLOPS = 157.3    # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: bf16 MFMA, dense
PEAK_HBM_GBS = 8000.0

CONFIGS = {
    # name: (nu, nv, multi_scale, default scaling, what one step is)
    "c2": (250, 200, False, "weak", "train"),
    "c3": (250, 100, False, "weak", "train"),
    "c4": (1000, 500, False, "strong", "train"),
    "c5": (500, 500, True, "strong", "denoise"),
}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", choices=sorted(CONFIGS), default="c2")
    ap.add_argument("--nu", type=int, default=0, help="torus quads around the large circle (default: from --config)")
    ap.add_argument("--nv", type=int, default=0)
    ap.add_argument("--multi-scale", action="store_true", help="three-head network, step = multi-scale denoising forward")
    ap.add_argument("--dtype", choices=["f32", "bf16"], default=None,
                    help="storage of the activations: f32 (default, the headline) or bf16 (default of --config c3)")
    ap.add_argument("--graph", type=int, default=-1,
                    help="1: replay the step from hipGraphs (one GPU: the whole step as one graph; facet-sharded: one graph "
                         "per stretch of launches between two exchanges, falling back to eager if capture raises), 0: eager "
                         "launches, -1 (default): one GPU training = 1 (replay is 1 %% faster at 100k facets, and the only "
                         "stable timing at 50k), everything else = 0 (3 - 5 %% less host time per step on two gloo ranks, but "
                         "collectives next to replays have not run on a real node).  Needs DEBUG_CLR_GRAPH_PACKET_CAPTURE=0, which the package sets at import: with "
                         "the runtime's pre-built graph packets a replay after a stream synchronise computes garbage on "
                         "this ROCm stack (DESIGN.md section 6)")
    ap.add_argument("--repeats", type=int, default=5, help="--full: untimed-extra repeats of the K-step block (min / median)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--dump-kernels", type=str, default="", help="write the full per-kernel table to this file")
    ap.add_argument("--mode", choices=["shard", "replicas"], default="shard", help="multi-GPU decomposition")
    ap.add_argument("--scaling", choices=["weak", "strong"], default=None)
    ap.add_argument("--full", action="store_true",
                    help="also run every untimed extra (per-kernel roofline, repeat blocks, eager / hipGraph comparison, "
                         "forward-only rate, bf16 extras, CPU baseline, sharded exchange costs and strong scaling)")
    ap.add_argument("--dump-outputs", type=str, default="",
                    help="after the timed steps, write what the last of them computed as DIR/<name>.npy (rank 0; float32 "
                         "or float64, at most 64 MB in all)")
    args = ap.parse_args(argv)
    nu, nv, ms, scaling, what = CONFIGS[args.config]
    args.nu = args.nu or nu
    args.nv = args.nv or nv
    args.multi_scale = args.multi_scale or ms
    args.scaling = args.scaling or scaling
    args.dtype = args.dtype or ("bf16" if args.config == "c3" else "f32")      # BASELINE config 3 is the bf16 train step
    args.what = "denoise" if args.multi_scale else what
    return args


# ---------------------------------------------------------------------------------------------------
# N > 1 from a plain shell: a fresh torchrun child, started before this process touches the GPU
# ---------------------------------------------------------------------------------------------------
def launcher_command(gpus, argv, port):
    """The command the driver itself uses for N > 1 (one rank per GPU over RCCL).  Only the contract's own flags travel
    on the command line; everything else goes through FGC_BENCH_ARGV (torchrun's argparse claims abbreviations of its
    own options in the script's arguments: `--nu` reads as `--numa-binding`)."""
    keep = []
    it = iter(range(len(argv)))
    for i in it:
        if argv[i] in ("--gpus", "--steps", "--warmup") and i + 1 < len(argv):
            keep += [argv[i], argv[i + 1]]
            next(it, None)
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + keep


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(args, argv):
    """`python bench.py --gpus N` without torchrun's environment: run the N ranks as a CHILD process group (never an
    exec of a process that may have touched the GPU) and relay rank 0's JSON line and the exit code."""
    cmd = launcher_command(args.gpus, argv, _free_port())
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", FGC_BENCH_ARGV=json.dumps(list(argv)))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    def run_group(cmd, env):
        proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
        line = None
        for l in proc.stdout.splitlines():
            if l.startswith("{") and '"metric"' in l:
                line = l
            else:
                print(l, file=sys.stderr)
        return proc.returncode, line

    rc, line = run_group(cmd, env)
    if line is None and args.graph == 1:
        # The rank group died without a line (a rank killed by a signal leaves nothing to catch in-process).  If the step
        # was being replayed from hipGraph segments, ONE fresh child group - new processes, never a re-exec - runs the same
        # bench with eager launches, and the line says so.
        print("bench: the rank group ended with code %d and no result line; one more group with --graph 0" % rc, file=sys.stderr)
        argv2 = [a for i, a in enumerate(argv) if a != "--graph" and (i == 0 or argv[i - 1] != "--graph")] + ["--graph", "0"]
        env2 = dict(env, FGC_BENCH_ARGV=json.dumps(argv2), FGC_BENCH_RETRY_NOTE="first rank group ended with code %d and no "
                    "result line; this line is from a second, fresh group with --graph 0 (eager launches)" % rc)
        rc, line = run_group(launcher_command(args.gpus, argv2, _free_port()), env2)
    if line:
        print(line)
    return rc if (rc or line) else 1


# ---------------------------------------------------------------------------------------------------
def build_mesh(nu, nv, seed):
    from facet_graph_convolution_amd.meshgen import torus, add_noise
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    V, F = torus(nu, nv)
    ds = TrainingSet()
    ds.addMeshWithGT(add_noise(V, F, 0.2, seed=1 + seed), F, V, seed=seed)
    return ds, F.shape[0]


def build_mesh_shared(nu, nv, seed, rank, world, backend, dev):
    """N > 1, ONE mesh for all ranks: rank 0 preprocesses it (native coarsening, seconds at 8 x 100k facets) and broadcasts
    the tensor contract - features, ground truth, the three K-lists as int32 - over the job's own back end; the other ranks
    do not repeat the preprocessing (round 4: 7.5 - 8.9 s of CPU per rank, eight times over).  Every rank still derives its
    shard plan from the global K-lists (shard.ShardPlan)."""
    import types
    import torch
    import torch.distributed as dist
    where = dev if backend == "nccl" else "cpu"
    meta = [None]
    if rank == 0:
        ds, F = build_mesh(nu, nv, seed)
        arrs = [np.ascontiguousarray(ds.in_list[0], dtype=np.float64), np.ascontiguousarray(ds.gt_list[0], dtype=np.float64)] + \
               [np.ascontiguousarray(a, dtype=np.int32) for a in ds.adj_list[0]]
        meta[0] = (F, [(a.shape, str(a.dtype)) for a in arrs])
    dist.broadcast_object_list(meta, src=0)
    F, specs = meta[0]
    out = []
    for i, (shape, dt) in enumerate(specs):
        t = torch.from_numpy(arrs[i]).to(where) if rank == 0 else torch.empty(shape, dtype=getattr(torch, dt), device=where)
        dist.broadcast(t, src=0)
        out.append(arrs[i] if rank == 0 else t.cpu().numpy())
    ds = types.SimpleNamespace(in_list=[out[0]], gt_list=[out[1]], adj_list=[out[2:5]])
    return ds, F


def kernel_flops(kind, n, nnz, cin, cout, M=9):
    """Algorithmic FLOPs of one launch: the dense contraction 2*n*M*cin*cout plus the per-edge
    aggregation 2*nnz*M*C (C = gathered width)."""
    gemm = 2.0 * n * M * cin * cout
    if kind == "fwd":          # gathers cin-wide rows
        return gemm + 2.0 * nnz * M * cin
    if kind == "bwd_logits":   # dz GEMM + per-edge dots over cin
        return gemm + 2.0 * nnz * M * cin
    if kind == "bwd_data":     # gathers cout-wide rows of s
        return gemm + 2.0 * nnz * M * cout
    if kind == "bwd_weight":   # r^T x
        return gemm
    raise ValueError(kind)


def pair_kernel_flops(kern, nc, npairs, cin, cout, M=9):
    """EXECUTED FLOPs of one launch of a layer in the pair form (csrc/fgc_conv_pair.hip): the layer runs on its nc = n / 4
    coarse rows and npairs (block, parent) pairs, so these are about a quarter of kernel_flops of the same layer - the
    SURVEY-convention figure, which the line reports beside them (`pair_form`) and never divides a pair launch's time by."""
    if "pair_transform" in kern:      # h = W0 xc and the two logit tiles
        return 2.0 * nc * cin * (M * cout + 2 * M)
    if "pair_fwd" in kern:            # t = sum_m q h, y += mult t
        return 2.0 * npairs * cout * (M + 4)
    if "pair_bwd_logits" in kern:     # dt = sum mult s, dq = <dt, h>
        return 2.0 * npairs * cout * (M + 4)
    if "conv_w8_kernel<data>" in kern:
        return kernel_flops("bwd_data", nc, npairs, cin, cout)
    if "gemm_tn" in kern:
        return kernel_flops("bwd_weight", nc, npairs, cin, cout)
    return None


def kernel_bytes(kind, layer, n, nnz, cin, cout, elem):
    """Algorithmic HBM bytes of one conv launch (SURVEY.md section 8d convention: every tensor of the layer once, the CSR
    once; weights, logit tables and per-edge scratch are not algorithmic).  An up-convolution reads the coarse tensor:
    cin / 4 per fine node."""
    cin_eff = cin / 4.0 if layer.startswith("upconv") else cin
    csr = 4.0 * (n + nnz)
    if kind == "fwd":
        return elem * n * (cin_eff + cout) + csr
    if kind == "bwd_logits":       # dy, y, x
        return elem * n * (2 * cout + cin_eff) + csr
    if kind == "bwd_data":         # s in, dx out
        return elem * n * (cout + cin_eff) + csr
    return None


def algorithmic_bytes_fwd_bwd(net, elem=4):
    """SURVEY.md section 8d convention: each tensor crossing a layer boundary written once, read once per consumer;
    CSR read once per conv; weights and fused ops free.  Backward moves the same tensors as gradients plus
    the saved activations again (x2.45 of forward in the survey's accounting: 3879/1584).  elem: bytes per stored
    activation element (2 with --dtype bf16; the 6-channel input, the 3-channel output and the CSR stay 4 bytes)."""
    dims = {name: (n, nnz, cin, cout) for name, n, nnz, cin, cout in net.layer_dims()}
    n0, n1, n2 = dims["conv1"][0], dims["conv2"][0], dims["conv3"][0]
    d0, d1, d2 = (dims[k][1] / dims[k][0] for k in ("conv1", "conv2", "conv3"))
    e = elem
    fwd = (n0 * (4 * 6 + e * 32 + 4 * (1 + d0)) + n1 * (e * (32 + 64) + 4 * (1 + d1)) + n2 * (e * (64 + 128) + 4 * (1 + d2)) +
           n2 * (e * (128 + 128) + 4 * (1 + d2)) + n1 * (e * (32 + 64) + 4 * (1 + d1)) + n1 * (e * (128 + 64) + 4 * (1 + d1)) +
           n0 * (e * (16 + 32) + 4 * (1 + d0)) + n0 * (e * (64 + 32) + 4 * (1 + d0)) + n0 * (e * 32 + 4 * 3) + n1 * e * 32 +
           n2 * e * 64)
    return fwd, fwd * 3879.0 / 1584.0


def cpu_model():
    try:
        for l in open("/proc/cpuinfo"):
            if l.startswith("model name"):
                return l.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def physical_cores():
    """Distinct (physical id, core id) pairs; falls back to the logical count."""
    seen, phys, core = set(), None, None
    try:
        for l in open("/proc/cpuinfo"):
            if l.startswith("physical id"):
                phys = l.split(":")[1].strip()
            elif l.startswith("core id"):
                core = l.split(":")[1].strip()
            elif not l.strip():
                if phys is not None and core is not None:
                    seen.add((phys, core))
                phys = core = None
    except OSError:
        pass
    return len(seen) or (os.cpu_count() or 1)


def usable_cpus():
    """CPUs this process may really use: the affinity mask, cut down to the cgroup's CPU quota where there is one (a GPU
    box hands a job its share of the host - e.g. 16 of 256 logical CPUs - through cpu.max, not through the mask; torch
    started with one thread per CPU of the MASK then runs hundreds of threads on a sixteenth of them)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]) + 0.5)))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, int(q / per + 0.5)))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def cpu_baseline(sample_faces=(60, 60), full=(250, 200)):
    """The oracle timed on this host as BASELINE.md section 3 prescribes, on a BOUNDED sample (about 30 s of CPU work in
    all, so that the default bench run stays within minutes): the reference-shaped torch-CPU restatement
    (oracle/model_ref.py: zero-row pad -> K-padded gather -> per-edge softmax -> multiply -> reduce) on a 7 200-facet
    torus of the same family as the headline mesh (mesh seed 0 and weight seed 0 as in the GPU run) -
      * forward + backward and forward only, 2 warm-ups then the median of 5 runs, torch threads = all cores in the
        affinity mask (`value`, `forward`);
      * the same with 32 threads (1 warm-up, median of 3): on the 128-core boxes the K-padded ops stop scaling there;
      * ONE forward on the full 100 000-facet headline mesh (its backward keeps the materialised [N0,23,288] tensors of
        every layer alive and does not fit in host memory)."""
    import torch
    from oracle import model_ref as R
    logical = os.cpu_count() or 1
    mask = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else logical
    affinity = usable_cpus()         # "all cores" = all the cores this job may use (mask and cgroup quota)

    def note(msg):
        print("bench: cpu_baseline: " + msg, file=sys.stderr, flush=True)

    def tensors(nu, nv):
        ds, F = build_mesh(nu, nv, seed=0)       # (the GPU run's seed: the full mesh below IS the headline mesh)
        x = torch.tensor(ds.in_list[0].astype(np.float32))
        gt = torch.tensor(ds.gt_list[0].astype(np.float32))
        adjs = [torch.tensor(a.astype(np.int32)) for a in ds.adj_list[0]]
        return x, gt, adjs, F

    x, gt, adjs, F = tensors(*sample_faces)
    params = [p.requires_grad_(True) for p in R.init_params(0)]
    plain = [p.detach() for p in params]
    samp = np.random.RandomState(2).randint(x.shape[1], size=4000)

    def fwd_bwd():
        for p in params:
            p.grad = None
        t0 = time.perf_counter()
        loss, _ = R.train_loss(x, adjs, gt, params, samp, torch.eye(3))
        loss.backward()
        return time.perf_counter() - t0

    def fwd():
        with torch.no_grad():
            t0 = time.perf_counter()
            R.normalizeTensor(R.get_model_reg_multi_scale(x, adjs, plain))
            return time.perf_counter() - t0

    def timed(fn, threads, warm, runs, what):
        torch.set_num_threads(threads)
        t0 = time.perf_counter()
        first = fn()
        # (bounded: a run that takes longer than expected gets fewer repeats, never an open-ended wait)
        if first > 15.0:
            warm, runs = 1, min(runs, 3)
        for _ in range(warm - 1):
            fn()
        ts = sorted(fn() for _ in range(runs))
        note("%s at %d threads: median %.2f s over %d runs (%.0f s)" % (what, threads, ts[len(ts) // 2], runs,
                                                                          time.perf_counter() - t0))
        return ts[len(ts) // 2], ts

    t_all0 = time.perf_counter()
    note("%d facets, %d usable CPUs (mask %d, logical %d)" % (F, affinity, mask, logical))
    fb_all, fb_all_ts = timed(fwd_bwd, affinity, 2, 5, "forward+backward")
    f_all, _ = timed(fwd, affinity, 2, 5, "forward")
    t32 = min(mask, 32)
    if t32 == affinity:     # the two thread counts are the same measurement
        fb_32, f_32 = fb_all, f_all
    else:
        fb_32, _ = timed(fwd_bwd, t32, 1, 3, "forward+backward")
        f_32, _ = timed(fwd, t32, 1, 3, "forward")
    best_threads, fb_best = (affinity, fb_all) if fb_all <= fb_32 else (t32, fb_32)
    out = {"value": F / fb_best, "unit": "facets/s", "cores": best_threads, "kind": "port",
           "cpu_model": cpu_model(), "logical_cpus": logical, "physical_cores": physical_cores(),
           "cpus_in_affinity_mask": mask, "usable_cpus": affinity,
           "forward_backward": {"all_cores": {"threads": affinity, "facets_per_s": F / fb_all,
                                              "median_s": fb_all, "runs_s": [round(t, 3) for t in fb_all_ts]},
                                "threads_32": {"threads": t32, "facets_per_s": F / fb_32, "median_s": fb_32}},
           "forward": {"all_cores": {"threads": affinity, "facets_per_s": F / f_all, "median_s": f_all},
                       "threads_32": {"threads": t32, "facets_per_s": F / f_32, "median_s": f_32}},
           "sample": "oracle/model_ref.py (reference-shaped K-padded torch CPU fp32), full net on a torus %dx%d = %d facets "
                     "(N0=%d): forward+backward and forward, 2 warm-ups + median of 5 at %d threads, 1 + median of 3 at %d "
                     "threads; `value` = forward+backward at the faster thread count; %.0f s of CPU time in all" % (
                         sample_faces[0], sample_faces[1], F, x.shape[1], affinity, t32, time.perf_counter() - t_all0)}
    del x, gt, adjs
    if full:
        torch.set_num_threads(best_threads)
        note("one forward on the full %dx%d mesh" % full)
        x, gt, adjs, F = tensors(*full)
        with torch.no_grad():
            t0 = time.perf_counter()
            y = R.normalizeTensor(R.get_model_reg_multi_scale(x, adjs, plain))
            dtf = time.perf_counter() - t0
        out["forward_only_full_mesh"] = {"value": F / dtf, "unit": "facets/s", "threads": best_threads,
                                         "sample": "1 forward (not warmed) of the full net on the torus %dx%d = %d facets "
                                                   "(N0=%d), %.1f s" % (full[0], full[1], F, x.shape[1], dtf)}
        del y
    return out


def csrc_sha16():
    """sha256 over the kernel sources (csrc/*.hip, *.h and include/fgc.h, sorted by name), first 16 hex digits: what a
    PMC pass under profiles/ is valid for.  (.git does not travel to the GPU box; file contents do.)"""
    import glob
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(REPO, "facet_graph_convolution_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))) + \
            [os.path.join(REPO, "include", "fgc.h")]:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def load_traffic_db(dtype, nu, nv):
    """PMC traffic (FETCH_SIZE x 2 + WRITE_SIZE, separate rocprofv3 --pmc passes; tools/pmc_traffic.sh) of the newest
    pass kept under profiles/ - used only when it was taken on THIS build's kernel sources and on this workload.
    Returns (db, note)."""
    import glob
    suffix = "_bf16" if dtype == "bf16" else ""
    cands = sorted(glob.glob(os.path.join(REPO, "profiles", "r*_traffic_families%s.json" % suffix)), reverse=True)
    if not cands or (nu, nv) != (250, 200):
        return {}, "no PMC pass recorded for this workload"
    db = json.load(open(cands[0]))
    meta = db.get("meta", {})
    have = meta.get("csrc_sha16")
    if have != csrc_sha16():
        return {}, "stale: %s was taken on kernel sources %s (commit %s), this build is %s - rerun tools/pmc_traffic.sh" % (
            os.path.basename(cands[0]), have, meta.get("commit"), csrc_sha16())
    return db, "%s (commit %s, kernel sources %s)" % (os.path.basename(cands[0]), meta.get("commit"), have)


def load_binds(dtype):
    """What the SQ counter passes found binding the dominant kernels (tools/pmc_sq.sh): a sentence kept next to the counter
    tables under profiles/ (r*_binds.json: {"csrc_sha16", "f32", "bf16"}) and quoted only when those passes were taken on THIS
    build's kernel sources; None otherwise - counter findings do not outlive the kernels they were measured on."""
    import glob
    cands = sorted(glob.glob(os.path.join(REPO, "profiles", "r*_binds.json")), reverse=True)
    if not cands:
        return None
    try:
        b = json.load(open(cands[0]))
    except (OSError, ValueError):
        return None
    return b.get(dtype) if b.get("csrc_sha16") == csrc_sha16() else None


# kernel name -> family (the kernel FUNCTION, all template instances and both directions of the shared core together)
def family_of(kern):
    if "conv_w8_kernel" in kern or "conv_fwd_kernel" in kern or "conv_bwd_data_kernel" in kern:
        return "conv_w8"
    if "conv_bwd_logits" in kern:
        return "conv_bwd_logits"
    if "mlp_bwd_kernel" in kern or "mlp_fwd_kernel" in kern:
        return "mlp"
    if "gemm_tn" in kern:
        return "gemm_tn"
    if "conv_narrow" in kern or "narrow_" in kern:
        return "conv_narrow"
    return kern.split("<")[0]


DUMP_LIMIT_BYTES = 64 << 20


def write_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: every array as out_dir/<name>.npy, float64 kept, anything else as float32.  If they hold more than
    `limit` bytes in all, an array larger than its equal share of the limit keeps a seeded sample of its rows (sorted; the
    same rows for the same shape on every run), so that two builds stay comparable output for output.  Returns the names."""
    os.makedirs(out_dir, exist_ok=True)
    arrs = {}
    for name, a in arrays.items():
        a = np.atleast_1d(np.asarray(a))
        arrs[name] = a if a.dtype == np.float64 else a.astype(np.float32)
    if sum(a.nbytes for a in arrs.values()) > limit:
        share = limit // len(arrs)
        for name, a in arrs.items():
            if a.nbytes > share:
                keep = max(1, share // (a.nbytes // a.shape[0]))
                arrs[name] = a[np.sort(np.random.RandomState(0).choice(a.shape[0], keep, replace=False))]
    for name, a in arrs.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return sorted(arrs)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if os.environ.get("FGC_BENCH_ARGV") and "WORLD_SIZE" in os.environ:
        argv = json.loads(os.environ["FGC_BENCH_ARGV"])      # a rank of our own self-launch: the parent's full argv
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args, argv))

    # a rank that dies by a signal (SIGABRT from the runtime, SIGSEGV) leaves its Python stack on stderr
    faulthandler.enable(file=sys.stderr, all_threads=True)
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    # FGC_BENCH_BACKEND=gloo rehearses the N > 1 path with several ranks on ONE GPU (host-staged exchange)
    backend = os.environ.get("FGC_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    local_dev = local_rank % max(ndev, 1) if backend == "gloo" else local_rank
    torch.cuda.set_device(local_dev)
    dev = torch.device("cuda", local_dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from facet_graph_convolution_amd.net import FacetDenoiser
    from facet_graph_convolution_amd.utils import rand_rotation_matrix

    train = args.what == "train"
    shard = world > 1 and args.mode == "shard"
    mk = dict(seed=0, multi_scale=args.multi_scale, dtype=args.dtype)
    startup = {}
    t_start = time.perf_counter()
    if shard:
        from facet_graph_convolution_amd.shard import ShardPlan, DistComm, graphs_to_host_csr
        nu = args.nu * world if args.scaling == "weak" else args.nu
        # rank 0 preprocesses, the others receive the K-lists (FGC_BENCH_LOCAL_PREP=1: every rank builds the same seeded mesh)
        if os.environ.get("FGC_BENCH_LOCAL_PREP"):
            ds, F_total = build_mesh(nu, args.nv, seed=0)
        else:
            ds, F_total = build_mesh_shared(nu, args.nv, 0, rank, world, backend, dev)
        startup["preprocess_s"] = time.perf_counter() - t_start
        t1 = time.perf_counter()
        plan = ShardPlan(graphs_to_host_csr(ds.adj_list[0]), rank, world)
        startup["shard_plan_s"] = time.perf_counter() - t1
        t1 = time.perf_counter()
        net = FacetDenoiser(dev, **mk).bind_mesh(ds.in_list[0], ds.adj_list[0], gt=ds.gt_list[0] if train else None,
                                                 plan=plan, comm=DistComm())
        startup["bind_s"] = time.perf_counter() - t1
        n0 = ds.in_list[0].shape[1]            # samples are drawn over the WHOLE mesh, same stream on every rank
        rs = np.random.RandomState(100)
        F = F_total / world                    # facets per GPU (for the per-GPU accounting below)
        halo_frac = [net._mesh["nh"][l] / max(net._mesh["ns"][l], 1) for l in range(3)]
    else:
        nu = args.nu
        ds, F = build_mesh(args.nu, args.nv, seed=rank)
        startup["preprocess_s"] = time.perf_counter() - t_start
        F_total = F * world
        t1 = time.perf_counter()
        net = FacetDenoiser(dev, **mk).bind_mesh(ds.in_list[0], ds.adj_list[0], gt=ds.gt_list[0] if train else None)
        startup["bind_s"] = time.perf_counter() - t1
        n0 = ds.in_list[0].shape[1]
        rs = np.random.RandomState(100 + rank)
        halo_frac = None

    # per-step random inputs (train.py:561-565) for the whole run, uploaded ONCE: inside the loop they are refreshed by
    # device-to-device copies (stream-ordered with the hipGraph replay); a sharded rank keeps, per step, the samples
    # that fall into its own rows
    nrep = max(args.repeats, 1)
    nsteps_total = args.warmup + args.steps
    samp_host = [rs.randint(n0, size=4000) for _ in range(nsteps_total)]
    rot_host = [rand_rotation_matrix(randnums=rs.uniform(size=3)) for _ in range(nsteps_total)]
    SR_all = FacetDenoiser.pack_step_inputs(samp_host, rot_host, dev)    # row k: samples + rotation of step k
    S_loc = [net.local_samples_device(s) for s in samp_host] if (shard and train) else None
    torch.cuda.synchronize()
    counter = [0]
    auto_graph = args.graph < 0
    args.graph = 0 if auto_graph else args.graph
    if auto_graph and world == 1 and train:
        # A single-GPU training step is timed as ONE replayed hipGraph (the whole forward + backward enqueue captured in the
        # first warm-up step; bit-identical to eager launches: tests/test_gpu_net.py, and `hipgraph_replay.matches_eager` of
        # this line, which also carries the eager time of the same steps).  Config 3 (50k facets, 0.7 ms of GPU time) is
        # shorter on the GPU than its ~45 launches are on the host (0.8 ms of Python + ctypes per step): timed with eager
        # launches it measures the host's jitter.  The 100k-facet headline was GPU-bound with eager launches at 1.78 ms; at
        # 1.61 ms the gaps between its 48 launches show: replay 1.594 - 1.600 against 1.616 - 1.618 eager on two of three
        # boxes (profiles/r5_c_bench_three_boxes.txt).  `--graph 0` times eager launches.
        args.graph = 1
    # A facet-sharded training run times EAGER launches unless --graph 1 asks for hipGraph segments between the exchanges
    # (3 - 5 % less host time per step on two gloo ranks; the GPU time of a step exceeds the host's either way).  Round 3
    # made segments the default of N > 1; one full-suite run of that round aborted for a reason its lost output no longer
    # tells, a rank that dies by a signal takes the driver's whole scaling run with it, and RCCL
    # next to graph replays has never run on a real node: the default is the path with nothing unknown in it.
    graph_mode = [bool(shard and train and args.graph == 1)]
    if graph_mode[0]:
        args.graph = 0          # (segments, not the whole-step graph of the single-GPU --graph 1)

    def step():
        k = counter[0] % nsteps_total
        counter[0] += 1
        if not train:
            net.forward_multi_scale() if args.multi_scale else net.forward(rotate=False)
            return
        net.set_step_inputs_packed(SR_all[k], S_loc[k] if S_loc else None, in_place=True)
        net.forward_backward(rotate=True, capture=bool(args.graph) or graph_mode[0])
        if world > 1 and not shard:
            if backend == "nccl":
                dist.all_reduce(net.params.grad, op=dist.ReduceOp.AVG)
            else:
                g = net.params.grad.cpu()
                dist.all_reduce(g)
                net.params.grad.copy_(g / world)
        net.adam_step()
        if os.environ.get("FGC_BENCH_TRACE"):
            print("trace loss %.3f" % net.buffers["loss"][0].item(), file=sys.stderr)

    def sync_barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    def timed_block():
        import gc as _gc
        was = _gc.isenabled()
        _gc.disable()
        try:
            sync_barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            sync_barrier()
            dt = time.perf_counter() - t0
        finally:
            if was:
                _gc.enable()
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = t.item()
        return dt

    if graph_mode[0]:
        try:
            step()                           # eager warm-up step + capture of the schedule's segments
            step()
        except Exception as e:               # noqa: BLE001 - any capture problem: the eager schedule is the same arithmetic
            print("bench: hipGraph segments unavailable (%s: %s), timing eager launches" % (type(e).__name__, e), file=sys.stderr)
            graph_mode[0] = False
            net._graph_fb = None
    launch_mode = "hipGraph segments between the exchanges" if graph_mode[0] else "eager launches"
    # (the collector OFF for the measurement - gc.disable() around every timed block, not only gc.freeze(), which keeps
    #  collecting what is allocated afterwards: a full collection of this process's heap - meshes, plans, job tables - is a
    #  host pause of 10 - 40 ms, which eager launches turn into an idle GPU: one K-step block in five read 3.5 instead of
    #  1.65 ms in round 5's eager rows)
    import gc
    gc.collect()
    gc.freeze()
    # Facet-sharded: HOW MUCH of the schedule overlaps its exchanges is a latency question.  An exchange that nothing overlaps is
    # one blocking call - a synchronous collective on the compute stream; an overlapped one is asynchronous, i.e. on RCCL's own
    # stream behind two cross-stream dependencies that cost ~20 us by themselves (tools/rccl_call_cost_probe.py), which pays
    # only if the collective lasts longer than that.  Three things overlap: the interior tiles of a layer with at least
    # net.split_min_tiles of them (at the price of a second, half-empty launch), and - net.dw_in_window - the previous layer's
    # weight-gradient stage inside a layer's backward exchange window.  The defaults (1024, window) were set on an EMULATED
    # latency (two shards in one process, tools/shard_latency_probe.py: they win above ~30 us per collective, lose 2 - 3 % below);
    # what a grouped all-to-all costs on xGMI is not known here.  So the job measures on ITS OWN collectives, before the
    # warm-up: a few steps per candidate, two interleaved passes, max over ranks through an all-reduce (every rank reads the same
    # numbers and takes the same decision); the default is kept unless a candidate is 3 % faster.  FGC_SPLIT_MIN_TILES or
    # FGC_NO_DW_IN_WINDOW set: no tuning.
    split_tune = None
    if shard and train and not graph_mode[0] and "FGC_SPLIT_MIN_TILES" not in os.environ and "FGC_NO_DW_IN_WINDOW" not in os.environ \
            and getattr(net, "overlap", False):
        default = (net.split_min_tiles, net.dw_in_window)
        cands = [default, (default[0], False), (1 << 30, False), (256, True), (64, True)]
        label = lambda c: "%s/%s" % ("none" if c[0] >= 1 << 30 else c[0], "window" if c[1] else "behind")
        try:
            ntune = max(3, min(8, args.steps))
            res = {}
            for _pass in range(2):           # (two interleaved passes, the minimum per candidate: one slow block must not decide)
                for c in cands:
                    net.split_min_tiles, net.dw_in_window = c
                    step()
                    step()
                    sync_barrier()
                    t0 = time.perf_counter()
                    for _ in range(ntune):
                        step()
                    sync_barrier()
                    tt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
                    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                    res[c] = min(res.get(c, 1e30), tt.item() / ntune * 1e3)
            best = min(res, key=res.get)
            chosen = best if res[best] < 0.97 * res[default] else default
            net.split_min_tiles, net.dw_in_window = chosen
            split_tune = {"ms_per_step": {label(c): round(v, 4) for c, v in res.items()}, "steps_each": ntune, "passes": 2,
                          "chosen": label(chosen), "default": label(default),
                          "candidates": "split threshold (interior tiles) / weight-gradient stage in the next layer's exchange window or behind its data kernel",
                          "rule": "a candidate replaces the default if it is 3 % faster"}
        except Exception as e:               # noqa: BLE001 - an optimisation: its failure leaves the default schedule
            net.split_min_tiles, net.dw_in_window = default
            split_tune = {"error": "%s: %s" % (type(e).__name__, str(e)[:200]), "chosen": label(default), "default": label(default)}
            print("bench: schedule tuning failed (%s), default kept" % split_tune["error"], file=sys.stderr)
    w_done = 0
    graph_note = None
    if args.graph and world == 1 and train:
        # (also with --warmup 0: the capture is never part of the timed block)
        # the first warm-up step captures the step's hipGraph: if this runtime refuses (it never has), the same arithmetic is
        # timed with eager launches and the line says so, instead of there being no line
        try:
            step()
        except Exception as e:               # noqa: BLE001
            graph_note = "hipGraph capture failed (%s: %s); timed with eager launches" % (type(e).__name__, str(e)[:200])
            print("bench: " + graph_note, file=sys.stderr)
            net._graph_fb = None
            args.graph = 0
            torch.cuda.synchronize()
            step()
        w_done = 1
    # Clock warm-up: min(K, 50) eager steps of the same work as the timed region, behind the capture step and in front of the
    # other warm-up steps, so that no host-only stretch separates them from the timed block.  The contract's W steps are too
    # short for it: a GPU that idled through the mesh preprocessing runs its first ~15 steps 3 - 15 % slow
    # (profiles/r5_first_steps_probe.txt; the driver's --warmup 5 --steps 20 sat inside that ramp).  With --full the same steps
    # carry the per-kernel durations (hipEvents recorded by the library around every launch, same stream); a plain run takes
    # them without, so both walk the same steps and compute the same outputs.  The timed region itself is unchanged: W untimed
    # steps, then exactly K steps between barriers.  Facet-sharded: every rank runs the steps (they hold collectives), rank
    # 0's table is the one reported; a layer that runs as interior | exchange | boundary launches counts with the SUM of its
    # launches.
    prof = None
    ramp = min(args.steps, 50) if train and (shard or world == 1) else 0
    if ramp:
        profile = args.full and not args.no_roofline
        if profile:
            net.profile_start()
        for k in range(ramp):
            kk = k % nsteps_total
            net.set_step_inputs_packed(SR_all[kk], S_loc[kk] if S_loc else None, in_place=True)
            net.forward_backward(rotate=True, capture=False)
            net.adam_step()
        if profile:
            prof = net.profile_stop()
    for _ in range(args.warmup - w_done):
        step()
    dt = timed_block()                       # THE timed region: exactly K steps, max over ranks
    loss = net.buffers["loss"][0].item() if train else None
    if args.dump_outputs and rank == 0:
        # what the last timed step handed its caller (a sharded run: rank 0's rows), before any extra touches the network
        B = net.buffers
        outs = ({"loss": B["loss"], "normals": B["nconv"], "grad": net.params.grad, "weights": net.params.theta} if train else
                {"normals": B["nconv"]})
        if args.multi_scale:
            outs.update(normals_level1=B["nconv1"], normals_level2=B["nconv2"])
        write_outputs(args.dump_outputs, {k: (t.detach() if t.dtype == torch.float64 else t.detach().float()).cpu().numpy()
                                          for k, t in outs.items()})
    # the same K-step block again (extras: spread of the measurement)
    rep_ms = [dt / args.steps * 1e3] + ([timed_block() / args.steps * 1e3 for _ in range(nrep - 1)] if args.full else [])

    # the same steps as hipGraph replays (one graph per step holds the whole forward+backward enqueue), untimed extra:
    # a second network from the same seed walks the same inputs, so its final loss must equal the eager one bit for bit
    hipgraph = None
    if args.full and world == 1 and train and (not args.graph or auto_graph):
        net_g = FacetDenoiser(dev, **mk).bind_mesh(ds.in_list[0], ds.adj_list[0], gt=ds.gt_list[0])
        net_e = FacetDenoiser(dev, **mk).bind_mesh(ds.in_list[0], ds.adj_list[0], gt=ds.gt_list[0])

        def walk(nn, capture):
            for k in range(args.warmup):
                nn.set_step_inputs_packed(SR_all[k], in_place=True)
                nn.forward_backward(rotate=True, capture=capture)
                nn.adam_step()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for k in range(args.warmup, nsteps_total):
                nn.set_step_inputs_packed(SR_all[k], in_place=True)
                nn.forward_backward(rotate=True, capture=capture)
                nn.adam_step()
            torch.cuda.synchronize()
            return time.perf_counter() - t, nn.buffers["loss"][0].item()

        try:
            te, loss_e = walk(net_e, False)
            tg, loss_g = walk(net_g, True)
            hipgraph = {"ms_per_step": tg / args.steps * 1e3, "loss_deg": loss_g, "matches_eager": loss_g == loss_e,
                        "eager_ms_per_step": te / args.steps * 1e3, "timed_region": "hipgraph" if args.graph else "eager"}
        except Exception as e:               # noqa: BLE001 - an extra: its failure is recorded, the headline's line is printed
            hipgraph = {"error": "%s: %s" % (type(e).__name__, str(e)[:200]), "timed_region": "hipgraph" if args.graph else "eager"}
            print("bench: the eager / replay comparison failed (%s)" % hipgraph["error"], file=sys.stderr)
        del net_g, net_e
    elif args.full and shard and train and graph_mode[0]:
        # sharded: the timed region replayed one hipGraph per stretch of launches between two exchanges (the exchanges
        # eager in between); the same K steps with eager launches beside it
        graph_mode[0] = False
        te = timed_block()
        graph_mode[0] = True
        hipgraph = {"ms_per_step": dt / args.steps * 1e3, "eager_ms_per_step": te / args.steps * 1e3,
                    "graphs_per_step": sum(1 for sg in net._graph_fb[0] for g, _ in sg if g is not None), "matches_eager": None,
                    "timed_region": "hipgraph"}

    # forward-only rate (BASELINE config 2 wording), untimed extra
    fwd_ms = None
    if args.full:
        torch.cuda.synchronize()
        nf = max(3, args.steps // 2)
        t1 = time.perf_counter()
        for _ in range(nf):
            net.forward(rotate=False)
        torch.cuda.synchronize()
        fwd_ms = (time.perf_counter() - t1) / nf * 1e3
        if world > 1:
            dist.barrier()

    # sharded runs: what the exchanges cost when nothing overlaps them (blocking, timed on the host around device
    # synchronises), and how many collectives a step issues
    exchange = None
    if args.full and shard:
        exchange = net.measure_exchanges(lambda: step(), steps=max(2, min(5, args.steps)))
        dist.barrier()

    def analyse(net_, prof, steps_, dtype_, nu_, nv_, dump_=""):
        """(roofline, families, pair_form, kernels) from a table of hipEvent durations (net.profile_stop) taken over steps_
        eager training steps of net_: the dominant kernel FAMILY through its launch with the most algorithmic work."""
        roofline, families, kernels = None, None, {}
        peak = PEAK_BF16_MFMA_TFLOPS if dtype_ == "bf16" else PEAK_F32_MFMA_TFLOPS
        dims = {name: (n, nnz, cin, cout) for name, n, nnz, cin, cout in net_.layer_dims()}
        pdims = net_.pair_dims()
        pair_form = {name: {"coarse_rows": nc, "pairs": npairs, "executed_gflop": 0.0, "us_per_step": 0.0,
                            # what the SURVEY convention counts for the layer (forward + d-logits + data + weight gradient)
                            "survey_gflop": round(sum(kernel_flops(k, *dims[name]) for k in
                                                      ("fwd", "bwd_logits", "bwd_data", "bwd_weight")) / 1e9, 3)}
                     for name, (nc, npairs) in pdims.items()}
        total_ms = sum(ms for _, ms in prof.values())
        rows = []
        abytes = {}
        row_peak = {}
        from facet_graph_convolution_amd import _lib as _l
        mlp_on_bf16_pipe = _l.get_option("NO_MLP_SPLIT") != 1
        for key, (cnt, ms) in prof.items():
            tag, kern = key.split("/", 1)
            phase, layer = (tag.split(":") + [""])[:2]
            kind = None
            if layer in dims:
                if "conv_fwd_kernel" in kern or "conv_w8_kernel<fwd>" in kern:
                    kind = "fwd"
                elif "conv_bwd_logits" in kern:
                    kind = "bwd_logits"
                elif "conv_bwd_data_kernel" in kern or "conv_w8_kernel<data>" in kern:
                    kind = "bwd_data"
                elif "gemm_tn" in kern and cnt == steps_:
                    kind = "bwd_weight"
            avg_us = ms / cnt * 1e3
            if kind in ("fwd", "bwd_data") and cnt > steps_ and cnt % steps_ == 0:
                avg_us = ms / steps_ * 1e3        # interior + boundary launches of one layer: their sum
            fl = kernel_flops(kind, *dims[layer]) if kind else None
            by = kernel_bytes(kind, layer, *dims[layer], 2 if dtype_ == "bf16" else 4) if kind else None
            if layer == "reduce" and "gemm_tn" in kern:
                # the weight-gradient GEMMs of all layers, grouped into one launch per kernel form at the end of the backward
                # pass (FGC_CONV_DEFER_DW): the work of all of them over these launches; pair layers with what they execute
                # (fp32 groups only the layers whose r is small - net.grouped_dw_layers -, bf16 all of them)
                in_group = getattr(net_, "grouped_dw_layers", None) or set(dims)
                dw = {name: (pair_kernel_flops("gemm_tn", pdims[name][0], pdims[name][1], dims[name][2], dims[name][3])
                             if name in pdims else kernel_flops("bwd_weight", *dims[name])) for name in dims if name in in_group}
                fl = sum(dw.values()) / max(cnt / steps_, 1.0)
                for name in pdims:
                    if name in dw:
                        pair_form[name]["executed_gflop"] += dw[name] / 1e9
            if layer in pdims:      # pair form: the FLOPs the launch executes, not the fine-form convention
                fl = pair_kernel_flops(kern, pdims[layer][0], pdims[layer][1], dims[layer][2], dims[layer][3])
                by = None
                pair_form[layer]["executed_gflop"] += (fl or 0.0) * cnt / steps_ / 1e9
                pair_form[layer]["us_per_step"] += ms / steps_ * 1e3
            if layer == "mlp" and ("mlp_fwd_kernel" in kern or "mlp_bwd_kernel" in kern) and dtype_ == "f32" and mlp_on_bf16_pipe:
                # the fp32 network's MLP on the bf16 matrix pipe (three-term operand splits: six bf16 products per fp32
                # product): its roofline is that pipe's peak over six, in fp32-equivalent FLOPs
                row_peak[key] = PEAK_BF16_MFMA_TFLOPS / 6.0
            if layer == "mlp" and ("mlp_fwd_kernel" in kern or "mlp_bwd_kernel" in kern):
                # 32 -> 1024 -> 3 per padded node; the backward recomputes the hidden layer and adds dW and dx
                fl = 2.0 * dims["conv1"][0] * 1024 * (32 + 3) * (3 if "mlp_bwd_kernel" in kern else 1)
                if "<" in kern:      # the bf16 backward is two launches (dx: 2 of the 3 products, w: 2 of the 3)
                    fl = fl * 2.0 / 3.0
                by = dims["conv1"][0] * (32 * (2 if dtype_ == "bf16" else 4) + 12.0) * (2 if "bwd" in kern else 1)
            rows.append((ms, key, cnt, avg_us, fl))
            abytes[key] = by
        rows.sort(reverse=True)
        if dump_ and rank == 0:
            with open(dump_, "w") as fh:
                for ms, key, cnt, avg_us, fl in rows:
                    fh.write("%-60s launches/step %4.1f  avg %9.2f us  per-step %9.2f us  share %5.2f%%  %s\n" % (
                        key, cnt / steps_, avg_us, ms / steps_ * 1e3, 100 * ms / total_ms,
                        ("%.1f TFLOP/s" % (fl / (avg_us * 1e-6) / 1e12)) if fl else ""))
        for ms, key, cnt, avg_us, fl in rows[:12]:
            kernels[key] = {"launches": cnt, "avg_us": round(avg_us, 2), "share": round(ms / total_ms, 4),
                            "tflops": round(fl / (avg_us * 1e-6) / 1e12, 2) if fl else None,
                            "frac_of_its_pipe": round(fl / (avg_us * 1e-6) / 1e12 / row_peak.get(key, peak), 4) if fl else None}
        # families = kernel FUNCTIONS (conv_w8 forward and data-gradient are the same kernel over the graph and its
        # transpose); HBM bytes per launch of each family's reported launch from the PMC passes kept under profiles/
        # (FETCH_SIZE x 2 + WRITE_SIZE, gfx950 correction of MI355X_MICROARCH.md); null when no pass is recorded
        traffic_db, traffic_note = ({}, "PMC passes are taken on the single-GPU run") if shard else \
            load_traffic_db(dtype_, nu_, nv_)
        fam = {}
        for ms, key, cnt, avg_us, fl in rows:
            f = fam.setdefault(family_of(key.split("/", 1)[1]), {"ms": 0.0, "flop": 0.0, "rows": []})
            f["ms"] += ms
            f["flop"] += (fl or 0.0) * cnt
            f["rows"].append((ms, key, cnt, avg_us, fl))
        ranked = sorted((k for k in fam if fam[k]["flop"] > 0), key=lambda k: -fam[k]["ms"])
        families = []
        for name in ranked[:3]:
            f = fam[name]
            # the launch with the most algorithmic work (ties: first by name, so the choice does not flip from run to run)
            top = sorted((r for r in f["rows"] if r[4]), key=lambda r: (-r[4], r[1]))[0]
            ach = top[4] / (top[3] * 1e-6) / 1e12
            tr = traffic_db.get(top[1])
            ab = abytes.get(top[1])
            fpeak = row_peak.get(top[1], peak)
            families.append({"family": name, "share_of_step": round(f["ms"] / total_ms, 4),
                             "algorithmic_bytes": ab,
                             "hbm_gbs": round(ab / (top[3] * 1e-6) / 1e9, 1) if ab else None,
                             "hbm_frac": round(ab / (top[3] * 1e-6) / 1e9 / PEAK_HBM_GBS, 4) if ab else None,
                             "us_per_step": round(f["ms"] / steps_ * 1e3, 1),
                             "family_tflops": round(f["flop"] / (f["ms"] * 1e-3) / 1e12, 2),
                             "family_frac": round(f["flop"] / (f["ms"] * 1e-3) / 1e12 / fpeak, 4),
                             "kernel": top[1], "avg_kernel_us": round(top[3], 2), "launch_flops": top[4],
                             "achieved": round(ach, 2), "frac": round(ach / fpeak, 4), "peak": round(fpeak, 1),
                             "pipe": ("bf16 MFMA, fp32 operands as three-term splits (6 bf16 products per fp32 product): peak = "
                                      "%.0f / 6 fp32-equivalent TFLOP/s" % PEAK_BF16_MFMA_TFLOPS) if fpeak != peak else
                                     ("bf16 MFMA" if dtype_ == "bf16" else "fp32 MFMA"),
                             "traffic": tr["hbm_bytes_per_launch"] if tr else None})
        # The launch `roofline` names is the one that takes the most TIME per step among the launches with a work model
        # (round-5 review: the family's best launch is not the launch that dominates time); the best launch of its family
        # rides along as `family_best`.
        def launch_row(r):
            ms_, key_, cnt_, avg_, fl_ = r
            ab_ = abytes.get(key_)
            pk_ = row_peak.get(key_, peak)
            tr_ = traffic_db.get(key_)
            ach_ = fl_ / (avg_ * 1e-6) / 1e12
            return {"kernel": key_, "family": family_of(key_.split("/", 1)[1]), "avg_kernel_us": round(avg_, 2),
                    "us_per_step": round(ms_ / steps_ * 1e3, 2), "launch_flops": fl_, "achieved": round(ach_, 2),
                    "frac": round(ach_ / pk_, 4), "peak": round(pk_, 1), "algorithmic_bytes": ab_,
                    "hbm_gbs": round(ab_ / (avg_ * 1e-6) / 1e9, 1) if ab_ else None,
                    "hbm_frac": round(ab_ / (avg_ * 1e-6) / 1e9 / PEAK_HBM_GBS, 4) if ab_ else None,
                    "traffic": tr_["hbm_bytes_per_launch"] if tr_ else None}
        modelled = [r for r in rows if r[4] and (dtype_ != "bf16" or abytes.get(r[1]))]
        dom = launch_row(max(modelled, key=lambda r: (r[0], r[1]))) if modelled else None
        fam_best = None
        if dom:
            same = [launch_row(r) for r in modelled if family_of(r[1].split("/", 1)[1]) == dom["family"]]
            bkey = "hbm_frac" if dtype_ == "bf16" else "frac"
            b = max(same, key=lambda d_: (d_[bkey] or 0.0, d_["kernel"]))
            fam_best = {k_: b[k_] for k_ in ("kernel", "avg_kernel_us", "achieved", "frac", "hbm_gbs", "hbm_frac")}
            fshare = {f_["family"]: f_ for f_ in families}.get(dom["family"], {})
            dom["share_of_step"] = fshare.get("share_of_step", round(fam[dom["family"]]["ms"] / total_ms, 4))
            dom["family_frac"] = fshare.get("family_frac")
        if dom and dtype_ == "bf16":
            # bf16 storage: the matrix products are 16x cheaper, the bound to quote is HBM - the
            # kernels are far from it too: they are bound by vector-ALU issue in the aggregation
            d = dom
            roofline = {"bound": "hbm", "kernel": d["kernel"], "family": d["family"], "achieved": d["hbm_gbs"],
                        "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": d["hbm_frac"], "traffic": d["traffic"],
                        "avg_kernel_us": d["avg_kernel_us"], "launch_bytes": d["algorithmic_bytes"],
                        "mfma_tflops": d["achieved"], "mfma_frac": d["frac"],
                        "selected_by": "largest time per step among the launches with a work model", "family_best": fam_best,
                        # what the counters say binds the bf16 kernels (the contract's `bound` is the roofline quoted)
                        "binds": load_binds("bf16"),
                        "family_share_of_step": d["share_of_step"],
                        "eager_step_ms_sum_of_kernels": round(total_ms / steps_, 3),
                        "traffic_whole_step": traffic_db.get("whole_step", {}).get("hbm_bytes_per_step"),
                        "traffic_source": traffic_note,
                        "launches_per_step": round(sum(c for c, _ in prof.values()) / steps_, 1)}
        elif dom:
            d = dom
            roofline = {"bound": "mfma", "kernel": d["kernel"], "family": d["family"], "achieved": d["achieved"],
                        "peak": d["peak"], "unit": "TFLOP/s", "frac": d["frac"], "traffic": d["traffic"],
                        "avg_kernel_us": d["avg_kernel_us"], "launch_flops": d["launch_flops"],
                        "selected_by": "largest time per step among the launches with a work model", "family_best": fam_best,
                        "family_share_of_step": d["share_of_step"], "family_frac": d["family_frac"],
                        "binds": load_binds("f32"),
                        "eager_step_ms_sum_of_kernels": round(total_ms / steps_, 3),
                        "traffic_whole_step": traffic_db.get("whole_step", {}).get("hbm_bytes_per_step"),
                        "traffic_source": traffic_note,
                        "launches_per_step": round(sum(c for c, _ in prof.values()) / steps_, 1)}

        return roofline, families, pair_form, kernels

    roofline = None
    families = None
    pair_form = None
    kernels = {}
    if prof is not None:
        # per-kernel durations from hipEvents recorded by the library around every launch (same stream), over
        # `steps` eager steps of the same work as the timed region.  Facet-sharded: every rank runs the steps (they hold
        # collectives), rank 0's table is the one reported; a layer that runs as interior | exchange | boundary launches
        # counts with the SUM of its launches
        roofline, families, pair_form, kernels = analyse(net, prof, ramp, args.dtype, args.nu, args.nv, args.dump_kernels)

    fwd_b, fb_b = algorithmic_bytes_fwd_bwd(net, elem=2 if args.dtype == "bf16" else 4)
    n0_line = n0
    # ---- beside the headline, after the timed region, never part of `value` --------------------------------------------
    def side_step_bench(ds_, dtype_, nu_, nv_, label, warm=10, steps_=30):
        """One more training-step measurement on one GPU: eager launches AND the step replayed from one hipGraph (a step
        shorter on the GPU than its launches are on the host - config 3 - is trained from the graph), with the roofline of
        its dominant launch.  Own network, own step inputs (seed 200)."""
        n0_ = ds_.in_list[0].shape[1]
        rs_ = np.random.RandomState(200)
        tot = warm + steps_
        SR = FacetDenoiser.pack_step_inputs([rs_.randint(n0_, size=4000) for _ in range(tot)],
                                            [rand_rotation_matrix(randnums=rs_.uniform(size=3)) for _ in range(tot)], dev)
        res = {"workload": label, "dtype": dtype_, "steps": steps_, "warmup": warm}
        for mode in ("eager", "hipgraph"):
            nn = FacetDenoiser(dev, seed=0, dtype=dtype_).bind_mesh(ds_.in_list[0], ds_.adj_list[0], gt=ds_.gt_list[0])
            for k in range(warm):
                nn.set_step_inputs_packed(SR[k], in_place=True)
                nn.forward_backward(rotate=True, capture=(mode == "hipgraph"))
                nn.adam_step()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for k in range(warm, tot):
                nn.set_step_inputs_packed(SR[k], in_place=True)
                nn.forward_backward(rotate=True, capture=(mode == "hipgraph"))
                nn.adam_step()
            torch.cuda.synchronize()
            res["ms_per_step_" + mode] = (time.perf_counter() - t) / steps_ * 1e3
            res["loss_deg_" + mode] = nn.buffers["loss"][0].item()
            if mode == "eager" and not args.no_roofline:
                nn.profile_start()
                for k in range(steps_):
                    nn.set_step_inputs_packed(SR[k % tot], in_place=True)
                    nn.forward_backward(rotate=True, capture=False)
                    nn.adam_step()
                rl, fams, _, _ = analyse(nn, nn.profile_stop(), steps_, dtype_, nu_, nv_)
                res["roofline"] = rl
                res["launches_per_step"] = rl["launches_per_step"] if rl else None
                res["algorithmic_bytes_per_step"] = algorithmic_bytes_fwd_bwd(nn, elem=2 if dtype_ == "bf16" else 4)[1]
            del nn
        F_ = 2 * nu_ * nv_
        best = min(res["ms_per_step_eager"], res["ms_per_step_hipgraph"])
        res["facets"] = F_
        res["facets_per_s"] = F_ / (best * 1e-3)
        res["matches_eager"] = res["loss_deg_eager"] == res["loss_deg_hipgraph"]
        if "algorithmic_bytes_per_step" in res:
            res["hbm_roofline_frac_whole_step"] = res["algorithmic_bytes_per_step"] / (best * 1e-3) / (PEAK_HBM_GBS * 1e9)
        return res

    def make_record(also, strong, cpu):
        ms_step = dt / args.steps * 1e3
        step_bytes = fb_b if train else fwd_b
        mesh_txt = "torus %dx%d quads = %d facets%s (N0=%d padded nodes%s)" % (
            nu, args.nv, int(F_total if shard else F), "" if shard else " per GPU", n0_line, " in the whole mesh" if shard else "")
        what_txt = ("rotate + forward + angular loss + backward + Adam" if train else
                    "multi-scale denoising forward (three heads, each normalised)")
        out = {
            "metric": ("facets/sec (fwd+bwd) on 100k-facet mesh" if train else "facets/sec (multi-scale denoising forward)"),
            "value": F_total * args.steps / dt,
            "unit": "facets/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_step,
            "higher_is_better": True,
            "scaling": args.scaling if shard else "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {"workload": "%s: %s, full graph U-Net + MLP%s: %s, %s%s" % (
                           args.config, mesh_txt, " with the multi-scale heads" if args.multi_scale else "", what_txt,
                           "fp32" if args.dtype == "f32" else "bf16 storage / fp32 accumulate, fp32 master weights",
                           ", hipGraph replay" if (args.graph and not shard) else ""),
                       "parallelism": ("single GPU" if world == 1 else
                                       ("one %d-facet mesh facet-sharded over %d GPUs (%s world size %d), halo all-to-all per "
                                        "conv + flat-gradient all-reduce; halo/owned rows per level on rank 0: %s; %s%s" %
                                        (F_total, world, "RCCL" if backend == "nccl" else backend, dist.get_world_size(),
                                         ", ".join("%.3f" % h for h in halo_frac),
                                         "%d collectives per step, %.3f ms per step when exchanged blocking; " % (
                                             exchange["collectives_per_step"], exchange["blocking_ms_per_step"])
                                         if exchange else "", launch_mode)) if shard else
                                       "1 mesh per GPU, flat-gradient all-reduce (%s world size %d)" % (
                                           "RCCL" if backend == "nccl" else backend, dist.get_world_size()))},
            "loss_deg": loss,
            # what the process ran, in order (round 6: the hipEvent pass moved in front; the timed region is W + K steps as ever)
            "timeline": ("%s%sW = %d untimed warm-up steps -> K = %d timed steps between barriers%s" % (
                "schedule tuning (`split_tune`) -> " if split_tune is not None else "",
                ("per-kernel hipEvent pass (%d eager steps; also warms the clocks) -> " % ramp if prof is not None else
                 "clock warm-up (%d eager steps) -> " % ramp if ramp else ""),
                args.warmup, args.steps, " -> untimed extras" if args.full else "")),
            "startup_s": {k: round(v, 2) for k, v in startup.items()},
            "world_check": world_check,
            "repeats_ms_per_step": [round(v, 4) for v in rep_ms],
            "ms_per_step_min": min(rep_ms),
            "ms_per_step_median": float(np.median(rep_ms)),
            "hipgraph_replay": hipgraph,
            "retry_note": os.environ.get("FGC_BENCH_RETRY_NOTE") or graph_note,
            "split_tune": split_tune,
            "forward_only_ms": fwd_ms,
            "forward_only_facets_per_s": F_total / (fwd_ms * 1e-3) if fwd_ms else None,
            "hbm_roofline_frac_whole_step": step_bytes / (ms_step * 1e-3) / (PEAK_HBM_GBS * 1e9),
            "algorithmic_bytes_per_step": step_bytes,
            "exchange": exchange,
            "roofline": roofline,
            "families": families,
            # layers run on their coarse source rows (pair form): executed vs SURVEY-convention FLOPs, summed kernel time
            "pair_form": ({k: {kk: (round(vv, 3) if isinstance(vv, float) else vv) for kk, vv in v.items()}
                           for k, v in pair_form.items()} if pair_form else None),
            "kernels": kernels,
            # config 3 (bf16 train step, 50k facets) and the headline mesh in bf16: eager and replayed, with their rooflines
            "also": also,
            # N > 1, weak: the strong-scaling reading of the same metric (one 100k-facet mesh over the N ranks)
            "strong": strong,
            "cpu_baseline": cpu,
        }
        return out

    # the world as the collective back end itself counts it: every rank contributes a one to an all-reduce
    world_check = None
    if world > 1:
        one = torch.ones(1, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(one)
        world_check = {"backend": "RCCL" if backend == "nccl" else backend, "ranks_in_all_reduce": int(one.item()),
                       "get_world_size": dist.get_world_size()}

    def emit_early(rec, why):
        """The headline record BEFORE any extra runs (stderr and, where gpurun_out/ exists, a file): an extra that dies by a
        signal or never returns must not cost the measurement that was already taken (round-5 advisor finding)."""
        if rank != 0:
            return
        txt = json.dumps(rec)
        print("bench: headline record %s: %s" % (why, txt), file=sys.stderr, flush=True)
        d = os.path.join(REPO, "gpurun_out")
        if os.path.isdir(d):
            try:
                with open(os.path.join(d, "bench_headline_early.json"), "w") as fh:
                    fh.write(txt + "\n")
            except OSError:
                pass

    also = None
    if args.full and world == 1:
        emit_early(make_record(None, None, None), "before the bf16 extras and the CPU baseline")
    if args.full and world == 1 and train and args.config == "c2" and args.dtype == "f32" and (args.nu, args.nv) == (250, 200) \
            and not args.multi_scale and not os.environ.get("FGC_BENCH_NO_ALSO"):
        # BASELINE config 3 (train step, bf16 storage / fp32 accumulate) at its own 50k facets and at the headline's 100k: a
        # few seconds, so that the driver's record carries them.  A build extension (the reference is fp32 only): accepted at
        # the bf16 tolerances of tests/test_gpu_bf16.py / test_gpu_scale.py (normals 5e-3, loss 1e-2 relative, gradients
        # 8e-2 of each tensor's largest entry), never the headline.
        torch.cuda.synchronize()
        t_also = time.perf_counter()
        try:                                    # (an extra: a failure here is recorded, it does not cost the headline's line)
            ds3, _ = build_mesh(250, 100, seed=0)
            also = {"c3_bf16_50k": side_step_bench(ds3, "bf16", 250, 100, "c3: torus 250x100 = 50000 facets, train step, bf16 storage / "
                                                   "fp32 accumulate"),
                    "c2_bf16_100k": side_step_bench(ds, "bf16", 250, 200, "torus 250x200 = 100000 facets, train step, bf16 storage / "
                                                    "fp32 accumulate"),
                    "note": "untimed extras measured after the headline's timed region; bf16 storage is a build extension accepted "
                            "at the tolerances of tests/test_gpu_bf16.py (normals 5e-3, loss 1e-2, gradients 8e-2 of each tensor's "
                            "maximum)"}
            del ds3
            also["seconds"] = round(time.perf_counter() - t_also, 1)
        except Exception as e:                  # noqa: BLE001
            print("bench: the bf16 extras failed: %s: %s" % (type(e).__name__, e), file=sys.stderr)
            also = {"error": "%s: %s" % (type(e).__name__, e)}

    # N > 1, facet-sharded, weak scaling (the driver's run): the OTHER reading of "facets/s on a 100k-facet mesh at N GPUs" -
    # the one 100 000-facet mesh sharded over the N ranks (strong scaling) - measured by the same ranks behind the weak
    # region, with the same barriers and the max over ranks
    strong = None
    line_out = False
    strong_extra = args.full and shard and train and args.scaling == "weak" and args.config == "c2" and \
        not os.environ.get("FGC_BENCH_NO_STRONG")
    if world > 1:
        # N > 1: the ONE JSON line is printed HERE, before the strong-scaling extra, which re-shards, binds a new network and
        # issues collectives: a rank that raises or aborts in there would leave its peers waiting in a collective and the
        # weak-scaling value unprinted.  The extra reports on stderr (`bench: strong-scaling extra: {...}`) and in
        # gpurun_out/bench_strong.json; a watchdog ends the process (exit 0: the line is out) if it does not return.
        if rank == 0:
            print(json.dumps(make_record(None, {"note": "measured after this line was printed: see `bench: strong-scaling "
                                                        "extra` on stderr"} if strong_extra else None, None)), flush=True)
        line_out = True
    if strong_extra:
        import threading
        limit = float(os.environ.get("FGC_BENCH_STRONG_LIMIT_S", "180"))

        def _give_up():
            print("bench: strong-scaling extra did not return within %.0f s on rank %d; leaving (the headline line is out)"
                  % (limit, rank), file=sys.stderr, flush=True)
            os._exit(0)
        watchdog = threading.Timer(limit, _give_up)
        watchdog.daemon = True
        watchdog.start()
        # (an extra behind the headline: whatever goes wrong here - the same thing on every rank, these are the calls the weak
        #  region has just made - must not cost the line; it is recorded instead)
        try:
            del net
            torch.cuda.empty_cache()
            t1 = time.perf_counter()
            ds_s, F_s = build_mesh_shared(args.nu, args.nv, 0, rank, world, backend, dev)
            plan_s = ShardPlan(graphs_to_host_csr(ds_s.adj_list[0]), rank, world)
            net = FacetDenoiser(dev, **mk).bind_mesh(ds_s.in_list[0], ds_s.adj_list[0], gt=ds_s.gt_list[0], plan=plan_s, comm=DistComm())
            n0 = ds_s.in_list[0].shape[1]
            rs_s = np.random.RandomState(300)      # (same stream on every rank: samples are drawn over the whole mesh)
            samp_host = [rs_s.randint(n0, size=4000) for _ in range(nsteps_total)]
            rot_host = [rand_rotation_matrix(randnums=rs_s.uniform(size=3)) for _ in range(nsteps_total)]
            SR_all = FacetDenoiser.pack_step_inputs(samp_host, rot_host, dev)
            S_loc = [net.local_samples_device(sm) for sm in samp_host]
            graph_mode[0] = False
            args.graph = 0
            counter[0] = 0
            setup_s = time.perf_counter() - t1
            for _ in range(args.warmup):
                step()
            dts = timed_block()
            strong = {"scaling": "strong", "workload": "ONE torus %dx%d = %d facets facet-sharded over %d GPUs, train step, eager launches"
                      % (args.nu, args.nv, F_s, world), "facets": F_s, "value": F_s * args.steps / dts, "unit": "facets/s",
                      "ms_per_step": dts / args.steps * 1e3, "steps": args.steps, "warmup": args.warmup,
                      "loss_deg": net.buffers["loss"][0].item(), "setup_s": round(setup_s, 2),
                      "halo_over_owned_rows_rank0": [round(net._mesh["nh"][l] / max(net._mesh["ns"][l], 1), 4) for l in range(3)]}
        except Exception as e:      # noqa: BLE001
            print("bench: strong-scaling extra failed on rank %d: %s: %s" % (rank, type(e).__name__, e), file=sys.stderr)
            strong = {"error": "%s: %s" % (type(e).__name__, e)}
            # (the peers may be waiting in a collective this rank will never join: leave together through the watchdog)
        if rank == 0:
            print("bench: strong-scaling extra: %s" % json.dumps(strong), file=sys.stderr, flush=True)
            d_ = os.path.join(REPO, "gpurun_out")
            if os.path.isdir(d_):
                with open(os.path.join(d_, "bench_strong.json"), "w") as fh:
                    fh.write(json.dumps(strong) + "\n")
        if "error" in strong:
            sys.stderr.flush()
            os._exit(0)
        watchdog.cancel()

    cpu = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        cpu = cpu_baseline()

    if rank == 0 and not line_out:
        print(json.dumps(make_record(also, strong, cpu)))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
