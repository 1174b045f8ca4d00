"""Timing of the closest-point query through the bounding-box tree (ops.closest_point_tree, include/fgc.h:
fgc_closest_point_tree).  Run it on the GPU box:

    python tools/closest_probe.py [OUT.json]          (kept as profiles/closest_probe.json)

Two meshes: the 100k-facet torus(250, 200) and torus(2500, 200) with a million; the points are the mesh's own vertices
displaced by meshgen.add_noise (50 000 and 500 000).  Device events, medians of 10 (the exhaustive search: fewer, it is
points x faces pairs), the build timed separately.  Per mesh: the build (Morton order + tree, tree alone); one
ops.closest_point_tree call with sort_points on (the sort, the scatter and the square root included) and off; the kernel
alone on points already sorted; exhaustive=True; how many points differ between the tree and the exhaustive search (the
invariant says none); the pairs and the boxes a point's lane tested and the nodes and leaves its wave went through, from
the counting build libfgc_cpcount.so.  Last, the wall time of computeMetrics without an option (after a warm-up run), with
--surface and with --surface-only on a folder with the 100k-facet torus and one noisy copy."""
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from facet_graph_convolution_amd import ops  # noqa: E402
from facet_graph_convolution_amd.meshgen import add_noise, torus  # noqa: E402

REPS = 10


def event_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(times))


def count_lib():
    """The probe-only build of csrc/fgc_closest.hip (per-point counters), loaded beside libfgc.so."""
    from facet_graph_convolution_amd import _lib
    csrc = os.path.dirname(_lib.LIB_PATH)
    path = os.path.join(csrc, "libfgc_cpcount.so")
    if not os.path.exists(path):
        import subprocess
        subprocess.check_call(["make", "-C", csrc, "libfgc_cpcount.so"])
    _lib.lib()
    L = ctypes.CDLL(path)
    L.fgc_closest_point_tree_count.restype = ctypes.c_int
    L.fgc_closest_point_tree_count.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                               ctypes.c_uint32] + [ctypes.c_void_p] * 5
    return L


def tested_per_point(L, tree, points):
    """(pairs, boxes, wave_nodes, wave_leaves) [nq] each: what the lane of every point tested and what its wave popped and
    loaded, points in the order given; and the faces found."""
    from facet_graph_convolution_amd._lib import ptr, stream_ptr
    nq = points.shape[0]
    d2 = torch.empty(nq, dtype=torch.float32, device="cuda")
    f = torch.empty(nq, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(nq, 4, dtype=torch.int32, device="cuda")
    rc = L.fgc_closest_point_tree_count(ptr(tree.tree), tree.tree.numel(), tree.nf, ptr(points), nq, 0, ptr(d2), ptr(f), None,
                                        ptr(cnt), stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return cnt[:, 0].double(), cnt[:, 1].double(), cnt[:, 2].double(), cnt[:, 3].double(), f


def probe_mesh(L, n_major, n_minor, reps_exhaustive):
    V, F = torus(n_major, n_minor)
    V, F = np.ascontiguousarray(V, dtype=np.float32), np.asarray(F).astype(np.int32)
    Vd, Fd = torch.from_numpy(V).cuda(), torch.from_numpy(F).cuda()
    P = torch.from_numpy(add_noise(V, F.astype(np.int64))).cuda()
    nf, nq = F.shape[0], P.shape[0]
    out = {"mesh": "torus(%d, %d)" % (n_major, n_minor), "faces": nf, "points": nq}
    order = ops.ray_tree_order(Vd, Fd)
    out["build_ms_order_and_tree"] = event_ms(lambda: ops.ray_tree(Vd, Fd), REPS)
    out["build_ms_tree_alone"] = event_ms(lambda: ops.ray_tree(Vd, Fd, order), REPS)
    tree = ops.ray_tree(Vd, Fd)
    perm = torch.sort(ops._morton30(P), stable=True).indices
    Ps = P[perm].contiguous()
    ms = {"sort_on": [], "sort_off": [], "kernel_on_sorted_points": []}
    for rep in range(2):          # in turns, and again
        ms["sort_on"].append(event_ms(lambda: ops.closest_point_tree(tree, P, sort_points=True), REPS))
        ms["sort_off"].append(event_ms(lambda: ops.closest_point_tree(tree, P, sort_points=False), REPS))
        ms["kernel_on_sorted_points"].append(event_ms(lambda: ops.closest_point_tree(tree, Ps, sort_points=False), REPS))
    for k in ms:
        out["ms_tree_" + k] = float(np.median(ms[k]))
    out["ms_exhaustive"] = event_ms(lambda: ops.closest_point_tree(tree, Ps, sort_points=False, exhaustive=True),
                                    reps_exhaustive, warm=1)
    out["reps_exhaustive"] = reps_exhaustive
    out["pairs_exhaustive"] = float(nq) * nf
    out["pairs_per_s_exhaustive"] = float(nq) * nf / (out["ms_exhaustive"] * 1e-3)
    got = ops.closest_point_tree(tree, P, want_bary=True)
    full = ops.closest_point_tree(tree, P, want_bary=True, exhaustive=True)
    differ = torch.zeros(nq, dtype=torch.bool, device="cuda")
    for a, b in zip(got, full):
        differ |= (a.view(torch.int32) != b.view(torch.int32)).reshape(nq, -1).any(1)
    out["points_that_differ"] = int(differ.sum().item())
    out["dist_mean"], out["dist_max"] = got[0].mean().item(), got[0].max().item()
    for label, pts in (("sort_on", Ps), ("sort_off", P)):
        pairs, boxes, w_nodes, w_leaves, fc = tested_per_point(L, tree, pts)
        out["nodes_per_wave_" + label] = {"mean": w_nodes.mean().item(), "max": w_nodes.max().item()}
        out["leaves_per_wave_" + label] = {"mean": w_leaves.mean().item(), "max": w_leaves.max().item()}
        out["pairs_per_point_" + label] = {"mean": pairs.mean().item(), "max": pairs.max().item()}
        out["boxes_per_point_" + label] = {"mean": boxes.mean().item(), "max": boxes.max().item()}
    assert torch.equal(fc, got[1])          # (the counting build finds what the library finds)
    out["speedup_sort_on_over_exhaustive"] = out["ms_exhaustive"] / out["ms_tree_sort_on"]
    return out


def time_cli():
    from facet_graph_convolution_amd.computeMetrics import computeMetrics
    from facet_graph_convolution_amd.utils import write_mesh
    V, F = torus(250, 200)
    out = {"facets": int(F.shape[0]), "vertices": int(V.shape[0])}
    for label, kw in (("warm_up", {}), ("default", {}), ("surface", {"surface": True}), ("surface_only", {"surface_only": True})):
        with tempfile.TemporaryDirectory() as tmp:
            gt, res = os.path.join(tmp, "gt"), os.path.join(tmp, "res")
            os.makedirs(gt)
            os.makedirs(res)
            write_mesh(V.astype(np.float32), F, os.path.join(gt, "torus.obj"))
            write_mesh(add_noise(V, F, sigma_rel=0.1, seed=1).astype(np.float32), F, os.path.join(res, "torus_n1_denoised.obj"))
            t0 = time.time()
            computeMetrics(gt, res, log=lambda *a: None, **kw)
            out["wall_s_" + label] = time.time() - t0
            if kw:
                out["csv_" + label] = open(os.path.join(res, "results_surface.csv")).read().strip()
    return out


def main():
    L = count_lib()
    out = {"probe": "closest", "reps": REPS, "meshes": [probe_mesh(L, 250, 200, 5), probe_mesh(L, 2500, 200, 2)],
           "computeMetrics_100k_facets": time_cli()}
    s = json.dumps(out)
    print(s)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
