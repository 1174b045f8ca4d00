"""GPU probe of the bilateral normal filter: device-event times (median of 20 after warm-up) of ONE pass of
fgc_bilateral_filter at 20 480 faces (icosphere 5) and on the 100k-facet torus (meshgen.torus(250, 200)), noisy as in
the fixtures, sigma_s = one mean edge length: for P = 1 and P = 12 (4 sigma_s x 3 sigma_r) pairs, on the reference's
10 x 10 x 10 grid and on the `auto` grid of the bilateral tool; pairs of faces per second against the issue-rate floor;
then the wall time of bilateral.denoise_mesh on the 100k torus, split into host preprocessing, filter passes and vertex
update.  Prints one JSON line (also written to the file given as the only argument).

Pairs: sum over the occupied cells of population x window (what the filter has to visit); `issued` counts every cell's
population rounded up to whole 64-lane tasks (what the kernel's lanes actually run).  Floor: the inner loop of
csrc/fgc_bilateral.hip is 20 wave64 vector instructions per pair for P = 1 (--save-temps ISA: 17 plain fp32, 2 v_exp_f32,
1 v_pk_fma_f32) and 59.6 for the 4 x 3 launch (24.4 plain, 7 v_exp_f32, 28.2 packed); at the issue costs measured per
SIMD with two or more waves (profiles/r5_issue_rates.txt: 1.1 ns plain, 3.47 ns v_exp_f32, 1.91 ns packed) 64 pairs
cost a SIMD 27.6 ns (105.1 ns for the 12 pairs), and the card has 256 CUs x 4 SIMDs.
    python tools/bilateral_probe.py [OUT.json]

--guided: instead, for the same two meshes and both grids, the device-event times (median of 20) of the guidance launches
(fgc_guided_normals: gd_patch_kernel + gd_pick_kernel), of one guided filter pass (fgc_bilateral_filter_guided) and of the
plain pass of the same run, P = 1.
    python tools/bilateral_probe.py --guided [OUT.json]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from facet_graph_convolution_amd import bilateral, ops, utils  # noqa: E402
from facet_graph_convolution_amd.meshgen import icosphere, torus, add_noise  # noqa: E402

NS_PER_64_PAIRS = {1: 17 * 1.1 + 2 * 3.47 + 1.91, 12: 24.4 * 1.1 + 7 * 3.47 + 28.2 * 1.91}
SIMDS = 256 * 4


def pair_counts(cell, grid):
    sx, sy, sz = grid
    count = np.zeros((sx + 2, sy + 2, sz + 2), dtype=np.int64)
    np.add.at(count, tuple((cell[(cell >= 0).all(1)] + 1).T), 1)
    window = sum(count[i:i + sx, j:j + sy, k:k + sz] for i in range(3) for j in range(3) for k in range(3))
    pop = count[1:-1, 1:-1, 1:-1]
    return int((pop * window).sum()), int(((pop + 63) // 64 * 64 * window).sum()), int((pop > 0).sum())


def time_pass(V, F, slices, ss_list, sr_list, reps=20):
    Fc = utils.getTrianglesBarycenter(V, F, normalize=False).astype(np.float32)
    Fa = utils.getTrianglesArea(V, F).astype(np.float32)
    Fn = utils.computeFacesNormals(V, F)
    el = float(utils.getAverageEdgeLength(V, F)[0])
    auto = slices == "auto"
    grid = bilateral.auto_slices(Fc, el) if auto else utils.bilateral_grid(slices)
    cell = utils.bilateral_cells(Fc, grid, flat_axis_one_cell=auto)
    order, ptr = utils.bilateral_order(cell, grid)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    c, n, a, order, ptr = put(Fc), put(Fn), put(Fa), put(order), put(ptr)
    ss, sr = [el * s for s in ss_list], sr_list
    for _ in range(3):
        ops.bilateral_filter(c, n, a, ss, sr, order, ptr, grid)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(reps):
        ev[0].record()
        ops.bilateral_filter(c, n, a, ss, sr, order, ptr, grid)
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    ms = float(np.median(times))
    pairs, issued, cells = pair_counts(cell, grid)
    P = len(ss) * len(sr)
    floor_ms = 1e-6 * issued / 64.0 * NS_PER_64_PAIRS[P] / SIMDS
    return {"faces": int(F.shape[0]), "grid": list(grid), "occupied_cells": cells, "P": P, "ms_median": ms,
            "ms_min": float(min(times)), "pairs": pairs, "issued_pairs": issued, "pairs_per_s": pairs / (ms * 1e-3),
            "floor_ms_issued": floor_ms, "share_of_floor": floor_ms / ms}


def time_guided(V, F, slices, reps=20):
    Fc = utils.getTrianglesBarycenter(V, F, normalize=False).astype(np.float32)
    Fa = utils.getTrianglesArea(V, F).astype(np.float32)
    Fn = utils.computeFacesNormals(V, F)
    el = float(utils.getAverageEdgeLength(V, F)[0])
    auto = slices == "auto"
    grid = bilateral.auto_slices(Fc, el) if auto else utils.bilateral_grid(slices)
    order, ptr = utils.bilateral_order(utils.bilateral_cells(Fc, grid, flat_axis_one_cell=auto), grid)
    ring, ld = utils.face_rings(F)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    c, n, a, order, ptr, ring, fe = (put(x) for x in (Fc, Fn, Fa, order, ptr, ring, utils.face_edge_neighbours(F)))
    g = ops.guidance_normals(n, a, ring, fe)
    steps = {"guidance": lambda: ops.guidance_normals(n, a, ring, fe),
             "guided_filter": lambda: ops.bilateral_filter(c, n, a, el, 0.35, order, ptr, grid, guide=g),
             "plain_filter": lambda: ops.bilateral_filter(c, n, a, el, 0.35, order, ptr, grid)}
    out = {"faces": int(F.shape[0]), "grid": list(grid), "ring_ld": int(ld)}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {k: [] for k in steps}
    for rep in range(reps + 3):                     # the three steps in turn, so that they share the clock they run at
        for k, fn in steps.items():
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if rep >= 3:
                times[k].append(ev[0].elapsed_time(ev[1]))
    for k, t in times.items():
        out[k + "_ms_median"], out[k + "_ms_min"] = float(np.median(t)), float(min(t))
    return out


def time_denoise(V, F):
    bilateral.denoise_mesh(V, F, iterations=1, vertex_iterations=1)          # warm-up
    tm = {}
    bilateral.denoise_mesh(V, F, timings=tm)
    return {"faces": int(F.shape[0]), "iterations": 10, "vertex_iterations": 60, "grid": list(tm["grid"]),
            "host_s": tm["host"], "filter_s": tm["filter"], "vertex_s": tm["vertex"]}


def main():
    meshes = {"ico5": icosphere(5), "torus100k": torus(250, 200)}
    out = {}
    args = [a for a in sys.argv[1:] if a != "--guided"]
    for name, (V, F) in meshes.items():
        F = F.astype(np.int32)
        Vn = add_noise(V, F, sigma_rel=0.2, seed=3).astype(np.float32)
        for slices in (10, "auto"):
            if "--guided" in sys.argv[1:]:
                out["%s_slices_%s_guided" % (name, slices)] = time_guided(Vn, F, slices)
                continue
            out["%s_slices_%s_P1" % (name, slices)] = time_pass(Vn, F, slices, [1.0], [0.35])
            out["%s_slices_%s_P12" % (name, slices)] = time_pass(Vn, F, slices, [0.5, 1.0, 1.5, 2.0], [0.2, 0.35, 0.5])
        if name == "torus100k" and "--guided" not in sys.argv[1:]:
            out["denoise_mesh_torus100k"] = time_denoise(Vn, F)
    s = json.dumps(out)
    print(s)
    if args:
        with open(args[0], "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
