"""GPU probe of the ray casting behind the virtual depth scans (include/fgc.h: fgc_ray_cast) on the 100k-facet torus
(meshgen.torus(250, 200): 50 000 vertices, 100 000 faces), camera (2.5, 0.4, 1.2) as in the tests:

  visible   one ray per vertex, what utils.visible_vertices casts: 50 000 x 100 000 pairs
  image     a 640 x 480 depth image, what utils.depth_image casts: 307 200 x 100 000 pairs

For each the device-event time of ONE ops.ray_cast call on tensors that are already on the device (median of 20 after
warm-up; the three launches together), pairs per second, and the wall time of the host function around it (upload, the
call, download, the host arithmetic).  Prints one JSON line (also written to the file given as the only argument).

Floor: every pair runs the first part of the loop of csrc/fgc_raycast.hip - p = d x e2, det, s, s . p, the division for u
and its test - FLOOR_COUNTS wave64 vector instructions (read off the gfx950 ISA of the build); the rest (v, t: two more
divisions) sits behind a branch that a wave takes only if one of its 64 rays has 0 <= u <= 1, and is NOT in the floor.
At the issue costs measured per SIMD with two or more waves (profiles/r5_issue_rates.txt: 1.1 ns plain fp32, 1.91 ns
packed, 3.47 ns v_rcp_f32, 1.8 ns v_cmp) 64 pairs cost a SIMD NS_PER_64_PAIRS, and the card has 256 CUs x 4 SIMDs.
`issued` counts the rays rounded up to whole 64-lane workgroups and the faces rounded up to whole rounds of the four waves.
    python tools/ray_cast_probe.py [OUT.json]

--tree: the cast through a bounding-box tree (fgc_ray_tree_build, fgc_ray_cast_tree) against the brute-force cast, both in
this one process and in turns, on the 100k-facet torus and on torus(2500, 200) (500 000 vertices, 1 000 000 faces).  Per
mesh: the device-event time of the build (ops.ray_tree: the Morton order made with torch plus fgc_ray_tree_build, and
fgc_ray_tree_build alone on a given order); per set of rays (the vertex rays and the 640 x 480 image) the time of one
ops.ray_cast call, of one ops.ray_cast_tree call with sort_rays on (the sort and the scatter included) and off, of the
tree's kernel alone on rays that are already sorted, how many rays differ between the two casts, and the pairs and boxes a
ray's lane actually tested (mean and maximum), counted on the device by the probe-only build csrc/libfgc_rtcount.so
(`make -C facet_graph_convolution_amd/csrc libfgc_rtcount.so`; made here if it is missing).  Medians of REPS_TREE (fewer
for the brute-force cast of the large mesh, which takes a second a call).
    python tools/ray_cast_probe.py --tree [OUT.json]          (kept as profiles/ray_tree_probe.json)
"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from facet_graph_convolution_amd import ops, utils  # noqa: E402
from facet_graph_convolution_amd.meshgen import torus  # noqa: E402

# per pair, the part every pair runs: 6 (p) + 3 (s) + 6 (det, s . p), 10 of the division that are plain (two v_div_scale_f32,
# three v_fma_f32, two v_fmac_f32, v_mul_f32, v_div_fmas_f32, v_div_fixup_f32) and its v_rcp_f32, the two compares of u and
# one v_mov_b32 of the select that follows
FLOOR_COUNTS = {"plain": 26, "packed": 0, "rcp": 1, "cmp": 2}
NS = {"plain": 1.1, "packed": 1.91, "rcp": 3.47, "cmp": 1.8}
NS_PER_64_PAIRS = sum(FLOOR_COUNTS[k] * NS[k] for k in NS)
SIMDS = 256 * 4
CAMERA = (2.5, 0.4, 1.2)


def time_cast(Vd, Fd, origins, dirs, reps=20):
    for _ in range(3):
        ops.ray_cast(Vd, Fd, origins, dirs)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(reps):
        ev[0].record()
        t, f = ops.ray_cast(Vd, Fd, origins, dirs)
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    nq, nf = dirs.shape[0], Fd.shape[0]
    ms = float(np.median(times))
    pairs = nq * nf
    issued = (nq + 63) // 64 * 64 * ((nf + 15) // 16 * 16)
    floor_ms = 1e-6 * issued / 64.0 * NS_PER_64_PAIRS / SIMDS
    return {"rays": nq, "faces": nf, "hits": int((f >= 0).sum().item()), "ms_median": ms, "ms_min": float(min(times)),
            "pairs": pairs, "pairs_per_s": pairs / (ms * 1e-3), "floor_ms_issued": floor_ms, "share_of_floor": floor_ms / ms}


def wall(fn, reps=3):
    fn()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


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
    """The probe-only build of csrc/fgc_raytree.hip (per-ray counters), loaded beside libfgc.so."""
    from facet_graph_convolution_amd import _lib
    csrc = os.path.dirname(_lib.LIB_PATH)
    path = os.path.join(csrc, "libfgc_rtcount.so")
    if not os.path.exists(path):
        import subprocess
        subprocess.check_call(["make", "-C", csrc, "libfgc_rtcount.so"])
    _lib.lib()
    L = ctypes.CDLL(path)
    L.fgc_ray_cast_tree_count.restype = ctypes.c_int
    L.fgc_ray_cast_tree_count.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                          ctypes.c_void_p, ctypes.c_int32, ctypes.c_float] + [ctypes.c_void_p] * 5
    return L


def tested_per_ray(L, tree, origins, dirs):
    """(pairs, boxes) [nq] each: what the lane of every ray tested, rays in the order given."""
    from facet_graph_convolution_amd._lib import ptr, stream_ptr
    nq = dirs.shape[0]
    t = torch.empty(nq, dtype=torch.float32, device="cuda")
    f = torch.empty(nq, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(nq, 2, dtype=torch.int32, device="cuda")
    rc = L.fgc_ray_cast_tree_count(ptr(tree.tree), tree.tree.numel(), tree.nf, ptr(origins), origins.shape[0], ptr(dirs), nq,
                                   0.0, ptr(t), ptr(f), None, ptr(cnt), stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return cnt[:, 0].double(), cnt[:, 1].double(), f


REPS_TREE = 10


def probe_tree_mesh(L, n_major, n_minor):
    V, F = torus(n_major, n_minor)
    V, F = np.ascontiguousarray(V, dtype=np.float32), np.asarray(F).astype(np.int32)
    Vd, Fd = torch.from_numpy(V).cuda(), torch.from_numpy(F).cuda()
    nf = F.shape[0]
    cam = torch.tensor([CAMERA], dtype=torch.float32, device="cuda")
    out = {"mesh": "torus(%d, %d)" % (n_major, n_minor), "faces": nf, "vertices": V.shape[0]}
    order = ops.ray_tree_order(Vd, Fd)
    out["build_ms_order_and_tree"] = event_ms(lambda: ops.ray_tree(Vd, Fd), REPS_TREE)
    out["build_ms_tree_alone"] = event_ms(lambda: ops.ray_tree(Vd, Fd, order), REPS_TREE)
    tree = ops.ray_tree(Vd, Fd)
    out["tree_bytes"] = tree.tree.numel()
    look = 0.5 * (V.astype(np.float64).min(0) + V.astype(np.float64).max(0))
    sets = {"visible": Vd - cam,
            "image": torch.from_numpy(utils.pixel_rays(CAMERA, look, (640, 480), 40.0).reshape(-1, 3)).cuda()}
    for name, dirs in sets.items():
        nq = dirs.shape[0]
        reps_brute = REPS_TREE if nq * nf < 1e11 else 3
        r = {"rays": nq}
        # in turns: brute force, tree sorted, tree unsorted, and again
        ms = {"brute": [], "tree_sorted": [], "tree_unsorted": []}
        for rep in range(2):
            ms["brute"].append(event_ms(lambda: ops.ray_cast(Vd, Fd, cam, dirs), reps_brute, warm=1))
            ms["tree_sorted"].append(event_ms(lambda: ops.ray_cast_tree(tree, cam, dirs, sort_rays=True), REPS_TREE))
            ms["tree_unsorted"].append(event_ms(lambda: ops.ray_cast_tree(tree, cam, dirs, sort_rays=False), REPS_TREE))
        r["ms_brute"], r["ms_tree_sort_on"], r["ms_tree_sort_off"] = (float(np.median(ms[k])) for k in ms)
        perm = torch.sort(ops._morton30(dirs / dirs.norm(dim=1, keepdim=True)), stable=True).indices
        sorted_dirs = dirs[perm].contiguous()
        r["ms_tree_kernel_on_sorted_rays"] = event_ms(lambda: ops.ray_cast_tree(tree, cam, sorted_dirs, sort_rays=False), REPS_TREE)
        tb, fb = ops.ray_cast(Vd, Fd, cam, dirs)
        tt, ft = ops.ray_cast_tree(tree, cam, dirs)
        r["hits"] = int((fb >= 0).sum().item())
        r["rays_that_differ"] = int(((fb != ft) | (tb.view(torch.int32) != tt.view(torch.int32))).sum().item())
        for label, dd in (("sort_on", sorted_dirs), ("sort_off", dirs)):
            pairs, boxes, fc = tested_per_ray(L, tree, cam, dd)
            r["pairs_per_ray_" + label] = {"mean": pairs.mean().item(), "max": pairs.max().item()}
            r["boxes_per_ray_" + label] = {"mean": boxes.mean().item(), "max": boxes.max().item()}
        assert torch.equal(fc, ft)          # (the counting build finds what the library finds)
        r["pairs_per_ray_brute"] = nf
        r["speedup_cast_sort_on"] = r["ms_brute"] / r["ms_tree_sort_on"]
        r["speedup_with_build"] = r["ms_brute"] / (r["ms_tree_sort_on"] + out["build_ms_order_and_tree"])
        out[name] = r
    out["wall_s_visible_vertices_none"] = wall(lambda: utils.visible_vertices(V, F, camera=CAMERA), reps=1)
    out["wall_s_visible_vertices_tree"] = wall(lambda: utils.visible_vertices(V, F, camera=CAMERA, accel="tree"), reps=1)
    return out


def main_tree(path):
    L = count_lib()
    out = {"probe": "ray_tree", "reps": REPS_TREE, "meshes": [probe_tree_mesh(L, 250, 200), probe_tree_mesh(L, 2500, 200)]}
    s = json.dumps(out)
    print(s)
    if path:
        with open(path, "w") as fh:
            fh.write(s + "\n")


def main():
    if "--tree" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--tree"]
        return main_tree(rest[0] if rest else None)
    V, F = torus(250, 200)
    V, F = np.ascontiguousarray(V, dtype=np.float32), np.asarray(F).astype(np.int32)
    Vd, Fd = torch.from_numpy(V).cuda(), torch.from_numpy(F).cuda()
    cam = torch.tensor([CAMERA], dtype=torch.float32, device="cuda")
    out = {"ns_per_64_pairs_floor": NS_PER_64_PAIRS}
    out["visible"] = time_cast(Vd, Fd, cam, Vd - cam)
    out["visible"]["wall_s_visible_vertices"] = wall(lambda: utils.visible_vertices(V, F, camera=CAMERA))
    look = 0.5 * (V.astype(np.float64).min(0) + V.astype(np.float64).max(0))
    rays = torch.from_numpy(utils.pixel_rays(CAMERA, look, (640, 480), 40.0).reshape(-1, 3)).cuda()
    out["image"] = time_cast(Vd, Fd, cam, rays)
    out["image"]["wall_s_depth_image"] = wall(lambda: utils.depth_image(V, F, CAMERA, size=(640, 480)))
    s = json.dumps(out)
    print(s)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
