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
"""
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


def main():
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
