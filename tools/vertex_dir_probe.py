"""Developer tool: device time of 60 iterations of fgc_vertex_update_dir beside 60 iterations of fgc_vertex_update on the
100 000-facet torus (50 000 vertices, 20 edge slots), for DESIGN 8.  Device events around each call, the two calls
alternating, after a warm-up of both; prints one JSON line (milliseconds per call: median, min, max) and the largest
difference of the ray-constrained result to the float64 restatement of tests/depth_cases.py after 3 iterations.

  python tools/vertex_dir_probe.py [--repeats 20] [--iters 60]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--iters", type=int, default=60)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("vertex_dir_probe needs the GPU: a time taken anywhere else says nothing")
    from facet_graph_convolution_amd import ops, utils
    from facet_graph_convolution_amd.meshgen import torus, add_noise
    import depth_cases as dc
    V, F = torus(250, 200)
    Vn = add_noise(V, F).astype(np.float32)
    n = utils.computeFacesNormals(V, F).astype(np.float32)
    em, vem = utils.getEdgeMap(F, maxEdges=20)
    rays = utils.view_rays(Vn, camera=(0.0, 0.0, 5.0 * float(np.abs(V).max())))
    dev = torch.device("cuda", 0)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    x, nd, e, ve, d = put(Vn), put(n), put(em), put(vem), put(rays)
    calls = {"vertex_update": lambda it: ops.vertex_update(x, nd, e, ve, it),
             "vertex_update_dir": lambda it: ops.vertex_update_dir(x, nd, e, ve, d, it)}
    got = calls["vertex_update_dir"](3).cpu().numpy()
    want, _ = dc.restate(Vn, n, em, vem, rays, 3)
    for f in calls.values():
        for _ in range(3):
            f(args.iters)
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.repeats):
        for k, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f(args.iters)
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    out = {"faces": int(F.shape[0]), "vertices": int(V.shape[0]), "iters": args.iters, "repeats": args.repeats,
           "err_vs_f64_3_iters": float(np.abs(got - want).max())}
    for k, v in times.items():
        out[k + "_ms"] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
