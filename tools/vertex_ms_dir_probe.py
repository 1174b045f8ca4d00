"""Developer tool: what the ray constraint costs the multi-scale vertex update, for DESIGN 8.  On the 100 000-facet torus
(50 000 vertices, 25 face slots), alternating in one process after a warm-up of both sides, device events around each call:

  1. (80, 20, 20) iterations of fgc_vertex_update_ms_dir beside fgc_vertex_update_ms (the forward alone, as inferNet runs it);
  2. the captured point-set step (network, update with its trajectory, fullLoss, both adjoints, Adam) of a clean mesh bound
     with the noise along the camera's rays, with and without ray_update.

Prints one JSON line (milliseconds per call: median, min, max).

  python tools/vertex_ms_dir_probe.py [--repeats 10] [--skip-step]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import facet_graph_convolution_amd  # noqa: E402,F401  (before the first torch.cuda call: the captured step needs it)


def _alternate(calls, repeats, warmup=3):
    for f in calls.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(repeats):
        for k, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k + "_ms": {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true", help="the forward pair only")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("vertex_ms_dir_probe needs the GPU: a time taken anywhere else says nothing")
    from facet_graph_convolution_amd import ops, utils
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    from facet_graph_convolution_amd.meshgen import torus
    from facet_graph_convolution_amd.net import FacetDenoiser
    V, F = torus(250, 200)
    ds = TrainingSet()
    ds.addCleanMeshWithVertices(V, F, seed=0)
    verts = np.asarray(ds.clean_vertices[0], dtype=np.float32).reshape(-1, 3)
    rays = utils.view_rays(verts, camera=(0.0, 0.0, 5.0 * float(np.abs(verts).max())))
    dev = torch.device("cuda", 0)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    # the clean normals in node order and their 4:1 means, renormalised, as the three fields
    n0 = put(np.asarray(ds.gt_list[0], dtype=np.float32).reshape(-1, 3))
    unit = lambda t: t / t.norm(dim=1, keepdim=True).clamp_min(1e-20)  # noqa: E731
    n1 = unit(n0.reshape(-1, 4, 3).mean(1))
    n2 = unit(n1.reshape(-1, 4, 3).mean(1))
    x = put(utils.normalizePointSets(verts, verts)[0].astype(np.float32))
    faces = put(np.asarray(ds.clean_faces_rows[0]).reshape(-1, 3).astype(np.int32))
    vf = put(np.asarray(ds.v_faces_list[0]).reshape(x.shape[0], -1).astype(np.int32))
    d = put(rays)
    its = (80, 20, 20)
    out = {"faces": int(F.shape[0]), "vertices": int(V.shape[0]), "nodes": int(faces.shape[0]), "iters": list(its),
           "repeats": args.repeats}
    out["forward"] = _alternate({"vertex_update_ms": lambda: ops.vertex_update_ms(x, [n0, n1, n2], faces, vf, its),
                                 "vertex_update_ms_dir": lambda: ops.vertex_update_ms_dir(x, [n0, n1, n2], faces, vf, d, its)},
                                args.repeats)
    if not args.skip_step:
        a = (ds.in_list[0], ds.adj_list[0], ds.clean_vertices[0], ds.clean_faces_rows[0], ds.v_faces_list[0],
             ds.clean_edge_len[0])
        rs = np.random.RandomState(0)
        nv = x.shape[0]
        i0, i1 = rs.randint(nv, size=500), rs.randint(nv, size=500)
        R = utils.rand_rotation_matrix(randnums=rs.uniform(size=3))
        nets = {}
        for name, ray_update in (("step_free", False), ("step_ray_update", True)):
            net = FacetDenoiser("cuda:0", multi_scale=True, seed=0)
            net.bind_clean_vertices(0, *a, direction=rays, ray_update=ray_update)
            nets[name] = net
        step = lambda net: net.pointset_step(i0, i1, R, capture=True, noise=(0, 0.2))  # noqa: E731
        out["captured_pointset_step"] = _alternate({k: (lambda n=n: step(n)) for k, n in nets.items()}, args.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
