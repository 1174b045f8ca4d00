"""GPU probe of the evaluation metrics: device-event times of fgc_nn_query (unmasked) at 100k x 100k and 1M x 1M points,
pairs per second and the share of the issue-rate floor; wall time of computeMetrics on a folder with one 100k-facet
torus (meshgen.torus + add_noise).  Prints one JSON line (also written to the file given as the only argument).

Floor: the scan's inner loop is 7.25 wave64 VALU instructions per (query, candidate) pair (--save-temps ISA of
csrc/fgc_metrics.hip: per 16 candidates x 4 queries per lane, 80 v_pk_add_f32 + 48 v_pk_mul_f32 + 32 v_cmp + 64 v_cndmask +
8 v_mov per 32 pairs); the card issues 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 7.86e13 lane-instructions per second.
    python tools/metrics_probe.py [OUT.json]
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from facet_graph_convolution_amd import ops  # noqa: E402

VALU_PER_PAIR = 7.25
LANE_INSTR_PER_S = 256 * 4 * 32 * 2.4e9


def time_nn(n, reps):
    rs = np.random.RandomState(n % 1000)
    q = torch.from_numpy(rs.uniform(-1, 1, size=(n, 3)).astype(np.float32)).cuda()
    p = torch.from_numpy(rs.uniform(-1, 1, size=(n, 3)).astype(np.float32)).cuda()
    ops.nn_query(q, p)                      # warm-up (code object load, workspace)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(reps):
        ev[0].record()
        ops.nn_query(q, p)
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    ms = float(np.median(times))
    pairs = float(n) * n
    floor_ms = 1e3 * pairs * VALU_PER_PAIR / LANE_INSTR_PER_S
    return {"n": n, "ms_median": ms, "ms_min": float(min(times)), "pairs_per_s": pairs / (ms * 1e-3),
            "floor_ms": floor_ms, "share_of_floor": floor_ms / ms}


def time_cli():
    from facet_graph_convolution_amd.meshgen import torus, add_noise
    from facet_graph_convolution_amd.utils import write_mesh
    from facet_graph_convolution_amd.computeMetrics import computeMetrics
    V, F = torus(250, 200)                  # 2 * 250 * 200 = 100 000 facets
    with tempfile.TemporaryDirectory() as tmp:
        gt, res = os.path.join(tmp, "gt"), os.path.join(tmp, "res")
        os.makedirs(gt)
        os.makedirs(res)
        write_mesh(V.astype(np.float32), F, os.path.join(gt, "torus.obj"))
        write_mesh(add_noise(V, F, sigma_rel=0.1, seed=1).astype(np.float32), F, os.path.join(res, "torus_n1_denoised.obj"))
        t0 = time.time()
        computeMetrics(gt, res, log=lambda *a: None)
        wall = time.time() - t0
        line = open(os.path.join(res, "results_heat.csv")).read().strip()
    return {"facets": int(F.shape[0]), "vertices": int(V.shape[0]), "wall_s": wall, "csv": line}


def main():
    out = {"nn_100k": time_nn(100_000, 20), "nn_1M": time_nn(1_000_000, 3), "computeMetrics_100k_facets": time_cli()}
    s = json.dumps(out)
    print(s)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
