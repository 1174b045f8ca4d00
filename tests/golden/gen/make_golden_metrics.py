#!/usr/bin/env python3
"""Generate tests/golden/metrics_*.npz by EXECUTING THE REFERENCE'S evaluation code (utils.py:227-240, 816-1006,
1168-1239, 1973-2031, 2322-2342 and computeMetrics.py), imported through tf_shim as make_golden.py does:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_metrics.py
    PYTHONDONTWRITEBYTECODE=1 TF_SHIM_DTYPE=float64 python tests/golden/gen/make_golden_metrics.py

The float64 run feeds the same point sets and normals as float64 arrays (the reference then computes in double): an
error budget for the float32 results, not a parity target.  The end-to-end computeMetrics case is float32 only.
Only data is written.
"""
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
OUT = os.path.abspath(os.path.join(HERE, ".."))
REF = "/root/reference/Code"

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "tf_shim"))
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
if not hasattr(time, "clock"):
    time.clock = time.perf_counter

import warnings  # noqa: E402

warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402
import scipy.io  # noqa: E402

import tensorflow  # noqa: E402,F401  (the shim)
import utils as ref_utils  # noqa: E402
import computeMetrics as ref_cm  # noqa: E402

from facet_graph_convolution_amd.meshgen import icosphere, torus, add_noise  # noqa: E402
from facet_graph_convolution_amd.utils import write_mesh  # noqa: E402

F64 = os.environ.get("TF_SHIM_DTYPE", "float32") == "float64"
DT = np.float64 if F64 else np.float32
SUFFIX = "_f64" if F64 else ""


def save(name, **arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrays)
    print("wrote %-32s %8.1f KB" % (name, os.path.getsize(path) / 1024.0))


def open_torus_patch(nfaces=450):
    """The first faces of the torus grid, vertices re-indexed (as make_golden.py's open vertex case): border faces."""
    Vt, Ft = torus(20, 16)
    used, Fo = np.unique(Ft[:nfaces], return_inverse=True)
    return Vt[used].astype(np.float32), Fo.reshape(-1, 3).astype(np.int32)


def quiet(fn, *a, **kw):
    """The reference prints its progress; keep the generator's output readable."""
    import io
    import contextlib
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def hausdorff_cases():
    out = {}
    rs = np.random.RandomState(0)
    A = rs.uniform(size=(2000, 3)).astype(np.float32)
    B = rs.uniform(size=(2100, 3)).astype(np.float32)
    V, F = icosphere(4)
    Vn = add_noise(V, F, seed=3).astype(np.float32)
    cases = {"clouds": (A, B, A, B), "ico4": (Vn, V.astype(np.float32), Vn, V.astype(np.float32))}
    # the raise case: V0 near the origin, every candidate point near the far corner (the one at the origin lies on a
    # slice bound and so in no cell): the query cell (0,0,0) holds points and its 2x2x2 candidate cells are empty
    C0 = np.concatenate([rs.uniform(0.0, 0.1, size=(50, 3)), [[1.0, 1.0, 1.0]]]).astype(np.float32)
    C1 = np.concatenate([rs.uniform(0.9, 1.0, size=(50, 3)), [[0.0, 0.0, 0.0]]]).astype(np.float32)
    cases["raise"] = (C0, C1, C0, C1)
    for name, arrs in cases.items():
        arrs = [a.astype(DT) for a in arrs]
        for k, a in zip(("V0", "V1", "sV0", "sV1"), arrs):
            out["%s_%s" % (name, k)] = a
        for acc in (True, False):
            tag = "%s_acc%d" % (name, int(acc))
            try:
                res = quiet(ref_utils.hausdorffOverSampled, *[a.copy() for a in arrs], accuracyOnly=acc)
                out[tag] = np.array([float(r) for r in res])
                out[tag + "_raised"] = np.array("")
            except Exception as e:  # noqa: BLE001  (what the reference raises is the datum)
                out[tag] = np.zeros(4)
                out[tag + "_raised"] = np.array(type(e).__name__)
            print("hausdorff %-10s -> %s %s" % (tag, out[tag], out[tag + "_raised"]))
    assert str(out["raise_acc1"+"_raised"]) == "ValueError", "the raise case must raise"
    # the reference's mean over its partition is above the exact mean: some nearest points lie outside the 2x2x2 cells
    d = np.sqrt(((A.astype(np.float64)[:, None] - B.astype(np.float64)[None]) ** 2).sum(-1)).min(1)
    lo = np.minimum(A.min(0), B.min(0)).astype(np.float64)
    hi = np.maximum(A.max(0), B.max(0)).astype(np.float64)
    exact_mean = d.mean() / np.sqrt(((hi - lo) ** 2).sum())
    assert out["clouds_acc1"][2] > exact_mean * 1.001, (out["clouds_acc1"][2], exact_mean)
    save("metrics_hausdorff%s.npz" % SUFFIX, **out)


def angular_cases():
    out = {}
    V, F = icosphere(3)
    meshes = {"closed": (V.astype(np.float32), F.astype(np.int32))}
    meshes["open"] = open_torus_patch()
    Vz, Fz = icosphere(2)
    Vz = Vz.astype(np.float32).copy()
    Vz[Fz[0, 2]] = Vz[Fz[0, 0]]           # face 0 collapses to a segment: a zero normal, a fake node
    meshes["fake"] = (Vz, Fz.astype(np.int32))
    for name, (Vg, Fg) in meshes.items():
        Vd = add_noise(Vg, Fg, seed=7).astype(np.float32)
        n0 = ref_utils.computeFacesNormals(Vd, Fg).astype(DT)
        n1 = ref_utils.computeFacesNormals(Vg, Fg).astype(DT)
        vec = ref_utils.angularDiffVec(n0, n1)
        mean, std = quiet(ref_utils.angularDiff, n0, n1)
        fake = np.all(np.less_equal(np.absolute(n1), 10e-4), axis=-1)
        border = ref_utils.getBorderFaces(Fg)
        angColor = np.maximum(1 - vec / ref_cm.HEATMAP_MAX_ANGLE, np.zeros_like(vec))
        colors = ref_utils.getHeatMapColor(1 - angColor)
        newV, newF = quiet(ref_utils.getColoredMesh, Vd, Fg, colors)
        out.update({name + "_verts": Vd, name + "_faces": Fg, name + "_n0": n0, name + "_n1": n1, name + "_vec": vec,
                    name + "_mean": np.float64(mean), name + "_std": np.float64(std), name + "_fake": fake,
                    name + "_border": border, name + "_colors": colors, name + "_newV": newV, name + "_newF": newF})
        print("angular %-6s faces %d border %d fake %d mean %.5f" % (name, Fg.shape[0], border.sum(), fake.sum(), mean))
    assert out["open_border"].sum() > 0 and out["closed_border"].sum() == 0 and out["fake_fake"].sum() >= 1
    save("metrics_angular%s.npz" % SUFFIX, **out)


def cli_case():
    """The reference computeMetrics() end to end, its module globals pointed at temporary folders."""
    out = {}
    gts = {"sphere": tuple(a for a in icosphere(3)), "patch": open_torus_patch(450)}
    with tempfile.TemporaryDirectory() as tmp:
        gt_dir, res_dir = os.path.join(tmp, "gt") + "/", os.path.join(tmp, "res") + "/"
        os.makedirs(gt_dir)
        os.makedirs(res_dir)
        for name, (Vg, Fg) in gts.items():
            Vg = Vg.astype(np.float32)
            assert ref_utils.getDensePC(Vg, Fg, res=1).shape == Vg.shape   # res = 1: the dense cloud is the GT itself
            write_mesh(Vg, Fg, gt_dir + name + ".obj")
            for k in (1, 2, 3):
                write_mesh(add_noise(Vg, Fg, sigma_rel=0.03 * k, seed=10 + k), Fg,
                           res_dir + "%s_n%d_denoised.obj" % (name, k))
        files = sorted(os.listdir(gt_dir)) + sorted(os.listdir(res_dir))
        for f in files:
            d = gt_dir if f in os.listdir(gt_dir) else res_dir
            out["file_" + f] = np.array(open(d + f).read())
        ref_cm.TEST_GT_DATA_PATH = gt_dir
        ref_cm.RESULTS_PATH = res_dir
        quiet(ref_cm.computeMetrics)
        lines = open(res_dir + "results_heat.csv").read().splitlines(True)
        out["csv_lines"] = np.array(lines)
        for name in gts:
            for k in (1, 2, 3):
                hm = "%s_n%d_heatmap.obj" % (name, k)
                rows = [ln.split() for ln in open(res_dir + hm)]
                out["heat_%s_n%d_V" % (name, k)] = np.array([[float(t) for t in r[1:]] for r in rows if r[0] == "v"])
                out["heat_%s_n%d_F" % (name, k)] = np.array([[int(t) for t in r[1:]] for r in rows if r[0] == "f"])
        mat = scipy.io.loadmat(res_dir + "angDiffFinal.mat")
        for key, val in mat.items():
            if not key.startswith("__"):
                out["mat_" + key] = val
    print("".join(lines))
    save("metrics_cli.npz", **out)


if __name__ == "__main__":
    hausdorff_cases()
    angular_cases()
    if not F64:
        cli_case()
