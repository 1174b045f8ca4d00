#!/usr/bin/env python3
"""Generate tests/golden/bilateral*.npz by EXECUTING THE REFERENCE'S bilateralFilter / FND / getTrianglesArea /
getAverageEdgeLength (utils.py:1242-1260, 2344-2526), imported through tf_shim as make_golden_metrics.py does:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_bilateral.py
    PYTHONDONTWRITEBYTECODE=1 TF_SHIM_DTYPE=float64 python tests/golden/gen/make_golden_bilateral.py

The inputs of every case (face centres, normals, areas) are float32 arrays made by THIS package's host functions from
meshgen meshes with fixed seeds; the float64 run feeds the same values as float64 arrays, so its results are the error
budget's yardstick: the float32 file stores, per case, dev32 = the largest absolute difference between the reference's
float32 and float64 results.  The reference prints the population of every occupied cell and the size of its 3 x 3 x 3
window; both lists are stored.  Inputs are stored where small; for the large cases a float64 checksum is (the tests
regenerate them).  Only data is written.  Needs the built library (host routines only, no GPU).
"""
import contextlib
import io
import os
import re
import sys
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

import tensorflow  # noqa: E402,F401  (the shim)
import utils as ref_utils  # noqa: E402

from facet_graph_convolution_amd import utils as pkg  # noqa: E402
from facet_graph_convolution_amd.meshgen import icosphere, torus, add_noise  # noqa: E402

F64 = os.environ.get("TF_SHIM_DTYPE", "float32") == "float64"
SUFFIX = "_f64" if F64 else ""
STORE_INPUTS_UP_TO = 2400      # faces


def save(name, **arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print("wrote %-24s %8.1f KB" % (name, size / 1024.0))
    assert size < 1 << 20, "fixture files stay under 1 MiB"


def open_torus_patch(nfaces=450):
    """The open patch of make_golden_metrics.py: the first faces of the torus grid, vertices re-indexed."""
    Vt, Ft = torus(20, 16)
    used, Fo = np.unique(Ft[:nfaces], return_inverse=True)
    return Vt[used].astype(np.float32), Fo.reshape(-1, 3).astype(np.int32)


def flat_grid(m=12):
    """m x m vertices in the plane z = 0, every quad split in two: 2 (m - 1)^2 faces."""
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    V = np.stack([i, j, np.zeros_like(i)], -1).reshape(-1, 3).astype(np.float32) / np.float32(m - 1)
    v = lambda a, b: (a * m + b)[:-1, :-1].reshape(-1)  # noqa: E731
    v00, v10, v11, v01 = v(i, j), v(i + 1, j), v(i + 1, j + 1), v(i, j + 1)
    F = np.concatenate([np.stack([v00, v10, v11], -1), np.stack([v00, v11, v01], -1)]).astype(np.int32)
    return V, F


def inputs(V, F):
    """(Fc, Fn, Fa) float32 of the mesh, by the package's host functions (what the tests regenerate)."""
    V, F = np.asarray(V, dtype=np.float32), np.asarray(F).astype(np.int32)
    return (pkg.getTrianglesBarycenter(V, F, normalize=False).astype(np.float32),
            pkg.computeFacesNormals(V, F).astype(np.float32), pkg.getTrianglesArea(V, F).astype(np.float32))


def checksum(Fc, Fn, Fa):
    return np.array([a.astype(np.float64).sum() for a in (Fc, Fn, Fa)] +
                    [np.abs(a.astype(np.float64)).sum() for a in (Fc, Fn, Fa)])


def run_ref(fn, *args):
    """The reference call with its printout captured: (result, cell populations, window sizes), the two lists in the
    reference's lexicographic cell order (of the LAST bilateralFilter call it made)."""
    buf = io.StringIO()
    t0 = time.time()
    with contextlib.redirect_stdout(buf):
        res = fn(*args)
    text = buf.getvalue()
    text = text[text.rindex("partitioning space..."):]
    pop = [int(m) for m in re.findall(r"^sliceFc shape = \((\d+),", text, flags=re.M)]
    win = [int(m) for m in re.findall(r"^bigSliceFc shape = \((\d+),", text, flags=re.M)]
    assert len(pop) == len(win)
    return res, np.array(pop, dtype=np.int64), np.array(win, dtype=np.int64), time.time() - t0


def noisy(V, F):
    return add_noise(V, F, sigma_rel=0.2, seed=3).astype(np.float32)


def cases():
    Vi, Fi = icosphere(3)
    Vt, Ft = torus(40, 30)
    Vo, Fo = open_torus_patch()
    Vf, Ff = flat_grid()
    V5, F5 = icosphere(5)
    ico3 = (noisy(Vi, Fi), Fi.astype(np.int32))
    return [
        ("ico3_a", ico3, [1.0], [0.35]),
        ("ico3_wide", ico3, [50.0], [0.35]),
        ("ico3_norange", ico3, [2.0], [-1]),
        ("torus2400", (noisy(Vt, Ft), Ft.astype(np.int32)), [1.5], [0.3]),
        ("open", (noisy(Vo, Fo), Fo), [1.0], [0.35]),
        ("flat", (Vf, Ff), [1.0], [0.35]),
        ("fnd", ico3, [0.5, 1.0, 2.0], [0.2, 0.5]),
        ("ico5", (noisy(V5, F5), F5.astype(np.int32)), [1.0], [0.35]),
    ]


def reference(Fc, Fn, Fa, ss, sr, dt):
    a = [x.astype(dt) for x in (Fc, Fn, Fa)]
    if len(ss) == 1 and len(sr) == 1:
        return run_ref(ref_utils.bilateralFilter, a[0], a[1], a[2], ss[0], sr[0])
    return run_ref(ref_utils.FND, a[0], a[1], a[2], ss, sr)


def main():
    out = {}
    names = []
    for name, (V, F), ss_rel, sr in cases():
        Fc, Fn, Fa = inputs(V, F)
        el, _ = pkg.getAverageEdgeLength(V, F)
        ss = [float(s) * float(el) for s in ss_rel]
        sr = [float(r) for r in sr]
        names.append(name)
        out[name + "_sigma_s"], out[name + "_sigma_r"] = np.array(ss), np.array(sr)
        out[name + "_checksum"] = checksum(Fc, Fn, Fa)
        if F.shape[0] <= STORE_INPUTS_UP_TO and not F64:
            out[name + "_Fc"], out[name + "_Fn"], out[name + "_Fa"] = Fc, Fn, Fa
        r64, pop, win, t64 = reference(Fc, Fn, Fa, ss, sr, np.float64)
        assert r64.dtype == np.float64 and np.isfinite(r64).all()
        if F64:
            out[name + "_out"] = r64
            print("%-13s float64 %.1f s" % (name, t64))
            continue
        r32, pop32, win32, t32 = reference(Fc, Fn, Fa, ss, sr, np.float32)
        assert r32.dtype == np.float32 and np.array_equal(pop, pop32) and np.array_equal(win, win32)
        dev32 = float(np.abs(r32.astype(np.float64) - r64).max())
        out[name + "_out"], out[name + "_dev32"] = r32, np.float64(dev32)
        out[name + "_pop"], out[name + "_win"] = pop, win
        print("%-13s faces %6d cells %4d mean window %7.1f dev32 %.2e  (float32 %.1f s, float64 %.1f s)" %
              (name, F.shape[0], len(pop), win.mean() if len(win) else 0.0, dev32, t32, t64))
    assert not np.any(out["flat_out"]) and ("flat_pop" not in out or len(out["flat_pop"]) == 0)
    out["cases"] = np.array(names)

    # getTrianglesArea / getAverageEdgeLength of the reference (float32 vertices, as load_mesh gives them)
    if not F64:
        for name, (V, F) in (("ico3", cases()[0][1]), ("open", cases()[4][1])):
            el, ne = ref_utils.getAverageEdgeLength(V, F)
            eln, _ = ref_utils.getAverageEdgeLength(V, F, normalize=True)
            out["mesh_%s_V" % name], out["mesh_%s_F" % name] = V, F
            out["mesh_%s_area" % name] = ref_utils.getTrianglesArea(V, F)
            out["mesh_%s_area_norm" % name] = ref_utils.getTrianglesArea(V, F, normalize=True)
            out["mesh_%s_edge" % name] = np.array([el, ne, eln], dtype=np.float64)
            out["mesh_%s_centres" % name] = ref_utils.getTrianglesBarycenter(V, F, normalize=False)

    # 100k faces: the whole mesh through the reference, 512 rows kept
    Vt, Ft = torus(250, 200)
    V, F = noisy(Vt, Ft), Ft.astype(np.int32)
    Fc, Fn, Fa = inputs(V, F)
    el, _ = pkg.getAverageEdgeLength(V, F)
    ss, sr = [float(el)], [0.35]
    rows = np.sort(np.random.RandomState(11).choice(F.shape[0], size=512, replace=False))
    r64, pop, win, t64 = reference(Fc, Fn, Fa, ss, sr, np.float64)
    out["torus100k_rows"], out["torus100k_sigma_s"], out["torus100k_sigma_r"] = rows, np.array(ss), np.array(sr)
    out["torus100k_checksum"] = checksum(Fc, Fn, Fa)
    if F64:
        out["torus100k_out_rows"] = r64[rows]
        print("torus100k     float64 %.1f s" % t64)
    else:
        r32, _, _, t32 = reference(Fc, Fn, Fa, ss, sr, np.float32)
        dev32 = float(np.abs(r32.astype(np.float64) - r64).max())
        out["torus100k_out_rows"], out["torus100k_dev32"] = r32[rows], np.float64(dev32)
        out["torus100k_pop"], out["torus100k_win"] = pop, win
        print("torus100k     faces %6d cells %4d mean window %7.1f dev32 %.2e  (float32 %.1f s, float64 %.1f s)" %
              (F.shape[0], len(pop), win.mean(), dev32, t32, t64))
    save("bilateral%s.npz" % SUFFIX, **out)


if __name__ == "__main__":
    main()
