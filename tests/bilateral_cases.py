"""What the two bilateral test files share: the fixture cases of tests/golden/bilateral*.npz (made by
tests/golden/gen/make_golden_bilateral.py), their inputs, and a float64 brute force of the filter."""
import os

import numpy as np

from facet_graph_convolution_amd import utils
from facet_graph_convolution_amd.meshgen import icosphere, torus, add_noise

CASES = ("ico3_a", "ico3_wide", "ico3_norange", "torus2400", "open", "flat", "fnd", "ico5")


def load(golden_dir):
    return (np.load(os.path.join(golden_dir, "bilateral.npz")), np.load(os.path.join(golden_dir, "bilateral_f64.npz")))


def mesh_inputs(V, F):
    """(Fc, Fn, Fa) float32, as the generator makes them."""
    V, F = np.asarray(V, dtype=np.float32), np.asarray(F).astype(np.int32)
    return (utils.getTrianglesBarycenter(V, F, normalize=False).astype(np.float32),
            utils.computeFacesNormals(V, F).astype(np.float32), utils.getTrianglesArea(V, F).astype(np.float32))


def noisy_mesh(name):
    V, F = {"ico4": lambda: icosphere(4), "ico5": lambda: icosphere(5), "torus100k": lambda: torus(250, 200)}[name]()
    return add_noise(V, F, sigma_rel=0.2, seed=3).astype(np.float32), F.astype(np.int32)


def checksum(Fc, Fn, Fa):
    return np.array([a.astype(np.float64).sum() for a in (Fc, Fn, Fa)] +
                    [np.abs(a.astype(np.float64)).sum() for a in (Fc, Fn, Fa)])


def case_inputs(z32, name):
    """The case's (Fc, Fn, Fa): stored where small, regenerated from meshgen otherwise; either way the checksum the
    generator stored must hold, so that a drift of meshgen or of the host functions shows as such."""
    if name + "_Fc" in z32.files:
        Fc, Fn, Fa = z32[name + "_Fc"], z32[name + "_Fn"], z32[name + "_Fa"]
    else:
        Fc, Fn, Fa = mesh_inputs(*noisy_mesh(name))
    want = z32[name + "_checksum"]
    got = checksum(Fc, Fn, Fa)
    assert np.all(np.abs(got - want) <= 1e-11 * (1 + np.abs(want))), ("inputs of %s drifted" % name, got, want)
    return Fc, Fn, Fa


def occupancy(cell, grid):
    """(populations, window sizes) of the occupied cells in lexicographic order: what the reference prints."""
    sx, sy, sz = grid
    ok = (cell >= 0).all(1)
    count = np.zeros((sx + 2, sy + 2, sz + 2), dtype=np.int64)
    np.add.at(count, tuple((cell[ok] + 1).T), 1)
    window = np.zeros((sx, sy, sz), dtype=np.int64)
    for di in range(3):
        for dj in range(3):
            for dk in range(3):
                window += count[di:di + sx, dj:dj + sy, dk:dk + sz]
    inner = count[1:-1, 1:-1, 1:-1]
    occ = inner > 0
    return inner[occ], window[occ]


def brute(Fc, Fn, Fa, sigma_s, sigma_r, cell, rows=None):
    """float64 rows of the filter (include/fgc.h: fgc_bilateral_filter) for one (sigma_s, sigma_r): windows from the
    given cell coordinates, weights a_j exp(-|dc|^2 / 2 ss^2) exp(-|dn|^2 / 2 sr^2), utils.normalize."""
    Fc, Fn, Fa = (np.asarray(a, dtype=np.float64) for a in (Fc, Fn, Fa))
    rows = np.arange(Fc.shape[0]) if rows is None else np.asarray(rows)
    out = np.zeros((len(rows), 3))
    valid = (cell >= 0).all(1)
    step = max(8, min(128, 4000000 // Fc.shape[0]))
    for s in range(0, len(rows), step):
        r = rows[s:s + step]
        near = (np.abs(cell[r][:, None, :] - cell[None, :, :]) <= 1).all(-1) & valid[None, :] & valid[r][:, None]
        w = np.exp(-((Fc[r][:, None, :] - Fc[None]) ** 2).sum(-1) / (2 * sigma_s ** 2)) * Fa[None, :]
        if sigma_r != -1:
            w = w * np.exp(-((Fn[r][:, None, :] - Fn[None]) ** 2).sum(-1) / (2 * sigma_r ** 2))
        out[s:s + step] = (np.where(near, w, 0.0)[:, :, None] * Fn[None]).sum(1)
    return utils.normalize(out)
