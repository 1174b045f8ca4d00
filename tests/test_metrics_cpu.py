"""CPU checks of the evaluation metrics (computeMetrics): the fgc_nn_query boundary refuses bad arguments before any
launch, and the host-side restatements of the reference's angular-error, border, heat-map and dense-cloud functions
match the fixtures made by running the reference (tests/golden/gen/make_golden_metrics.py).

Bounds: on the fixtures these functions are bit-identical to the reference (same numpy expressions in the same order).
The tolerances below leave room only for numpy's float32 transcendental kernels, which may differ by an ulp between CPUs
(1e-4 deg is thousands of ulps at these angles, and 50x below the 5e-3 deg the issue started from)."""
import ctypes as C
import os

import numpy as np
import pytest

from facet_graph_convolution_amd import _lib, settings, utils

MESHES = ("closed", "open", "fake")


@pytest.fixture(scope="module")
def ang(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics_angular.npz"))


def test_nn_query_rejects_bad_arguments():
    L = _lib.lib()
    buf = (C.c_char * 4096)()
    a = C.cast(buf, C.c_void_p)
    ws = C.c_void_p((C.addressof(buf) + 7) // 8 * 8)
    need = L.fgc_nn_workspace_bytes(10, 20)
    assert need >= 10 * 8
    cases = [
        (None, 10, a, 20, None, None, a, a, ws, need),       # null queries
        (a, 10, None, 20, None, None, a, a, ws, need),       # null candidates
        (a, 10, a, 20, None, None, None, a, ws, need),       # null dist
        (a, 10, a, 20, None, None, a, None, ws, need),       # null idx
        (a, 10, a, 20, None, None, a, a, None, need),        # null workspace
        (a, 0, a, 20, None, None, a, a, ws, need),           # empty query set
        (a, 10, a, 0, None, None, a, a, ws, need),           # empty candidate set
        (a, -3, a, 20, None, None, a, a, ws, need),
        (a, 10, a, 20, None, None, a, a, ws, need - 1),      # short workspace
        (a, 10, a, 20, a, None, a, a, ws, need),             # one mask without the other
    ]
    for args in cases:
        rc = L.fgc_nn_query(*args, None)
        assert rc == -22, args
        assert b"fgc_nn_query" in L.fgc_last_error()
    with pytest.raises(RuntimeError, match="fgc_nn_query"):
        _lib.check(L.fgc_nn_query(a, 10, a, 20, None, None, a, a, ws, need - 1, None), "fgc_nn_query")


def test_pack_cells():
    from facet_graph_convolution_amd.ops import pack_cells
    got = pack_cells(np.array([[0, 0, 0], [1, 2, 3], [-1, 0, 0], [4, 4, -1], [511, 511, 511]]))
    assert got.tolist() == [0, (1 << 20) | (2 << 10) | 3, -1, -1, (511 << 20) | (511 << 10) | 511]
    with pytest.raises(ValueError):
        pack_cells(np.array([[512, 0, 0]]))


@pytest.mark.parametrize("mesh", MESHES)
def test_angular_diff_matches_reference(ang, mesh):
    n0, n1 = ang[mesh + "_n0"], ang[mesh + "_n1"]
    vec = utils.angularDiffVec(n0, n1)
    assert vec.dtype == ang[mesh + "_vec"].dtype == np.float32
    assert np.abs(vec - ang[mesh + "_vec"]).max() <= 1e-4
    mean, std = utils.angularDiff(n0, n1)
    assert abs(mean - ang[mesh + "_mean"]) <= 1e-4 and abs(std - ang[mesh + "_std"]) <= 1e-4
    # the masks are equal, not close
    assert np.array_equal(utils.fakeNodes(n1), ang[mesh + "_fake"])
    assert np.array_equal(utils.getBorderFaces(ang[mesh + "_faces"]), ang[mesh + "_border"])


def test_masks_are_not_trivial(ang):
    assert ang["open_border"].sum() > 0 and ang["closed_border"].sum() == 0
    assert ang["fake_fake"].sum() >= 1 and ang["closed_fake"].sum() == 0
    # angularDiffVec keeps the fake faces, angularDiff leaves them out of the mean
    vec = ang["fake_vec"]
    assert vec.shape[0] == ang["fake_faces"].shape[0]
    assert abs(np.mean(vec[~ang["fake_fake"]]) - ang["fake_mean"]) <= 1e-4


@pytest.mark.parametrize("mesh", MESHES)
def test_heat_map_matches_reference(ang, mesh):
    vec = ang[mesh + "_vec"]
    angColor = np.maximum(1 - vec / settings.HEATMAP_MAX_ANGLE, np.zeros_like(vec))
    colors = utils.getHeatMapColor(1 - angColor)
    assert colors.dtype == np.float64
    assert np.abs(colors - ang[mesh + "_colors"]).max() <= 1e-6
    newV, newF = utils.getColoredMesh(ang[mesh + "_verts"], ang[mesh + "_faces"], ang[mesh + "_colors"])
    assert newV.shape == ang[mesh + "_newV"].shape and np.abs(newV - ang[mesh + "_newV"]).max() == 0
    assert np.array_equal(newF, ang[mesh + "_newF"])
    # the computation from the denoised vertices on: native face normals, then the angles
    n0 = utils.computeFacesNormals(ang[mesh + "_verts"], ang[mesh + "_faces"])
    assert np.abs(n0 - ang[mesh + "_n0"]).max() <= 1e-7


def test_heat_map_ramp_pieces():
    v = np.array([0.0, 0.1, 0.25, 0.3, 0.5, 0.6, 0.75, 0.9, 1.0, np.nan], dtype=np.float32)
    c = utils.getHeatMapColor(v)
    assert c[0].tolist() == [0, 0, 1] and c[2].tolist() == [0, 1, 1] and c[4].tolist() == [0, 1, 0]
    assert c[6].tolist() == [1, 1, 0] and c[8].tolist() == [1, 0, 0]
    assert np.isnan(c[9]).all()          # NaN falls to the last piece, as in the reference's if / elif chain


def test_dense_pc():
    from facet_graph_convolution_amd.meshgen import icosphere
    V, F = icosphere(1)
    V = V.astype(np.float32)
    assert np.array_equal(utils.getDensePC(V, F, res=1), V)
    d2 = utils.getDensePC(V, F, res=2)
    # res = 2: (b0, b1) in {(0,1), (1,0), (1,1)} -> three samples per face
    assert d2.shape == (V.shape[0] + 3 * F.shape[0], 3)
    assert np.allclose(d2[V.shape[0]:V.shape[0] + F.shape[0]], (V[F[:, 1]] + V[F[:, 2]]) / 2)


def test_heatmap_max_angle():
    assert settings.HEATMAP_MAX_ANGLE == 30.0


def test_float64_budget(golden_dir, ang):
    """The float32 angles against the reference run in double on the same normals: the budget of fp32 itself."""
    a64 = np.load(os.path.join(golden_dir, "metrics_angular_f64.npz"))
    for mesh in MESHES:
        assert abs(utils.angularDiff(ang[mesh + "_n0"], ang[mesh + "_n1"])[0] - a64[mesh + "_mean"]) < 1e-3
