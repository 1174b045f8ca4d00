"""CPU checks of the closest-point query: the float64 oracle of tests/closest_cases.py on hand-made cases of all seven
regions, what fp32 costs the definition (the float32 restatement against float64: the figure the GPU tolerance was derived
from), the argument checks of fgc_closest_point_tree (before any launch), the refusals of the host layers, and the two new
options of computeMetrics."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from facet_graph_convolution_amd import _lib, computeMetrics, meshgen, ops, utils

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closest_cases as cc  # noqa: E402

MAX_FACES = 1 << 30


def test_the_entry_point_is_exported_declared_and_bound():
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fgc.h")).read()
    assert "fgc_closest_point_tree" in _lib.EXPORTS and L.fgc_closest_point_tree.argtypes is not None
    assert "int fgc_closest_point_tree(" in header and "#define FGC_CP_EXHAUSTIVE 1u" in header
    assert ops.CP_EXHAUSTIVE == 1
    added = header[header.index("Added under"):header.index("#define FGC_ABI_VERSION")]
    assert "fgc_closest_point_tree" in added
    assert L.fgc_version() == _lib.ABI_VERSION


def test_the_oracle_on_hand_made_cases_of_all_seven_regions():
    """The triangle a = (0, 0, 0), b = (2, 0, 0), c = (0, 2, 0) and points whose closest point is known by hand."""
    V = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], dtype=np.float32)
    F = np.array([[0, 1, 2]])
    s = np.sqrt(0.5)
    cases = [  # q, region, (u, v), distance
        ((-1, -1, 1), 0, (0, 0), np.sqrt(3)),                 # vertex a
        ((3, -0.5, 0), 1, (1, 0), np.sqrt(1.25)),             # vertex b
        ((0.5, -1, 2), 2, (0.25, 0), np.sqrt(5)),             # edge ab
        ((-0.5, 3, 0), 3, (0, 1), np.sqrt(1.25)),             # vertex c
        ((-1, 1.5, 0), 4, (0, 0.75), 1.0),                    # edge ac
        ((2, 2, 0), 5, (0.5, 0.5), 2 * s),                    # edge bc
        ((0.5, 0.5, -3), 6, (0.25, 0.25), 3.0),               # inside
        ((1.5, 1.5, 1), 5, (0.5, 0.5), np.sqrt(1.5)),         # above the edge bc, beyond it
        ((0, 0, 0), 0, (0, 0), 0.0), ((2, 0, 0), 1, (1, 0), 0.0), ((0, 2, 0), 3, (0, 1), 0.0),          # the vertices
        ((1, 1, 0), 5, (0.5, 0.5), 0.0),                      # on the edge bc
    ]
    a, e1, e2 = cc.records(V, F, np.float64)
    for q, region, (u, v), dist in cases:
        d2, gu, gv, gr = cc.pair(np.array([q], dtype=np.float64), a, e1, e2)
        assert gr[0] == region, (q, gr)
        assert abs(gu[0] - u) < 1e-15 and abs(gv[0] - v) < 1e-15 and abs(np.sqrt(d2[0]) - dist) < 1e-15, q
    assert {c[1] for c in cases} == set(range(7))
    # over all pairs: the nearer of two triangles, ties to the lower index, no face that takes part
    V2 = np.concatenate([V, V + np.float32([0, 0, 5])])
    F2 = np.array([[0, 1, 2], [3, 4, 5], [0, 1, 2], [1, 1, 1], [0, 1, 9]])          # a duplicate, a point, an id out of range
    res = cc.closest(V2, F2, np.array([[0.5, 0.5, 1], [0.5, 0.5, 4.5], [0.5, 0.5, 2.5]], dtype=np.float32))
    assert res["face"].tolist() == [0, 1, 0] and np.allclose(res["dist"], [1, 0.5, 2.5], atol=1e-15)
    assert np.allclose(cc.dist_to_face(V2, F2, [[0.5, 0.5, 1]], np.array([1])), 4.0)
    assert np.allclose(cc.rebuilt(V2, F2, res["face"], res["u"], res["v"]), [[0.5, 0.5, 0], [0.5, 0.5, 5], [0.5, 0.5, 0]])
    none = cc.closest(V2, F2[3:], np.zeros((2, 3), dtype=np.float32))
    assert none["face"].tolist() == [-1, -1] and np.isposinf(none["dist"]).all() and not none["u"].any()
    # a collinear triangle and a NaN vertex never win
    V3 = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [np.nan, 0, 0], [0, 0, 9], [1, 0, 9], [0, 1, 9]], dtype=np.float32)
    res = cc.closest(V3, np.array([[0, 1, 3], [4, 5, 6]]), np.array([[0.2, 0.2, 1]], dtype=np.float32))
    assert res["face"].tolist() == [1] and res["dist"][0] == 8.0


def test_the_scenes_and_point_sets_are_the_ones_the_tests_were_sized_for():
    faces = {"icosphere": 1280, "torus": 1024, "cube": 300, "torus64": 4096, "icosphere5": 20480}
    for name in cc.SCENES:
        V, F = cc.mesh(name)
        assert F.shape == (faces[name], 3) and V.dtype == np.float32
        sets = cc.point_sets(name)
        assert {"noisy", "verts", "centroids", "midpoints", "box"} <= set(sets)
        assert sets["box"].shape == (600, 3) and sets["verts"].shape == V.shape == sets["noisy"].shape
        assert sets["centroids"].shape == F.shape and all(p.dtype == np.float32 for p in sets.values())
        assert ("centre" in sets) == (name != "cube") and ("diagonals" in sets) == (name == "cube")
        P, where = cc.all_points(name)
        assert P.shape[0] == sum(p.shape[0] for p in sets.values()) and np.array_equal(P[where["box"]], sets["box"])
    # the centre of the icosphere is nearly as far from all of its faces (a subdivided icosahedron: within 0.1 %, no box can be
    # culled before a face is found); the diagonal points tie in pairs
    V, F = cc.mesh("icosphere")
    a, e1, e2 = cc.records(V, F, np.float64)
    d = np.sqrt(cc.pair(np.zeros((1, 3)), a, e1, e2)[0])
    assert np.ptp(d) < 1e-3 * d.min()
    V, F = cc.mesh("cube")
    P = cc.point_sets("cube")["diagonals"]
    a, e1, e2 = cc.records(V, F, np.float64)
    d = np.sqrt(cc.pair(P[:, None].astype(np.float64), a[None], e1[None], e2[None])[0])
    two = np.sort(d, axis=1)[:, :2]
    assert np.allclose(two[:, 0], 0.1, atol=1e-7) and (two[:, 1] - two[:, 0] < 1e-7).all()


def test_the_float32_restatement_stays_within_two_units_of_float64():
    """What fp32 costs the definition: the same numpy code in float32 against float64, on every point set of the three
    small scenes, in units of 2^-24 (max|q| + max|V|).  Measured: 1.19 at worst (the 600 box points of this file's seed on
    the icosphere; vertices, centroids and noisy vertices stay within 0.4), the face chosen in float32 never worse than the
    float64 minimum by more than 6e-8 (0.35 units).  The GPU bound, 16 units, rests on it."""
    worst = 0.0
    for name in cc.RESTATED:
        V, F = cc.mesh(name)
        P, where = cc.all_points(name)
        ref = cc.oracle(name)
        got = cc.closest(V, F, P, dtype=np.float32)
        excess = cc.dist_to_face(V, F, P, got["face"]) - ref["dist"]
        for key, rows in where.items():
            u = cc.unit(V, P[rows])
            err = np.abs(got["dist"][rows].astype(np.float64) - ref["dist"][rows]).max() / u
            print("%s %s: %d points, |float32 - float64| %.2f units, face excess %.1e (%.2f units)"
                  % (name, key, P[rows].shape[0], err, excess[rows].max(), excess[rows].max() / u))
            assert err <= cc.RESTATEMENT_UNITS and excess[rows].max() <= cc.RESTATEMENT_UNITS * u
            worst = max(worst, err)
        assert (got["face"] >= 0).all() and (got["u"] >= 0).all() and (got["v"] >= 0).all()
        assert (got["u"] + got["v"] <= 1 + 2.0 ** -22).all()
    print("worst: %.2f units" % worst)


def test_argument_checks_answer_einval_before_any_launch():
    """Every call below must return FGC_EINVAL from the host checks: the pointers are made-up addresses nobody may touch."""
    L = _lib.lib()
    nf, nq = 196, 77
    need = L.fgc_ray_tree_bytes(nf)
    P = lambda k: C.c_void_p(0x10000 * (k + 1))  # noqa: E731
    good = dict(tree=P(0), tree_bytes=need, nf=nf, points=P(1), nq=nq, flags=0, dist2_out=P(2), face_out=P(3), bary_out=P(4),
                stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return L.fgc_closest_point_tree(a["tree"], a["tree_bytes"], a["nf"], a["points"], a["nq"], a["flags"], a["dist2_out"],
                                        a["face_out"], a["bary_out"], a["stream"])
    for name in ("tree", "points", "dist2_out", "face_out"):
        assert call(**{name: None}) == -22, name
        assert b"fgc_closest_point_tree" in L.fgc_last_error()
    for name in ("nf", "nq"):
        assert call(**{name: 0}) == -22 and call(**{name: -5}) == -22, name
    assert call(nf=2 ** 31 - 1) == -22 and call(nf=MAX_FACES + 1) == -22
    for flags in (2, 3, 4, 0x80000000, 0xFFFFFFFE):
        assert call(flags=flags) == -22, flags
        assert b"flags" in L.fgc_last_error()
    assert call(tree_bytes=need - 1) == -22 and b"too small" in L.fgc_last_error()
    assert call(tree_bytes=0) == -22 and call(nf=nf + 4) == -22          # a tree built of fewer faces
    assert call(tree=C.c_void_p(0x80008)) == -22 and b"alignment" in L.fgc_last_error()
    for flags in (0, 1):          # the two valid values pass the flag check: what refuses them is the next bad argument
        assert call(flags=flags, bary_out=None, tree_bytes=need - 1) == -22 and b"too small" in L.fgc_last_error()


def test_the_host_layers_refuse_before_anything_reaches_the_gpu():
    V, F = cc.mesh("cube")
    with pytest.raises(TypeError, match="RayTree"):
        ops.closest_point_tree(torch.zeros(16), torch.zeros(4, 3))
    handle = ops.RayTree(torch.zeros(16, dtype=torch.uint8), F.shape[0], V.shape[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.closest_point_tree(handle, torch.zeros(4, 3))
    for accel in ("tree", 3):
        with pytest.raises(ValueError, match="accel"):
            utils.closest_points(np.zeros((4, 3)), V, F, accel=accel)
        with pytest.raises(ValueError, match="accel"):
            utils.surface_distances(V, V, F, accel=accel)
    with pytest.raises(ValueError, match="built of a mesh"):
        utils.closest_points(np.zeros((4, 3)), V, F[:10], accel=handle)


def _folder(tmp_path, n_results=3):
    gt, res = tmp_path / "gt", tmp_path / "res"
    gt.mkdir()
    res.mkdir()
    V, F = meshgen.icosphere(1)
    utils.write_mesh(V, F, str(gt / "ball.obj"))
    for k in range(1, n_results + 1):
        utils.write_mesh(meshgen.add_noise(V, F, 0.1, seed=k), F, str(res / ("ball_n%d_denoised.obj" % k)))
    return str(gt), str(res)


def test_the_two_options_exclude_each_other(tmp_path, capsys):
    gt, res = _folder(tmp_path)
    with pytest.raises(SystemExit) as e:
        computeMetrics.main([gt, res, "--surface", "--surface-only"])
    assert e.value.code == 2 and "not allowed with" in capsys.readouterr().err
    with pytest.raises(ValueError, match="exclude"):
        computeMetrics.computeMetrics(gt, res, surface=True, surface_only=True)
    assert sorted(os.listdir(res)) == ["ball_n%d_denoised.obj" % k for k in (1, 2, 3)]          # nothing was written


def test_surface_only_skips_the_names_that_have_a_line(tmp_path):
    """A fake results_surface.csv that names all three files: nothing is scored (no GPU is needed here), nothing written."""
    gt, res = _folder(tmp_path, n_results=2)          # ball_n3 is missing: logged, skipped
    csv = os.path.join(res, "results_surface.csv")
    fake = "".join("ball_n%d_denoised.obj 0.1000000 0.0500000 0.0600000 nan nan nan \n" % k for k in (1, 2))
    with open(csv, "w") as fh:
        fh.write(fake)
    assert computeMetrics._surface_names(csv) == {"ball_n1_denoised.obj", "ball_n2_denoised.obj"}
    assert computeMetrics._surface_names(os.path.join(res, "none.csv")) == set()
    lines = []
    computeMetrics.computeMetrics(gt, res, surface_only=True, log=lines.append)
    assert [ln.split(":")[0] for ln in lines] == ["Skipping ball_n%d_denoised.obj" % k for k in (1, 2, 3)]
    assert "has a line" in lines[0] and "has a line" in lines[1] and "not found" in lines[2]
    assert open(csv).read() == fake
    assert sorted(os.listdir(res)) == ["ball_n1_denoised.obj", "ball_n2_denoised.obj", "results_surface.csv"]
    # the format the skip rule reads is the format the scorer writes
    row = computeMetrics._csv_lines(["x.obj"], [[0.1, 0.05, 0.06, np.nan, np.nan, np.nan]])[0]
    assert row == "x.obj 0.1000000 0.0500000 0.0600000 nan nan nan \n"
    assert computeMetrics.SURFACE_KEYS == ("ev_max", "ev_mean", "ev_rms", "comp_max", "comp_mean", "hausdorff")
