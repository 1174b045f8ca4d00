"""CPU checks of the surface loss: the oracle of tests/surface_loss_cases.py against central differences and against its
float32 restatement, the data path (TrainingSet.addMeshWithVerticesAndGTMesh, preprocess --gt-surface, train
--surface-loss) and the argument checks of the two new entry points."""
import ctypes as C
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_loss_cases as sc     # noqa: E402
from facet_graph_convolution_amd import _lib, meshgen, preprocess, train as T          # noqa: E402
from facet_graph_convolution_amd.dataClasses import TrainingSet          # noqa: E402
from facet_graph_convolution_amd.utils import normalizePointSets, write_mesh          # noqa: E402

MARGIN = 1e-3          # what the winner of a sample beats the runner-up face by, in distance
H = 1e-6               # the step of the central differences


@pytest.mark.parametrize("name", ["sparser", "torus"])
def test_oracle_gradient_is_the_central_difference_of_the_oracle_loss(name):
    """On the float64 path that keeps the perturbed vertices as they are.  Samples: winner strictly inside its face (the
    closest point is a smooth function there, and an edge shared by two faces is no tie) and ahead of every other face
    by MARGIN.  The distance to the plane of a triangle is linear in the point and smooth in the triangle's vertices on the
    scale of its altitudes, so the bound per coordinate is (the terms on the row) x H^2 / h_min^2, the third derivative, plus
    8 x 2^-52 x loss / H, the rounding of the two losses."""
    c = sc.case(name)
    V0, V1 = c["V0"].astype(np.float64), c["V1"].astype(np.float64)
    F0, F1 = c["F0"], c["F1"]

    def clear(V, F, P, d_all):
        res = sc._closest(V, F, P, np.float64, True)
        d = np.sqrt(np.sort(res["all_dist2"], 1)[:, :2])
        inside = (res["u"] > 0.02) & (res["v"] > 0.02) & (res["u"] + res["v"] < 0.98)
        return np.nonzero(inside & (d[:, 1] - d[:, 0] > MARGIN) & (d_all >= sc.D_FLOOR))[0]
    rows0, rows1 = clear(V1, F1, V0, c["d0"]), clear(V0, F0, V1, c["d1"])
    assert rows0.size >= 20 and rows1.size >= 20, (rows0.size, rows1.size)
    rs = np.random.RandomState(3)
    i0, i1 = rows0[rs.randint(rows0.size, size=40)], rows1[rs.randint(rows1.size, size=30)]
    i0[:3] = i0[3]
    ref = sc.surface_loss(V0, F0, V1, F1, i0, i1, exact=True)
    touched = np.nonzero(ref["terms"])[0]
    assert set(i0) <= set(touched) and touched.size > np.unique(i0).size          # completeness terms land on other rows too
    worst = 0.0
    for r in np.concatenate([touched[rs.randint(touched.size, size=10)], i0[:2]]):
        for k in range(3):
            lo, hi = V0.copy(), V0.copy()
            lo[r, k] -= H
            hi[r, k] += H
            fd = (sc.surface_loss(hi, F0, V1, F1, i0, i1, exact=True)["loss"] -
                  sc.surface_loss(lo, F0, V1, F1, i0, i1, exact=True)["loss"]) / (2 * H)
            bound = ref["terms"][r] * H * H / c["h_min"] ** 2 + 8 * 2.0 ** -52 * ref["loss"] / H
            worst = max(worst, abs(fd - ref["grad"][r, k]) / bound)
            assert abs(fd - ref["grad"][r, k]) <= bound, (r, k, fd, ref["grad"][r, k], bound)
    assert np.abs(ref["grad"][touched]).max() > 0.1
    print("%s: central differences within %.3f of their bound" % (name, worst))


@pytest.mark.parametrize("name", sc.CASES)
def test_restatement_stays_within_its_figure(name):
    c = sc.case(name)
    assert all(0.8 <= k <= 0.99 for k in c["kept"]), c["kept"]
    r32 = sc.surface_loss(c["V0"], c["F0"], c["V1"], c["F1"], c["i0"], c["i1"], dtype=np.float32)
    k = sc.grad_figure(c, c["ref"], r32["grad"])
    rel = abs(float(r32["loss"]) - float(c["ref"]["loss"])) / float(c["ref"]["loss"])
    print("%s: restatement K %.3f (RESTATEMENT_K %.2f), loss %.6g rel err %.1e, rows kept %.0f%% / %.0f%%"
          % (name, k, sc.RESTATEMENT_K, c["ref"]["loss"], rel, 100 * c["kept"][0], 100 * c["kept"][1]))
    assert k <= 2 * sc.RESTATEMENT_K and rel <= 2.0 ** -20
    assert sc.GPU_K == 8 * sc.RESTATEMENT_K
    assert (c["ref"]["terms"] == 0).any() and np.unique(c["i0"]).size < c["i0"].size
    # a row with precision and completeness terms exists
    comp_rows = np.unique(c["F0"][c["ref"]["comp"]["face"]])
    assert np.intersect1d(comp_rows, c["i0"]).size > 0


def _pair():
    V, F = meshgen.icosphere(2)
    Vg, Fg = meshgen.icosphere(1)
    return meshgen.add_noise(V, F.astype(np.int64), seed=1) * 3.0, F, Vg * 3.0, Fg


def test_gt_mesh_set_shapes_normalisation_and_faces(tmp_path):
    Vn, F, Vg, Fg = _pair()
    ds = TrainingSet()
    ds.addMeshWithVerticesAndGTMesh(Vn, F, Vg, Fg, seed=0)
    ref = TrainingSet()
    ref.addMeshWithVertices(Vn, F, seed=0)
    assert len(ds.in_list) == len(ds.v_list) == len(ds.gtv_list) == len(ds.gtf_list) == 1 and ds.gt_list == []
    assert np.array_equal(ds.in_list[0], ref.in_list[0]) and np.array_equal(ds.faces_list[0], ref.faces_list[0])
    assert np.array_equal(ds.v_faces_list[0], ref.v_faces_list[0])
    assert all(np.array_equal(a, b) for a, b in zip(ds.adj_list[0], ref.adj_list[0]))
    want_v, want_gt = normalizePointSets(np.asarray(Vn, np.float32), np.asarray(Vg, np.float32))
    assert ds.v_list[0].shape == (1, Vn.shape[0], 3) and np.array_equal(ds.v_list[0][0], want_v)
    assert ds.gtv_list[0].shape == (1, Vg.shape[0], 3) and np.array_equal(ds.gtv_list[0][0], want_gt)
    assert not np.array_equal(ds.v_list[0], ref.v_list[0])          # (the joint box is not the noisy mesh's own)
    assert ds.gtf_list[0].dtype == np.int32 and ds.gtf_list[0].shape == (1, Fg.shape[0], 3)
    assert np.array_equal(ds.gtf_list[0][0], Fg) and Vg.shape[0] != Vn.shape[0] and Fg.shape[0] != F.shape[0]
    # the file form reads each OBJ with its own faces; preprocess --gt-surface writes the set train --with-vertices loads
    noisy, gt, dump = tmp_path / "noisy", tmp_path / "gt", tmp_path / "dump"
    noisy.mkdir(), gt.mkdir()
    write_mesh(Vn, F, str(noisy / "ball_n1.obj"))
    write_mesh(Vg, Fg, str(gt / "ball.obj"))
    preprocess.main([str(noisy), str(gt), str(dump), "--with-vertices", "--gt-surface"])
    with open(str(dump / "trainingSetWithVertices.pkl"), "rb") as fp:
        got = pickle.load(fp)
    assert got.gtf_list[0].shape == (1, Fg.shape[0], 3) and np.array_equal(got.gtf_list[0][0], Fg)
    assert got.gtv_list[0].shape == (1, Vg.shape[0], 3) and got.gt_list == []
    # the mesh records of the trainers: the set's own faces with surface_loss, nothing without
    m, = T._vertex_meshes(got, False, True)
    assert np.array_equal(m.bind_kw["gt_faces"], Fg) and m.rows == (Vn.shape[0], Vg.shape[0])
    assert T._vertex_meshes(got, False)[0].bind_kw is None
    # a paired set of one topology: the mesh's own rows, -1 rows included
    paired = TrainingSet()
    paired.addMeshWithVerticesAndGT(Vn, F, Vn, seed=0)
    m, = T._vertex_meshes(paired, False, True)
    assert np.array_equal(m.bind_kw["gt_faces"], paired.faces_list[0][0]) and (m.bind_kw["gt_faces"] < 0).any()
    # ground-truth vertices of another count without faces: nothing to measure a surface on
    odd = TrainingSet()
    odd.addMeshWithVerticesAndGTMesh(Vn, F, Vg, Fg, seed=0)
    del odd.__dict__["gtf_list"]
    with pytest.raises(ValueError, match="no ground-truth faces"):
        T._vertex_meshes(odd, False, True)


def test_refusals_of_the_data_path_and_the_commands(tmp_path, capsys):
    Vn, F, Vg, Fg = _pair()
    ds = TrainingSet()
    ds.addMeshWithVerticesAndGTMesh(Vn, F, Vg, Fg, seed=0)
    with pytest.raises(ValueError, match=r"no ground-truth face normals \(gt_list\) for the double loss"):
        T.trainDoubleLossNet(ds, 1, log=lambda s: None)
    with pytest.raises(ValueError, match=r"no ground-truth face normals \(gt_list\) for the double loss"):
        T.trainDoubleLossNet(ds, 1, log=lambda s: None, surface_loss=True)
    small = TrainingSet(maxSize=100)
    with pytest.raises(NotImplementedError, match="patch mode"):
        small.addMeshWithVerticesAndGTMesh(Vn, F, Vg, Fg)
    assert small.in_list == [] and "gtf_list" not in small.__dict__
    with pytest.raises(ValueError, match="ground-truth faces index"):
        TrainingSet().addMeshWithVerticesAndGTMesh(Vn, F, Vg, Fg + Vg.shape[0])
    with pytest.raises(ValueError, match="needs vertices"):
        TrainingSet().addMeshWithVerticesAndGTMesh(Vn, F, Vg, np.zeros((0, 3), np.int32))
    with pytest.raises(ValueError, match="gtSurface"):
        preprocess.pickleData(str(tmp_path), str(tmp_path), str(tmp_path / "d"), gtSurface=True)
    for argv, msg in (([str(tmp_path), str(tmp_path), str(tmp_path), "--gt-surface"], "--gt-surface needs --with-vertices"),
                      ([str(tmp_path), str(tmp_path), "--clean", "--with-vertices", "--gt-surface"], "--gt-surface needs")):
        with pytest.raises(SystemExit):
            preprocess.main(argv)
        assert msg in capsys.readouterr().err
    for argv, msg in (([str(tmp_path), str(tmp_path), "--surface-loss"], "--surface-loss is the point loss of the vertex"),
                      ([str(tmp_path), str(tmp_path), "--surface-loss", "--synth-noise"], "it needs --with-vertices")):
        with pytest.raises(SystemExit):
            T.main(argv)
        assert msg in capsys.readouterr().err


def test_new_entry_points_answer_einval_before_any_launch():
    """Every call below must return FGC_EINVAL from the host checks: the pointers are made-up addresses nobody may touch."""
    L = _lib.lib()
    P = lambda k: C.c_void_p(0x10000 * (k + 1))  # noqa: E731
    nv, nf, nq = 100, 196, 77
    need = L.fgc_closest_point_workspace_bytes(nf, nq)
    assert need == L.fgc_ray_cast_workspace_bytes(nf, nq) > 0
    assert L.fgc_closest_point_workspace_bytes(0, nq) == 0 and L.fgc_closest_point_workspace_bytes(nf, -1) == 0
    assert L.fgc_closest_point_workspace_bytes(2 ** 31 - 1, nq) == 0
    good = dict(verts=P(0), nv=nv, faces=P(1), nf=nf, points=P(2), nq=nq, d2=P(3), face=P(4), bary=P(5), ws=P(6),
                ws_bytes=need, stream=None)

    def cp(**kw):
        a = dict(good, **kw)
        return L.fgc_closest_point(*(a[k] for k in good))
    for k in ("verts", "faces", "points", "d2", "face", "ws"):
        assert cp(**{k: None}) == -22 and b"null" in L.fgc_last_error(), k
    for k in ("nv", "nf", "nq"):
        assert cp(**{k: 0}) == -22 and cp(**{k: -3}) == -22, k
    assert cp(nf=2 ** 31 - 1) == -22
    assert cp(ws_bytes=need - 1) == -22 and b"workspace" in L.fgc_last_error()
    assert cp(ws=C.c_void_p(0x80008)) == -22 and b"alignment" in L.fgc_last_error()

    np0, nf0, np1, nf1, ns0, ns1 = 100, 196, 60, 116, 500, 500
    need = L.fgc_surface_loss_workspace_bytes(nf0, nf1, ns0, ns1)
    assert need > 0 and need % 256 == 0
    for bad in ((0, nf1, ns0, ns1), (nf0, -1, ns0, ns1), (nf0, nf1, 0, ns1), (nf0, nf1, ns0, 0), (2 ** 31 - 1, nf1, ns0, ns1),
                (nf0, nf1, 16384 - 3 * 500 + 1, 500), (nf0, nf1, 1, 5462), (nf0, nf1, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert L.fgc_surface_loss_workspace_bytes(*bad) == 0, bad
    assert L.fgc_surface_loss_workspace_bytes(nf0, nf1, 16384 - 3 * 500, 500) > 0          # ns0 + 3 ns1 = the limit
    good2 = dict(p0=P(0), np0=np0, faces0=P(1), nf0=nf0, p1=P(2), np1=np1, faces1=P(3), nf1=nf1, i0=P(4), ns0=ns0, i1=P(5),
                 ns1=ns1, threshold=5000.0, loss=P(6), g=P(7), ws=C.c_void_p(0x100000), ws_bytes=need, stream=None)

    def sl(**kw):
        a = dict(good2, **kw)
        return L.fgc_surface_loss(*(a[k] for k in good2))
    for k in ("p0", "faces0", "p1", "faces1", "i0", "i1", "loss", "ws"):
        assert sl(**{k: None}) == -22 and b"null" in L.fgc_last_error(), k
    for k in ("np0", "nf0", "np1", "nf1", "ns0", "ns1"):
        assert sl(**{k: 0}) == -22 and sl(**{k: -1}) == -22, k
    assert sl(ns0=16384 - 3 * 500 + 1) == -22 and b"at most" in L.fgc_last_error()
    assert sl(ns1=5462) == -22 and sl(ns0=2 ** 31 - 1, ns1=2 ** 31 - 1) == -22
    assert sl(ws_bytes=need - 1) == -22 and b"workspace" in L.fgc_last_error()
    assert sl(ws=C.c_void_p(0x100010)) == -22 and b"alignment" in L.fgc_last_error()
    # fgc_point_loss, whose reduction the new loss shares, still checks as it did
    assert L.fgc_point_loss(P(0), 10, P(1), 10, P(2), 8192, P(3), 8193, 1.0, P(4), None, C.c_void_p(0x100000), 1 << 30,
                            None) == -22
