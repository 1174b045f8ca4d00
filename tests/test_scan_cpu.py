"""CPU checks of the virtual depth scans: the float64 oracle of tests/scan_cases.py on cases answerable by hand, the
argument checks of fgc_ray_cast (before any launch), the refusals of ops.ray_cast and of the scan tool, utils.range_mesh
and utils.pixel_rays (host code), and that an open scan passes downstream."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from facet_graph_convolution_amd import _lib, utils

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_cases as sc  # noqa: E402

TRI_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
TRI_F = np.array([[0, 1, 2]], dtype=np.int32)


def test_oracle_on_cases_answerable_by_hand():
    centroid = TRI_V.mean(0)
    # straight down onto the centroid from height 2.5: t = 2.5, u = v = 1/3
    t, f, u, v = sc.first_hit(TRI_V, TRI_F, centroid + [0, 0, 2.5], [[0, 0, -1]])
    assert f[0] == 0 and abs(t[0] - 2.5) < 1e-12 and abs(u[0] - 1 / 3) < 1e-7 and abs(v[0] - 1 / 3) < 1e-7
    # the direction is not normalised: twice as long, half the t; from below (two-sided) the same
    t, f, _, _ = sc.first_hit(TRI_V, TRI_F, centroid + [0, 0, 2.5], [[0, 0, -2]])
    assert f[0] == 0 and abs(t[0] - 1.25) < 1e-12
    t, f, _, _ = sc.first_hit(TRI_V, TRI_F, centroid - [0, 0, 2.5], [[0, 0, 1]])
    assert f[0] == 0 and abs(t[0] - 2.5) < 1e-12
    # a ray parallel to the plane misses; so does one that points away and one beside the triangle
    for o, d in (([0.2, 0.2, 1], [1, 0, 0]), (centroid + [0, 0, 2.5], [0, 0, 1]), ([2, 2, 1], [0, 0, -1])):
        t, f, u, v = sc.first_hit(TRI_V, TRI_F, o, [d])
        assert f[0] == -1 and np.isinf(t[0]) and u[0] == 0 and v[0] == 0
    # t_min cuts a hit
    assert sc.first_hit(TRI_V, TRI_F, centroid + [0, 0, 2.5], [[0, 0, -1]], t_min=2.4)[1][0] == 0
    assert sc.first_hit(TRI_V, TRI_F, centroid + [0, 0, 2.5], [[0, 0, -1]], t_min=2.5)[1][0] == -1
    # two coincident triangles: the lower index; a nearer one behind them in the list still wins
    F2 = np.array([[0, 1, 2], [0, 1, 2]], dtype=np.int32)
    assert sc.first_hit(TRI_V, F2, centroid + [0, 0, 2.5], [[0, 0, -1]])[1][0] == 0
    V3 = np.concatenate([TRI_V, TRI_V + np.float32([0, 0, 1])])
    F3 = np.array([[0, 1, 2], [0, 1, 2], [3, 4, 5]], dtype=np.int32)
    t, f, _, _ = sc.first_hit(V3, F3, centroid + [0, 0, 2.5], [[0, 0, -1]])
    assert f[0] == 2 and abs(t[0] - 1.5) < 1e-12


def test_a_sphere_seen_from_far_shows_a_little_under_half_of_its_vertices():
    V, F, _ = sc.scene("icosphere")
    cam = np.array([1.0, -0.7, 10.0])      # (off the mesh's axes of symmetry: on one, rays run through mirror vertices)
    o, d = sc.perspective_rays(V, cam)
    c = sc.classify_vertices(V, F, o, d)
    share = (c == 1).sum() / c.size
    # the cap seen from distance D ends at height 1 / D: 45 % of the area at D = 10; a polyhedron also shows the vertices just
    # behind that horizon which still have a face turned to the camera (a band of about half an edge, 0.07)
    print("visible from %s: %d of %d vertices, %d ambiguous" % (cam, (c == 1).sum(), c.size, (c < 0).sum()))
    h = V @ (cam / np.linalg.norm(cam))
    assert 0.42 < share < 0.5 and (c < 0).sum() <= sc.CAP * c.size
    assert ((c == 1) <= (h > 0)).all() and ((h > 0.2) <= (c == 1)).all()


def test_the_scenes_are_the_ones_the_tests_were_sized_for():
    """Skipped cases, counted here in float64: image rays 3 / 2 / 1 of 1 850, no ambiguous vertex on the icosphere and the
    torus in either view; the cube's silhouette vertices are over the cap (27 of 152), so it is an image scene only."""
    want = {"icosphere": (642, 1280, 3), "torus": (512, 1024, 2), "cube": (152, 300, 1)}
    for name, (nv, nf, skipped) in want.items():
        V, F, _ = sc.scene(name)
        ic = sc.image_case(name)
        assert V.shape == (nv, 3) and F.shape == (nf, 3) and ic["rays"].shape == (1850, 3)
        assert (~ic["robust"]).sum() == skipped <= sc.CAP * 1850
        assert 0.3 < (ic["face"] >= 0).mean() < 0.95          # the image holds surface and background
    for name in sc.VISIBILITY_SCENES:
        for view in ("camera", "dir"):
            assert (sc.visibility_case(name, view) < 0).sum() == 0
    V, F, cam = sc.scene("cube")
    assert (sc.classify_vertices(V, F, *sc.perspective_rays(V, cam)) < 0).sum() == 27
    # the torus occludes itself: hidden vertices that face the camera
    V, F, cam = sc.scene("torus")
    n = utils.areaWeightedVertexNormals(V, F)
    facing = (n * (V - np.asarray(cam))).sum(1) < 0
    assert (facing & (sc.visibility_case("torus", "camera") == 0)).sum() > 10


def test_argument_checks_answer_einval_before_any_launch():
    """Every call below must return FGC_EINVAL from the host checks: the pointers are made-up addresses nobody may touch."""
    L = _lib.lib()
    nv, nf, nq = 100, 196, 77
    need = L.fgc_ray_cast_workspace_bytes(nf, nq)
    assert need >= nf * 48 + nq * 8 and need % 16 == 0
    assert L.fgc_ray_cast_workspace_bytes(0, nq) == 0 and L.fgc_ray_cast_workspace_bytes(nf, 0) == 0
    assert L.fgc_ray_cast_workspace_bytes(-1, nq) == 0 and L.fgc_ray_cast_workspace_bytes(2 ** 31 - 1, nq) == 0
    P = lambda k: C.c_void_p(0x10000 * (k + 1))  # noqa: E731
    good = dict(verts=P(0), nv=nv, faces=P(1), nf=nf, origins=P(2), n_origins=1, dirs=P(3), nq=nq, t_min=0.0, t_out=P(4),
                face_out=P(5), bary_out=P(6), ws=P(7), ws_bytes=need, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return L.fgc_ray_cast(a["verts"], a["nv"], a["faces"], a["nf"], a["origins"], a["n_origins"], a["dirs"], a["nq"],
                              a["t_min"], a["t_out"], a["face_out"], a["bary_out"], a["ws"], a["ws_bytes"], a["stream"])
    for name in ("verts", "faces", "origins", "dirs", "t_out", "face_out", "ws"):
        assert call(**{name: None}) == -22, name
        assert b"fgc_ray_cast" in L.fgc_last_error()
    for name in ("nv", "nf", "nq"):
        assert call(**{name: 0}) == -22 and call(**{name: -5}) == -22, name
    for n_origins in (0, 2, nq - 1, nq + 1, -1):
        assert call(n_origins=n_origins) == -22, n_origins
    assert b"n_origins" in L.fgc_last_error()
    for t_min in (-1e-6, float("inf"), float("-inf"), float("nan")):
        assert call(t_min=t_min) == -22, t_min
    assert b"t_min" in L.fgc_last_error()
    assert call(ws_bytes=need - 1) == -22 and b"workspace" in L.fgc_last_error()
    assert call(ws_bytes=0) == -22
    assert call(ws=C.c_void_p(0x80008)) == -22 and b"alignment" in L.fgc_last_error()
    assert call(nf=2 ** 31 - 1) == -22


def test_ray_cast_refuses_cpu_tensors():
    import torch
    from facet_graph_convolution_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ray_cast(torch.from_numpy(TRI_V), torch.from_numpy(TRI_F), torch.zeros(1, 3), torch.ones(4, 3))


def test_scan_cli_refuses_contradictions(tmp_path, capsys):
    from facet_graph_convolution_amd import scan
    d = str(tmp_path)
    cases = [
        ([d, d, "--view-dir", "0,0,1", "--camera", "0,0,5"], "not allowed with"),
        ([d, d], "needs --view-dir or --camera"),
        ([d, d, "--image", "50,37", "--view-dir", "0,0,-1"], "--image needs --camera"),
        ([d, d, "--image", "50", "--camera", "0,0,5"], "W,H"),
        ([d, d, "--camera", "0,0"], "X,Y,Z"),
        ([d, d, "--view-dir", "0,0,0"], "zero vector"),
        ([d, d, "--camera", "0,0,5", "--max-angle", "0"], "--max-angle"),
        ([d, d, "--camera", "0,0,5", "--eps", "1"], "--eps"),
    ]
    for argv, msg in cases:
        with pytest.raises(SystemExit) as e:
            scan.main(argv)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err, argv
    # from Python: the same contradictions are ValueErrors before anything reaches the GPU
    V, F, cam = sc.scene("icosphere")
    with pytest.raises(ValueError, match="exactly one"):
        scan.scan_mesh(V, F)
    with pytest.raises(ValueError, match="exactly one"):
        scan.scan_mesh(V, F, camera=cam, view_dir=(0, 0, -1))
    with pytest.raises(ValueError, match="needs a camera"):
        scan.scan_mesh(V, F, view_dir=(0, 0, -1), image=(50, 37))
    with pytest.raises(ValueError, match="at the camera"):
        utils.visible_vertices(V, F, camera=V[5])
    with pytest.raises(ValueError, match="max_angle"):
        utils.scan_cut(V, F, camera=cam, max_angle=0.0)


def test_pixel_rays():
    V, F, cam = sc.scene("torus")
    look = 0.5 * (V.astype(np.float64).min(0) + V.astype(np.float64).max(0))
    r = utils.pixel_rays(cam, look, sc.IMAGE, sc.FOV)
    want = sc.pixel_rays(cam, look)
    assert r.dtype == np.float32 and r.shape == (37, 50, 3) and np.abs(r - want).max() <= 2.0 ** -24
    assert np.abs(np.linalg.norm(r.astype(np.float64), axis=-1) - 1).max() < 1e-7
    assert utils.pixel_rays(cam, look, sc.IMAGE, sc.FOV).tobytes() == r.tobytes()
    # the horizontal field of view spans the image's width, pixel centres half a pixel inside
    f = (look - cam) / np.linalg.norm(look - cam)
    half = np.degrees(np.arccos(np.clip(r[:, [0, -1]].astype(np.float64) @ f, -1, 1)))
    assert half.min() > 19.0 and half[18].max() < 20.0
    # row 0 is the top of the image: it looks further up (+z) than the last one; column 0 is on the left
    assert r[0, 25, 2] > r[-1, 25, 2]
    right = np.cross(f, [0, 0, 1.0])
    assert r[18, 0].astype(np.float64) @ right < 0 < r[18, -1].astype(np.float64) @ right
    # looking straight down: up falls back to (0, 1, 0), so the top row looks towards +y
    r = utils.pixel_rays((0, 0, 5), (0, 0, 0), (8, 6), 40.0)
    assert np.isfinite(r).all() and r[0, 4, 1] > 0 > r[-1, 4, 1] and r[3, 0, 0] * r[3, -1, 0] < 0
    with pytest.raises(ValueError):
        utils.pixel_rays((0, 0, 5), (0, 0, 5), (8, 6))
    with pytest.raises(ValueError):
        utils.pixel_rays((0, 0, 5), (0, 0, 0), (8, 6), fov=180.0)


def test_range_mesh_on_a_hand_made_depth_array():
    """3 x 3 pixels seen straight down from (0, 0, 5), one background pixel (top left) and one jump (bottom right): of the
    four blocks only the top right one and the bottom left one survive."""
    cam = (0.0, 0.0, 5.0)
    rays = utils.pixel_rays(cam, (0, 0, 0), (3, 3), 40.0)
    depth = np.full((3, 3), 5.0)
    depth[0, 0] = np.inf
    depth[2, 2] = 5.0 * 1.06                      # above jump = 0.05 of the nearest
    V, F, pix = utils.range_mesh(depth, rays, cam, return_pixels=True)
    assert V.dtype == np.float32 and F.dtype == np.int32
    assert pix.tolist() == [1, 2, 3, 4, 5, 6, 7]                      # row-major; pixels 0 and 8 are in no triangle
    assert pix[F].tolist() == [[1, 4, 2], [4, 5, 2], [3, 6, 4], [6, 7, 4]]
    want = np.asarray(cam) + depth.reshape(-1, 1)[pix] * rays.reshape(-1, 3)[pix].astype(np.float64)
    assert np.abs(V - want).max() <= 2.0 ** -24 * 5
    # oriented towards the camera
    T = V.astype(np.float64)[F]
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    assert ((n * (T.mean(1) - np.asarray(cam))).sum(1) < 0).all()
    # the rays come back from the vertices
    assert np.abs(utils.view_rays(V, camera=cam) - rays.reshape(-1, 3)[pix]).max() <= 2.0 ** -23
    # the oracle says the same; at jump = 0.07 the fourth block comes back
    Vo, Fo, ido, _ = sc.range_mesh(depth, rays, cam)
    assert ido.tolist() == pix.tolist() and Fo.tolist() == pix[F].tolist() and np.abs(Vo - V).max() <= 2.0 ** -24 * 5
    assert utils.range_mesh(depth, rays, cam, jump=0.07)[1].shape[0] == 6
    assert utils.range_mesh(depth, rays, cam)[0].tobytes() == V.tobytes()
    with pytest.raises(ValueError, match="no 2 x 2 block"):
        utils.range_mesh(np.full((3, 3), np.inf), rays, cam)
    with pytest.raises(ValueError):
        utils.range_mesh(depth[:2], rays, cam)


def test_an_open_scan_passes_downstream():
    """The oracle's cut of the icosphere - an open sheet with a border - is accepted by TrainingSet.addCleanMesh, and the
    arguments of makeNoisy.make_noisy(..., direction=view_rays(...)) pass their checks on it."""
    from facet_graph_convolution_amd import makeNoisy
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    V, F, cam = sc.scene("icosphere")
    Vc, Fc, ids, keep = sc.cut(V, F, sc.visibility_case("icosphere", "camera") == 1, camera=cam)
    assert 0 < Fc.shape[0] < F.shape[0] // 2 and Vc.shape[0] == ids.size and np.array_equal(Vc, V[ids])
    assert np.array_equal(ids[Fc], F[keep]) and utils.getBorderFaces(Fc).sum() > 0
    ds = TrainingSet()
    ds.addCleanMesh(Vc, Fc)
    assert ds.mesh_count == 1
    rays = utils.view_rays(Vc, camera=cam)
    assert utils.check_directions(rays, Vc.shape[0]).tobytes() == rays.tobytes()
    with pytest.raises(ValueError, match="one row per vertex"):
        makeNoisy.make_noisy(Vc, Fc, 0.1, direction=utils.view_rays(V, camera=cam))      # the closed mesh's rays
    # on host tensors the call passes every check of its arguments and stops at the kernel (tests/test_gpu_scan.py runs it)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        makeNoisy.make_noisy(Vc, Fc, 0.1, direction=rays, device="cpu")
