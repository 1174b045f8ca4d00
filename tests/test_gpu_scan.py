"""GPU checks of the virtual depth scans: fgc_ray_cast (ops.ray_cast) and the host functions built on it
(utils.visible_vertices, scan_cut, depth_image, range_mesh, the scan tool) against the float64 oracle of
tests/scan_cases.py, on the cases that oracle calls robust; every test asserts that it skipped at most 2 % of its cases.

The bound on t and on the barycentrics of a hit is C_BOUND x 2^-24 x t / |n . d| (n the unit normal of the hit face, d the
unit ray).  C_BOUND is not derived from the arithmetic; it is four times the largest normalised error measured against
the float64 oracle on the robust rays of the three image scenes (on an MI355X: 4.21 for t, the icosphere, and 11.47 for the
barycentrics, the torus; each test prints its figures; the factor covers other views of the same meshes).  The barycentrics are the larger figure because
they divide a position error by an edge length (0.14 to 0.3 here) where t does not."""
import os
import sys

import numpy as np
import pytest
import torch

from facet_graph_convolution_amd import ops, utils
from facet_graph_convolution_amd.meshgen import icosphere

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

MEASURED = 11.47
C_BOUND = 4 * MEASURED
EPS24 = 2.0 ** -24


def dev(a, dt=np.float32):
    return torch.from_numpy(np.array(a, dtype=dt, order="C")).cuda()


def cast(V, F, origins, dirs, t_min=0.0):
    t, f, b = ops.ray_cast(dev(V), dev(F, np.int32), dev(np.asarray(origins).reshape(-1, 3)), dev(dirs), t_min, want_bary=True)
    torch.cuda.synchronize()
    return t.cpu().numpy(), f.cpu().numpy(), b.cpu().numpy()


def image_oracle(name, rays):
    """The cached image case of the scene if `rays` are its rays bit for bit, otherwise the oracle of these rays."""
    ic = sc.image_case(name)
    rays = np.asarray(rays).reshape(-1, 3)
    if rays.tobytes() == ic["rays"].tobytes():
        return ic
    V, F, cam = sc.scene(name)
    mt = sc.moller_trumbore(V, F, np.asarray(cam).reshape(1, 3), rays)
    t, face, u, v = sc.first_hit(V, F, None, None, mt=mt)
    nd = np.abs(mt["nd"][np.arange(rays.shape[0]), np.maximum(face, 0)])
    return {"rays": rays, "t": t, "face": face, "u": u, "v": v, "robust": sc.robust_rays(mt),
            "scale": np.where(face >= 0, t / np.where(nd > 0, nd, 1.0), 0.0)}


@pytest.mark.parametrize("name", list(sc.SCENES))
def test_image_rays_equal_the_oracle_on_robust_rays(name):
    """1 850 pixel rays (29 workgroups, the last one partly filled) against 1 280 / 1 024 / 300 faces (300 is no multiple of
    the waves' 16 records per round): hit or miss and the face equal the oracle's, t and (u, v) are within C_BOUND."""
    V, F, cam = sc.scene(name)
    ic = sc.image_case(name)
    t, f, b = cast(V, F, cam, ic["rays"])
    rb = ic["robust"]
    assert (~rb).sum() <= sc.CAP * rb.size
    assert np.array_equal(f[rb], ic["face"][rb])
    miss = rb & (ic["face"] < 0)
    assert np.isposinf(t[miss]).all() and not b[miss].any()
    h = rb & (ic["face"] >= 0)
    unit = EPS24 * ic["scale"][h]
    errs = [np.abs(t[h] - ic["t"][h]) / unit, np.abs(b[h, 0] - ic["u"][h]) / unit, np.abs(b[h, 1] - ic["v"][h]) / unit]
    print("%s: %d robust hits, normalised error t %.3f, u %.3f, v %.3f (C_BOUND %.1f)"
          % (name, h.sum(), errs[0].max(), errs[1].max(), errs[2].max(), C_BOUND))
    assert max(e.max() for e in errs) <= C_BOUND
    # fp32 results are sane on the skipped rays too: a face of the mesh or a miss, (u, v) inside the triangle
    assert ((f >= -1) & (f < F.shape[0])).all() and (b >= 0).all() and (b.sum(1) <= 1).all()


@pytest.mark.parametrize("view", ["camera", "dir"])
@pytest.mark.parametrize("name", sc.VISIBILITY_SCENES)
def test_visible_vertices_equal_the_oracle(name, view):
    V, F, _ = sc.scene(name)
    want = sc.visibility_case(name, view)
    assert (want < 0).sum() <= sc.CAP * want.size          # (the orthographic view too: scan_cases.VIEW_DIR says why not -z)
    vis = utils.visible_vertices(V, F, **sc.view_kwargs(name, view))
    assert vis.dtype == bool and vis.shape == (V.shape[0],)
    sure = want >= 0
    assert np.array_equal(vis[sure], want[sure] == 1)
    assert 0.3 < vis.mean() < 0.6


@pytest.mark.parametrize("view", ["camera", "dir"])
@pytest.mark.parametrize("name", sc.VISIBILITY_SCENES)
def test_scan_cut_equals_the_oracle(name, view):
    V, F, _ = sc.scene(name)
    kw = sc.view_kwargs(name, view)
    cls = sc.visibility_case(name, view)
    Vc, Fc, ids = utils.scan_cut(V, F, **kw)
    Vo, Fo, ido, keep = sc.cut(V, F, cls == 1, **kw)
    assert Vc.dtype == np.float32 and Fc.dtype == np.int32 and np.array_equal(Vc, V[ids])
    if not (cls < 0).any():
        assert np.array_equal(ids, ido) and np.array_equal(Fc, Fo) and np.array_equal(Vc, Vo)
    else:          # faces without an ambiguous vertex
        sure = (cls[F] >= 0).all(1)
        kept = set(map(tuple, ids[Fc].tolist()))
        mine = np.array([tuple(row) in kept for row in F.tolist()])
        assert np.array_equal(mine[sure], keep[sure])
    # every kept vertex is visible, the old order is kept, and the sheet is open
    assert (np.diff(ids) > 0).all() and utils.visible_vertices(V, F, **kw)[ids].all()
    assert 0 < Fc.shape[0] < F.shape[0] and utils.getBorderFaces(Fc).sum() > 0
    if (name, view) == ("icosphere", "camera"):
        # the open scan passes downstream: noise along the scan's own rays moves every vertex along its ray only
        from facet_graph_convolution_amd import makeNoisy
        rays = utils.view_rays(Vc, camera=kw["camera"])
        Vn = makeNoisy.make_noisy(Vc, Fc, 0.2, direction=rays)
        step = Vn.astype(np.float64) - Vc
        along = (step * rays).sum(1, keepdims=True) * rays
        assert np.abs(step).max() > 1e-3 and np.abs(step - along).max() < 1e-6


def test_depth_image_and_range_mesh_on_the_torus():
    V, F, cam = sc.scene("torus")
    depth, face, rays = utils.depth_image(V, F, cam, size=sc.IMAGE, fov=sc.FOV)
    assert depth.shape == face.shape == (37, 50) and rays.shape == (37, 50, 3) and depth.dtype == rays.dtype == np.float32
    assert np.abs(rays.reshape(-1, 3) - sc.image_case("torus")["rays"]).max() <= EPS24
    ic = image_oracle("torus", rays)
    rb = ic["robust"].reshape(37, 50)
    assert (~rb).sum() <= sc.CAP * rb.size
    assert np.array_equal(face[rb], ic["face"].reshape(37, 50)[rb])
    assert np.array_equal(np.isinf(depth), face < 0)
    Vr, Fr, pix = utils.range_mesh(depth, rays, cam, return_pixels=True)
    to = ic["t"].reshape(37, 50)
    Vo, Fo, pixo, blocks = sc.range_mesh(to, rays, cam)
    # vertices: on the pixels both meshes use and the oracle calls robust, within the bound on t (the ray is a unit vector)
    common = np.intersect1d(pix, pixo)
    common = common[ic["robust"][common]]
    assert common.size > 0.9 * pixo.size
    err = np.abs(Vr[np.searchsorted(pix, common)] - Vo[np.searchsorted(pixo, common)]).max(1)
    bound = C_BOUND * EPS24 * ic["scale"][common] + EPS24 * 4          # (+ the rounding of the vertex itself, |v| < 4)
    assert (err <= bound).all(), (err / bound).max()
    # faces: the same where all four pixels of a block are robust and the jump test is not within 1e-4 of its threshold
    ok = rb[:-1, :-1] & rb[1:, :-1] & rb[:-1, 1:] & rb[1:, 1:] & (sc.jump_margin(to) >= 1e-4)
    assert (~ok).sum() <= 4 * sc.CAP * ok.size          # (a skipped pixel takes its four blocks along)

    def checked(faces_as_pixels):
        r, c = np.divmod(faces_as_pixels.min(1), 50)          # p00 of the block: the smallest pixel index of either triangle
        c = np.where(faces_as_pixels.min(1) == faces_as_pixels[:, 0], c, c - 1)      # ... of (p10, p11, p01) it is p01 - 1
        keep = ok[r, c]
        return set(map(tuple, faces_as_pixels[keep].tolist()))
    assert checked(pix[Fr]) == checked(Fo) and len(checked(Fo)) > 0.9 * Fo.shape[0]
    # the torus occludes itself: the range mesh has a border, and jumps were cut
    assert utils.getBorderFaces(Fr).sum() > 0
    assert np.isfinite(sc.jump_margin(depth.astype(np.float64))).sum() > Fr.shape[0] // 2
    assert np.abs(utils.view_rays(Vr, camera=cam) - rays.reshape(-1, 3)[pix]).max() <= 2.0 ** -23


def test_kernel_edges():
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    one = np.array([[0, 1, 2]], dtype=np.int32)
    o = np.array([[0.25, 0.25, 2.0]], dtype=np.float32)
    down = np.array([[0, 0, -1]], dtype=np.float32)
    # nq = 1, nf = 1; the direction is not normalised
    t, f, b = cast(tri, one, o, down)
    assert f.tolist() == [0] and t.tolist() == [2.0] and b.tolist() == [[0.25, 0.25]]
    t, f, b = cast(tri, one, o, 4 * down)
    assert f.tolist() == [0] and t.tolist() == [0.5] and b.tolist() == [[0.25, 0.25]]
    # two-sided; a parallel ray, one that points away and one beside the triangle miss: inf, -1, (0, 0)
    t, f, b = cast(tri, one, [[0.25, 0.25, -2.0]], -down)
    assert f.tolist() == [0] and t.tolist() == [2.0]
    d4 = np.array([[1, 0, 0], [0, 0, 1], [0, 0, -1], [0, 0, -1]], dtype=np.float32)
    o4 = np.array([[0.25, 0.25, 2], [0.25, 0.25, 2], [2, 2, 2], [0.25, 0.25, 2]], dtype=np.float32)
    t, f, b = cast(tri, one, o4, d4)
    assert f.tolist() == [-1, -1, -1, 0] and np.isposinf(t[:3]).all() and not b[:3].any() and t[3] == 2.0
    # rows with an id >= nv or < 0 and a zero-area triangle are skipped; a duplicate face gives the lower index
    V2 = np.concatenate([tri + np.float32([0, 0, 1]), tri])          # the upper triangle is nearer
    F2 = np.array([[0, 1, 6], [0, -1, 2], [0, 0, 1], [1, 1, 1], [3, 4, 5], [3, 4, 5], [2 ** 31 - 1, 1, 2]], dtype=np.int64)
    t, f, b = cast(V2, F2.astype(np.int32), o, down)
    assert f.tolist() == [4] and t.tolist() == [2.0]
    F3 = np.array([[3, 4, 5], [0, 1, 2], [0, 1, 2]], dtype=np.int32)
    t, f, b = cast(V2, F3, o, down)
    assert f.tolist() == [1] and t.tolist() == [1.0]
    # t_min: from a point ON the lower face, t_min = 1e-4 skips that face (t = 0) and finds the one above
    on = np.array([[0.25, 0.25, 0.0]], dtype=np.float32)
    t, f, b = cast(V2, F3, on, -down, t_min=1e-4)
    assert f.tolist() == [1] and t.tolist() == [1.0]
    t, f, b = cast(V2, F3, on, -down, t_min=1.0)          # t > t_min is strict
    assert f.tolist() == [-1]
    # without the barycentrics, and with every row invalid
    t, f = ops.ray_cast(dev(V2), dev(F3, np.int32), dev(o), dev(down))
    assert t.cpu().tolist() == [1.0] and f.cpu().tolist() == [1]
    t, f, b = cast(tri, np.array([[0, 1, 3], [5, 5, 5]], dtype=np.int32), o, down)
    assert f.tolist() == [-1] and np.isposinf(t).all()
    with pytest.raises(ValueError, match="origins"):
        ops.ray_cast(dev(tri), dev(one, np.int32), dev(o4[:2]), dev(d4))
    with pytest.raises(ValueError, match="t_min"):
        ops.ray_cast(dev(tri), dev(one, np.int32), dev(o), dev(down), t_min=-1.0)


def test_the_result_does_not_depend_on_the_launch_geometry():
    """icosphere(5), 20 480 faces.  3 rays: one workgroup of rays and 20 slabs of 1 024 records over blockIdx.y; the same
    rays inside the 1 850-ray image: 29 workgroups x 20 slabs, other lanes; inside 19 200 rays: 300 workgroups x 7 slabs
    of 2 928 records (the scenes of the other tests have one slab).  All three give the same bits, and the oracle's answer."""
    V, F = icosphere(5)
    V, F = np.ascontiguousarray(V, dtype=np.float32), np.asarray(F).astype(np.int32)
    cam = sc.scene("icosphere")[2]
    rays = sc.image_case("icosphere")["rays"]
    pick = np.array([18 * 50 + 25, 9 * 50 + 31, 0])          # the centre, a pixel up and to the right, a corner (background)
    mt = sc.moller_trumbore(V, F, np.asarray(cam).reshape(1, 3), rays[pick])
    assert sc.robust_rays(mt).all()
    to, fo, uo, vo = sc.first_hit(V, F, None, None, mt=mt)
    assert (fo[:2] >= 0).all() and fo[2] == -1
    t3, f3, b3 = cast(V, F, cam, rays[pick])
    assert np.array_equal(f3, fo) and np.isposinf(t3[2])
    nd = np.abs(mt["nd"][[0, 1], fo[:2]])
    assert (np.abs(t3[:2] - to[:2]) <= C_BOUND * EPS24 * to[:2] / nd).all()
    assert (np.abs(b3[:2] - np.stack([uo, vo], 1)[:2]) <= (C_BOUND * EPS24 * to[:2] / nd)[:, None]).all()
    tb, fb, bb = cast(V, F, cam, rays)
    assert t3.tobytes() == tb[pick].tobytes() and f3.tobytes() == fb[pick].tobytes() and b3.tobytes() == bb[pick].tobytes()
    big = np.tile(rays[pick], (6400, 1))
    tg, fg, bg = cast(V, F, cam, big)
    for k in range(3):
        assert (tg[k::3].view(np.int32) == t3[k:k + 1].view(np.int32)).all() and (fg[k::3] == f3[k]).all()
        assert (bg[k::3].view(np.int32) == b3[k].view(np.int32)).all()


def test_one_origin_gives_the_bits_of_the_broadcast_call():
    V, F, cam = sc.scene("torus")
    rays = sc.image_case("torus")["rays"]
    one = cast(V, F, np.asarray(cam).reshape(1, 3), rays)
    full = cast(V, F, np.tile(np.asarray(cam, dtype=np.float32).reshape(1, 3), (rays.shape[0], 1)), rays)
    for a, b in zip(one, full):
        assert a.tobytes() == b.tobytes()


def test_two_runs_and_a_replayed_graph_give_the_same_bits():
    V, F, cam = sc.scene("torus")
    Vd, Fd, od, dd = dev(V), dev(F, np.int32), dev(np.asarray(cam).reshape(1, 3)), dev(sc.image_case("torus")["rays"])
    first = [x.clone() for x in ops.ray_cast(Vd, Fd, od, dd, want_bary=True)]
    second = ops.ray_cast(Vd, Fd, od, dd, want_bary=True)
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ray_cast(Vd, Fd, od, dd, want_bary=True)          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.ray_cast(Vd, Fd, od, dd, want_bary=True)
    for x in out:
        x.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, out):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_scan_cli(tmp_path, capsys):
    from facet_graph_convolution_amd import scan
    V, F, cam = sc.scene("icosphere")
    clean, cut, img = tmp_path / "clean", tmp_path / "cut", tmp_path / "img"
    clean.mkdir()
    utils.write_mesh(V, F, str(clean / "ball.obj"), fmt="%.9g")
    camera = ",".join(str(c) for c in cam)
    written = scan.main([str(clean), str(cut), "--camera", camera])
    Vw, Fw, ids = utils.scan_cut(V, F, camera=cam)
    assert written == [str(cut / "ball.obj")] and "%d of 642 vertices" % Vw.shape[0] in capsys.readouterr().out
    Vc, _, _, Fc, _ = utils.load_mesh(str(cut), "ball.obj")
    assert np.array_equal(Vc, Vw) and np.array_equal(Fc.astype(np.int32), Fw)
    # a second run skips the file, --overwrite rewrites it
    stamp = os.stat(cut / "ball.obj").st_mtime_ns
    assert scan.main([str(clean), str(cut), "--camera", camera]) == [] and "Skipping ball.obj" in capsys.readouterr().out
    assert os.stat(cut / "ball.obj").st_mtime_ns == stamp
    (cut / "ball.obj").write_text("")
    assert scan.main([str(clean), str(cut), "--camera", camera, "--overwrite"]) == [str(cut / "ball.obj")]
    assert np.array_equal(utils.load_mesh(str(cut), "ball.obj")[0], Vw)
    # a view that sees nothing is reported and skipped (from inside the sphere every face is turned away)
    assert scan.main([str(clean), str(tmp_path / "none"), "--camera", "0,0,0.1"]) == []
    assert "Skipping ball.obj" in capsys.readouterr().out and not (tmp_path / "none" / "ball.obj").exists()
    # --image: the range mesh; its vertices give the pixel rays back
    assert scan.main([str(clean), str(img), "--camera", camera, "--image", "50,37"]) == [str(img / "ball.obj")]
    Vi, _, _, Fi, _ = utils.load_mesh(str(img), "ball.obj")
    depth, _, rays = utils.depth_image(V, F, cam, size=(50, 37), fov=40.0)
    Vr, Fr, pix = utils.range_mesh(depth, rays, cam, return_pixels=True)
    assert np.array_equal(Vi, Vr) and np.array_equal(Fi.astype(np.int32), Fr)
    assert np.abs(utils.view_rays(Vi, camera=cam) - rays.reshape(-1, 3)[pix]).max() <= 2.0 ** -23
    Vs, Fs = scan.scan_mesh(V, F, camera=cam, image=(50, 37))
    assert np.array_equal(Vs, Vr) and np.array_equal(Fs, Fr)
