"""GPU checks of the ray cast through a bounding-box tree: fgc_ray_tree_build / fgc_ray_cast_tree (ops.ray_tree,
ops.ray_cast_tree) and accel= of the host functions, against ops.ray_cast and the float64 oracle on the scenes of
tests/scan_tree_cases.py.

What is asserted.  The tree runs the function of the brute-force kernel on a subset of the pairs, so
  on EVERY ray its (t, face) is never smaller in key order than ops.ray_cast's (a miss is the largest key);
  on ROBUST rays (scan_cases.robust_rays, in float64) t, face, u, v equal ops.ray_cast's bit for bit and the face is the
  oracle's;
and every test asserts that it skipped at most scan_cases.CAP = 2 % of its cases.  fp32 Moeller-Trumbore is not watertight:
on a grazed triangle it can report a hit although the exact ray misses the triangle's box, and the tree may cull that."""
import os
import sys

import numpy as np
import pytest
import torch

from facet_graph_convolution_amd import ops, utils

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_cases as sc  # noqa: E402
import scan_tree_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a, dt=np.float32):
    return torch.from_numpy(np.array(a, dtype=dt, order="C")).cuda()


def host(out):
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def brute(V, F, origins, rays, t_min=0.0):
    return host(ops.ray_cast(dev(V), dev(F, np.int32), dev(origins), dev(rays), t_min, want_bary=True))


def through_tree(V, F, origins, rays, t_min=0.0, order=None, sort_rays=True):
    tree = ops.ray_tree(dev(V), dev(F, np.int32), None if order is None else dev(order, np.int32))
    return host(ops.ray_cast_tree(tree, dev(origins), dev(rays), t_min, want_bary=True, sort_rays=sort_rays))


def same_bits(a, b, rows=slice(None)):
    return all(np.array_equal(np.ascontiguousarray(x[rows]).view(np.int32), np.ascontiguousarray(y[rows]).view(np.int32))
               for x, y in zip(a, b))


def check(got, want, robust, nf, oracle_face=None):
    """The two assertions, the cap, and sane outputs on every ray."""
    (t, f, b), (tb, fb, bb) = got, want
    assert (~robust).sum() <= sc.CAP * robust.size
    big = np.int64(2) ** 31
    key = lambda t, f: (t, np.where(f < 0, big, f.astype(np.int64)))  # noqa: E731
    (kt, kf), (bt, bf) = key(t, f), key(tb, fb)
    assert ((kt > bt) | ((kt == bt) & (kf >= bf))).all()
    assert same_bits((t, f, b), (tb, fb, bb), robust)
    if oracle_face is not None:
        assert np.array_equal(f[robust], oracle_face[robust])
    assert ((f >= -1) & (f < nf)).all() and (b >= 0).all() and (b.sum(1) <= 1).all()
    assert np.array_equal(np.isposinf(t), f < 0) and not b[f < 0].any() and (t > 0).all()


@pytest.mark.parametrize("kind,name", tc.CASES)
def test_every_scene(kind, name):
    """Pixel rays of one camera (the cube has flat boxes), 5 120 faces under a tree of five levels, and parallel rays with
    per-ray origins and one or two zero direction components (1 / d is an infinity there)."""
    c = tc.case(kind, name)
    got = through_tree(c["V"], c["F"], c["origins"], c["rays"])
    want = brute(c["V"], c["F"], c["origins"], c["rays"])
    print("%s %s: %d rays, %d skipped, %d differ from the brute-force cast (all among the skipped)"
          % (kind, name, c["robust"].size, (~c["robust"]).sum(), (got[1] != want[1]).sum()))
    check(got, want, c["robust"], c["F"].shape[0], c["face"])
    assert (got[1] >= 0).sum() > 0.1 * got[1].size


@pytest.mark.parametrize("k", tc.PREFIXES)
def test_tree_shapes(k):
    """The first k faces: one leaf (1, 3, 4), one node (5 .. 32), a node plus one leaf (33), ragged last nodes."""
    c = tc.prefix_case(k)
    got = through_tree(c["V"], c["F"], c["origins"], c["rays"])
    check(got, brute(c["V"], c["F"], c["origins"], c["rays"]), c["robust"], k, c["face"])
    assert (got[1] >= 0).any() == (c["face"] >= 0).any()


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 1850])
@pytest.mark.parametrize("name", ["icosphere", "torus64"])
def test_ray_counts(name, nq):
    """The FIRST nq robust rays of an image (all 1 850 rays for the last count): below 1 850 nothing is skipped, everything
    equals the brute-force cast."""
    c = tc.case("image", name)
    rays = c["rays"][np.flatnonzero(c["robust"])[:nq]] if nq < 1850 else c["rays"]
    robust = np.ones(nq, dtype=bool) if nq < 1850 else c["robust"]
    assert rays.shape[0] == nq
    got = through_tree(c["V"], c["F"], c["origins"], rays)
    check(got, brute(c["V"], c["F"], c["origins"], rays), robust, c["F"].shape[0])


@pytest.mark.parametrize("kind,name", [("image", "torus64"), ("tilt", "icosphere")])
def test_a_ray_does_not_depend_on_its_neighbours(kind, name):
    """On ALL rays, bit for bit: sorted or not, reversed, a prefix of a longer call, and (one origin) the origin broadcast."""
    c = tc.case(kind, name)
    V, F, o, rays = c["V"], c["F"], c["origins"], c["rays"]
    nq = rays.shape[0]
    tree = ops.ray_tree(dev(V), dev(F, np.int32))
    cast = lambda o, r, **kw: host(ops.ray_cast_tree(tree, dev(o), dev(r), want_bary=True, **kw))  # noqa: E731
    base = cast(o, rays, sort_rays=False)
    assert same_bits(cast(o, rays, sort_rays=True), base)
    rev = slice(None, None, -1)
    back = cast(o if o.shape[0] == 1 else o[rev], rays[rev], sort_rays=False)
    assert same_bits(tuple(x[rev] for x in back), base)
    for n in (1, 37, 64, 1000):          # other lanes are dead, other waves are gone
        assert same_bits(cast(o if o.shape[0] == 1 else o[:n], rays[:n], sort_rays=False), base, slice(0, n))
    if o.shape[0] == 1:
        assert same_bits(cast(np.tile(o, (nq, 1)), rays, sort_rays=False), base)
        assert same_bits(cast(np.tile(o, (nq, 1)), rays, sort_rays=True), base)


def test_two_runs_and_a_replayed_graph_give_the_same_bits():
    c = tc.case("image", "torus64")
    tree = ops.ray_tree(dev(c["V"]), dev(c["F"], np.int32))
    od, dd = dev(c["origins"]), dev(c["rays"])
    first = [x.clone() for x in ops.ray_cast_tree(tree, od, dd, want_bary=True, sort_rays=False)]
    second = ops.ray_cast_tree(tree, od, dd, want_bary=True, sort_rays=False)
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ray_cast_tree(tree, od, dd, want_bary=True, sort_rays=False)          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):          # one linear capture: the single launch of the cast
        out = ops.ray_cast_tree(tree, od, dd, want_bary=True, sort_rays=False)
    for x in out:
        x.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, out):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", ["icosphere4", "cube"])
def test_any_order_of_the_records_gives_the_same_bits(name):
    """Identity, reversed, a seeded random permutation and the default (Morton) order: correctness does not depend on it."""
    c = tc.case("image", name)
    V, F, o, rays, rb = c["V"], c["F"], c["origins"], c["rays"], c["robust"]
    nf = F.shape[0]
    want = brute(V, F, o, rays)
    orders = {"identity": np.arange(nf), "reversed": np.arange(nf)[::-1], "random": np.random.RandomState(11).permutation(nf),
              "default": None}
    for label, order in orders.items():
        got = through_tree(V, F, o, rays, order=order)
        print("%s %s: %d faces differ from the brute-force cast" % (name, label, (got[1] != want[1]).sum()))
        check(got, want, rb, nf, c["face"])


def test_ties_go_to_the_lower_index():
    """The mesh with 40 of its faces appended again at the end, under a random order of the records: exact ties, and the
    copy never wins."""
    c = tc.case("image", "icosphere4")
    V, F, o, rays, rb = c["V"], c["F"], c["origins"], c["rays"], c["robust"]
    seen = np.unique(c["face"][rb & (c["face"] >= 0)])
    twice = seen[:: max(1, seen.size // 40)][:40]          # faces the image sees
    F2 = np.concatenate([F, F[twice]])
    order = np.random.RandomState(5).permutation(F2.shape[0])
    got = through_tree(V, F2, o, rays, order=order)
    check(got, brute(V, F2, o, rays), rb, F2.shape[0], c["face"])
    assert np.isin(c["face"][rb], twice).sum() >= 40 and (got[1][rb] < F.shape[0]).all()
    # and the other way round: the copies first in the list, so THEY win
    F3 = np.concatenate([F[twice], F])
    got = through_tree(V, F3, o, rays, order=np.random.RandomState(6).permutation(F3.shape[0]))
    check(got, brute(V, F3, o, rays), rb, F3.shape[0])
    hit_twice = rb & np.isin(c["face"], twice)
    assert (got[1][hit_twice] < 40).all() and np.array_equal(twice[got[1][hit_twice]], c["face"][hit_twice])


def test_bad_faces_and_vertices():
    """Faces with an id out of range, a zero-area face and a vertex with a NaN (appended: the valid faces, on which
    robustness is decided, stay what they were) change nothing, in any order and in the default one."""
    c = tc.case("image", "torus64")
    V, F, o, rays, rb = c["V"], c["F"], c["origins"], c["rays"], c["robust"]
    nv = V.shape[0]
    V2 = np.concatenate([V, np.float32([[np.nan, 0.5, 0.5]])])
    bad = np.array([[0, 1, nv + 1], [-1, 2, 3], [2 ** 31 - 1, 5, 6], [7, 7, 8], [9, 9, 9], [10, 11, nv], [nv, 12, 13],
                    [nv, nv, nv]], dtype=np.int64)
    F2 = np.concatenate([bad[:4], F, bad[4:]]).astype(np.int32)
    want = brute(V2, F2, o, rays)
    assert np.array_equal(want[1][rb], np.where(c["face"][rb] >= 0, c["face"][rb] + 4, -1))
    for order in (None, np.random.RandomState(3).permutation(F2.shape[0]), np.arange(F2.shape[0])):
        got = through_tree(V2, F2, o, rays, order=order)
        check(got, want, rb, F2.shape[0])
    # an order with entries outside [0, nf): zero records, the rest of the tree is found as before
    order = np.arange(F2.shape[0])
    order[[0, 1, 2, 3]] = [-1, F2.shape[0], 2 ** 31 - 1, -2 ** 31]
    got = through_tree(V2, F2, o, rays, order=order)
    check(got, want, rb, F2.shape[0])
    # no valid face at all: every ray misses
    got = through_tree(V2, bad.astype(np.int32), o, rays)
    assert (got[1] == -1).all() and np.isposinf(got[0]).all() and not got[2].any()


@pytest.mark.parametrize("name", ["icosphere4", "torus64"])
def test_t_min_finds_the_second_hit(name):
    c = tc.case("image", name)
    V, F, o, rays, rb = c["V"], c["F"], c["origins"], c["rays"], c["robust"]
    first = brute(V, F, o, rays)
    tree = ops.ray_tree(dev(V), dev(F, np.int32))
    pick = np.flatnonzero(rb & (first[1] >= 0))[::16]          # t_min is one number per call: one call per picked ray
    second_hits = 0
    for q in pick:
        t_min = float(first[0][q])
        got = host(ops.ray_cast_tree(tree, dev(o), dev(rays[q:q + 1]), t_min, want_bary=True))
        want = brute(V, F, o, rays[q:q + 1], t_min)
        assert same_bits(got, want) and got[1][0] != first[1][q] and (got[1][0] < 0 or got[0][0] > t_min)
        second_hits += int(got[1][0] >= 0)
    assert pick.size >= 90 and second_hits > 0.9 * pick.size          # closed surfaces: what goes in comes out
    # and in one call, with the smallest first t of the image: rays whose first hit lies behind it keep it
    t_min = float(first[0][first[1] >= 0].min())
    got = host(ops.ray_cast_tree(tree, dev(o), dev(rays), t_min, want_bary=True))
    check(got, brute(V, F, o, rays, t_min), rb, F.shape[0])


@pytest.mark.parametrize("view", ["camera", "dir"])
@pytest.mark.parametrize("name", list(tc.BIG))
def test_visible_vertices_through_the_tree(name, view):
    V, F, _ = tc.mesh(name)
    want = tc.visibility_case(name, view)
    sure = want >= 0
    assert (~sure).sum() <= sc.CAP * want.size
    kw = tc.view_kwargs(name, view)
    vis = utils.visible_vertices(V, F, accel="tree", **kw)
    assert vis.dtype == bool and vis.shape == (V.shape[0],)
    assert np.array_equal(vis[sure], want[sure] == 1)
    assert np.array_equal(vis[sure], utils.visible_vertices(V, F, accel="none", **kw)[sure])
    assert np.array_equal(vis[sure], utils.visible_vertices(V, F, **kw)[sure])          # the default is "none"


@pytest.mark.parametrize("name", list(tc.BIG))
def test_depth_image_and_a_reused_handle(name):
    V, F, cam = tc.mesh(name)
    c = tc.case("image", name)
    rb = c["robust"].reshape(37, 50)
    assert (~rb).sum() <= sc.CAP * rb.size
    depth, face, rays = utils.depth_image(V, F, cam, size=sc.IMAGE, fov=sc.FOV, accel="tree")
    assert np.abs(rays.reshape(-1, 3) - c["rays"]).max() <= 2.0 ** -24
    if rays.reshape(-1, 3).tobytes() != c["rays"].tobytes():          # (utils.pixel_rays may differ from the oracle's by a rounding)
        rb = tc.oracle(V, F, np.asarray(cam).reshape(1, 3), rays.reshape(-1, 3))["robust"].reshape(37, 50) & rb
        assert (~rb).sum() <= sc.CAP * rb.size
    assert np.array_equal(face[rb], c["face"].reshape(37, 50)[rb])
    plain = utils.depth_image(V, F, cam, size=sc.IMAGE, fov=sc.FOV)
    assert np.array_equal(depth[rb].view(np.int32), plain[0][rb].view(np.int32)) and np.array_equal(face[rb], plain[1][rb])
    # one handle over two views gives what two fresh builds give
    handle = utils.ray_tree(V, F)
    assert (handle.nf, handle.nv) == (F.shape[0], V.shape[0])
    for view in ("camera", "dir"):
        kw = tc.view_kwargs(name, view)
        assert np.array_equal(utils.visible_vertices(V, F, accel=handle, **kw), utils.visible_vertices(V, F, accel="tree", **kw))
    again = utils.depth_image(V, F, cam, size=sc.IMAGE, fov=sc.FOV, accel=handle)
    assert again[0].tobytes() == depth.tobytes() and again[1].tobytes() == face.tobytes()
    with pytest.raises(ValueError, match="the tree was built of"):
        utils.visible_vertices(V, F[:-1], accel=handle, camera=cam)


def test_scan_cli_with_accel_tree(tmp_path, capsys):
    from facet_graph_convolution_amd import scan
    V, F, cam = tc.mesh("torus64")
    clean, cut, img = tmp_path / "clean", tmp_path / "cut", tmp_path / "img"
    clean.mkdir()
    utils.write_mesh(V, F, str(clean / "ring.obj"), fmt="%.9g")
    camera = ",".join(str(x) for x in cam)
    assert scan.main([str(clean), str(cut), "--camera", camera, "--accel", "tree"]) == [str(cut / "ring.obj")]
    Vw, Fw, ids = utils.scan_cut(V, F, camera=cam, accel="tree")
    assert "%d of %d vertices" % (Vw.shape[0], V.shape[0]) in capsys.readouterr().out
    Vc, _, _, Fc, _ = utils.load_mesh(str(cut), "ring.obj")
    assert np.array_equal(Vc, Vw) and np.array_equal(Fc.astype(np.int32), Fw) and 0 < Fw.shape[0] < F.shape[0]
    # the cut is the oracle's where no ambiguous vertex is involved
    cls = tc.visibility_case("torus64", "camera")
    _, _, _, keep = sc.cut(V, F, cls == 1, camera=cam)
    sure = (cls[F] >= 0).all(1)
    kept = set(map(tuple, ids[Fw].tolist()))
    mine = np.array([tuple(row) in kept for row in F.tolist()])
    assert np.array_equal(mine[sure], keep[sure])
    # --image, and scan_mesh
    assert scan.main([str(clean), str(img), "--camera", camera, "--image", "50,37", "--accel", "tree"]) == [str(img / "ring.obj")]
    Vi, _, _, Fi, _ = utils.load_mesh(str(img), "ring.obj")
    depth, _, rays = utils.depth_image(V, F, cam, size=(50, 37), fov=40.0, accel="tree")
    Vr, Fr = utils.range_mesh(depth, rays, cam)
    assert np.array_equal(Vi, Vr) and np.array_equal(Fi.astype(np.int32), Fr)
    Vs, Fs = scan.scan_mesh(V, F, camera=cam, image=(50, 37), accel="tree")
    assert np.array_equal(Vs, Vr) and np.array_equal(Fs, Fr)
    Vs, Fs = scan.scan_mesh(V, F, camera=cam, accel=utils.ray_tree(V, F))
    assert np.array_equal(Vs, Vw) and np.array_equal(Fs, Fw)
