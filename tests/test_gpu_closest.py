"""GPU checks of the closest-point query through the bounding-box tree: fgc_closest_point_tree (ops.closest_point_tree),
utils.closest_points / surface_distances and the two surface options of computeMetrics, on the scenes, the point sets and
the float64 oracle of tests/closest_cases.py.

What is asserted.  With the unit 2^-24 (max|q| + max|V|) of a scene and point set, and TOL = 16 units (closest_cases.py:
15 x what the float32 restatement of the definition costs, test_closest_cpu.py):
  dist is within TOL of the oracle's;
  the float64 distance to the RETURNED face exceeds the oracle's minimum by at most TOL - face indices are never compared
  with the oracle's, a point above a shared edge has two right answers;
  (u, v) lies in the triangle and the point rebuilt from it is as far from q as dist says, within TOL;
  a call without FGC_CP_EXHAUSTIVE returns the bits of the call with it, on every point of every scene - and with that a
  point's result does not depend on its neighbours, the order of the points or of the records, eager or replayed.
No case is left out of any test."""
import os
import sys

import numpy as np
import pytest
import torch

from facet_graph_convolution_amd import computeMetrics, meshgen, ops, utils

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closest_cases as cc  # noqa: E402
import scan_tree_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = cc.TOL_UNITS


def dev(a, dt=np.float32):
    return torch.from_numpy(np.array(a, dtype=dt, order="C")).cuda()


def host(out):
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def tree_of(V, F, order=None):
    return ops.ray_tree(dev(V), dev(F, np.int32), None if order is None else dev(order, np.int32))


def query(tree, P, **kw):
    return host(ops.closest_point_tree(tree, dev(P), want_bary=True, **kw))


def same_bits(a, b, rows=slice(None)):
    return all(np.array_equal(np.ascontiguousarray(x[rows]).view(np.int32), np.ascontiguousarray(y[rows]).view(np.int32))
               for x, y in zip(a, b))


def against_oracle(V, F, P, got, ref, what=""):
    """The assertions of the module docstring on one point set; prints each figure before it asserts."""
    dist, face, bary = got
    u = cc.unit(V, P)
    assert ((face >= 0) & (face < F.shape[0])).all()
    err = np.abs(dist.astype(np.float64) - ref["dist"]).max() / u
    excess = (cc.dist_to_face(V, F, P, face) - ref["dist"]).max() / u
    p = cc.rebuilt(V, F, face, bary[:, 0], bary[:, 1])
    back = np.abs(np.linalg.norm(p - P.astype(np.float64), axis=1) - dist).max() / u
    print("%s: %d points, |dist - oracle| %.2f units, face excess %.2f units, |rebuilt - q| against dist %.2f units, "
          "u + v - 1 at most %.1e" % (what, P.shape[0], err, excess, back, (bary.sum(1) - 1).max()))
    assert err <= TOL and excess <= TOL and back <= TOL
    assert (bary >= 0).all() and (bary.sum(1) <= 1 + 2.0 ** -22).all()


@pytest.mark.parametrize("name", cc.SMALL)
def test_every_scene_and_point_set_against_the_oracle(name):
    V, F = cc.mesh(name)
    P, where = cc.all_points(name)
    ref = cc.oracle(name)
    got = query(tree_of(V, F), P)
    for key, rows in where.items():
        against_oracle(V, F, P[rows], tuple(x[rows] for x in got), {k: x[rows] for k, x in ref.items()}, "%s %s" % (name, key))
    assert not got[0][where["verts"]].any()          # dist == 0 on the vertices


@pytest.mark.parametrize("name", cc.SCENES)
def test_the_tree_returns_the_bits_of_the_exhaustive_search(name):
    """THE invariant, on every point of every scene; icosphere5 is a tree of depth 5 with ragged upper levels."""
    V, F = cc.mesh(name)
    P = cc.all_points(name)[0]
    tree = tree_of(V, F)
    got, full = query(tree, P), query(tree, P, exhaustive=True)
    differ = (got[0].view(np.int32) != full[0].view(np.int32)) | (got[1] != full[1])
    print("%s: %d points x %d faces, %d differ from the exhaustive search" % (name, P.shape[0], F.shape[0], differ.sum()))
    assert same_bits(got, full)
    assert same_bits(query(tree, P, exhaustive=True, sort_points=False), full)


def _icosphere_points():
    s = cc.point_sets("icosphere")
    return np.concatenate([s["box"], s["noisy"], s["verts"]])[:1850]


@pytest.mark.parametrize("k", tc.PREFIXES)
def test_tree_shapes(k):
    """The first k faces: one leaf (1, 3, 4), one node (5 .. 32), a node plus one leaf (33), ragged last nodes."""
    V, F = cc.mesh("icosphere")
    F, P = F[:k], _icosphere_points()
    tree = tree_of(V, F)
    got = query(tree, P)
    assert same_bits(got, query(tree, P, exhaustive=True))
    against_oracle(V, F, P, got, cc.closest(V, F, P), "first %d faces" % k)


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 1850])
@pytest.mark.parametrize("name", ["icosphere", "torus64"])
def test_point_counts(name, nq):
    """A last wave that is partly dead, one wave, one lane."""
    V, F = cc.mesh(name)
    sets = cc.point_sets(name)
    P = np.concatenate([sets["box"], sets["noisy"], sets["verts"]])[:1850][:nq]
    tree = tree_of(V, F)
    got = query(tree, P)
    assert got[0].shape == (nq,) and same_bits(got, query(tree, P, exhaustive=True))
    against_oracle(V, F, P, got, cc.closest(V, F, P), "%s, %d points" % (name, nq))


@pytest.mark.parametrize("name", ["torus64", "cube"])
def test_a_point_does_not_depend_on_its_neighbours(name):
    """A subset of the points, in reverse order, with and without sort_points, gives the bits of the full call."""
    V, F = cc.mesh(name)
    P = cc.all_points(name)[0]
    tree = tree_of(V, F)
    base = query(tree, P, sort_points=False)
    assert same_bits(query(tree, P, sort_points=True), base)
    pick = np.random.RandomState(5).choice(P.shape[0], P.shape[0] // 3, replace=False)[::-1]
    for rows in (pick, np.arange(P.shape[0])[::-1], np.arange(37), np.arange(64), np.array([P.shape[0] - 1])):
        for sort_points in (False, True):
            assert same_bits(query(tree, P[rows], sort_points=sort_points), tuple(x[rows] for x in base))


@pytest.mark.parametrize("name", ["icosphere", "cube", "torus64"])
def test_any_order_of_the_records_gives_the_same_bits(name):
    """Identity, a seeded random permutation and the reversed Morton order against the default (Morton) order."""
    V, F = cc.mesh(name)
    P = cc.all_points(name)[0]
    nf = F.shape[0]
    base = query(tree_of(V, F), P)
    morton = ops.ray_tree_order(torch.from_numpy(V.copy()), torch.from_numpy(F.copy())).numpy()
    for order in (np.arange(nf), np.random.RandomState(3).permutation(nf), morton[::-1]):
        assert same_bits(query(tree_of(V, F, np.ascontiguousarray(order)), P), base)


def test_ties_go_to_the_lower_face_index():
    """cube(4): its coordinates and the points above its diagonals are dyadic, every product of the pair function is exact
    in fp32, so the two faces along a diagonal give the SAME dist2 and the key decides.  And every face duplicated: the
    copy, at index nf + f, never wins against f."""
    V, F = meshgen.cube(4)
    V, F = np.asarray(V, dtype=np.float32), np.asarray(F).astype(np.int32)
    nf = F.shape[0]
    P = cc.cube_diagonal_points(V, F, height=0.125)
    ref = cc.closest(V, F, P)
    a, e1, e2 = cc.records(V, F, np.float64)
    d2 = cc.pair(P[:, None].astype(np.float64), a[None], e1[None], e2[None])[0]
    assert ((d2 == d2.min(1, keepdims=True)).sum(1) == 2).all() and np.array_equal(d2.argmin(1), ref["face"])
    for order in (None, np.arange(nf)[::-1].copy(), np.random.RandomState(9).permutation(nf)):
        tree = tree_of(V, F, order)
        for kw in ({}, {"exhaustive": True}):
            dist, face, bary = query(tree, P, **kw)
            assert np.array_equal(face, ref["face"]) and np.array_equal(dist, np.full(P.shape[0], 0.125, dtype=np.float32))
    Q = np.concatenate([P, cc.point_sets("cube")["box"], V])
    one = query(tree_of(V, F), Q)
    F2 = np.concatenate([F, F])
    for order in (None, np.arange(2 * nf)[::-1].copy()):
        two = query(tree_of(V, F2, order), Q)
        assert same_bits(two, one) and (two[1] < nf).all()


def test_bad_input_never_wins():
    V, F = cc.mesh("torus")
    V, F = V.copy(), F.copy()
    P = cc.all_points("torus")[0]
    nf = F.shape[0]
    F[5] = [0, 1, V.shape[0]]          # an id out of range
    F[77] = [-1, 2, 3]
    F[100] = [7, 7, 7]                 # a face collapsed to a point
    V = np.concatenate([V, np.float32([[np.nan, 0, 0], [np.inf, 0, 0]])])
    F[200] = [0, 1, V.shape[0] - 2]    # a NaN vertex
    F[300] = [V.shape[0] - 1, 4, 5]    # an infinite one
    bad = [5, 77, 100, 200, 300]
    Pb = np.concatenate([P, V[[7]], np.float32([[np.nan, 0, 0]])])          # vertex 7 itself, and a NaN point
    tree = tree_of(V, F)
    got, full = query(tree, Pb), query(tree, Pb, exhaustive=True)
    assert same_bits(got, full)
    assert not np.isin(got[1], bad).any()
    assert got[1][-1] == -1 and np.isposinf(got[0][-1]) and not got[2][-1].any()          # the NaN point finds nothing
    keep = np.ones(nf, dtype=bool)
    keep[bad] = False
    ids = np.flatnonzero(keep)
    ref = cc.closest(V[:-2], F[keep], P)
    dist, face, bary = (x[:-2] for x in got)
    assert keep[face].all()
    against_oracle(V[:-2], F[keep], P, (dist, np.searchsorted(ids, face).astype(np.int32), bary), ref, "torus, five bad rows")
    # a mesh of only such rows
    only = tree_of(V, F[bad])
    for kw in ({}, {"exhaustive": True}, {"sort_points": False}):
        dist, face, bary = query(only, Pb, **kw)
        assert np.isposinf(dist).all() and (face == -1).all() and not bary.any()


def test_two_runs_and_a_replayed_graph_give_the_same_bits():
    V, F = cc.mesh("torus64")
    tree = tree_of(V, F)
    pd = dev(cc.all_points("torus64")[0])
    first = [x.clone() for x in ops.closest_point_tree(tree, pd, want_bary=True, sort_points=False)]
    second = ops.closest_point_tree(tree, pd, want_bary=True, sort_points=False)
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.closest_point_tree(tree, pd, want_bary=True, sort_points=False)          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):          # one linear capture: the launch of the query and the square root
        out = ops.closest_point_tree(tree, pd, want_bary=True, sort_points=False)
    for x in out:
        x.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, out):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _oracle_surface(V0, GT, F, shift, both):
    """surface_distances restated on the oracle: the float32 translation utils makes, distances in float64 over all pairs,
    divided by the diagonal of V0 u GT; and the bound of each value: TOL units of the translated coordinates over the
    diagonal (a mean or a root mean square of errors is no larger than their maximum), the float32 rounding of the value
    and half a unit of the CSV's seventh decimal."""
    lo, hi = np.minimum(V0.min(0), GT.min(0)), np.maximum(V0.max(0), GT.max(0))
    diag = float(np.linalg.norm(hi.astype(np.float64) - lo.astype(np.float64)))
    A, B = (V0 - shift).astype(np.float32), (GT - shift).astype(np.float32)
    ev = cc.closest(B, F, A)["dist"] / diag
    want = [ev.max(), ev.mean(), np.sqrt((ev * ev).mean())] + [np.nan] * 3
    if both:
        comp = cc.closest(A, F, B)["dist"] / diag
        want[3:] = [comp.max(), comp.mean(), max(ev.max(), comp.max())]
    tol = TOL * cc.unit(B, A) / diag
    return np.array(want), [tol + 2.0 ** -24 * abs(w) + 5e-8 for w in want]


def _read_csv(path):
    rows = {}
    for line in open(path):
        w = line.split()
        rows[w[0]] = np.array([float(x) for x in w[1:]])
    return rows


def test_surface_distances_and_compute_metrics(tmp_path):
    gt_dir, res_dir, cut_dir = (tmp_path / n for n in ("gt", "res", "cut"))
    for d in (gt_dir, res_dir, cut_dir):
        d.mkdir()
    V, F = cc.mesh("icosphere")
    utils.write_mesh(V, F, str(gt_dir / "ball.obj"))
    for k in (1, 2, 3):
        utils.write_mesh(meshgen.add_noise(V, F.astype(np.int64), 0.1 * k, seed=k), F, str(res_dir / ("ball_n%d_denoised.obj" % k)))
    GT = utils.load_mesh(str(gt_dir), "ball.obj")[0]
    noisy = {k: utils.load_mesh(str(res_dir), "ball_n%d_denoised.obj" % k)[0] for k in (1, 2, 3)}
    Fi = F.astype(np.int64)

    # utils.surface_distances on its own: the corner of V0 u V1, with and without F0
    for both in (True, False):
        V0 = noisy[2]
        got = utils.surface_distances(V0, GT, Fi, F0=Fi if both else None)
        assert list(got) == list(computeMetrics.SURFACE_KEYS) and all(v.dtype == np.float32 for v in got.values())
        want, tol = _oracle_surface(V0, GT, Fi, np.minimum(V0.min(0), GT.min(0)).astype(np.float32)[None], both)
        for key, w, t in zip(got, want, tol):
            print("surface_distances %s: %.9f, oracle %.9f, bound %.2e" % (key, got[key], w, t))
            assert (np.isnan(w) and np.isnan(got[key])) or abs(float(got[key]) - w) <= t, key
    # closest_points: the rebuilt point lies where dist says, a shared handle gives the same answer
    handle = utils.ray_tree(GT, Fi)
    dist, face, point = utils.closest_points(noisy[1], GT, Fi, accel=handle)
    again = utils.closest_points(noisy[1], GT, Fi)
    assert np.array_equal(dist, again[0]) and np.array_equal(face, again[1]) and np.array_equal(point, again[2])
    assert point.dtype == np.float64 and dist.dtype == np.float32 and face.dtype == np.int32
    assert np.abs(np.linalg.norm(point - noisy[1], axis=1) - dist).max() <= TOL * cc.unit(GT, noisy[1])

    # a default run writes no results_surface.csv
    computeMetrics.main([str(gt_dir), str(res_dir)])
    assert not (res_dir / "results_surface.csv").exists() and (res_dir / "results_exact.csv").exists()
    # --surface: one line per scored file, both directions
    computeMetrics.main([str(gt_dir), str(res_dir), "--surface", "--overwrite"])
    rows = _read_csv(str(res_dir / "results_surface.csv"))
    assert sorted(rows) == ["ball_n%d_denoised.obj" % k for k in (1, 2, 3)]
    shift = GT.min(0).astype(np.float32)[None]          # the ground truth's own corner: its tree is shared
    for k in (1, 2, 3):
        want, tol = _oracle_surface(noisy[k], GT, Fi, shift, True)
        got = rows["ball_n%d_denoised.obj" % k]
        print("--surface n%d: %s, oracle %s" % (k, got, want))
        assert got.shape == (6,) and (np.abs(got - want) <= tol).all(), k
        assert got[0] >= got[2] >= got[1] > 0 and got[5] == max(got[0], got[3])

    # --surface-only: a cut scan of the noisy mesh, another vertex count, against the whole ground truth
    Vc, Fc, _ = utils.scan_cut(noisy[1], Fi, camera=(0.3, -0.2, 3.0))
    assert 0 < Vc.shape[0] < GT.shape[0]
    utils.write_mesh(Vc, Fc, str(cut_dir / "ball_n1_denoised.obj"))
    Vc = utils.load_mesh(str(cut_dir), "ball_n1_denoised.obj")[0]
    with pytest.raises(ValueError, match="vertices"):
        computeMetrics.main([str(gt_dir), str(cut_dir)])
    computeMetrics.main([str(gt_dir), str(cut_dir), "--surface-only"])
    assert sorted(os.listdir(str(cut_dir))) == ["ball_n1_denoised.obj", "results_surface.csv"]
    text = (cut_dir / "results_surface.csv").read_text()
    got = _read_csv(str(cut_dir / "results_surface.csv"))["ball_n1_denoised.obj"]
    want, tol = _oracle_surface(Vc, GT, Fi, shift, False)
    print("--surface-only: %s, oracle %s" % (got, want))
    assert (np.abs(got[:3] - want[:3]) <= tol[:3]).all() and np.isnan(got[3:]).all()
    computeMetrics.main([str(gt_dir), str(cut_dir), "--surface-only"])          # the name has its line: skipped
    assert (cut_dir / "results_surface.csv").read_text() == text
    computeMetrics.main([str(gt_dir), str(cut_dir), "--surface-only", "--overwrite"])
    assert (cut_dir / "results_surface.csv").read_text() == text + text
