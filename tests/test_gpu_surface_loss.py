"""GPU checks of the closest point without a tree (fgc_closest_point: bit for bit the tree's answer) and of the surface loss
(fgc_surface_loss: loss and gradient against the float64 oracle of tests/surface_loss_cases.py at the bounds written
there; masks, repeats, coincident vertices, bad indices; the same bits eager and replayed), of the point-set step bound with
gt_faces, and of the trainers with surface_loss=True.  Measured figures are printed before they are asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closest_cases as cc          # noqa: E402
import surface_loss_cases as sc     # noqa: E402
from facet_graph_convolution_amd import meshgen, ops          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _bits_equal(got, want):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _both(V, F, P):
    Vd, Fd, Pd = _t(V, torch.float32), _t(F, torch.int32), _t(P, torch.float32)
    brute = ops.closest_point(Vd, Fd, Pd, want_bary=True)
    tree = ops.closest_point_tree(ops.ray_tree(Vd, Fd), Pd, want_bary=True)
    torch.cuda.synchronize()
    return brute, tree


@pytest.mark.parametrize("name", cc.SCENES)
def test_closest_point_is_the_tree_bit_for_bit(name):
    V, F = cc.mesh(name)
    P, _ = cc.all_points(name)
    brute, tree = _both(V, F, P)
    _bits_equal(brute, tree)
    assert (brute[1] >= 0).all() and torch.isfinite(brute[0]).all()
    assert len(ops.closest_point(_t(V), _t(F), _t(P))) == 2


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 500])
def test_closest_point_point_counts(nq):
    V, F = cc.mesh("torus64")          # 4 096 faces: four slabs under few points
    P = cc.point_sets("torus64")["box"][:nq]
    brute, tree = _both(V, F, P)
    _bits_equal(brute, tree)
    assert brute[0].shape == (nq,) and brute[2].shape == (nq, 2) and (brute[1] >= 0).all()


def test_closest_point_skips_bad_rows():
    V, F = cc.mesh("icosphere")
    F = F.copy()
    dead = np.array([0, 1, 2, 3, 4, 5, 640, 1277, 1279])
    F[dead[:-2]] = -1
    F[1277, 1] = V.shape[0]          # an id >= nv
    F[1279, 2] = -7
    P = cc.point_sets("icosphere")["centroids"]
    brute, tree = _both(V, F, P)
    _bits_equal(brute, tree)
    face = brute[1].cpu().numpy()
    assert not np.isin(face, dead).any() and (face >= 0).all()
    alive = np.setdiff1d(np.arange(F.shape[0]), dead)
    assert (face[alive] == alive).mean() > 0.99          # a centroid's face is its own
    # no face takes part at all: (+inf, -1, (0, 0))
    none = ops.closest_point(_t(V), _t(np.full((5, 3), -1), torch.int32), _t(P[:70]), want_bary=True)
    assert torch.isinf(none[0]).all() and (none[1] == -1).all() and (none[2] == 0).all()


def _run(c, i0, i1, threshold=sc.THRESHOLD, want_grad=True):
    loss, g = ops.surface_loss(_t(c["V0"]), _t(c["F0"]), _t(c["V1"]), _t(c["F1"]), _t(i0, torch.int32), _t(i1, torch.int32),
                               float(threshold), want_grad)
    torch.cuda.synchronize()
    return loss.item(), None if g is None else g.cpu().numpy()


def _hold(tag, c, ref, loss, g):
    k = sc.grad_figure(c, ref, g)
    err = abs(loss - float(ref["loss"]))
    print("%s: loss %.6g (oracle %.6g, err %.2e of %.2e), gradient K %.3f (GPU_K %.2f)"
          % (tag, loss, ref["loss"], err, sc.loss_bound(c, ref), k, sc.GPU_K))
    assert err <= sc.loss_bound(c, ref)
    assert k <= sc.GPU_K
    untouched = ref["terms"] == 0
    assert untouched.any() and not g[untouched].any() and np.isfinite(g).all()


@pytest.mark.parametrize("name", sc.CASES)
def test_surface_loss_meets_the_oracle(name):
    c = sc.case(name)
    loss, g = _run(c, c["i0"], c["i1"])
    _hold(name, c, c["ref"], loss, g)
    # repeats and a row shared by precision and completeness terms are in every case (the CPU test asserts it); the loss
    # alone is the same number
    assert _run(c, c["i0"], c["i1"], want_grad=False) == (loss, None)
    # -1 rows in the refined mesh's table (a node-ordered table) change nothing
    F0 = np.concatenate([np.full((3, 3), -1, np.int32), c["F0"], np.full((2, 3), -1, np.int32)])
    loss_p, g_p = ops.surface_loss(_t(c["V0"]), _t(F0), _t(c["V1"]), _t(c["F1"]), _t(c["i0"], torch.int32),
                                   _t(c["i1"], torch.int32), sc.THRESHOLD)
    assert loss_p.item() == loss and np.array_equal(g_p.cpu().numpy(), g)


@pytest.mark.parametrize("name", ["same", "torus"])
def test_surface_loss_masked(name):
    c = sc.case(name)
    thr, i0, i1, ref = sc.masked(name)
    kept = np.concatenate([ref["prec"]["dist"], ref["comp"]["dist"]]) <= thr
    assert 0.35 < kept.mean() < 0.65, kept.mean()
    loss, g = _run(c, i0, i1, thr)
    _hold("%s masked at %.4g" % (name, thr), c, ref, loss, g)
    assert loss < _run(c, i0, i1)[0]


def test_a_surface_holds_its_vertices():
    """Same samples, same topology, no mask: the distance to a surface is at most the distance to its nearest vertex."""
    c = sc.case("same")
    loss, _ = _run(c, c["i0"], c["i1"])
    point, _ = ops.point_loss(_t(c["V0"]), _t(c["V1"]), _t(c["i0"], torch.int32), _t(c["i1"], torch.int32), sc.THRESHOLD)
    print("surface loss %.6g, point loss %.6g" % (loss, point.item()))
    assert loss <= point.item() + sc.loss_bound(c, c["ref"])


def test_coincident_vertices_and_bad_indices():
    c = sc.case("same")
    V0 = c["V0"].copy()
    j = int(c["F0"][10, 1])
    V0[j] = c["V1"][j]          # bit-equal on both sides
    d = dict(c, V0=V0)
    one = np.array([j], np.int32)
    loss, g = _run(d, one, one)
    assert loss == 0.0 and np.isfinite(g).all() and not g.any()
    # among other samples: exactly what the oracle says of it, a term of 0
    i0, i1 = np.append(c["i0"][:63], j).astype(np.int32), np.append(c["i1"][:63], j).astype(np.int32)
    ref = sc.surface_loss(V0, c["F0"], c["V1"], c["F1"], i0, i1)
    assert ref["prec"]["dist"][-1] == 0 and ref["comp"]["dist"][-1] == 0
    loss, g = _run(d, i0, i1)
    assert abs(loss - float(ref["loss"])) <= sc.loss_bound(c, ref) and np.isfinite(g).all()
    # an index out of range on either side: a NaN loss, no gradient from that sample
    for side in (0, 1):
        for bad in (-1, c["V0"].shape[0] if side == 0 else c["V1"].shape[0]):
            ind = [c["i0"][:64].copy(), c["i1"][:64].copy()]
            ind[side][5] = bad
            loss, g = _run(c, ind[0], ind[1])
            assert np.isnan(loss) and np.isfinite(g).all(), (side, bad)


def test_surface_loss_same_bits_eager_and_replayed():
    c = sc.case("denser")          # several slabs: the atomic minimum is exact whatever the order
    args = (_t(c["V0"]), _t(c["F0"]), _t(c["V1"]), _t(c["F1"]), _t(c["i0"], torch.int32), _t(c["i1"], torch.int32), sc.THRESHOLD)
    first = ops.surface_loss(*args)
    second = ops.surface_loss(*args)
    torch.cuda.synchronize()
    _bits_equal(first, second)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.surface_loss(*args)          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.surface_loss(*args)
    for x in out:
        x.fill_(7)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    _bits_equal(first, out)


def _bound_net(z, with_faces=True):
    from facet_graph_convolution_amd.net import FacetDenoiser
    V2, F2 = meshgen.icosphere(2)
    gt3 = z["gt_verts"].astype(np.float64)
    centre = gt3.mean(0)
    gt2 = (centre + np.linalg.norm(gt3 - centre, axis=1).mean() * V2.astype(np.float64)).astype(np.float32)
    net = FacetDenoiser(DEV, multi_scale=True, seed=0)
    net.bind_vertices(0, z["x"], [z["adj%d" % k].astype(np.int32) for k in range(3)], z["verts"], z["faces"],
                      z["v_faces"].astype(np.int32), gt2, gt_faces=F2.astype(np.int32) if with_faces else None)
    rs = np.random.RandomState(21)
    net.set_point_samples(z["sample_ind0"], rs.randint(gt2.shape[0], size=z["sample_ind1"].shape[0]))
    net.set_rotation(z["R"])
    return net, F2


def test_pointset_step_bound_with_gt_faces(golden_dir):
    z = np.load(os.path.join(golden_dir, "points_ico3.npz"))
    net, F2 = _bound_net(z)
    loss = net.pointset_forward_backward(rotate=True).clone()
    torch.cuda.synchronize()
    V = net._mesh["verts"]
    nv = z["verts"].shape[0]
    refined = V["traj"][-3 * nv:].reshape(nv, 3)
    want_loss, want_g = ops.surface_loss(refined, V["faces"], V["gtr"], _t(F2, torch.int32), V["i0"], V["i1"], V["threshold"])
    torch.cuda.synchronize()
    _bits_equal((loss, V["g_p"]), (want_loss, want_g))
    assert torch.isfinite(loss).all() and loss.item() > 0 and V["g_p"].abs().max().item() > 0
    grads = net.params.grad.clone()
    assert torch.isfinite(grads).all() and grads.abs().max().item() > 0
    # the loss alone, and the step replayed from a hipGraph
    _bits_equal((net.pointset_loss(rotate=True),), (loss,))
    for _ in range(2):
        got = net.pointset_forward_backward(rotate=True, capture=True)
        torch.cuda.synchronize()
        _bits_equal((got, net.params.grad), (loss, grads))
    # the same mesh bound without the faces measures to vertices: another number; a key keeps what it was bound with
    plain, _ = _bound_net(z, with_faces=False)
    other = plain.pointset_forward_backward(rotate=True)
    print("step loss to surfaces %.6g, to vertices %.6g" % (loss.item(), other.item()))
    assert other.item() > loss.item()
    with pytest.raises(ValueError, match="ground-truth faces"):
        net.bind_vertices(0, z["x"], [z["adj%d" % k].astype(np.int32) for k in range(3)], z["verts"], z["faces"],
                          z["v_faces"].astype(np.int32), z["gt_verts"])
    with pytest.raises(ValueError, match="gt_faces"):
        net.bind_vertices(1, z["x"], [z["adj%d" % k].astype(np.int32) for k in range(3)], z["verts"], z["faces"],
                          z["v_faces"].astype(np.int32), z["gt_verts"], gt_faces=np.zeros((4, 2), np.int32))


def _weights_moved(net):
    from facet_graph_convolution_amd.net import FacetDenoiser
    fresh = FacetDenoiser(DEV, multi_scale=True, seed=0)
    return not torch.equal(fresh.params.theta, net.params.theta)


def test_trainers_run_on_the_surface_loss():
    from facet_graph_convolution_amd import train as T
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    V, F = meshgen.icosphere(2)
    Vg, Fg = meshgen.icosphere(1)
    ds = TrainingSet()
    for s in (1, 2):
        ds.addMeshWithVerticesAndGTMesh(meshgen.add_noise(V, F.astype(np.int64), seed=s), F, Vg, Fg, seed=s)
    logs = []
    net, _, hist = T.trainAccuracyNet(ds, 3, seed=0, log=logs.append, validSet=ds, surface_loss=True)
    assert hist.shape == (3,) and np.isfinite(hist).all() and (hist > 0).all() and _weights_moved(net)
    assert sum("surfaceLoss" in s for s in logs) == 1
    # the same set without the option: fullLoss on ground-truth vertices of another count
    logs = []
    _, _, hist_p = T.trainAccuracyNet(ds, 3, seed=0, log=logs.append)
    assert np.isfinite(hist_p).all() and sum("fullLoss" in s for s in logs) == 1 and hist_p[0] > hist[0]
    clean = TrainingSet()
    clean.addCleanMeshWithVertices(V, F, seed=1)
    net, _, hist = T.trainAccuracyNet(clean, 3, seed=0, log=lambda s: None, validSet=clean, noise_levels=(0.2,),
                                      surface_loss=True)
    assert hist.shape == (3,) and np.isfinite(hist).all() and (hist > 0).all() and _weights_moved(net)
    _, _, hist_d = T.trainDoubleLossNet(clean, 3, seed=0, log=lambda s: None, noise_levels=(0.2,), surface_loss=True)
    assert hist_d.shape == (3, 3) and np.isfinite(hist_d).all()
