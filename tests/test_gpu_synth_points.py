"""Training the vertex networks from clean meshes: fgc_point_sets_prepare (the two point sets of fullLoss normalised
together and rotated on the device) bit for bit against utils.normalizePointSets + rotate_rows and against its float64
definition, FacetDenoiser.bind_clean_vertices against a second network fed host-made inputs, and the trainers and
command lines on synthesised noise."""
import functools
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_cases as sc  # noqa: E402

from facet_graph_convolution_amd import ops, utils
from facet_graph_convolution_amd.dataClasses import TrainingSet
from facet_graph_convolution_amd.meshgen import icosphere, torus, flip_edges

pytestmark = pytest.mark.gpu

SEED = 1234
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _mesh(tag):
    if tag == "ico3":
        return icosphere(3)
    V, F = torus(24, 20)
    return V, flip_edges(F, 400, seed=1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _clean_set(tag):
    V, F = _mesh(tag)
    ds = TrainingSet()
    ds.addCleanMeshWithVertices(V, F, seed=0)
    return ds


def _rotation(seed=3):
    return utils.rand_rotation_matrix(randnums=np.random.RandomState(seed).uniform(size=3)).astype(np.float32)


# 262 145 = 1 024 x 256 + 1: the first size at which the noise launch's partial boxes are capped and a workgroup strides
SIZES = [(642, 642), (257, 1), (1, 300), (255, 256), (256, 255), (262145, 642)]


@pytest.mark.parametrize("nv,ngt", SIZES)
def test_point_sets_prepare_bit_for_bit_and_against_float64(nv, ngt):
    """Bound against float64 (divide by the double diagonal, rotate in double), per coordinate: 2^-20 max|q|, q the
    normalised coordinates - two roundings in front of the rotation (diagonal, division; the fp32 extents the diagonal is
    taken from add a third) and three inside it, each at most 2^-24 of a term bounded by |q| sum_j |R_ij| <= sqrt(3) |q|:
    6 sqrt(3) 2^-24 < 2^-20."""
    rs = np.random.RandomState(nv + 7 * ngt)
    # the union box is set by v along x and by gt along y; off-centre, so that min and max both matter
    v0 = (rs.uniform(-1, 1, (nv, 3)) * [3.0, 1.0, 0.5] + [0.3, -0.2, 0.1]).astype(np.float32)
    gt = (rs.uniform(-1, 1, (ngt, 3)) * [1.0, 3.0, 0.5] + [0.3, -0.2, 0.1]).astype(np.float32)
    Rm = _rotation()
    gt_d = torch.as_tensor(gt, device=DEV)
    scratch = torch.zeros(max(6 * min((nv + 255) // 256, 1024), 1), dtype=torch.float32, device=DEV)
    # the vertices the noise launch leaves, with its boxes in `scratch`
    vd = ops.synth_noise(torch.as_tensor(v0, device=DEV), 0.05, 3, seed=SEED, scratch=scratch)
    v = vd.cpu().numpy()
    assert not np.array_equal(v, v0)
    if nv > 1 and ngt > 1:
        lo_v, hi_v, lo_g, hi_g = v.min(0), v.max(0), gt.min(0), gt.max(0)
        assert lo_v[0] < lo_g[0] and hi_v[0] > hi_g[0] and lo_g[1] < lo_v[1] and hi_g[1] > hi_v[1]
    qv, qg = utils.normalizePointSets(v, gt)
    assert qv.dtype == np.float32 and qg.dtype == np.float32
    lo = np.minimum(v.min(0), gt.min(0)).astype(np.float64)
    hi = np.maximum(v.max(0), gt.max(0)).astype(np.float64)
    diag = np.sqrt(((hi - lo) ** 2).sum())
    assert diag > 0
    q64 = [v.astype(np.float64) / diag, gt.astype(np.float64) / diag]
    bound = 2.0 ** -20 * max(np.abs(q64[0]).max(), np.abs(q64[1]).max())
    worst = 0.0
    for R in (Rm, None):
        want = [torch.as_tensor(qv, device=DEV), torch.as_tensor(qg, device=DEV)]
        want64 = q64
        if R is not None:
            want = [ops.rotate_rows(w, R) for w in want]
            want64 = [q @ R.astype(np.float64).T for q in q64]
        for have_bbox in (True, False):
            got = ops.point_sets_prepare(vd, gt_d, R=R, scratch=scratch if have_bbox else None, have_bbox=have_bbox)
            torch.cuda.synchronize()
            for name, g, w, w64 in zip(("v", "gt"), got, want, want64):
                differ = int((g != w).sum().item())
                err = np.abs(g.cpu().numpy().astype(np.float64) - w64).max()
                worst = max(worst, err / bound)
                print("(%d, %d) R %s boxes %s %s: %d words differ, max err %.3e (bound %.3e)"
                      % (nv, ngt, "given" if R is not None else "NULL", "from the noise launch" if have_bbox else "computed",
                         name, differ, err, bound))
                assert g.shape == w.shape and torch.equal(g, w), (nv, ngt, R is not None, have_bbox, name, differ)
                assert err <= bound, (nv, ngt, R is not None, have_bbox, name, err, bound)
    print("(%d, %d): worst error / bound = %.3f" % (nv, ngt, worst))


def _host_rows(ds, V):
    """utils.face_features on the vertices V, in node order with zero fake rows: what bind_vertices would be fed."""
    rows = ds.clean_faces_rows[0][0]
    F = rows[np.asarray(ds.permutations[0])][:ds.num_faces[0]].astype(np.uint32)
    nrm, ctr = utils.face_features(V, F)
    per_face = np.concatenate([nrm.astype(np.float32), ctr.astype(np.float32)], axis=1)
    return sc.rows_in_node_order(per_face, ds.permutations[0], ds.in_list[0].shape[1])


def _noisy(tag, level, step, direction="random", stream=0):
    V, F = _mesh(tag)
    normals = None
    if direction == "normal":
        normals = torch.as_tensor(utils.areaWeightedVertexNormals(V, F).astype(np.float32), device=DEV)
    sigma = np.float32(level) * np.float32(utils.getAverageEdgeLength(V, F)[0])
    return ops.synth_noise(torch.as_tensor(V, device=DEV), sigma, step, seed=SEED, stream=stream, normals=normals).cpu().numpy()


def _bound_net(tag, double=False, direction="random", seed=SEED, key="m", net=None):
    from facet_graph_convolution_amd.net import FacetDenoiser
    ds = _clean_set(tag)
    net = net or FacetDenoiser(DEV, multi_scale=True, seed=0)
    net.bind_clean_vertices(key, ds.in_list[0], ds.adj_list[0], ds.clean_vertices[0], ds.clean_faces_rows[0],
                            ds.v_faces_list[0], ds.clean_edge_len[0], gt_normals=ds.gt_list[0] if double else None,
                            seed=seed, direction=direction)
    return net, ds


def _samples(ds):
    nv = ds.clean_vertices[0].shape[1]
    rs = np.random.RandomState(2)
    return rs.randint(nv, size=500), rs.randint(nv, size=500)


def _step(net, double, capture=False):
    if double:
        net.double_loss_forward_backward(rotate=True, capture=capture)
    else:
        net.pointset_forward_backward(rotate=True, capture=capture)
    torch.cuda.synchronize()
    V = net._mesh["verts"]
    nv = V["x"].shape[0]
    loss = V["dl_out"].clone() if double else V["loss"].clone()
    return loss, V["traj"][-3 * nv:].clone(), [g.clone() for g in net.params.grads]


def _assert_same_step(a, b, what):
    assert torch.equal(a[0], b[0]), (what, a[0], b[0])
    assert torch.equal(a[1], b[1]), what
    assert len(a[2]) == len(b[2]) == 52
    for k, (p, q) in enumerate(zip(a[2], b[2])):
        assert torch.equal(p, q), (what, k)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("tag,direction", [("ico3", "random"), ("flipped", "normal")])
def test_a_synthesised_step_equals_a_step_on_host_made_inputs(tag, direction, double):
    from facet_graph_convolution_amd.net import FacetDenoiser
    net, ds = _bound_net(tag, double, direction)
    V = ds.clean_vertices[0][0]
    i0, i1 = _samples(ds)
    Rm = _rotation()
    net.set_point_samples(i0, i1)
    net.set_rotation(Rm)

    def reference(step, level):
        """A second network of the same seed, bound by bind_vertices on host-made inputs of the vertices the first drew."""
        Vn = net.noisy_vertices().cpu().numpy()
        assert np.array_equal(Vn.view(np.uint32), _noisy(tag, level, step, direction).view(np.uint32))
        a, b = utils.normalizePointSets(Vn, V)
        ref = FacetDenoiser(DEV, multi_scale=True, seed=0)
        ref.bind_vertices(0, _host_rows(ds, Vn), ds.adj_list[0], a, ds.clean_faces_rows[0], ds.v_faces_list[0], b,
                          gt_normals=ds.gt_list[0] if double else None)
        ref.set_point_samples(i0, i1)
        ref.set_rotation(Rm)
        return Vn, _step(ref, double)

    net.set_noise(7, 0.2)
    eager7 = _step(net, double)
    V7, ref7 = reference(7, 0.2)
    assert np.isfinite(eager7[0].cpu().numpy()).all() and eager7[0][0].item() > 0
    _assert_same_step(eager7, ref7, "eager")
    _step(net, double, capture=True)                      # records, then replays
    _assert_same_step(_step(net, double, capture=True), ref7, "captured")
    assert set(net._mesh["captured"]) == {"double" if double else "points"}
    # the graph reads the counter from device memory: a replay after set_noise draws the noise of counter 8
    net.set_noise(8, 0.2)
    replay8 = _step(net, double, capture=True)
    V8, ref8 = reference(8, 0.2)
    assert not np.array_equal(V7, V8)
    _assert_same_step(replay8, ref8, "replay at counter 8")
    assert not torch.equal(replay8[0], eager7[0]) and not torch.equal(replay8[1], eager7[1])
    _assert_same_step(_step(net, double), replay8, "eager at counter 8")


@pytest.mark.parametrize("tag", ["ico3", "flipped"])
def test_level_zero_and_the_off_word_give_the_plain_step_on_the_clean_mesh(tag):
    from facet_graph_convolution_amd.net import FacetDenoiser
    V, F = _mesh(tag)
    plain_set = TrainingSet()
    plain_set.addMeshWithVerticesAndGT(V, F, V, seed=0)
    net, ds = _bound_net(tag)
    i0, i1 = _samples(ds)
    Rm = _rotation()
    plain = FacetDenoiser(DEV, multi_scale=True, seed=0)
    plain.bind_vertices(0, plain_set.in_list[0], plain_set.adj_list[0], plain_set.v_list[0], plain_set.faces_list[0],
                        plain_set.v_faces_list[0], plain_set.gtv_list[0])
    for n in (net, plain):
        n.set_point_samples(i0, i1)
        n.set_rotation(Rm)
    want = _step(plain, False)
    assert np.isfinite(want[0].item())
    # zero noise words right after binding: the launches of the synthesis return at once, the clean mesh is what is there
    assert not net.buffers["noise"].any().item()
    _assert_same_step(_step(net, False), want, "off right after binding")
    net.set_noise(7, 0.3)                   # a noisy step first: level 0 must REBUILD the clean inputs, not find them
    noisy = _step(net, False)
    assert not torch.equal(noisy[0], want[0]) and not torch.equal(noisy[1], want[1])
    net.set_noise(8, 0.0)
    _assert_same_step(_step(net, False), want, "level 0")
    assert np.array_equal(net.noisy_vertices().cpu().numpy().view(np.uint32), V.view(np.uint32))
    # off again: the step runs on what the last ON step left
    net.set_noise(9, 0.3)
    noisy9 = _step(net, False)
    net.set_noise(10, None)
    _assert_same_step(_step(net, False), noisy9, "off after counter 9")
    # the loss alone, without the rotation launch argument
    net.set_noise(8, 0.0)
    assert torch.equal(net.pointset_loss(rotate=False), plain.pointset_loss(rotate=False))


def test_a_synthesised_step_has_one_launch_more_than_a_plain_one():
    from facet_graph_convolution_amd.net import FacetDenoiser
    V, F = _mesh("ico3")
    plain_set = TrainingSet()
    plain_set.addMeshWithVerticesAndGT(V, F, V, seed=0)
    net, ds = _bound_net("ico3")
    plain = FacetDenoiser(DEV, multi_scale=True, seed=0)
    plain.bind_vertices(0, plain_set.in_list[0], plain_set.adj_list[0], plain_set.v_list[0], plain_set.faces_list[0],
                        plain_set.v_faces_list[0], plain_set.gtv_list[0])
    i0, i1 = _samples(ds)
    counts = []
    for n in (net, plain):
        n.set_point_samples(i0, i1)
        n.set_rotation(_rotation())
        if n is net:
            n.set_noise(7, 0.2)
        _step(n, False)                      # (one-time set-up inside the library is not part of the count)
        n.profile_start()
        _step(n, False)
        counts.append(n.profile_stop())
    synth, base = counts
    total = lambda prof: sum(c for c, _ in prof.values())  # noqa: E731
    print("launches of an eager point-set step: %d synthesised, %d plain" % (total(synth), total(base)))
    print("  in front:", {k: v[0] for k, v in synth.items() if k.startswith(("fwd:synth", "pts:prepare", "pts:rotate"))},
          "against", {k: v[0] for k, v in base.items() if k.startswith(("fwd:synth", "pts:prepare", "pts:rotate"))})
    assert total(synth) == total(base) + 1
    assert sum(c for k, (c, _) in base.items() if k.startswith("pts:") and "rotate_rows_kernel" in k) == 2
    assert not [k for k in synth if k.startswith("pts:") and "rotate_rows_kernel" in k]
    assert sum(c for k, (c, _) in synth.items() if "point_sets_prepare_kernel" in k) == 1
    assert not [k for k in base if "point_sets_prepare_kernel" in k or "synth" in k]


def _own_full_loss(ds, levels, seed):
    """fullLoss of the noisy INPUT vertices of the validation meshes against the clean ones: what a network must beat."""
    from facet_graph_convolution_amd.makeNoisy import make_noisy
    V = ds.clean_vertices[0][0]
    rows = ds.clean_faces_rows[0][0]
    F = rows[np.asarray(ds.permutations[0])][:ds.num_faces[0]].astype(np.uint32)
    rs = np.random.RandomState(5)
    out = []
    for k, level in enumerate(levels):
        a, b = utils.normalizePointSets(make_noisy(V, F, level, seed=seed, stream=1, step=k), V)
        i0, i1 = (torch.as_tensor(rs.randint(len(V), size=500), device=DEV) for _ in range(2))
        out.append(ops.point_loss(torch.as_tensor(a, device=DEV), torch.as_tensor(b, device=DEV), i0, i1,
                                  want_grad=False)[0].item())
    return out


def test_training_on_synthesised_noise_lowers_the_validation_loss():
    from facet_graph_convolution_amd import train as T
    from facet_graph_convolution_amd.net import FacetDenoiser
    ds = _clean_set("ico3")
    levels = (0.1, 0.2, 0.3)
    valid = T._clean_vertex_meshes(ds, "validation set")
    fixed = lambda net: T.synthVertexValidationLoss(net, valid, levels, np.eye(3), np.random.RandomState(5), seed=0)[0]  # noqa: E731
    before = fixed(FacetDenoiser(DEV, multi_scale=True, seed=0))
    lines = []
    net, loss_array, hist = T.trainAccuracyNet(ds, 300, seed=0, log=lines.append, validSet=ds, noise_levels=levels)
    after = fixed(net)
    own = _own_full_loss(ds, levels, 0)
    print("fixed-noise validation loss: %.4f before, %.4f after 300 iterations; the noisy input's own fullLoss at "
          "0.1 / 0.2 / 0.3: %.4f / %.4f / %.4f" % ((before, after) + tuple(own)))
    assert any("validation loss" in s for s in lines) and any("training loss" in s for s in lines)
    assert hist.shape == (300,) and np.isfinite(hist).all() and loss_array.shape == (50, 2)
    assert np.isfinite(after) and np.isfinite(before) and after < before
    # the same noisy validation meshes at every call
    assert fixed(net) == after


def test_offline_loop_with_vertices_end_to_end(tmp_path, capsys):
    from facet_graph_convolution_amd import train as T, preprocess, infer, makeNoisy
    V, F = icosphere(2)
    clean, noisy, dump, path = (tmp_path / k for k in ("clean", "noisy", "dump", "net"))
    clean.mkdir()
    utils.write_mesh(V, F, str(clean / "ball.obj"))
    assert len(makeNoisy.main([str(clean), str(noisy), "--seed", "3"])) == 3
    preprocess.main([str(clean), str(dump), "--clean", "--with-vertices", "--valid", str(clean)])
    assert sorted(os.listdir(dump)) == ["trainingSetCleanWithVertices.pkl", "validSetCleanWithVertices.pkl"]
    capsys.readouterr()
    assert T.main([str(dump), str(path), "--with-vertices", "--synth-noise", "0.1,0.2,0.3", "--num-iterations", "12",
                   "--net-name", "syn", "--seed", "3"]) == "trainAccuracyNet"
    out = capsys.readouterr().out
    assert "Iteration 0, validation loss" in out and "Iteration 10, training loss" in out and "NAN" not in out
    files = os.listdir(path)
    assert "syn.csv" in files and "checkpoint" in files and any(f.startswith("syn-12") for f in files), files
    # a second call resumes at the saved iteration, on the double loss and from a captured step
    assert T.main([str(dump), str(path), "--with-vertices", "--double-loss", "--synth-noise", "0.2", "--noise-direction",
                   "normal", "--num-iterations", "3", "--net-name", "syn", "--capture"]) == "trainDoubleLossNet"
    out = capsys.readouterr().out
    assert "Iteration 0, validation loss = " in out and "(points " in out and "Iteration 0, training loss" in out
    assert "NAN" not in out and "nan" not in out
    assert any(f.startswith("syn-15") for f in os.listdir(path))
    one = tmp_path / "one"
    one.mkdir()
    shutil.copy(str(noisy / "ball_n2.obj"), str(one / "ball_n2.obj"))
    res = tmp_path / "res"
    infer.main([str(one), str(res), str(path), "--with-vertices"])
    assert sorted(os.listdir(res)) == ["ball_n2_d_coarse.obj", "ball_n2_d_mid.obj", "ball_n2_denoised.obj"]
    for name in os.listdir(res):
        got = np.loadtxt(str(res / name), usecols=(1, 2, 3), max_rows=len(V))
        assert got.shape == V.shape and np.isfinite(got).all(), name


def test_refusals():
    from facet_graph_convolution_amd.net import FacetDenoiser
    from facet_graph_convolution_amd.shard import make_sim_shards
    ds = _clean_set("ico3")
    x, adjs = ds.in_list[0], ds.adj_list[0]
    args = (x, adjs, ds.clean_vertices[0], ds.clean_faces_rows[0], ds.v_faces_list[0], ds.clean_edge_len[0])
    sharded = make_sim_shards(x, adjs, ds.gt_list[0], 2, device=DEV, multi_scale=True)[0]
    with pytest.raises(NotImplementedError):
        sharded.bind_clean_vertices("m", *args)
    with pytest.raises(NotImplementedError):
        FacetDenoiser(DEV, multi_scale=True, dtype="bf16").bind_clean_vertices("m", *args)
    with pytest.raises(NotImplementedError):
        FacetDenoiser(DEV, seed=0).bind_clean_vertices("m", *args)
    net = FacetDenoiser(DEV, multi_scale=True, seed=0)
    with pytest.raises(ValueError):
        net.bind_clean_vertices("m", x, adjs, ds.clean_vertices[0], ds.clean_faces_rows[0][:, :-4], ds.v_faces_list[0],
                                ds.clean_edge_len[0])
    with pytest.raises(ValueError):
        net.bind_clean_vertices("m", *args, direction="sideways")
    assert "m" not in net._mesh_cache
    net.bind_clean_vertices("m", *args, seed=1)
    assert "synth" in net._mesh and "verts" in net._mesh
    net.bind_clean_vertices("m", *args, seed=1)          # a cached mesh: a lookup
    with pytest.raises(ValueError):
        net.bind_clean_vertices("m", *args, seed=2)      # the cached mesh keeps its Philox key
    plain = FacetDenoiser(DEV, multi_scale=True, seed=0).bind_mesh(x, adjs)
    with pytest.raises(RuntimeError):
        plain.set_noise(0, 0.1)
