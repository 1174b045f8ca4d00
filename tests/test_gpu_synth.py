"""Training from clean meshes: the per-step noise synthesis on the GPU (include/fgc.h: fgc_synth_noise,
fgc_face_features_rows; FacetDenoiser.bind_clean) against a float64 oracle of its definitions (tests/synth_cases.py), the
host feature routine, and a second network fed host-made features."""
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
STEPS = (0, 1, 7)
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _mesh(tag):
    if tag == "torus":
        return torus(250, 200)
    if tag == "ico3":
        return icosphere(3)
    V, F = torus(24, 20)
    return V, flip_edges(F, 400, seed=1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _clean_set(tag):
    V, F = _mesh(tag)
    ds = TrainingSet()
    ds.addCleanMesh(V, F, seed=0)
    return ds


def _sigma(tag, level):
    V, F = _mesh(tag)
    return np.float32(level) * np.float32(utils.getAverageEdgeLength(V, F)[0])


def _noisy(tag, level, step, seed=SEED, stream=0, direction="random"):
    V, F = _mesh(tag)
    normals = None
    if direction == "normal":
        normals = torch.as_tensor(utils.areaWeightedVertexNormals(V, F).astype(np.float32), device=DEV)
    out = ops.synth_noise(torch.as_tensor(V, device=DEV), _sigma(tag, level), step, seed=seed, stream=stream, normals=normals)
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _host_rows(ds, V):
    """utils.face_features on the vertices V, in node order with zero fake rows: what bind_mesh would be fed."""
    F = _faces_of(ds)
    nrm, ctr = utils.face_features(V, F)
    per_face = np.concatenate([nrm.astype(np.float32), ctr.astype(np.float32)], axis=1)
    return sc.rows_in_node_order(per_face, ds.permutations[0], ds.in_list[0].shape[1])


def _faces_of(ds):
    rows = ds.clean_faces_rows[0][0]
    return rows[np.asarray(ds.permutations[0])][:ds.num_faces[0]].astype(np.uint32)


def test_device_philox_known_answers():
    """The three published answers through the DEVICE generator, and a run of counters against the numpy helper."""
    for counter, key, want in sc.KNOWN_ANSWERS:
        got = ops.philox_words(counter[0], 1, counter[1] | (counter[2] << 32), seed=key[0] | (key[1] << 32),
                               stream=counter[3], device=DEV).cpu().numpy().view(np.uint32)[0]
        assert tuple(int(g) for g in got) == want, [hex(int(g)) for g in got]
    n, step, seed, stream = 1000, (5 << 32) | 7, (9 << 32) | SEED, 3
    got = ops.philox_words(0xFFFFFF00, n, step, seed=seed, stream=stream, device=DEV).cpu().numpy().view(np.uint32)
    i = (np.arange(n, dtype=np.uint64) + np.uint64(0xFFFFFF00)) & np.uint64(sc.MASK)       # (wraps past 2^32)
    full = lambda v: np.full(n, v, dtype=np.uint64)
    want = sc.philox4x32_10((i, full(7), full(5), full(stream)), (SEED, 9))
    assert np.array_equal(got.astype(np.uint64), np.stack(want, axis=1))


@pytest.mark.parametrize("tag", ["torus", "ico3", "flipped"])
@pytest.mark.parametrize("direction", ["random", "normal"])
def test_noise_matches_the_float64_oracle(tag, direction):
    V, F = _mesh(tag)
    worst = 0.0
    for level in (0.1, 0.3):
        sigma = _sigma(tag, level)
        bound = 1e-5 * float(sigma) + 2.0 ** -23 * float(np.abs(V).max())
        for step in STEPS:
            got = _noisy(tag, level, step, direction=direction).astype(np.float64)
            want = sc.oracle(V, F, sigma, step, SEED, 0, direction)
            err = np.abs(got - want).max()
            print("%s %s level %.1f step %d: max |V' - oracle| = %.3e (bound %.3e, sigma %.3e)"
                  % (tag, direction, level, step, err, bound, sigma))
            assert np.isfinite(got).all() and err <= bound, (tag, direction, level, step, err, bound)
            worst = max(worst, err / bound)
    print("%s %s: worst error / bound = %.3f" % (tag, direction, worst))


def test_noise_statistics_on_the_torus():
    V, F = _mesh("torus")
    n = V.shape[0]
    assert n == 50000
    sigma = float(_sigma("torus", 0.2))
    for step in STEPS:
        disp = _noisy("torus", 0.2, step).astype(np.float64) - V.astype(np.float64)
        d = sc.directions(sc.gaussians(n, step, SEED, 0))
        s = (disp * d).sum(1) / sigma
        std_err, mean_err = abs(s.std(ddof=1) - 1.0) * np.sqrt(2 * n), abs(s.mean()) * np.sqrt(n)
        # the directions the DEVICE moved the vertices along
        dd = disp / np.linalg.norm(disp, axis=1, keepdims=True) * np.sign(s)[:, None]
        dir_err = np.abs(dd.mean(0)) * np.sqrt(3 * n)
        print("step %d: std %.5f (%.2f se), mean %.5f (%.2f se), mean direction %s (%.2f se)"
              % (step, s.std(ddof=1), std_err, s.mean(), mean_err, dd.mean(0), dir_err.max()))
        assert std_err <= 4.0 and mean_err <= 4.0 and (dir_err <= 4.0).all()
        big = np.abs(s) > 0.1          # (a short displacement's direction is lost in the rounding of the final add)
        assert np.abs((dd * d).sum(1) - 1.0)[big].max() < 1e-6
    clean = utils.computeFacesNormals(V, F)
    ang = []
    for level in (0.1, 0.2, 0.3):
        noisy = utils.computeFacesNormals(_noisy("torus", level, 0), F)
        ang.append(float(np.degrees(np.arccos(np.clip((clean * noisy).sum(1), -1, 1))).mean()))
    print("mean angular error of the noisy face normals at 0.1 / 0.2 / 0.3: %.2f / %.2f / %.2f degrees" % tuple(ang))
    assert 0 < ang[0] < ang[1] < ang[2]


def _bound_net(tag, seed=0, dtype="f32", stream=0, direction="random", key="m"):
    from facet_graph_convolution_amd.net import FacetDenoiser
    ds = _clean_set(tag)
    net = FacetDenoiser(DEV, seed=seed, dtype=dtype)
    net.bind_clean(key, ds.in_list[0], ds.adj_list[0], ds.gt_list[0], ds.clean_vertices[0], ds.clean_faces_rows[0],
                   ds.clean_edge_len[0], seed=SEED, stream=stream, direction=direction)
    return net, ds


@pytest.mark.parametrize("tag", ["torus", "ico3", "flipped"])
def test_level_zero_is_the_identity(tag):
    V, F = _mesh(tag)
    assert np.array_equal(_bits(_noisy(tag, 0.0, 3)), _bits(V))
    net, ds = _bound_net(tag)
    x0 = net.buffers["x"].cpu().numpy()
    assert np.array_equal(_bits(x0), _bits(ds.in_list[0][0]))
    net.set_noise(7, 0.3)                    # a noisy step first: level 0 must REBUILD the clean rows, not find them
    net.forward(rotate=False)
    torch.cuda.synchronize()
    assert not np.array_equal(_bits(net.buffers["x"].cpu().numpy()), _bits(x0))
    net.set_noise(8, 0.0)
    net.forward(rotate=False)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(net.noisy_vertices().cpu().numpy()), _bits(V))
    assert np.array_equal(_bits(net.buffers["x"].cpu().numpy()), _bits(x0))
    # synthesis off: nothing is touched
    net.set_noise(9, 0.3)
    net.forward(rotate=False)
    xn, vn = net.buffers["x"].clone(), net.noisy_vertices().clone()
    net.set_noise(10, None)
    net.forward(rotate=False)
    torch.cuda.synchronize()
    assert torch.equal(xn, net.buffers["x"]) and torch.equal(vn, net.noisy_vertices())


@pytest.mark.parametrize("tag", ["torus", "ico3", "flipped"])
def test_features_are_bit_identical_to_the_host_routine(tag):
    ds = _clean_set(tag)
    V, F = _mesh(tag)
    assert np.array_equal(_faces_of(ds), F)
    rows = torch.as_tensor(ds.clean_faces_rows[0][0], device=DEV)
    for level, step in ((0.2, 0), (0.3, 7)):
        Vn = _noisy(tag, level, step)
        want = _host_rows(ds, Vn)
        got = ops.face_features_rows(torch.as_tensor(Vn, device=DEV), rows).cpu().numpy()
        fake = (ds.clean_faces_rows[0][0] < 0).any(1)
        assert not got[fake].any() and fake.sum() == want.shape[0] - F.shape[0]
        diff = _bits(got) != _bits(want)
        print("%s level %.1f: %d of %d words differ" % (tag, level, int(diff.sum()), diff.size))
        assert not diff.any()
        # ... and with the bounding-box partials the noise launch leaves behind (the two launches of a training step)
        Vd = torch.as_tensor(V, device=DEV)
        scratch = torch.empty(6 * 1024, dtype=torch.float32, device=DEV)
        Vo = ops.synth_noise(Vd, _sigma(tag, level), step, seed=SEED, scratch=scratch)
        got2 = ops.face_features_rows(Vo, rows, scratch=scratch, have_bbox=True).cpu().numpy()
        assert np.array_equal(_bits(got2), _bits(want))


def test_noise_is_deterministic_and_moves_with_step_and_stream():
    a = _noisy("torus", 0.2, 7, stream=2)
    assert np.array_equal(_bits(a), _bits(_noisy("torus", 0.2, 7, stream=2)))
    for other in (_noisy("torus", 0.2, 8, stream=2), _noisy("torus", 0.2, 7, stream=3), _noisy("torus", 0.2, 7, seed=SEED + 1, stream=2),
                  _noisy("torus", 0.2, 7 + (1 << 32), stream=2), _noisy("torus", 0.2, 7, seed=SEED + (1 << 32), stream=2)):
        assert (np.abs(other - a).max(1) > 0).mean() > 0.99


def _step_state(net):
    torch.cuda.synchronize()
    return (net.buffers["loss"].clone(), net.buffers["nconv"].clone(), [g.clone() for g in net.params.grads])


def _assert_same_step(a, b, what):
    assert torch.equal(a[0], b[0]), (what, a[0], b[0])
    assert torch.equal(a[1], b[1]), what
    assert len(a[2]) == len(b[2]) == 44
    for k, (p, q) in enumerate(zip(a[2], b[2])):
        assert torch.equal(p, q), (what, k)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag,direction", [("ico3", "random"), ("flipped", "normal")])
def test_a_synthetic_step_equals_a_step_on_host_made_features(tag, direction, dtype):
    from facet_graph_convolution_amd.net import FacetDenoiser
    from facet_graph_convolution_amd.utils import rand_rotation_matrix
    net, ds = _bound_net(tag, dtype=dtype, direction=direction)
    n0 = ds.in_list[0].shape[1]
    samp = np.random.RandomState(2).randint(n0, size=4000)
    Rm = rand_rotation_matrix(randnums=np.random.RandomState(3).uniform(size=3))
    net.set_samples(samp)
    net.set_rotation(Rm)

    def reference(step, level):
        """A second network of the same seed, bound on host-made features of the vertices the first one drew."""
        Vn = _noisy(tag, level, step, direction=direction)
        ref = FacetDenoiser(DEV, seed=0, dtype=dtype).bind_mesh(_host_rows(ds, Vn), ds.adj_list[0], gt=ds.gt_list[0])
        ref.set_samples(samp)
        ref.set_rotation(Rm)
        ref.forward_backward(rotate=True)
        return Vn, _step_state(ref)

    net.set_noise(7, 0.2)
    net.forward_backward(rotate=True)
    eager7 = _step_state(net)
    V7, ref7 = reference(7, 0.2)
    assert np.array_equal(_bits(net.noisy_vertices().cpu().numpy()), _bits(V7))
    assert np.isfinite(eager7[0][0].item()) and eager7[0][0].item() > 0
    _assert_same_step(eager7, ref7, "eager")
    net.forward_backward(rotate=True, capture=True)      # records, then replays
    net.forward_backward(rotate=True, capture=True)
    _assert_same_step(_step_state(net), ref7, "captured")
    # the graph reads the counter from device memory: a replay after set_noise draws the noise of counter 8
    net.set_noise(8, 0.2)
    net.forward_backward(rotate=True, capture=True)
    replay8 = _step_state(net)
    V8, ref8 = reference(8, 0.2)
    assert np.array_equal(_bits(net.noisy_vertices().cpu().numpy()), _bits(V8)) and not np.array_equal(V7, V8)
    _assert_same_step(replay8, ref8, "replay at counter 8")
    assert not torch.equal(replay8[0], eager7[0])
    net.forward_backward(rotate=True)
    _assert_same_step(_step_state(net), replay8, "eager at counter 8")
    # the same words through a packed row (pack_step_inputs(noise=...)), level and sigma being the same number here
    row = FacetDenoiser.pack_step_inputs([samp], [Rm], DEV, noise=[(7, np.float32(0.2) * np.float32(ds.clean_edge_len[0]))])
    net.set_step_inputs_packed(row[0])
    net.forward_backward(rotate=True, capture=True)
    _assert_same_step(_step_state(net), ref7, "packed row")
    # a row without noise words switches the synthesis off: x stays as the last step left it
    net.set_step_inputs_packed(FacetDenoiser.pack_step_inputs([samp], [Rm], DEV)[0])
    net.forward_backward(rotate=True, capture=True)
    _assert_same_step(_step_state(net), ref7, "packed row without noise")


def _own_angular_error(ds, levels, seed):
    """Mean angular error (degrees) of the noisy INPUT normals of the validation meshes: what a network must beat."""
    from facet_graph_convolution_amd.makeNoisy import make_noisy
    F = _faces_of(ds)
    V = ds.clean_vertices[0][0]
    clean = utils.computeFacesNormals(V, F)
    out = []
    for k, level in enumerate(levels):
        noisy = utils.computeFacesNormals(make_noisy(V, F, level, seed=seed, stream=1, step=k), F)
        out.append(float(np.degrees(np.arccos(np.clip((clean * noisy).sum(1), -1, 1))).mean()))
    return out


def test_training_on_synthetic_noise_lowers_the_validation_loss():
    from facet_graph_convolution_amd import train as T
    from facet_graph_convolution_amd.net import FacetDenoiser
    ds = _clean_set("ico3")
    levels = (0.1, 0.2, 0.3)
    valid = T._clean_meshes(ds, "validation set")
    fixed = lambda net: T.synthValidationLoss(net, valid, levels, np.eye(3), np.random.RandomState(5), seed=0)
    before = fixed(FacetDenoiser(DEV, seed=0))
    lines = []
    net, loss_array = T.trainNet(ds, 60, seed=0, log=lines.append, validSet=ds, noise_levels=levels)
    after = fixed(net)
    own = _own_angular_error(ds, levels, 0)
    print("fixed-noise validation loss: %.3f degrees before, %.3f after 60 iterations; the noisy input's own mean angular "
          "error at 0.1 / 0.2 / 0.3: %.2f / %.2f / %.2f degrees" % ((before, after) + tuple(own)))
    assert any("validation loss" in s for s in lines) and loss_array.shape == (1, 2)
    assert np.isfinite(after) and np.isfinite(before) and after < before
    # the same noisy validation meshes at every call
    assert fixed(net) == after


def test_offline_loop_end_to_end(tmp_path, capsys):
    from facet_graph_convolution_amd import train as T, preprocess, infer, makeNoisy
    from facet_graph_convolution_amd.settings import getGTFilename
    V, F = icosphere(2)
    clean, noisy, dump, path = (tmp_path / k for k in ("clean", "noisy", "dump", "net"))
    clean.mkdir()
    utils.write_mesh(V, F, str(clean / "ball.obj"))
    written = makeNoisy.main([str(clean), str(noisy), "--seed", "3"])
    assert sorted(os.listdir(noisy)) == ["ball_n1.obj", "ball_n2.obj", "ball_n3.obj"] and len(written) == 3
    assert all(getGTFilename(f) == "ball.obj" for f in os.listdir(noisy))
    n2 = utils.load_mesh(str(noisy), "ball_n2.obj")[0]
    assert n2.shape == V.shape and 0 < np.abs(n2 - V).max() < 0.5
    assert makeNoisy.main([str(clean), str(noisy), "--seed", "3"]) == []          # existing files are skipped
    preprocess.main([str(clean), str(dump), "--clean", "--valid", str(clean)])
    assert sorted(os.listdir(dump)) == ["trainingSetClean.pkl", "validSetClean.pkl"]
    capsys.readouterr()
    assert T.main([str(dump), str(path), "--synth-noise", "0.1,0.2,0.3", "--num-iterations", "12", "--net-name", "syn",
                   "--seed", "3"]) == "trainNet"
    out = capsys.readouterr().out
    assert "Iteration 0, validation loss" in out and "Iteration 0, training loss" in out and "NAN" not in out
    files = os.listdir(path)
    assert "syn.csv" in files and "checkpoint" in files and any(f.startswith("syn-12") for f in files), files
    # a second call resumes at the saved iteration (and goes on with new noise: the counter is the global iteration)
    T.main([str(dump), str(path), "--synth-noise", "0.2", "--noise-direction", "normal", "--num-iterations", "3",
            "--net-name", "syn", "--capture"])
    assert any(f.startswith("syn-15") for f in os.listdir(path))
    one = tmp_path / "one"
    one.mkdir()
    shutil.copy(str(noisy / "ball_n2.obj"), str(one / "ball_n2.obj"))
    res = tmp_path / "res"
    infer.main([str(one), str(res), str(path)])
    assert "ball_n2_denoised.obj" in os.listdir(res)
    got = np.loadtxt(str(res / "ball_n2_denoised.obj"), usecols=(1, 2, 3), max_rows=len(V))
    assert got.shape == V.shape and np.isfinite(got).all()


def test_refusals():
    from facet_graph_convolution_amd.net import FacetDenoiser
    from facet_graph_convolution_amd.shard import make_sim_shards
    ds = _clean_set("ico3")
    x, adjs, gt = ds.in_list[0], ds.adj_list[0], ds.gt_list[0]
    args = (x, adjs, gt, ds.clean_vertices[0], ds.clean_faces_rows[0], ds.clean_edge_len[0])
    sharded = make_sim_shards(x, adjs, gt, 2, device=DEV)[0]
    with pytest.raises(NotImplementedError):
        sharded.bind_clean("m", *args)
    net = FacetDenoiser(DEV, seed=0)
    with pytest.raises(ValueError):
        net.bind_clean("m", x, adjs, gt, ds.clean_vertices[0], ds.clean_faces_rows[0][:, :-4], ds.clean_edge_len[0])
    with pytest.raises(ValueError):
        net.bind_clean("m", *args, direction="sideways")
    with pytest.raises(ValueError):
        net.bind_clean("m", x, adjs, gt, ds.clean_vertices[0][:, :-1], ds.clean_faces_rows[0], ds.clean_edge_len[0])
    plain = FacetDenoiser(DEV, seed=0).bind_mesh(x, adjs, gt=gt)
    with pytest.raises(RuntimeError):
        plain.set_noise(0, 0.1)
    with pytest.raises(RuntimeError):
        plain.noisy_vertices()
    # a mesh already cached by bind_cached (and captured) gains the synthesis: its captured step is recorded again
    net.bind_cached("k", x, adjs, gt=gt)
    net.set_samples(np.arange(4000) % x.shape[1])
    net.forward_backward(rotate=True, capture=True)
    assert net._mesh["captured"]
    net.bind_clean("k", *args)
    assert "synth" in net._mesh and not net._mesh["captured"]
    net.bind_clean("m", *args, seed=1)
    with pytest.raises(ValueError):
        net.bind_clean("m", *args, seed=2)          # the cached mesh keeps its Philox key
