"""CPU checks of the double-loss training path (trainDoubleLossNet): the dense face-normal loss entry points refuse bad
arguments before any launch, the reference fixture is self-consistent (a float64 numpy restatement of faceNormalsLoss on
its stored head 0 and rotated ground truth gives its normal loss; total = points + normals), and the training command
parses its arguments and dispatches to the right trainer."""
import ctypes as C
import math
import os
import pickle

import numpy as np
import pytest

from facet_graph_convolution_amd import _lib
from facet_graph_convolution_amd import train as T


def _buf(n=1 << 16):
    b = (C.c_char * n)()
    return b, C.c_void_p((C.addressof(b) + 255) // 256 * 256)


def _rejects(rc, name):
    assert rc == -22, rc
    msg = _lib.lib().fgc_last_error()
    assert msg and name.encode() in msg, msg


def test_dense_normals_loss_rejects_bad_arguments():
    L = _lib.lib()
    keep, p = _buf()
    q = C.c_void_p(p.value + 4096)
    assert L.fgc_dense_normals_loss_scratch_floats(1) == 2
    assert L.fgc_dense_normals_loss_scratch_floats(256) == 2
    assert L.fgc_dense_normals_loss_scratch_floats(257) == 4
    assert L.fgc_dense_normals_loss_scratch_floats(0) == 0
    need = L.fgc_dense_normals_loss_scratch_floats(1000)
    names = ("fn", "gt", "R", "n", "loss", "add", "total", "scr", "sf", "st")
    base = dict(fn=p, gt=p, R=None, n=1000, loss=p, add=None, total=None, scr=p, sf=need, st=None)
    f = lambda **kw: L.fgc_dense_normals_loss_fwd(*[kw.get(k, base[k]) for k in names])  # noqa: E731
    for k in ("fn", "gt", "loss", "scr"):
        _rejects(f(**{k: None}), "fgc_dense_normals_loss_fwd")
    for n in (0, -5):
        _rejects(f(n=n), "fgc_dense_normals_loss_fwd")
    _rejects(f(sf=need - 1), "scratch too small")
    _rejects(f(add=p), "add and total")
    _rejects(f(total=p), "add and total")
    names = ("fn", "gt", "R", "n", "scr", "sf", "dloss", "g", "st")
    base = dict(fn=p, gt=p, R=None, n=1000, scr=p, sf=need, dloss=1.0, g=q, st=None)
    f = lambda **kw: L.fgc_dense_normals_loss_bwd(*[kw.get(k, base[k]) for k in names])  # noqa: E731
    for k in ("fn", "gt", "scr", "g"):
        _rejects(f(**{k: None}), "fgc_dense_normals_loss_bwd")
    _rejects(f(n=0), "fgc_dense_normals_loss_bwd")
    _rejects(f(sf=need - 1), "scratch too small")
    _rejects(f(g=p), "distinct")


def _face_normals_loss_f64(fn, gt_fn):
    """faceNormalsLoss (train.py:1272-1294) in float64 numpy."""
    fn, gt_fn = np.asarray(fn, np.float64), np.asarray(gt_fn, np.float64)
    dt = (fn * gt_fn).sum(-1)
    ang = np.arccos(np.clip(dt, -0.9999999, 0.9999999)) * 180 / math.pi
    real = np.abs(gt_fn).sum(-1) > 10e-4
    return ang[real].sum() / real.sum()


@pytest.mark.parametrize("name", ["double_ico3.npz", "double_ico3_f64.npz"])
def test_double_fixture_is_self_consistent(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    f64 = "f64" in name
    nl = _face_normals_loss_f64(z["n_conv0"], z["gtfn_rot"])
    # (the fixture stores its fp32 run's head 0 and rotated ground truth rounded to fp32 in both files)
    assert abs(nl - float(z["loss_normals"])) <= 2e-6 * nl, (nl, float(z["loss_normals"]))
    total, pts, nrm = float(z["loss"]), float(z["loss_points"]), float(z["loss_normals"])
    assert abs(total - (pts + nrm)) <= (1e-12 if f64 else 2.0 ** -22) * total
    # fake nodes: zero rows of the ground truth in node order, none of them counted
    fake = np.abs(z["gt_normals"]).sum(1) <= 10e-4
    assert 0 < fake.sum() < fake.size and (np.abs(z["gtfn_rot"][fake]).sum(1) == 0).all()
    real = ~fake
    np.testing.assert_allclose(np.linalg.norm(z["gt_normals"][real], axis=1), 1.0, atol=1e-5)
    np.testing.assert_allclose(z["gtfn_rot"], z["gt_normals"].astype(np.float64) @ z["R"].astype(np.float64).T, atol=1e-5)
    p = np.load(os.path.join(golden_dir, "points_ico3.npz"))
    assert (z["sample_ind0"] == p["sample_ind0"]).all() and (z["sample_ind1"] == p["sample_ind1"]).all()
    assert (z["R"] == p["R"]).all() and int(z["n_vars"]) == int(p["n_vars"])


def _dump(tmp_path, names):
    d = tmp_path / "dump"
    d.mkdir(exist_ok=True)
    for n in names:
        with open(d / n, "wb") as fh:
            pickle.dump({"name": n}, fh)
    return d


def _fake_trainers(monkeypatch):
    calls = []

    def fake(name):
        def run(trainSet, num_iterations, **kw):
            calls.append((name, trainSet, num_iterations, kw))
        return run
    for name in ("trainNet", "trainAccuracyNet", "trainDoubleLossNet"):
        monkeypatch.setattr(T, name, fake(name))
    return calls


def test_training_command_needs_vertices_for_the_double_loss(tmp_path, capsys, monkeypatch):
    calls = _fake_trainers(monkeypatch)
    d = _dump(tmp_path, ["trainingSetWithVertices.pkl", "trainingSet.pkl"])
    with pytest.raises(SystemExit) as e:
        T.main([str(d), str(tmp_path / "net"), "--double-loss"])
    assert e.value.code == 2 and "--with-vertices" in capsys.readouterr().err
    assert calls == [] and not (tmp_path / "net").exists()


@pytest.mark.parametrize("flags", [[], ["--with-vertices"], ["--with-vertices", "--double-loss"]])
def test_training_command_reports_a_missing_pickle(tmp_path, capsys, monkeypatch, flags):
    calls = _fake_trainers(monkeypatch)
    d = _dump(tmp_path, ["validSet.pkl", "validSetWithVertices.pkl"])
    with pytest.raises(SystemExit) as e:
        T.main([str(d), str(tmp_path / "net")] + flags)
    err = capsys.readouterr().err
    want = "trainingSetWithVertices.pkl" if flags else "trainingSet.pkl"
    assert e.value.code == 2 and want in err and "preprocess" in err, err
    assert calls == []


@pytest.mark.parametrize("flags,trainer,pkl", [
    ([], "trainNet", "trainingSet.pkl"),
    (["--with-vertices"], "trainAccuracyNet", "trainingSetWithVertices.pkl"),
    (["--with-vertices", "--double-loss"], "trainDoubleLossNet", "trainingSetWithVertices.pkl"),
])
@pytest.mark.parametrize("with_valid", [False, True])
def test_training_command_dispatches(tmp_path, monkeypatch, flags, trainer, pkl, with_valid):
    calls = _fake_trainers(monkeypatch)
    names = ["trainingSet.pkl", "trainingSetWithVertices.pkl"]
    if with_valid:
        names += ["validSet.pkl", "validSetWithVertices.pkl"]
    d = _dump(tmp_path, names)
    net_dir = tmp_path / "nets" / "run1"
    T.main([str(d), str(net_dir), "--num-iterations", "7", "--net-name", "dbl", "--seed", "3", "--capture"] + flags)
    assert len(calls) == 1
    name, ts, iters, kw = calls[0]
    assert name == trainer and ts == {"name": pkl} and iters == 7
    assert kw["network_path"] == str(net_dir) and kw["net_name"] == "dbl" and kw["seed"] == 3 and kw["capture"] is True
    want_valid = {"name": pkl.replace("training", "valid")} if with_valid else None
    assert kw["validSet"] == want_valid
    assert net_dir.is_dir()


def test_training_command_defaults(tmp_path, monkeypatch):
    from facet_graph_convolution_amd.settings import NUM_ITERATIONS
    calls = _fake_trainers(monkeypatch)
    d = _dump(tmp_path, ["trainingSet.pkl"])
    T.main([str(d), str(tmp_path / "net")])
    name, _, iters, kw = calls[0]
    assert name == "trainNet" and iters == NUM_ITERATIONS
    assert kw["net_name"] == "net" and kw["seed"] == 0 and kw["capture"] is False and kw["validSet"] is None


def test_train_double_loss_net_names_a_mesh_without_normals():
    """Checked before the network is created: no GPU needed."""
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    from facet_graph_convolution_amd.meshgen import icosphere, add_noise
    V, F = icosphere(1)
    ds = TrainingSet()
    ds.addMeshWithVerticesAndGT(add_noise(V, F, seed=1), F, V, seed=0)
    assert len(ds.gt_list) == len(ds.gtv_list) == 1
    for name in ("in_list", "adj_list", "v_list", "faces_list", "v_faces_list", "gtv_list"):
        getattr(ds, name).append(getattr(ds, name)[0])
    with pytest.raises(ValueError, match="mesh 1 has no ground-truth face normals"):
        T.trainDoubleLossNet(ds, 1, log=lambda s: None)
