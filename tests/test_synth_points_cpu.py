"""CPU checks of training the vertex networks from clean meshes: fgc_point_sets_prepare refuses bad arguments before any
launch, the clean vertex training set, and the `preprocess --clean --with-vertices` / `train --with-vertices
--synth-noise` command lines.  No GPU compute here."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from facet_graph_convolution_amd import _lib
from facet_graph_convolution_amd.dataClasses import TrainingSet
from facet_graph_convolution_amd.meshgen import icosphere
from facet_graph_convolution_amd.utils import write_mesh, getAverageEdgeLength


def _buf(n=1 << 16):
    b = (C.c_char * n)()
    return b, C.c_void_p((C.addressof(b) + 255) // 256 * 256)


def _rejects(rc, name):
    assert rc == -22, rc
    msg = _lib.lib().fgc_last_error()
    assert msg and name.encode() in msg, msg


def test_point_sets_prepare_rejects_bad_arguments():
    L = _lib.lib()
    assert L.fgc_version() == _lib.ABI_VERSION >= 112
    keep, p = _buf()
    q = [C.c_void_p(p.value + 4096 * k) for k in range(1, 4)]
    need = L.fgc_synth_scratch_floats(1000)
    assert need == 6 * 4
    names = ("v", "nv", "gt", "ngt", "box", "R", "have", "vo", "go", "sc", "scf", "st")
    base = dict(v=p, nv=1000, gt=q[0], ngt=10, box=p, R=None, have=1, vo=q[1], go=q[2], sc=p, scf=need, st=None)
    f = lambda **kw: L.fgc_point_sets_prepare(*[kw.get(k, base[k]) for k in names])  # noqa: E731
    for k in ("v", "gt", "box", "vo", "go", "sc"):
        _rejects(f(**{k: None}), "fgc_point_sets_prepare: null pointer")
    for have in (0, 1):
        _rejects(f(nv=0, have=have), "fgc_point_sets_prepare: nv=0")
        _rejects(f(ngt=0, have=have), "fgc_point_sets_prepare: nv=1000, ngt=0")
        _rejects(f(nv=-5, have=have), "fgc_point_sets_prepare")
        _rejects(f(scf=need - 1, have=have), "scratch too small")
    _rejects(f(vo=p), "buffers of their own")
    _rejects(f(go=q[0]), "buffers of their own")


def test_add_clean_mesh_with_vertices_matches_add_mesh_with_vertices_and_gt():
    V, F = icosphere(3)
    a, b = TrainingSet(), TrainingSet()
    a.addCleanMeshWithVertices(V, F, seed=5)
    b.addMeshWithVerticesAndGT(V, F, V, seed=5)
    assert a.is_clean() and not b.is_clean()
    extra = {"clean_vertices", "clean_faces_rows", "clean_edge_len"}
    assert set(a.__dict__) == set(b.__dict__) | extra

    def same(p, q):
        if isinstance(p, (list, tuple)):
            return len(p) == len(q) and all(same(x, y) for x, y in zip(p, q))
        if isinstance(p, np.ndarray):
            return p.dtype == q.dtype and p.shape == q.shape and np.array_equal(p, q)
        return p == q
    for name in b.__dict__:
        assert same(a.__dict__[name], b.__dict__[name]), name
    assert len(a.gtv_list) == len(a.v_list) == len(a.gt_list) == 1 and np.array_equal(a.gtv_list[0], a.v_list[0])
    rows = a.clean_faces_rows[0]
    assert rows.dtype == np.int32 and rows.shape == a.faces_list[0].shape and np.array_equal(rows, a.faces_list[0])
    assert a.clean_vertices[0].dtype == np.float32 and np.array_equal(a.clean_vertices[0][0], V)
    assert a.clean_edge_len == [float(getAverageEdgeLength(V, F)[0])]
    # the same three fields addCleanMesh stores
    c = TrainingSet()
    c.addCleanMesh(V, F, seed=5)
    for name in extra:
        assert same(a.__dict__[name], c.__dict__[name]), name


def test_add_clean_mesh_with_vertices_refuses_patch_mode():
    V, F = icosphere(3)
    ds = TrainingSet(maxSize=1000)
    with pytest.raises(NotImplementedError):
        ds.addCleanMeshWithVertices(V, F)
    assert ds.mesh_count == 0 and not ds.v_list


def test_preprocess_clean_with_vertices(tmp_path, capsys):
    from facet_graph_convolution_amd import preprocess
    clean = tmp_path / "clean"
    clean.mkdir()
    with pytest.raises(SystemExit) as e:                       # no OBJ file there
        preprocess.main([str(clean), str(tmp_path / "a"), "--clean", "--with-vertices"])
    assert e.value.code == 2 and "no OBJ file" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                       # three folders with --clean
        preprocess.main([str(clean), str(tmp_path / "a"), str(tmp_path / "b"), "--clean", "--with-vertices"])
    assert e.value.code == 2
    V, F = icosphere(2)
    write_mesh(V, F, str(clean / "ball.obj"))
    preprocess.main([str(clean), str(tmp_path / "dump"), "--clean", "--with-vertices", "--valid", str(clean),
                     "--redundancy", "2"])
    assert sorted(os.listdir(tmp_path / "dump")) == ["trainingSetCleanWithVertices.pkl", "validSetCleanWithVertices.pkl"]
    with open(tmp_path / "dump" / "trainingSetCleanWithVertices.pkl", "rb") as fp:
        ds = pickle.load(fp)
    assert ds.is_clean() and ds.mesh_count == 2 and len(ds.v_list) == len(ds.gtv_list) == len(ds.v_faces_list) == 2
    assert np.array_equal(ds.clean_faces_rows[1], ds.faces_list[1]) and ds.clean_vertices[1].shape == (1, len(V), 3)
    with open(tmp_path / "dump" / "validSetCleanWithVertices.pkl", "rb") as fp:
        assert pickle.load(fp).mesh_count == 1
    # without --with-vertices the names are the old ones
    preprocess.main([str(clean), str(tmp_path / "dump2"), "--clean"])
    assert os.listdir(tmp_path / "dump2") == ["trainingSetClean.pkl"]


def test_train_with_vertices_synth_noise_arguments(tmp_path, capsys):
    from facet_graph_convolution_amd import train as T
    dump = tmp_path / "dump"
    dump.mkdir()
    for extra in ([], ["--double-loss"]):
        with pytest.raises(SystemExit) as e:
            T.main([str(dump), str(tmp_path / "net"), "--with-vertices", "--synth-noise", "0.1"] + extra)
        err = capsys.readouterr().err
        assert e.value.code == 2 and "trainingSetCleanWithVertices.pkl" in err and "--clean --with-vertices" in err, err
    for argv in ([str(dump), str(tmp_path / "net"), "--with-vertices", "--synth-noise", "0.1,abc"],
                 [str(dump), str(tmp_path / "net"), "--with-vertices", "--synth-noise", "0.1,-0.2"],
                 [str(dump), str(tmp_path / "net"), "--double-loss", "--synth-noise", "0.1"]):
        with pytest.raises(SystemExit) as e:
            T.main(argv)
        assert e.value.code == 2, argv
    # a pickle of the plain vertex form does not serve the clean path: the clean one is asked for by name
    (dump / "trainingSetWithVertices.pkl").write_bytes(b"")
    with pytest.raises(SystemExit) as e:
        T.main([str(dump), str(tmp_path / "net"), "--with-vertices", "--synth-noise"])
    assert e.value.code == 2 and "trainingSetCleanWithVertices.pkl" in capsys.readouterr().err


@pytest.mark.parametrize("trainer", ["trainAccuracyNet", "trainDoubleLossNet"])
def test_vertex_trainers_with_noise_levels_need_a_clean_vertex_set(trainer):
    from facet_graph_convolution_amd import train as T
    fn = getattr(T, trainer)
    V, F = icosphere(2)
    plain = TrainingSet()
    plain.addMeshWithVerticesAndGT(V, F, V, seed=0)
    normals_only = TrainingSet()
    normals_only.addCleanMesh(V, F, seed=0)                  # clean, but without the vertex data
    for ds in (plain, normals_only):
        with pytest.raises(ValueError):
            fn(ds, 1, noise_levels=(0.1, 0.2), log=lambda s: None)
    clean = TrainingSet()
    clean.addCleanMeshWithVertices(V, F, seed=0)
    with pytest.raises(ValueError):
        fn(clean, 1, noise_levels=(), log=lambda s: None)
    with pytest.raises(ValueError):
        fn(clean, 1, noise_levels=(0.1, -0.1), log=lambda s: None)
    with pytest.raises(ValueError):
        fn(clean, 1, noise_levels=(0.1,), noise_direction="sideways", log=lambda s: None)
    with pytest.raises(ValueError):
        fn(clean, 1, noise_levels=(0.1,), validSet=plain, log=lambda s: None)
