"""CPU checks of training from clean meshes (noise synthesised per step on the GPU): the random-number definition, the
clean training set, the packed step inputs and the command lines.  No GPU compute here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_cases as sc  # noqa: E402

from facet_graph_convolution_amd.dataClasses import TrainingSet
from facet_graph_convolution_amd.meshgen import icosphere


def test_philox_known_answers():
    for counter, key, want in sc.KNOWN_ANSWERS:
        got = sc.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], key)
        assert tuple(int(g[0]) for g in got) == want, [hex(int(g[0])) for g in got]


def test_uniforms_are_never_0_or_1_and_u_or_its_complement_is_exact_in_fp32():
    """u = ((x >> 8) + 0.5) 2^-24 needs 25 bits: exact in fp32 below 1/2 only; above, 1 - u is (what the kernel feeds
    log1pf and the angle with).  The largest u ROUNDS to 1.0 in fp32."""
    for x in (0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):
        u = ((x >> 8) + 0.5) * 2.0 ** -24
        assert 0.0 < u < 1.0
        exact = u if (x >> 8) < (1 << 23) else 1.0 - u
        assert float(np.float32(exact)) == exact
    assert float(np.float32(((0xFFFFFFFF >> 8) + 0.5) * 2.0 ** -24)) == 1.0


def test_noise_words_layout():
    from facet_graph_convolution_amd import ops, _lib
    w = ops.noise_words((5 << 32) | 7, 0.25)
    assert w.dtype == np.uint32 and list(w) == [7, 5, 0x80000000 | 0x3E800000] and _lib.SYNTH_ON == 0x80000000
    assert list(ops.noise_words(3, 0.0)) == [3, 0, 0x80000000]       # level 0 is ON: the clean input is rebuilt
    assert list(ops.noise_words(3, None)) == [0, 0, 0]               # off
    with pytest.raises(ValueError):
        ops.noise_words(0, -1.0)


def test_add_clean_mesh_matches_add_mesh_with_gt():
    V, F = icosphere(3)
    a, b = TrainingSet(), TrainingSet()
    a.addCleanMesh(V, F, seed=5)
    b.addMeshWithGT(V, F, V, seed=5)
    assert a.is_clean() and not b.is_clean()
    assert np.array_equal(a.in_list[0], b.in_list[0]) and np.array_equal(a.gt_list[0], b.gt_list[0])
    assert len(a.adj_list[0]) == 3 and all(np.array_equal(p, q) for p, q in zip(a.adj_list[0], b.adj_list[0]))
    rows = a.clean_faces_rows[0]
    n0 = a.in_list[0].shape[1]
    assert rows.dtype == np.int32 and rows.shape == (1, n0, 3) and a.clean_vertices[0].dtype == np.float32
    assert np.array_equal(a.clean_vertices[0][0], V)
    fake = np.abs(a.in_list[0][0]).sum(1) == 0
    assert fake.sum() == n0 - F.shape[0]
    assert np.array_equal((rows[0] == -1).all(1), fake) and np.array_equal((rows[0] < 0).any(1), fake)
    # mapped back through the permutation: the input faces, then the padding
    back = rows[0][np.asarray(a.permutations[0])]
    assert np.array_equal(back[:F.shape[0]], F.astype(np.int32)) and (back[F.shape[0]:] == -1).all()
    from facet_graph_convolution_amd.utils import getAverageEdgeLength
    assert a.clean_edge_len == [float(getAverageEdgeLength(V, F)[0])]


def test_add_clean_mesh_refuses_patch_mode():
    V, F = icosphere(3)
    ds = TrainingSet(maxSize=1000)
    with pytest.raises(NotImplementedError):
        ds.addCleanMesh(V, F)
    assert ds.mesh_count == 0


def test_area_weighted_vertex_normals():
    from facet_graph_convolution_amd.utils import areaWeightedVertexNormals
    V, F = icosphere(3)
    n = areaWeightedVertexNormals(V, F)
    assert n.shape == V.shape and np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-12)
    assert (n * V).sum(1).min() > 0.999            # a sphere's normals point along its vertices
    assert np.allclose(n, sc.vertex_normals(V, F), atol=1e-12)


def test_pack_step_inputs_default_rows_are_unchanged():
    """The rows bench.py builds: without noise= the three spare words stay zero; with it they hold the control words."""
    from facet_graph_convolution_amd.net import FacetDenoiser
    from facet_graph_convolution_amd import ops
    rs = np.random.RandomState(0)
    S = [rs.randint(100, size=16) for _ in range(3)]
    R = [rs.normal(size=(3, 3)) for _ in range(3)]
    rows = FacetDenoiser.pack_step_inputs(S, R, "cpu").numpy()
    want = np.zeros((3, 28), dtype=np.int32)
    want[:, :16] = np.stack(S)
    want[:, 16:25] = np.stack([np.asarray(r, dtype=np.float32).reshape(9) for r in R]).view(np.int32)
    assert rows.dtype == np.int32 and np.array_equal(rows, want)
    assert np.array_equal(FacetDenoiser.pack_step_inputs(S, R, "cpu", noise=None).numpy(), want)
    noisy = FacetDenoiser.pack_step_inputs(S, R, "cpu", noise=[(9, 0.5), None, (1 << 40, 0.0)]).numpy()
    assert np.array_equal(noisy[:, :25], want[:, :25]) and not noisy[1, 25:].any()
    assert np.array_equal(noisy[0, 25:].view(np.uint32), ops.noise_words(9, 0.5))
    assert np.array_equal(noisy[2, 25:].view(np.uint32), ops.noise_words(1 << 40, 0.0))
    with pytest.raises(ValueError):
        FacetDenoiser.pack_step_inputs(S, R, "cpu", noise=[(0, 0.1)])


def test_preprocess_clean_arguments(tmp_path, capsys):
    from facet_graph_convolution_amd import preprocess
    from facet_graph_convolution_amd.utils import write_mesh
    clean = tmp_path / "clean"
    clean.mkdir()
    for argv in ([str(clean), str(tmp_path / "a"), str(tmp_path / "b"), "--clean"],       # three folders with --clean
                 [str(clean), str(tmp_path / "a"), "--clean", "--with-vertices"],
                 [str(clean), str(tmp_path / "a")],                                         # two folders without it
                 [str(clean), str(tmp_path / "a"), "--clean"]):                             # no OBJ file there
        with pytest.raises(SystemExit) as e:
            preprocess.main(argv)
        assert e.value.code == 2, argv
    V, F = icosphere(2)
    write_mesh(V, F, str(clean / "ball.obj"))
    capsys.readouterr()
    preprocess.main([str(clean), str(tmp_path / "dump"), "--clean", "--valid", str(clean), "--redundancy", "2"])
    assert sorted(os.listdir(tmp_path / "dump")) == ["trainingSetClean.pkl", "validSetClean.pkl"]
    import pickle
    with open(tmp_path / "dump" / "trainingSetClean.pkl", "rb") as fp:
        ds = pickle.load(fp)
    assert ds.is_clean() and ds.mesh_count == 2 and ds.clean_faces_rows[1].shape[1] == ds.in_list[1].shape[1]


def test_train_synth_noise_arguments(tmp_path):
    from facet_graph_convolution_amd import train as T
    dump = tmp_path / "dump"
    dump.mkdir()
    for argv in ([str(dump), str(tmp_path / "net"), "--synth-noise", "0.1", "--with-vertices"],
                 [str(dump), str(tmp_path / "net"), "--synth-noise", "0.1,abc"],
                 [str(dump), str(tmp_path / "net"), "--synth-noise", "0.1,-0.2"],
                 [str(dump), str(tmp_path / "net"), "--synth-noise", "0.1", "--noise-direction", "sideways"],
                 [str(dump), str(tmp_path / "net"), "--synth-noise"]):                     # no trainingSetClean.pkl
        with pytest.raises(SystemExit) as e:
            T.main(argv)
        assert e.value.code == 2, argv
    assert T.DEFAULT_NOISE_LEVELS == (0.1, 0.2, 0.3)


def test_train_net_with_noise_levels_needs_a_clean_set():
    from facet_graph_convolution_amd import train as T
    V, F = icosphere(2)
    plain = TrainingSet()
    plain.addMeshWithGT(V, F, V, seed=0)
    for levels in ((0.1, 0.2), ()):
        with pytest.raises(ValueError):
            T.trainNet(plain, 1, noise_levels=levels, log=lambda s: None)
    clean = TrainingSet()
    clean.addCleanMesh(V, F, seed=0)
    with pytest.raises(ValueError):
        T.trainNet(clean, 1, noise_levels=(0.1,), noise_direction="sideways", log=lambda s: None)
