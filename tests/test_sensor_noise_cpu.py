"""CPU checks of the depth-sensor noise model (include/fgc.h: fgc_synth_noise_sensor): the float64 oracle against the plain
one, utils.sensor_model by hand, the control words, the refusals of the C entry point before any launch, of the trainers and
of the two command lines.  No GPU compute here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sensor_noise_cases as sn  # noqa: E402
import synth_cases as sc  # noqa: E402

from facet_graph_convolution_amd import _lib, ops, utils
from facet_graph_convolution_amd.dataClasses import TrainingSet
from facet_graph_convolution_amd.meshgen import icosphere


def test_oracle_without_the_model_is_the_plain_oracle_on_the_rays():
    """power 0, quant 0: V + d sigma z3 - synth_cases.oracle with the table of rays in the place of the vertex normals."""
    for tag in ("ico3", "flipped"):
        V, F = sn.mesh(tag)
        rays = utils.view_rays(V, camera=sn.CAMERA)
        z = sc.gaussians(V.shape[0], 7, sn.SEED, 0)
        plain = V.astype(np.float64) + rays.astype(np.float64) * (0.01 * z[:, 3:4])
        got, k, x, through = sn.oracle(V, rays, sn.CAMERA, 0.01, 7, sn.SEED, 0, 0, 2.7, 0.0)
        assert np.array_equal(got, plain) and k is None and x is None and not through.any()
        # ... and synth_cases.oracle itself, fed these rays as its direction
        keep = sc.vertex_normals
        sc.vertex_normals = lambda V_, F_: rays.astype(np.float64)
        try:
            assert np.array_equal(got, sc.oracle(V, F, 0.01, 7, sn.SEED, 0, "normal"))
        finally:
            sc.vertex_normals = keep


def test_oracle_robust_vertices_are_nearly_all():
    """The condition of the quantised GPU test, on the oracle alone at the far larger margin 1e-3: at most 1 % of the
    vertices lie that close to a half-integer disparity, and no sample reaches rt <= 0."""
    for tag in ("ico3", "flipped"):
        V, F = sn.mesh(tag)
        edge = utils.getAverageEdgeLength(V, F)[0]
        rays = utils.view_rays(V, camera=sn.CAMERA)
        for quant in sn.QUANTS:
            m = utils.sensor_model(V, sn.CAMERA, edge, 2, quant)
            for level in sn.LEVELS:
                near = 0
                for step in sn.STEPS:
                    _, k, x, through = sn.oracle(V, rays, m.camera, level * edge, step, sn.SEED, 0, 2, m.r_ref, m.q)
                    near += int((np.abs(np.abs(x - np.floor(x)) - 0.5) <= 1e-3).sum())
                    assert not through.any() and k.min() >= 1 and k.max() < sn.K_MAX
                print("%s quant %.1f level %.1f: %d of %d within 1e-3 of a half-integer" % (tag, quant, level, near, 3 * len(V)))
                assert near <= 0.01 * 3 * len(V)


def test_sensor_model_by_hand():
    V = np.array([[0.0, 0.0, 0.0], [2.0, 4.0, 4.0]], dtype=np.float32)      # box centre (1, 2, 2)
    m = utils.sensor_model(V, (1.0, 2.0, 5.0), 0.25, power=2, quant=2.0)
    assert m == utils.SensorModel(2, 3.0, float(np.float32(2.0 * 0.25 / 9.0)), (1.0, 2.0, 5.0))
    m = utils.sensor_model(V, (4.0, 6.0, 2.0), 0.5)                          # defaults: power 2, no quantisation
    assert (m.power, m.r_ref, m.q) == (2, 5.0, 0.0)
    m = utils.sensor_model(V, (4.0, 6.0, 2.0), 0.5, power=1, quant=0.5, ref_range=2.0)
    assert (m.power, m.r_ref, m.q) == (1, 2.0, 0.0625)
    # the distance is rounded to fp32 once, q is taken from the rounded value
    m = utils.sensor_model(V, (1.1, 2.0, 2.0), 1.0, quant=1.0)
    r = np.float32(abs(1.1 - 1.0))
    assert m.r_ref == float(r) and m.q == float(np.float32(1.0 / float(r) ** 2))
    for kw, text in ((dict(power=3), "power"), (dict(power=1.5), "power"), (dict(power=-1), "power"), (dict(quant=-0.5), "quant"),
                     (dict(quant=np.nan), "quant"), (dict(ref_range=0.0), "reference range"),
                     (dict(ref_range=np.inf), "reference range")):
        with pytest.raises(ValueError, match="sensor.*" + text):
            utils.sensor_model(V, (4.0, 6.0, 2.0), 0.5, **kw)
    with pytest.raises(ValueError, match="sensor.*reference range"):
        utils.sensor_model(V, (1.0, 2.0, 2.0), 0.5)                          # the camera at the centre of the box
    with pytest.raises(ValueError, match="sensor.*camera"):
        utils.sensor_model(V, None, 0.5)
    assert utils.parse_sensor("2") == (2, 0.0) and utils.parse_sensor("1:0.5") == (1, 0.5) and utils.parse_sensor("0:2") == (0, 2.0)
    for bad in ("3", "2:-1", "x", "2:", ":1", "1:2:3", "1.5", "2:nan"):
        with pytest.raises(ValueError):
            utils.parse_sensor(bad)


def test_sensor_words_bit_patterns():
    assert ops.sensor_words(None, 1.0, 0.0).dtype == np.uint32 and ops.sensor_words(None, None, None).tolist() == [0, 0, 0, 0]
    assert ops.sensor_words(2, 1.0, 0.5).tolist() == [0x80000002, 0x3F800000, 0x3F000000, 0]
    assert ops.sensor_words(0, 2.0, 0.0).tolist() == [0x80000000, 0x40000000, 0, 0]        # power 0 is ON
    assert ops.sensor_words(1, 2.0, -0.0).tolist() == [0x80000001, 0x40000000, 0, 0]
    for power, r_ref, q in ((3, 1.0, 0.0), (-1, 1.0, 0.0), (1.5, 1.0, 0.0), (2, 0.0, 0.0), (2, -1.0, 0.0), (2, np.inf, 0.0),
                            (2, np.nan, 0.0), (2, 1e-45, 0.0), (2, 1.0, -0.5), (2, 1.0, np.inf), (2, 1.0, np.nan),
                            (2, 1.0, 1e-45), (2, 1e39, 0.0)):
        with pytest.raises(ValueError, match="sensor"):
            ops.sensor_words(power, r_ref, q)


def _buf(n=1 << 16):
    b = (C.c_char * n)()
    return b, C.c_void_p((C.addressof(b) + 255) // 256 * 256)


def _rejects(rc, text):
    assert rc == -22, rc
    msg = _lib.lib().fgc_last_error()
    assert msg and text.encode() in msg, msg


def test_entry_point_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()
    keep, p = _buf()
    q = [C.c_void_p(p.value + 4096 * k) for k in range(1, 6)]
    nv = 1000
    need = L.fgc_synth_scratch_floats(nv)
    cam = (C.c_float * 3)(2.5, 0.4, 1.2)
    names = ("v", "dirs", "nv", "ctl", "sctl", "cam", "seed", "stream", "vo", "sc", "scf", "st")
    base = dict(v=p, dirs=q[0], nv=nv, ctl=q[1], sctl=q[2], cam=cam, seed=1, stream=0, vo=q[3], sc=q[4], scf=need, st=None)
    f = lambda **kw: L.fgc_synth_noise_sensor(*[kw.get(k, base[k]) for k in names])  # noqa: E731
    for k in ("v", "dirs", "ctl", "sctl", "cam", "vo", "sc"):
        _rejects(f(**{k: None}), "fgc_synth_noise_sensor: null pointer")
    _rejects(f(nv=0), "nv=0")
    _rejects(f(nv=-5), "nv=-5")
    _rejects(f(vo=p), "must be distinct")
    _rejects(f(scf=need - 1), "scratch too small")
    _rejects(f(cam=(C.c_float * 3)(2.5, float("nan"), 1.2)), "camera")
    _rejects(f(cam=(C.c_float * 3)(float("inf"), 0.4, 1.2)), "camera")


def _clean(trainer):
    V, F = icosphere(2)
    clean = TrainingSet()
    (clean.addCleanMesh if trainer == "trainNet" else clean.addCleanMeshWithVertices)(V, F, seed=0)
    return clean, V, F


@pytest.mark.parametrize("trainer", ["trainNet", "trainAccuracyNet", "trainDoubleLossNet"])
def test_trainers_check_sensor(trainer):
    """Before anything reaches the GPU, each message naming the option."""
    from facet_graph_convolution_amd import train as T
    clean, V, F = _clean(trainer)
    fn = getattr(T, trainer)
    quiet = dict(log=lambda s: None)
    cam = {"camera": sn.CAMERA}
    with pytest.raises(ValueError, match="sensor needs noise_levels"):
        plain = TrainingSet()
        (plain.addMeshWithGT if trainer == "trainNet" else plain.addMeshWithVerticesAndGT)(V, F, V, seed=0)
        fn(plain, 1, sensor=(2, 0.5), **quiet)
    with pytest.raises(ValueError, match="sensor.*view_dir"):
        fn(clean, 1, noise_levels=(0.1,), noise_direction={"view_dir": (0, 0, 1)}, sensor=(2, 0.5), **quiet)
    for direction in ("random", "normal", utils.view_rays(V, camera=sn.CAMERA)):
        with pytest.raises(ValueError, match="sensor needs a noise_direction"):
            fn(clean, 1, noise_levels=(0.1,), noise_direction=direction, sensor=(2, 0.5), **quiet)
    with pytest.raises(ValueError, match="sensor does not combine with lf_levels"):
        fn(clean, 1, noise_levels=(0.1,), noise_direction=cam, lf_levels=(0.3,), sensor=(2, 0.5), **quiet)
    with pytest.raises(ValueError, match="sensor: power"):
        fn(clean, 1, noise_levels=(0.1,), noise_direction=cam, sensor=(3, 0.5), **quiet)
    with pytest.raises(ValueError, match="sensor: quant"):
        fn(clean, 1, noise_levels=(0.1,), noise_direction=cam, sensor=(2, -0.5), **quiet)
    with pytest.raises(ValueError, match="sensor: a pair"):
        fn(clean, 1, noise_levels=(0.1,), noise_direction=cam, sensor=2, **quiet)


def test_the_model_is_resolved_per_mesh_from_the_view():
    from facet_graph_convolution_amd import train as T
    clean, V, F = _clean("trainNet")
    m = T._clean_meshes(clean, "training set")[0]
    got = T._mesh_sensor((2, 0.5), {"camera": sn.CAMERA}, m)
    assert got == utils.sensor_model(clean.clean_vertices[0], sn.CAMERA, clean.clean_edge_len[0], 2, 0.5)
    assert T._mesh_sensor((2, 0.5), {"camera": sn.CAMERA}, m) is got          # built once per mesh, view and setting
    centre = (np.asarray(V).min(0).astype(np.float64) + np.asarray(V).max(0).astype(np.float64)) / 2
    with pytest.raises(ValueError, match="sensor.*centre"):
        T._mesh_sensor((2, 0.5), {"camera": tuple(centre)}, m)


def test_train_command_line(tmp_path, capsys):
    from facet_graph_convolution_amd import train as T
    dump = tmp_path / "dump"
    dump.mkdir()
    head = [str(dump), str(tmp_path / "net"), "--synth-noise", "0.1"]
    ray = ["--noise-direction", "ray"]
    for argv, text in ((["--sensor", "2:0.5"] + ray, "--camera"),
                       (["--sensor", "2:0.5", "--view-dir", "0,0,1"] + ray, "--view-dir"),
                       (["--sensor", "2:0.5", "--noise-direction", "random"], "--noise-direction"),
                       (["--sensor", "2:0.5", "--noise-direction", "normal"], "--noise-direction"),
                       (["--sensor", "2:0.5", "--camera", "2.5,0.4,1.2", "--lf-noise", "0.3"] + ray, "--lf-noise"),
                       (["--sensor", "3", "--camera", "2.5,0.4,1.2"] + ray, "POWER is 0, 1 or 2"),
                       (["--sensor", "2:-1", "--camera", "2.5,0.4,1.2"] + ray, "QUANT must be >= 0"),
                       (["--sensor", "x", "--camera", "2.5,0.4,1.2"] + ray, "POWER")):
        with pytest.raises(SystemExit) as e:
            T.main(head + argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and "--sensor" in err and text in err, (argv, err)
    # well-formed: the run gets as far as asking for the clean pickle
    with pytest.raises(SystemExit) as e:
        T.main(head + ["--sensor", "2:0.5", "--camera", "2.5,0.4,1.2"] + ray)
    assert e.value.code == 2 and "trainingSetClean.pkl" in capsys.readouterr().err


def test_make_noisy_command_line(tmp_path, capsys):
    from facet_graph_convolution_amd import makeNoisy
    clean = tmp_path / "clean"
    clean.mkdir()
    ray = ["--direction", "ray"]
    for argv, text in ((["--sensor", "2:0.5"] + ray, "--camera"),
                       (["--sensor", "2:0.5", "--view-dir", "0,0,1"] + ray, "--view-dir"),
                       (["--sensor", "2:0.5", "--direction", "random"], "--direction"),
                       (["--sensor", "2:0.5", "--direction", "normal"], "--direction"),
                       (["--sensor", "2:0.5", "--camera", "2.5,0.4,1.2", "--lf-levels", "0.3"] + ray, "--lf-levels"),
                       (["--sensor", "3", "--camera", "2.5,0.4,1.2"] + ray, "POWER is 0, 1 or 2"),
                       (["--sensor", "2:-1", "--camera", "2.5,0.4,1.2"] + ray, "QUANT must be >= 0")):
        with pytest.raises(SystemExit) as e:
            makeNoisy.main([str(clean), str(tmp_path / "out")] + argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and "--sensor" in err and text in err, (argv, err)
    assert makeNoisy.main([str(clean), str(tmp_path / "out"), "--sensor", "2:0.5", "--camera", "2.5,0.4,1.2"] + ray) == []
