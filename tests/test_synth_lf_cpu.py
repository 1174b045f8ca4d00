"""CPU checks of the low-frequency noise synthesis (include/fgc.h: fgc_synth_noise_lf): control-word bit patterns, the
amplitude formula, the refusals of the C entry point before any launch, the command lines, the ABI version and the
random stream of the training loops.  No GPU compute here."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lf_noise_cases as lf  # noqa: E402

from facet_graph_convolution_amd import _lib, ops
from facet_graph_convolution_amd.dataClasses import TrainingSet
from facet_graph_convolution_amd.meshgen import icosphere, torus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_version_triple():
    hdr = open(os.path.join(ROOT, "include", "fgc.h")).read()
    assert _lib.lib().fgc_version() == _lib.ABI_VERSION == int(re.search(r"#define FGC_ABI_VERSION (\d+)", hdr).group(1))
    assert _lib.ABI_VERSION >= 114
    assert _lib.SYNTH_LF_MAX_BUMPS == 1 << int(re.search(r"#define FGC_SYNTH_LF_MAX_BUMPS \(1 << (\d+)\)", hdr).group(1))


def test_lf_words_bit_patterns():
    assert ops.lf_words(None, 3.0).dtype == np.uint32 and ops.lf_words(None, None).tolist() == [0, 0, 0, 0]
    w = ops.lf_words(1.0, 0.5)
    assert w.dtype == np.uint32 and w.tolist() == [0x80000000 | 0x3F800000, 0x3F000000, 0, 0]
    assert ops.lf_words(0.0, 2.0).tolist() == [0x80000000, 0x40000000, 0, 0]          # amplitude 0 is ON
    assert ops.lf_words(-0.0, 2.0).tolist() == [0x80000000, 0x40000000, 0, 0]
    a = np.float32(0.0123)
    assert ops.lf_words(a, 7)[0] == (int(np.array([a]).view(np.uint32)[0]) | 0x80000000)
    for amp, width in ((-1.0, 1.0), (np.nan, 1.0), (np.inf, 1.0), (1.0, 0.0), (1.0, -2.0), (1.0, np.nan), (1.0, np.inf)):
        with pytest.raises(ValueError):
            ops.lf_words(amp, width)


def test_amplitude_formula():
    # dense: the planar shot-noise variance A^2 (K / area) pi w^2 equals (level * edge)^2
    level, edge, w, K, area = 0.3, 0.05, 0.15, 3000, 12.0
    A = ops.lf_amplitude(level, edge, w, K, area)
    assert K * np.pi * w * w / area > 1
    assert np.isclose(A * A * (K / area) * np.pi * w * w, (level * edge) ** 2, rtol=1e-12)
    # sparse: less than one bump per pi w^2 - the peak is the level
    assert ops.lf_amplitude(level, edge, w, 10, area) == level * edge
    assert ops.lf_amplitude(0.0, edge, w, K, area) == 0.0


def test_lf_plan():
    V, F = icosphere(3)
    K, width, area = ops.lf_plan(V, F, 0.2, 3.0, None)
    assert K == -(-len(F) // 6) == 214 and np.isclose(width, 0.6)
    assert 0.9 * 4 * np.pi < area < 4 * np.pi          # an inscribed polyhedron of the unit sphere
    assert ops.lf_plan(V, F, 0.2, 1.0, 17)[0] == 17
    for width_rel, bumps in ((0.0, None), (-1.0, None), (np.nan, None), (3.0, 0), (3.0, _lib.SYNTH_LF_MAX_BUMPS + 1)):
        with pytest.raises(ValueError):
            ops.lf_plan(V, F, 0.2, width_rel, bumps)


def test_the_level_gives_the_rms_it_names():
    """The float64 oracle with the host's amplitude: the RMS of the field over the vertices is the level x edge length
    within a factor of 2.  The formula is the planar shot-noise variance and one draw on a small closed mesh scatters
    around it (single numpy draws gave 0.99 ... 1.30 on six meshes); here about 15 bumps overlap (K pi w^2 / area), so a
    formula without the density term, or with the density instead of its root, is off by a factor of 3.5 or more."""
    from facet_graph_convolution_amd.utils import getAverageEdgeLength
    V, F = torus(60, 50)
    edge = float(getAverageEdgeLength(V, F)[0])
    K, width, area = ops.lf_plan(V, F, edge, 3.0, None)
    A = ops.lf_amplitude(0.3, edge, width, K, area)
    c, a = lf.bump_table(len(V), K, 0, 5, 0, A)
    s, _ = lf.field(V, c, a, width)
    ratio = np.sqrt((s * s).mean()) / (0.3 * edge)
    print("torus(60,50), K = %d, width 3 edges: RMS / (level x edge) = %.3f" % (K, ratio))
    assert 12.5 < K * np.pi * width ** 2 / area < 18
    assert 0.5 < ratio < 2.0


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
    nv, K = 1000, 300
    need = L.fgc_synth_lf_scratch_floats(nv, K)
    assert need >= L.fgc_synth_scratch_floats(nv) + 4 * K
    assert L.fgc_synth_lf_scratch_floats(nv, 0) == 0 and L.fgc_synth_lf_scratch_floats(0, K) == 0
    assert L.fgc_synth_lf_scratch_floats(nv, _lib.SYNTH_LF_MAX_BUMPS + 1) == 0
    # more bumps or more vertices never need less
    assert L.fgc_synth_lf_scratch_floats(nv, 5000) > need and L.fgc_synth_lf_scratch_floats(100000, K) > need
    names = ("v", "vn", "wn", "nv", "ctl", "lf", "K", "seed", "stream", "vo", "sc", "scf", "st")
    base = dict(v=p, vn=q[0], wn=None, nv=nv, ctl=q[1], lf=q[2], K=K, seed=1, stream=0, vo=q[3], sc=q[4], scf=need, st=None)
    f = lambda **kw: L.fgc_synth_noise_lf(*[kw.get(k, base[k]) for k in names])  # noqa: E731
    for k in ("v", "vn", "ctl", "lf", "vo", "sc"):
        _rejects(f(**{k: None}), "fgc_synth_noise_lf: null pointer")
    _rejects(f(nv=0), "nv=0")
    _rejects(f(K=0), "n_bumps=0")
    _rejects(f(K=_lib.SYNTH_LF_MAX_BUMPS + 1), "n_bumps=")
    _rejects(f(stream=0x80000000), "stream_id=2147483648")
    _rejects(f(stream=0xFFFFFFFF), "stream_id=")
    _rejects(f(vo=p), "must be distinct")
    _rejects(f(scf=need - 1), "scratch too small")
    _rejects(f(sc=C.c_void_p(q[4].value + 4)), "16-byte aligned")


def test_lf_noise_command_line(tmp_path, capsys):
    from facet_graph_convolution_amd import train as T
    assert T.parse_lf_noise("0.3", 3) == dict(lf_levels=(0.3, 0.3, 0.3), lf_width=3.0, lf_bumps=None)
    assert T.parse_lf_noise("0.3,0.2,0.1:2.5", 3) == dict(lf_levels=(0.3, 0.2, 0.1), lf_width=2.5, lf_bumps=None)
    assert T.parse_lf_noise("0.3:4:100", 1) == dict(lf_levels=(0.3,), lf_width=4.0, lf_bumps=100)
    for bad, n in (("0.3,0.2", 3), ("-0.1", 1), ("abc", 1), ("0.3:0", 1), ("0.3:3:0", 1), ("0.3:3:1:1", 1), ("0.3:3:1.5", 1),
                   ("nan", 1)):
        with pytest.raises(ValueError):
            T.parse_lf_noise(bad, n)
    dump = tmp_path / "dump"
    dump.mkdir()
    with pytest.raises(SystemExit) as e:
        T.main([str(dump), str(tmp_path / "net"), "--lf-noise", "0.3"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--synth-noise 0" in err, err
    for bad in ("0.3,0.2", "0.3:-1", "x"):
        with pytest.raises(SystemExit) as e:
            T.main([str(dump), str(tmp_path / "net"), "--synth-noise", "0.1", "--lf-noise", bad])
        assert e.value.code == 2 and "--lf-noise" in capsys.readouterr().err
    # well-formed: the run gets as far as asking for the clean pickle
    with pytest.raises(SystemExit) as e:
        T.main([str(dump), str(tmp_path / "net"), "--synth-noise", "0,0.1", "--lf-noise", "0.3,0.2:3"])
    assert e.value.code == 2 and "trainingSetClean.pkl" in capsys.readouterr().err


def test_make_noisy_command_line(tmp_path, capsys):
    from facet_graph_convolution_amd import makeNoisy
    from facet_graph_convolution_amd import train as T
    assert makeNoisy.pair_lf_levels(["0.3"], 3) == (0.3, 0.3, 0.3)
    assert makeNoisy.pair_lf_levels((0.3, 0.2), 2) == (0.3, 0.2)
    assert T.pair_lf_levels is makeNoisy.pair_lf_levels          # one check for the trainers and the command line
    clean = tmp_path / "clean"
    clean.mkdir()
    for argv in (["--levels", "0,0.1", "--lf-levels", "0.3,0.2,0.1"], ["--lf-levels", "-0.3"], ["--lf-levels", "abc"],
                 ["--lf-levels", "0.3", "--lf-width", "0"], ["--lf-levels", "0.3", "--lf-bumps", "0"]):
        with pytest.raises(SystemExit) as e:
            makeNoisy.main([str(clean), str(tmp_path / "out")] + argv)
        assert e.value.code == 2 and "--lf-" in capsys.readouterr().err, argv


@pytest.mark.parametrize("trainer", ["trainNet", "trainAccuracyNet", "trainDoubleLossNet"])
def test_trainers_check_lf_levels(trainer):
    from facet_graph_convolution_amd import train as T
    V, F = icosphere(2)
    clean = TrainingSet()
    (clean.addCleanMesh if trainer == "trainNet" else clean.addCleanMeshWithVertices)(V, F, seed=0)
    fn = getattr(T, trainer)
    quiet = dict(log=lambda s: None)
    with pytest.raises(ValueError, match="lf_levels needs noise_levels"):
        plain = TrainingSet()
        (plain.addMeshWithGT if trainer == "trainNet" else plain.addMeshWithVerticesAndGT)(V, F, V, seed=0)
        fn(plain, 1, lf_levels=(0.3,), **quiet)
    with pytest.raises(ValueError, match="lf_levels: one level"):
        fn(clean, 1, noise_levels=(0.0, 0.1, 0.2), lf_levels=(0.3, 0.2), **quiet)
    with pytest.raises(ValueError, match="lf_levels: one level"):
        fn(clean, 1, noise_levels=(0.0,), lf_levels=(-0.3,), **quiet)
    with pytest.raises(ValueError, match="lf_width"):
        fn(clean, 1, noise_levels=(0.0,), lf_levels=(0.3,), lf_width=0.0, **quiet)
    with pytest.raises(ValueError, match="lf_bumps"):
        fn(clean, 1, noise_levels=(0.0,), lf_levels=(0.3,), lf_bumps=0, **quiet)


def test_draw_step_consumes_the_same_draws_with_and_without_lf_levels():
    from facet_graph_convolution_amd import train as T
    F = types.SimpleNamespace(samples=500)
    m = T._Mesh((), None, (642, 642))
    levels, lf_levels = (0.0, 0.1, 0.2), (0.3, 0.2, 0.1)
    a, b = np.random.RandomState(11), np.random.RandomState(11)
    for counter in range(20):
        sa, Ra, na = T._draw_step(a, F, m, levels, counter)
        sb, Rb, nb = T._draw_step(b, F, m, levels, counter, lf_levels)
        assert all(np.array_equal(x, y) for x, y in zip(sa, sb)) and np.array_equal(Ra, Rb)
        assert nb[:2] == na and len(nb) == 3 and nb[2] == lf_levels[levels.index(na[1])]      # the same draw picks the pair
        sta, stb = a.get_state(), b.get_state()
        assert sta[0] == stb[0] and np.array_equal(sta[1], stb[1]) and sta[2:] == stb[2:]
    # and the plain mode draws no level at all, as before
    c, d = np.random.RandomState(3), np.random.RandomState(3)
    assert T._draw_step(c, F, m, None, 0)[2] is None
    T._draw_samples(d, F, m), d.uniform(size=3)
    assert np.array_equal(c.get_state()[1], d.get_state()[1]) and c.get_state()[2] == d.get_state()[2]
