"""CPU checks of the depth-scan mode: the float64 restatement the GPU tests use as their oracle against the fixtures made
by running the reference's update_position_with_depth (tests/golden/gen/make_golden_depth.py), the argument checks of
fgc_vertex_update_dir (before any launch), utils.view_rays, the CLIs' parsing and the checks of a direction table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from facet_graph_convolution_amd import _lib, utils

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_cases as dc  # noqa: E402


@pytest.mark.parametrize("tag", dc.CASES)
def test_restatement_equals_the_reference_in_float64(golden_dir, tag):
    """The t form (position = input + t d) is the reference's chain of additions in exact arithmetic: 1e-12 in float64
    (measured 2e-15).  The fixtures hold what the issue lists, arrays only, 50 slots per vertex."""
    z, z64 = dc.load(golden_dir, tag)
    for f in (z, z64):
        assert {"verts", "faces", "normals", "edge_map", "v_e_map", "dirs", "x_1", "x_60", "dx_1", "dx_60"} <= set(f.files)
        assert all(f[k].dtype != object for k in f.files)
    assert z["v_e_map"].shape[1] == 50 and z["dirs"].shape[0] in (1, z["verts"].shape[0])
    assert z["x_60"].dtype == np.float32 and z64["x_60"].dtype == np.float64
    for k in ("verts", "normals", "edge_map", "v_e_map", "dirs"):
        assert np.array_equal(z[k], z64[k])
    for it in (1, 60):
        x, t = dc.restate(z["verts"], z["normals"], z["edge_map"], z["v_e_map"], z["dirs"], it)
        err = np.abs(x - z64["x_%d" % it]).max()
        errd = np.abs((x - z["verts"].astype(np.float64)) - z64["dx_%d" % it]).max()
        print("%s, %d iterations: |restatement - reference f64| %.2e (dx %.2e)" % (tag, it, err, errd))
        assert err <= 1e-12 and errd <= 1e-12
    # zero iterations: the input, t = 0
    x, t = dc.restate(z["verts"], z["normals"], z["edge_map"], z["v_e_map"], z["dirs"], 0)
    assert np.array_equal(x, z["verts"].astype(np.float64)) and not t.any()


def test_abi_version_is_116():
    assert _lib.lib().fgc_version() == 116 == _lib.ABI_VERSION
    assert _lib.lib().fgc_vertex_update_dir_workspace_floats(0) == 0
    assert _lib.lib().fgc_vertex_update_dir_workspace_floats(1000) >= 3000


def test_argument_checks_answer_einval_before_any_launch():
    """Every call below must return FGC_EINVAL from the host checks: the pointers are made-up addresses nobody may touch."""
    L = _lib.lib()
    nv, nf, ne, slots = 100, 196, 294, 20
    need = L.fgc_vertex_update_dir_workspace_floats(nv)
    P = lambda k: C.c_void_p(0x10000 * (k + 1))  # noqa: E731
    good = dict(x=P(0), x_out=P(1), t_out=P(2), ws=P(3), ws_floats=need, nv=nv, normals=P(4), nf=nf, e_map=P(5), ne=ne,
                v_e_map=P(6), max_edges=slots, dirs=P(7), n_dirs=nv, iters=3, lmbd=1.0 / 18, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return L.fgc_vertex_update_dir(a["x"], a["x_out"], a["t_out"], a["ws"], a["ws_floats"], a["nv"], a["normals"],
                                       a["nf"], a["e_map"], a["ne"], a["v_e_map"], a["max_edges"], a["dirs"], a["n_dirs"],
                                       a["iters"], a["lmbd"], a["stream"])
    for name in ("x", "x_out", "ws", "normals", "e_map", "v_e_map", "dirs"):
        assert call(**{name: None}) == -22, name
        assert b"fgc_vertex_update_dir" in L.fgc_last_error()
    for n_dirs in (0, 2, nv - 1, nv + 1, -1):
        assert call(n_dirs=n_dirs) == -22, n_dirs
    assert b"n_dirs" in L.fgc_last_error()
    assert call(iters=-1) == -22
    assert call(x_out=good["x"]) == -22
    assert call(ws=good["x"]) == -22
    assert call(ws_floats=need - 1) == -22 and b"workspace" in L.fgc_last_error()
    assert call(ws_floats=0) == -22
    assert call(nv=0, n_dirs=0) == -22 and call(max_edges=0) == -22


def test_view_rays():
    V = np.random.RandomState(0).standard_normal((300, 3)).astype(np.float32)
    r = utils.view_rays(V, camera=(0.3, -0.2, 4.0))
    assert r.dtype == np.float32 and r.shape == (300, 3)
    assert np.abs(np.linalg.norm(r.astype(np.float64), axis=1) - 1).max() < 1e-6
    want = V.astype(np.float64) - np.array([0.3, -0.2, 4.0])
    assert np.abs(r - want / np.linalg.norm(want, axis=1, keepdims=True)).max() < 1e-7
    assert utils.view_rays(V, camera=(0.3, -0.2, 4.0)).tobytes() == r.tobytes()
    d = utils.view_rays(V, view_dir=(0, 3, 4))
    assert d.dtype == np.float32 and d.shape == (1, 3) and np.array_equal(d, np.array([[0, 0.6, 0.8]], dtype=np.float32))
    assert utils.view_rays(V, view_dir=(0, 3, 4)).tobytes() == d.tobytes()
    with pytest.raises(ValueError, match="exactly one"):
        utils.view_rays(V)
    with pytest.raises(ValueError, match="exactly one"):
        utils.view_rays(V, camera=(0, 0, 1), view_dir=(0, 0, 1))
    with pytest.raises(ValueError, match="at the camera"):
        utils.view_rays(V, camera=V[17])
    with pytest.raises(ValueError):
        utils.view_rays(V, view_dir=(0, 0, 0))


def test_cli_parsing_refuses_contradictions(tmp_path, capsys):
    from facet_graph_convolution_amd import bilateral, infer, makeNoisy, train
    d = str(tmp_path)
    cases = [
        (bilateral, [d, d, "--view-dir", "0,0,1", "--camera", "0,0,5"], "not allowed with"),
        (infer, [d, d, "net.pt", "--view-dir", "0,0,1", "--camera", "0,0,5"], "not allowed with"),
        (infer, [d, d, "net.pt", "--with-vertices", "--view-dir", "0,0,1"], "no ray-constrained form"),
        (infer, [d, d, "net.pt", "--with-vertices", "--camera", "0,0,5"], "no ray-constrained form"),
        (makeNoisy, [d, d, "--direction", "ray"], "needs --view-dir or --camera"),
        (makeNoisy, [d, d, "--direction", "ray", "--view-dir", "0,0,1", "--camera", "0,0,5"], "not allowed with"),
        (makeNoisy, [d, d, "--camera", "0,0,5"], "--direction ray"),
        (train, [d, d, "--synth-noise", "0.1", "--noise-direction", "ray"], "needs --view-dir or --camera"),
        (train, [d, d, "--noise-direction", "ray", "--camera", "0,0,5"], "needs --synth-noise"),
        (bilateral, [d, d, "--view-dir", "0,0"], "X,Y,Z"),
        (bilateral, [d, d, "--view-dir", "0,0,0"], "zero vector"),
    ]
    for mod, argv, msg in cases:
        with pytest.raises(SystemExit) as e:
            mod.main(argv)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err, (mod.__name__, argv)


def test_direction_tables_are_checked():
    """Before anything reaches the GPU: make_noisy, the synthesis state of bind_clean / bind_clean_vertices and the
    trainers refuse a table with the wrong row count, a NaN, or a row of norm 0.5."""
    from facet_graph_convolution_amd import makeNoisy
    from facet_graph_convolution_amd import train as T
    from facet_graph_convolution_amd.meshgen import icosphere
    from facet_graph_convolution_amd.synth import NoiseSpec, SynthState
    V, F = icosphere(1)
    V = V.astype(np.float32)
    rays = utils.view_rays(V, camera=(0, 0, 5))
    nan, half = rays.copy(), rays.copy()
    nan[3, 1] = np.nan
    half[5] *= 0.5
    bad = [(rays[:-1], "one row per vertex"), (nan, "finite"), (half, "unit")]
    assert utils.check_directions(rays, V.shape[0]).tobytes() == rays.tobytes()
    near = rays * np.float32(1.0005)
    utils.check_directions(near, V.shape[0])           # within 1e-3 of 1
    x = np.zeros((1, F.shape[0], 6), dtype=np.float32)
    for d, msg in bad:
        with pytest.raises(ValueError, match=msg):
            utils.check_directions(d, V.shape[0])
        with pytest.raises(ValueError, match=msg):
            makeNoisy.make_noisy(V, F, 0.1, direction=d)
        with pytest.raises(ValueError, match=msg):
            SynthState(NoiseSpec(0, 0, d), x, V, F, 0.1, "cpu")      # (what bind_clean builds: refused before any device work)
    with pytest.raises(ValueError, match="direction must be"):
        makeNoisy.make_noisy(V, F, 0.1, direction="sideways")
    # the key two binds are compared by: hashable, equal for equal rows, different otherwise
    k = utils.direction_key(rays)
    assert k == utils.direction_key(rays.copy()) and hash(k) is not None and k[0] == "rays"
    assert k != utils.direction_key(utils.view_rays(V, camera=(0, 0, 6)))
    assert utils.direction_key("normal") == "normal"
    with pytest.raises(ValueError, match="a view is"):
        T._trainer_inputs("angular", None, None, (0.1,), {"eye": (0, 0, 1)})
