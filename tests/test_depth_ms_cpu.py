"""CPU checks of the ray-constrained multi-scale vertex update: the float64 restatement the GPU tests use as their oracle
(its t form against its x form, its autograd gradient against the per-iteration projected adjoint), the argument checks of
the three fgc_vertex_update_ms_dir entry points (before any launch), the CLIs' parsing and the binding's ABI check."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from facet_graph_convolution_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_ms_cases as mc  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(got, ref):
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


@pytest.mark.parametrize("kind", mc.DIR_SETS)
@pytest.mark.parametrize("its", mc.ITERS)
def test_t_form_equals_x_form_in_float64(golden_dir, its, kind):
    """x0 + t d against x + d (d . delta(x)): the same rule in exact arithmetic, 1e-12 in float64."""
    x, normals, faces, vf = mc.load(golden_dir, False)
    d = mc.directions(x, kind)
    with torch.no_grad():
        xt, t, dxt = mc.restate(x, normals, faces, vf, d, its, form="t")
        xx, t2, dxx = mc.restate(x, normals, faces, vf, d, its, form="x")
    err = max([(xt - xx).abs().max().item(), (t - t2).abs().max().item()] + [(a - b).abs().max().item()
                                                                              for a, b in zip(dxt, dxx)])
    print("%s %s: |t form - x form| %.2e, max |t| %.3e" % (its, kind, err, t.abs().max().item()))
    assert err <= 1e-12 and t.abs().max().item() > 1e-3
    # on the ray: the offset from the input is parallel to d
    off = xt - torch.as_tensor(x).double()
    dd = torch.as_tensor(np.broadcast_to(d, x.shape).astype(np.float64))
    assert torch.linalg.cross(off, dd).abs().max().item() <= 1e-15


@pytest.mark.parametrize("truncate", [False, True])
@pytest.mark.parametrize("kind", mc.DIR_SETS)
@pytest.mark.parametrize("its", mc.ITERS)
def test_autograd_equals_the_projected_adjoint(golden_dir, its, kind, truncate):
    """Autograd through the t form against the free adjoint with the incoming gradient projected where it enters delta,
    accumulated per iteration backwards over the trajectory: 1e-12 relative in float64."""
    x, normals, faces, vf = mc.load(golden_dir, truncate)
    d = mc.directions(x, kind)
    g_out = np.random.RandomState(7).standard_normal(x.shape)
    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    n64 = [torch.tensor(n, dtype=torch.float64, requires_grad=True) for n in normals]
    out = mc.restate(x64, n64, faces, vf, d, its)[0]
    (out * torch.tensor(g_out)).sum().backward()
    g_x, g_n = mc.projected_adjoint(x, normals, faces, vf, d, its, g_out)
    errs = [_rel(g_x, x64.grad)] + [_rel(g, n.grad) for g, n in zip(g_n, n64)]
    print("%s %s truncate=%s: rel err x %.2e n0 %.2e n1 %.2e n2 %.2e" % ((its, kind, truncate) + tuple(errs)))
    assert max(errs) <= 1e-12, errs


def test_vertex_without_faces_does_not_move_in_the_restatement(golden_dir):
    x, normals, faces, vf = mc.load(golden_dir, False)
    vf = vf.copy()
    vf[5] = -1
    with torch.no_grad():
        out, t, _ = mc.restate(x, normals, faces, vf, mc.directions(x, "camera"), (2, 1, 1))
    assert torch.equal(out[5], torch.as_tensor(x[5]).double()) and t[5] == 0 and torch.isfinite(out).all()


def test_abi_check_passes_and_the_new_entry_points_are_bound():
    """The new entry points are additions under the ABI number of the parent (nothing a binding of that number calls has
    moved): library, binding and header agree, and the binding declares - so _lib.lib() has found - all five."""
    hdr = open(os.path.join(REPO, "include", "fgc.h")).read()
    L = _lib.lib()
    assert L.fgc_version() == _lib.ABI_VERSION == int(re.search(r"#define FGC_ABI_VERSION (\d+)", hdr).group(1))
    for name in ("fgc_vertex_update_ms_dir", "fgc_vertex_update_ms_dir_traj", "fgc_vertex_update_ms_dir_bwd",
                 "fgc_vertex_update_ms_dir_scratch_floats", "fgc_vertex_update_ms_dir_bwd_workspace_floats"):
        assert name in _lib._SIGS and re.search(r"\b%s\(" % name, hdr), name
    assert L.fgc_vertex_update_ms_dir_scratch_floats(0, 16) == 0 and L.fgc_vertex_update_ms_dir_scratch_floats(10, 0) == 0
    assert L.fgc_vertex_update_ms_dir_scratch_floats(100, 160) == 7 * 100 + 3 * (160 + 40 + 10)
    assert L.fgc_vertex_update_ms_dir_bwd_workspace_floats(0, 16) == 0
    assert (L.fgc_vertex_update_ms_dir_bwd_workspace_floats(100, 160)
            == L.fgc_vertex_update_ms_bwd_workspace_floats(100, 160) + 300)


def test_a_library_without_a_declared_entry_point_is_named(monkeypatch):
    """New entry points came without a new ABI number: an older build of the same number must be told apart by name."""
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib._SIGS, "fgc_no_such_entry_point", (C.c_int, []))
    monkeypatch.delenv("FGC_DEV_PARTIAL", raising=False)
    with pytest.raises(RuntimeError, match="no entry point fgc_no_such_entry_point.*rebuild"):
        _lib.lib()


P = lambda k: C.c_void_p(0x100000 * (k + 1))  # noqa: E731  (made-up addresses nobody may touch, 1 MiB apart)
NV, N0, KV = 100, 160, 25


def _iters(*v):
    return (C.c_int32 * 3)(*v)


def test_forward_argument_checks_answer_einval_before_any_launch():
    L = _lib.lib()
    need = L.fgc_vertex_update_ms_dir_scratch_floats(NV, N0)
    good = dict(x=P(0), x_out=P(1), nv=NV, faces=P(2), n0=N0, v_faces=P(3), k_v=KV, na=P(4), nb=P(5), nc=P(6),
                iters=_iters(2, 1, 1), dirs=P(7), n_dirs=NV, t_out=P(8), dx_out=P(9), scratch=P(10), scratch_floats=need)

    def call(**kw):
        a = dict(good, **kw)
        return L.fgc_vertex_update_ms_dir(a["x"], a["x_out"], a["nv"], a["faces"], a["n0"], a["v_faces"], a["k_v"], a["na"],
                                          a["nb"], a["nc"], a["iters"], a["dirs"], a["n_dirs"], a["t_out"], a["dx_out"],
                                          a["scratch"], a["scratch_floats"], None)
    for name in ("x", "x_out", "faces", "v_faces", "na", "nb", "nc", "iters", "dirs", "scratch"):
        assert call(**{name: None}) == -22, name
        assert b"fgc_vertex_update_ms_dir" in L.fgc_last_error()
    for n_dirs in (0, 2, NV - 1, NV + 1, -1):
        assert call(n_dirs=n_dirs) == -22, n_dirs
        assert b"n_dirs" in L.fgc_last_error()
    assert call(x_out=good["x"]) == -22 and b"distinct" in L.fgc_last_error()      # aliased x and x_out
    assert call(x_out=C.c_void_p(good["x"].value + 12)) == -22 and b"distinct" in L.fgc_last_error()      # overlapping
    for other in ("x", "x_out", "scratch", "t_out"):
        assert call(dx_out=good[other]) == -22 and b"dx_out" in L.fgc_last_error(), other
    assert call(dx_out=C.c_void_p(good["x"].value - 12 * NV)) == -22      # its third stage would lie on x
    assert call(scratch=good["x"]) == -22 and call(scratch=good["x_out"]) == -22
    assert call(t_out=good["x"]) == -22 and call(t_out=good["scratch"]) == -22
    assert call(scratch_floats=need - 1) == -22 and b"scratch too small" in L.fgc_last_error()
    assert call(scratch_floats=0) == -22
    assert call(iters=_iters(1, -1, 0)) == -22
    assert call(nv=0, n_dirs=0) == -22 and call(n0=N0 + 4) == -22 and call(k_v=0) == -22


def test_trajectory_argument_checks_answer_einval_before_any_launch():
    L = _lib.lib()
    need = L.fgc_vertex_update_ms_dir_scratch_floats(NV, N0)
    need_traj = (4 + 1) * 3 * NV
    good = dict(x=P(0), nv=NV, faces=P(2), n0=N0, v_faces=P(3), k_v=KV, na=P(4), nb=P(5), nc=P(6), iters=_iters(2, 1, 1),
                dirs=P(7), n_dirs=1, traj=P(1), traj_floats=need_traj, t_out=None, scratch=P(10), scratch_floats=need)

    def call(**kw):
        a = dict(good, **kw)
        return L.fgc_vertex_update_ms_dir_traj(a["x"], a["nv"], a["faces"], a["n0"], a["v_faces"], a["k_v"], a["na"],
                                               a["nb"], a["nc"], a["iters"], a["dirs"], a["n_dirs"], a["traj"],
                                               a["traj_floats"], a["t_out"], a["scratch"], a["scratch_floats"], None)
    for name in ("x", "faces", "v_faces", "na", "nb", "nc", "iters", "dirs", "traj", "scratch"):
        assert call(**{name: None}) == -22, name
        assert b"fgc_vertex_update_ms_dir_traj" in L.fgc_last_error()
    for n_dirs in (0, 2, NV - 1, NV + 1):
        assert call(n_dirs=n_dirs) == -22, n_dirs
    assert call(traj_floats=need_traj - 1) == -22 and b"traj too small" in L.fgc_last_error()
    assert call(scratch_floats=NV + 3 * (N0 + N0 // 4 + N0 // 16) - 1) == -22 and b"scratch too small" in L.fgc_last_error()
    assert call(traj=good["x"]) == -22 and call(scratch=good["x"]) == -22 and call(t_out=good["traj"]) == -22
    assert call(iters=_iters(-1, 3, 3)) == -22


def test_adjoint_argument_checks_answer_einval_before_any_launch():
    L = _lib.lib()
    need = L.fgc_vertex_update_ms_dir_bwd_workspace_floats(NV, N0)
    need_traj = (4 + 1) * 3 * NV
    names = ("traj", "faces", "v_faces", "na", "nb", "nc", "iters", "dirs", "slot_ptr", "slot_vert", "inc_ptr", "inc_face",
             "g_out", "g_x", "g_n0", "g_n1", "g_n2", "ws")
    good = {n: P(k) for k, n in enumerate(names)}
    good.update(iters=_iters(2, 1, 1), traj_floats=need_traj, n_dirs=NV, ws_floats=need)

    def call(**kw):
        a = dict(good, **kw)
        return L.fgc_vertex_update_ms_dir_bwd(a["traj"], a["traj_floats"], NV, a["faces"], N0, a["v_faces"], KV, a["na"],
                                              a["nb"], a["nc"], a["iters"], a["dirs"], a["n_dirs"], a["slot_ptr"],
                                              a["slot_vert"], a["inc_ptr"], a["inc_face"], a["g_out"], a["g_x"], a["g_n0"],
                                              a["g_n1"], a["g_n2"], a["ws"], a["ws_floats"], None)
    for name in names:
        assert call(**{name: None}) == -22, name
        assert b"fgc_vertex_update_ms_dir_bwd" in L.fgc_last_error()
    for n_dirs in (0, 2, NV - 1, NV + 1):
        assert call(n_dirs=n_dirs) == -22, n_dirs
    assert call(ws_floats=need - 1) == -22 and b"workspace too small" in L.fgc_last_error()
    assert call(ws_floats=L.fgc_vertex_update_ms_bwd_workspace_floats(NV, N0)) == -22      # the free adjoint's size
    assert call(traj_floats=need_traj - 1) == -22 and b"traj too small" in L.fgc_last_error()
    assert call(g_x=good["g_out"]) == -22


def test_cli_parsing(tmp_path, capsys):
    """--ray-update without a view or without --with-vertices is refused, by train and by infer; infer --with-vertices with
    a view and no --ray-update is refused as before; the full train command passes the option checks (and stops at the
    missing pickle, which it names)."""
    from facet_graph_convolution_amd import infer, train
    d = str(tmp_path)
    refused = [
        (train, [d, d, "--with-vertices", "--ray-update"], "--ray-update"),
        (train, [d, d, "--with-vertices", "--synth-noise", "0.1", "--ray-update"], "--ray-update"),
        (train, [d, d, "--with-vertices", "--synth-noise", "0.1", "--noise-direction", "normal", "--ray-update"],
         "--ray-update"),
        (train, [d, d, "--synth-noise", "0.1", "--noise-direction", "ray", "--view-dir", "0,0,1", "--ray-update"],
         "needs --with-vertices"),
        (train, [d, d, "--with-vertices", "--ray-update", "--view-dir", "0,0,1"], "--noise-direction ray"),
        (infer, [d, d, "net.pt", "--with-vertices", "--ray-update", "--view-dir", "0,0,1", "--camera", "0,0,5"],
         "not allowed with"),
        (infer, [d, d, "net.pt", "--with-vertices", "--ray-update", "--view-dir", "0,0,0"], "zero vector"),
        (infer, [d, d, "net.pt", "--with-vertices", "--view-dir", "0,0,1"], "unless --ray-update"),
        (infer, [d, d, "net.pt", "--with-vertices", "--ray-update"], "it needs --with-vertices and"),
        (infer, [d, d, "net.pt", "--ray-update", "--view-dir", "0,0,1"], "it needs --with-vertices and"),
    ]
    for mod, argv, msg in refused:
        with pytest.raises(SystemExit) as e:
            mod.main(argv)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err, (mod.__name__, argv)
    # accepted: the option checks pass, the missing clean pickle is what stops the command
    for view in (["--view-dir", "0,0,1"], ["--camera", "0,0,5"]):
        for double in ([], ["--double-loss"]):
            with pytest.raises(SystemExit) as e:
                train.main([d, d, "--with-vertices", "--synth-noise", "0.1", "--noise-direction", "ray", "--ray-update"]
                           + view + double)
            assert e.value.code == 2 and "no clean training set at" in capsys.readouterr().err


def test_ray_update_needs_rays():
    """Before anything reaches the GPU: the trainers refuse ray_update without noise along rays."""
    from facet_graph_convolution_amd import train as T
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    from facet_graph_convolution_amd.meshgen import icosphere
    V, F = icosphere(2)
    ds = TrainingSet()
    ds.addCleanMeshWithVertices(V, F, seed=0)
    for kw in (dict(noise_levels=(0.1,), noise_direction="normal"), dict(noise_levels=(0.1,))):
        for trainer in (T.trainAccuracyNet, T.trainDoubleLossNet):
            with pytest.raises(ValueError, match="ray_update"):
                trainer(ds, 1, ray_update=True, **kw)
