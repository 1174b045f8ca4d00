"""GPU checks of the point-set training path (trainAccuracyNet, train.py:636-916): the adjoint of the multi-scale vertex
update and the point-set loss fullLoss against float64 autograd (the oracle's update_position_MS, a float64 torch.cdist
restatement of fullLoss), the whole step against float64 autograd through the oracle's multi-scale network, determinism
(eager and hipGraph replay), and the training driver end to end.

Bounds (errors relative to each tensor's largest entry, measured values printed): vertex-update adjoint 1e-5, the whole
step 1e-3 (the angular-loss fp32 step reaches 2e-4)."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from facet_graph_convolution_amd import ops

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


def _full_loss_f64(P0, P1, i0, i1, threshold=5000.0):
    """fullLoss (train.py:1373-1424) restated in float64 torch: sampled two-sided nearest-point distances."""
    prec = torch.cdist(P0[torch.as_tensor(i0, dtype=torch.long)], P1).min(1).values
    comp = torch.cdist(P0, P1[torch.as_tensor(i1, dtype=torch.long)]).min(0).values
    prec = torch.where(prec <= threshold, prec, torch.zeros_like(prec))
    comp = torch.where(comp <= threshold, comp, torch.zeros_like(comp))
    return 1000 * (prec.mean() + comp.mean())


def _truncated_mesh(z):
    """The fixture's mesh with a 4-slot v_faces table (vertices of degree 5 and 6 lose slots)."""
    vf = z["v_faces"][:, :4].copy()
    assert (z["v_faces"][:, 4] >= 0).any() and (z["faces_perm"] < 0).all(1).any()     # truncation happens; fake rows
    return vf


@pytest.mark.parametrize("truncate", [False, True])
@pytest.mark.parametrize("its", [(2, 1, 1), (80, 20, 20)])
def test_vertex_update_adjoint_matches_autograd(golden_dir, its, truncate):
    from oracle import model_ref as R
    z = np.load(os.path.join(golden_dir, "msvertex_ico3.npz"))
    vf = _truncated_mesh(z) if truncate else z["v_faces"]
    x = z["verts_norm"].astype(np.float32)
    rs = np.random.RandomState(7)
    normals = [z["n0"], z["n1"] * 0.5, z["n2"] * 0.3]          # raw coarse heads are not unit vectors
    g_out = rs.standard_normal(x.shape).astype(np.float32)
    t = lambda a: torch.tensor(a, device=DEV)  # noqa: E731
    traj = ops.vertex_update_ms_traj(t(x), [t(n) for n in normals], t(z["faces_perm"]), t(vf), its)
    ref_out, _ = ops.vertex_update_ms(t(x), [t(n) for n in normals], t(z["faces_perm"]), t(vf), its)
    assert torch.equal(traj[-1], ref_out)               # the trajectory form computes the same bits
    g_x, g_n = ops.vertex_update_ms_bwd(traj, [t(n) for n in normals], t(z["faces_perm"]), t(vf), t(g_out), its)
    torch.cuda.synchronize()
    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    n64 = [torch.tensor(n, dtype=torch.float64, requires_grad=True) for n in normals]
    out, _ = R.update_position_MS(x64, n64, z["faces_perm"], vf, 2, its)
    (out * torch.tensor(g_out, dtype=torch.float64)).sum().backward()
    errs = [_rel(g_x.cpu(), x64.grad)] + [_rel(g.cpu(), n.grad) for g, n in zip(g_n, n64)]
    print("adjoint %s truncate=%s: rel err x %.2e n0 %.2e n1 %.2e n2 %.2e" % ((its, truncate) + tuple(errs)))
    assert max(errs) < 1e-5, errs


@pytest.mark.parametrize("case", ["default", "masked", "p1_larger"])
def test_point_loss_matches_float64(case):
    rs = np.random.RandomState({"default": 1, "masked": 2, "p1_larger": 3}[case])
    n0, n1 = (700, 400) if case != "p1_larger" else (300, 2000)
    P0 = rs.uniform(-1, 1, (n0, 3)).astype(np.float32)
    P1 = rs.uniform(-1, 1, (n1, 3)).astype(np.float32)
    i0 = rs.randint(n0, size=500)
    i1 = rs.randint(n1, size=500)
    i0[:20] = i0[20]                     # repeated sample rows
    i1[:20] = i1[20]
    thr = 0.15 if case == "masked" else 5000.0
    # nearest vs second nearest: fp32 and float64 must choose the same neighbours
    d0 = np.sort(np.linalg.norm(P0[i0, None].astype(np.float64) - P1[None], axis=-1), 1)
    d1 = np.sort(np.linalg.norm(P0[:, None].astype(np.float64) - P1[None, i1], axis=-1), 0)
    margin = min((d0[:, 1] - d0[:, 0]).min(), (d1[1] - d1[0]).min())
    assert margin > 1e-5, margin
    if case == "masked":
        kept = (d0[:, 0] <= thr).mean()
        assert 0.1 < kept < 0.9, kept
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=DEV)  # noqa: E731
    loss, g = ops.point_loss(t(P0, torch.float32), t(P1, torch.float32), t(i0, torch.int32), t(i1, torch.int32), thr)
    torch.cuda.synchronize()
    P064 = torch.tensor(P0, dtype=torch.float64, requires_grad=True)
    ref = _full_loss_f64(P064, torch.tensor(P1, dtype=torch.float64), i0, i1, thr)
    ref.backward()
    err_l = abs(loss.item() - ref.item()) / abs(ref.item())
    err_g = _rel(g.cpu(), P064.grad)
    print("point loss %s: loss %.6g rel err %.2e, grad rel err %.2e" % (case, ref.item(), err_l, err_g))
    assert err_l < 1e-6 and err_g < 2e-6


def _mesh_set(kind):
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    from facet_graph_convolution_amd.meshgen import icosphere, torus, add_noise
    V, F = icosphere(3) if kind == "ico3" else torus(100, 100)
    ds = TrainingSet()
    ds.addMeshWithVerticesAndGT(add_noise(V, F, seed=1), F, V, seed=0)
    return ds


def _bind_step(ds, seed=0):
    from facet_graph_convolution_amd.net import FacetDenoiser
    from facet_graph_convolution_amd.utils import rand_rotation_matrix
    net = FacetDenoiser(DEV, multi_scale=True, seed=seed)
    nv = ds.v_list[0].shape[1]
    net.bind_vertices(0, ds.in_list[0], ds.adj_list[0], ds.v_list[0][0], ds.faces_list[0][0], ds.v_faces_list[0][0],
                      ds.gtv_list[0][0])
    rs = np.random.RandomState(5)
    i0, i1 = rs.randint(nv, size=500), rs.randint(ds.gtv_list[0].shape[1], size=500)
    Rm = rand_rotation_matrix(randnums=rs.uniform(size=3))
    net.set_point_samples(i0, i1)
    net.set_rotation(Rm)
    return net, i0, i1, Rm


@pytest.mark.parametrize("kind", ["ico3", "torus20k"])
def test_pointset_step_matches_oracle(kind):
    from oracle import model_ref as R
    ds = _mesh_set(kind)
    net, i0, i1, Rm = _bind_step(ds)
    loss = net.pointset_forward_backward(rotate=True).item()
    grads = [g.detach().cpu().numpy().copy() for g in net.params.grads]
    params = [p.detach().cpu().double().requires_grad_(True) for p in net.params.values]
    R64 = torch.tensor(Rm, dtype=torch.float64)
    x = torch.tensor(ds.in_list[0], dtype=torch.float64)
    adjs = [torch.tensor(a.astype(np.int32)) for a in ds.adj_list[0]]
    xr, _ = R.rotate_inputs(x, None, R64)
    y0, y1, y2 = R.get_model_reg_multi_scale(xr, adjs, params, multiScale=True)
    n0 = R.normalizeTensor(y0)
    v = torch.tensor(ds.v_list[0][0], dtype=torch.float64) @ R64.t()
    gtv = torch.tensor(ds.gtv_list[0][0], dtype=torch.float64) @ R64.t()
    out, _ = R.update_position_MS(v, [n0[0], y1[0], y2[0]], ds.faces_list[0][0], ds.v_faces_list[0][0], 2, (80, 20, 20))
    ref = _full_loss_f64(out, gtv, i0, i1)
    ref.backward()
    err_l = abs(loss - ref.item()) / abs(ref.item())
    print("%s: loss %.6g (oracle %.6g, rel err %.2e)" % (kind, loss, ref.item(), err_l))
    worst = 0.0
    for (name, shape), g, p in zip(net.params.spec, grads, params):
        e = _rel(g, p.grad)
        worst = max(worst, e)
        print("  %-24s %-16s max|g| %.3e  rel err %.2e" % (name, tuple(shape), p.grad.abs().max().item(), e))
        assert np.abs(p.grad.numpy()).max() > 0, name          # every weight tensor gets a gradient
    print("%s: worst rel grad err %.2e" % (kind, worst))
    assert err_l < 1e-4 and worst < 1e-3


def test_pointset_step_is_deterministic_and_replays_bit_exactly():
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r)
        import facet_graph_convolution_amd
        import torch
        sys.path.insert(0, %r)
        from test_gpu_points import _mesh_set, _bind_step
        ds = _mesh_set("ico3")
        net, i0, i1, Rm = _bind_step(ds)
        runs = []
        for capture in (False, False, True, True):
            net.pointset_forward_backward(rotate=True, capture=capture)
            torch.cuda.synchronize()
            runs.append((net._mesh["verts"]["loss"].clone(), net.params.grad.clone()))
        for k in range(1, 4):
            assert torch.equal(runs[0][0], runs[k][0]) and torch.equal(runs[0][1], runs[k][1]), k
        # a new sample count reallocates the step inputs, whose rotation the recorded step reads: it is recorded again
        import numpy as np
        from facet_graph_convolution_amd.utils import rand_rotation_matrix
        g0 = net._mesh["captured"]["points"][0]
        net.set_samples(np.arange(1000))
        assert not net._mesh["captured"]
        net.set_rotation(rand_rotation_matrix(randnums=np.random.RandomState(9).uniform(size=3)))
        net.pointset_forward_backward(rotate=True)
        torch.cuda.synchronize()
        eager = (net._mesh["verts"]["loss"].clone(), net.params.grad.clone())
        net.pointset_forward_backward(rotate=True, capture=True)
        torch.cuda.synchronize()
        assert net._mesh["captured"]["points"][0] is not g0
        assert torch.equal(eager[0], net._mesh["verts"]["loss"]) and torch.equal(eager[1], net.params.grad)
        assert not torch.equal(eager[0], runs[0][0])
        print("deterministic ok", runs[0][0].item())
    """ % (REPO, os.path.join(REPO, "tests")))
    env = dict(os.environ)
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "deterministic ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def _small_set(seeds, sub=2):
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    from facet_graph_convolution_amd.meshgen import icosphere, add_noise
    V, F = icosphere(sub)
    ds = TrainingSet()
    for s in seeds:
        ds.addMeshWithVerticesAndGT(add_noise(V, F, seed=s), F, V, seed=s)
    return ds


def test_train_accuracy_net_end_to_end(tmp_path):
    from facet_graph_convolution_amd import train as T
    from facet_graph_convolution_amd.dataClasses import InferenceMesh
    from facet_graph_convolution_amd.meshgen import icosphere, add_noise
    from facet_graph_convolution_amd.utils import write_mesh
    from facet_graph_convolution_amd import infer
    path = str(tmp_path / "net")
    logs = []
    net, arr, hist = T.trainAccuracyNet(_small_set([1, 2]), 60, network_path=path, net_name="acc", validSet=_small_set([3]),
                                        log=logs.append)
    assert np.isfinite(hist).all() and hist.shape == (60,)
    assert any("validation loss" in s for s in logs) and any("training loss" in s for s in logs)
    files = os.listdir(path)
    assert "acc.csv" in files and "checkpoint" in files and any(f.startswith("acc-60") for f in files), files
    assert np.loadtxt(os.path.join(path, "acc.csv"), delimiter=",").shape == (50, 2)
    # resume: the second run starts from iteration 60 with the saved weights
    net2, _, _ = T.trainAccuracyNet(_small_set([1, 2]), 10, network_path=path, net_name="acc", log=logs.append)
    assert any(f.startswith("acc-70") for f in os.listdir(path))
    assert net2.params.step == net.params.step + 10
    # infer --with-vertices on the saved network = inferNet
    V, F = icosphere(2)
    noisy = tmp_path / "noisy"
    noisy.mkdir()
    write_mesh(add_noise(V, F, seed=9), F, str(noisy / "ball.obj"))
    res = tmp_path / "res"
    infer.main([str(noisy), str(res), path, "--with-vertices"])
    assert sorted(os.listdir(res)) == ["ball_d_coarse.obj", "ball_d_mid.obj", "ball_denoised.obj"]
    mesh = InferenceMesh()
    mesh.addMeshWithVertices(str(noisy), "ball.obj")
    want = T.inferNet(mesh, net2)
    for name, w in zip(("ball_denoised.obj", "ball_d_mid.obj", "ball_d_coarse.obj"), want[:3]):
        got = np.loadtxt(str(res / name), usecols=(1, 2, 3), max_rows=len(V))
        np.testing.assert_allclose(got, w, atol=1.5e-6)


def test_train_accuracy_net_lowers_the_loss():
    from facet_graph_convolution_amd import train as T
    _, _, hist = T.trainAccuracyNet(_small_set([4], sub=3), 300, seed=0, log=lambda s: None)
    first, last = hist[:20].mean(), hist[-20:].mean()
    print("point-set loss: first 20 iterations %.4f, last 20 %.4f" % (first, last))
    assert np.isfinite(hist).all() and last < first


@pytest.mark.parametrize("synth", [False, True])
@pytest.mark.parametrize("double", [False, True])
def test_vertex_trainers_capture_equals_eager_across_mesh_switches_and_validation(monkeypatch, double, synth):
    """trainAccuracyNet / trainDoubleLossNet(capture=True) on two meshes with a validation set, plain and on synthesised
    noise: each training mesh's step is recorded once and kept with the mesh across the switches and the validation
    passes (iteration 20; on synthesised noise iteration 0 too), and the run computes bit for bit what the eager run does."""
    from facet_graph_convolution_amd import train as T
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    from facet_graph_convolution_amd.meshgen import icosphere
    from facet_graph_convolution_amd.net import FacetDenoiser

    def clean_set(seeds):
        V, F = icosphere(2)
        ds = TrainingSet()
        for s in seeds:
            ds.addCleanMeshWithVertices(V, F, seed=s)
        return ds
    ts, vs = (clean_set([1, 2]), clean_set([3])) if synth else (_small_set([1, 2]), _small_set([3]))
    form = "double" if double else "points"
    trainer = T.trainDoubleLossNet if double else T.trainAccuracyNet
    extra = dict(noise_levels=(0.1, 0.3)) if synth else {}
    steps = []
    adam = FacetDenoiser.adam_step

    def adam_step(self, *a, **k):     # (right behind each step's forward + backward)
        steps.append((self._mesh["captured"].get(form) or (None,))[0])
        return adam(self, *a, **k)
    monkeypatch.setattr(FacetDenoiser, "adam_step", adam_step)
    logs = []
    net, arr, hist = trainer(ts, 25, capture=True, validSet=vs, log=logs.append, **extra)
    graphs = list(steps)
    switches = sum(1 for a, b in zip(graphs, graphs[1:]) if a is not b)
    assert len(graphs) == 25 and None not in graphs and len({id(g) for g in graphs}) == 2 and switches >= 3
    assert all(set(net._mesh_cache[b]["captured"]) == {form} for b in (0, 1))
    logs_e = []
    net_e, arr_e, hist_e = trainer(ts, 25, validSet=vs, log=logs_e.append, **extra)
    assert sum("validation loss" in s for s in logs) == (2 if synth else 1) and logs == logs_e
    assert np.isfinite(hist).all() and hist.shape == ((25, 3) if double else (25,))
    assert np.array_equal(hist, hist_e) and np.array_equal(arr, arr_e) and torch.equal(net.params.theta, net_e.params.theta)


def test_pointset_step_matches_reference_fixture(golden_dir):
    """One point-set step against the reference's own chain executed on tf_shim (tests/golden/gen/make_golden_points.py):
    refined vertices, loss and every weight gradient (large tensors at the fixture's sampled entries), relative to each
    tensor's largest entry.  The float64 run of the same chain is the error budget."""
    from facet_graph_convolution_amd.net import FacetDenoiser
    z = np.load(os.path.join(golden_dir, "points_ico3.npz"))
    z64 = np.load(os.path.join(golden_dir, "points_ico3_f64.npz"))
    net = FacetDenoiser(DEV, multi_scale=True, seed=0)
    assert len(net.params.spec) == int(z["n_vars"])
    net.bind_vertices(0, z["x"], [z["adj%d" % k].astype(np.int32) for k in range(3)], z["verts"], z["faces"],
                      z["v_faces"].astype(np.int32), z["gt_verts"])
    net.set_point_samples(z["sample_ind0"], z["sample_ind1"])
    net.set_rotation(z["R"])
    loss = net.pointset_forward_backward(rotate=True).item()
    V = net._mesh["verts"]
    nv = z["verts"].shape[0]
    refined = V["traj"][-3 * nv:].reshape(nv, 3).cpu().numpy()
    err_x = np.abs(refined - z["refined"]).max()
    err_l = abs(loss - float(z["loss"])) / float(z["loss"])
    err_l64 = abs(float(z["loss"]) - float(z64["loss"])) / float(z64["loss"])
    print("reference fixture: refined vertices max err %.2e, loss %.6g rel err %.2e (fixture fp32 vs f64 %.2e)"
          % (err_x, float(z["loss"]), err_l, err_l64))
    worst, worst64 = 0.0, 0.0
    for i, g in enumerate(net.params.grads):
        flat = g.detach().cpu().numpy().reshape(-1)
        assert flat.size == int(z["gsize%02d" % i])
        n = flat.size
        idx = np.arange(n) if n <= int(z["sampled"]) else np.sort(np.random.RandomState(i).choice(n, int(z["sampled"]),
                                                                                                  replace=False))
        scale = float(z64["gmax%02d" % i])
        assert scale > 0, str(z["name%02d" % i])
        e = np.abs(flat[idx] - z64["g%02d" % i]).max() / scale
        e32 = np.abs(z["g%02d" % i] - z64["g%02d" % i]).max() / scale
        worst, worst64 = max(worst, e), max(worst64, e32)
        print("  g%02d %-12s n %7d  max|g| %.3e  rel err %.2e (fixture fp32 %.2e)" % (i, z["name%02d" % i], n, scale, e, e32))
    print("reference fixture: worst rel grad err %.2e (fixture fp32 vs f64 %.2e)" % (worst, worst64))
    assert err_x < 1e-5 and err_l < 1e-4 and worst < 1e-3
