"""The ray-constrained multi-scale vertex update on the GPU (fgc_vertex_update_ms_dir, _traj, _bwd; a build extension)
against the float64 restatement of tests/depth_ms_cases.py, through ops, update_position_MS / inferNet, the bound-mesh
steps, the trainers and the infer command.

TOL_FWD, the bound of the forward tests: the worst absolute deviation of x_out, t_out and the three dx from the float64
restatement over (2,1,1) and (80,20,20), the three direction sets and both slot tables, measured on an MI355X, is 5.0e-8
(at (80,20,20), x_out and the fine stage's dx of the camera set, 4-slot table; coordinates are at most 0.29 in magnitude, t up to 0.06;
the worst t_out 3.6e-8).  The free update's deviation from its own float64 restatement
(oracle.model_ref.update_position_MS) in the same run: 3.7e-8 at (2,1,1), 1.0e-7 (full table) and 1.5e-7 (4 slots) at
(80,20,20) - the constrained form rebuilds every position from the input and one scalar and stays closer.  The bound is 8
times the measured value, the margin __graft_entry__.py names for the fp32 kernels.  One step from rest (test 4) measured
1.5e-8 and is held to the same bound."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from facet_graph_convolution_amd import ops, utils
from facet_graph_convolution_amd import train as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_cases as dc  # noqa: E402
import depth_ms_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_FWD = 8 * 5.0e-8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)  # noqa: E731
_bits = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)  # noqa: E731
_np = lambda t: t.detach().cpu().numpy()  # noqa: E731


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


@functools.lru_cache(maxsize=None)
def _case(kind, truncate):
    x, normals, faces, vf = mc.load(GOLDEN, truncate)
    return dict(x=x, normals=normals, faces=faces, vf=vf, d=mc.directions(x, kind), g_out=np.random.RandomState(7)
                .standard_normal(x.shape).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _ref(its, kind, truncate):
    """The float64 restatement and its autograd gradients for g_out, computed once and shared."""
    c = _case(kind, truncate)
    x64 = torch.tensor(c["x"], dtype=torch.float64, requires_grad=True)
    n64 = [torch.tensor(n, dtype=torch.float64, requires_grad=True) for n in c["normals"]]
    out, t, dxs = mc.restate(x64, n64, c["faces"], c["vf"], c["d"], its)
    (out * torch.tensor(c["g_out"], dtype=torch.float64)).sum().backward()
    return dict(x=_np(out), t=_np(t), dx=[_np(a) for a in dxs], g_x=_np(x64.grad), g_n=[_np(n.grad) for n in n64])


def _gpu(c, its, **kw):
    return ops.vertex_update_ms_dir(_dev(c["x"]), [_dev(n) for n in c["normals"]], _dev(c["faces"]), _dev(c["vf"]),
                                    _dev(c["d"]), its, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("truncate", [False, True])
@pytest.mark.parametrize("kind", mc.DIR_SETS)
@pytest.mark.parametrize("its", mc.ITERS)
def test_forward_matches_float64(its, kind, truncate):
    from oracle import model_ref as R
    c, ref = _case(kind, truncate), _ref(its, kind, truncate)
    out, dx, t = _gpu(c, its, return_t=True)
    free, _ = ops.vertex_update_ms(_dev(c["x"]), [_dev(n) for n in c["normals"]], _dev(c["faces"]), _dev(c["vf"]), its)
    torch.cuda.synchronize()
    with torch.no_grad():
        free64, _ = R.update_position_MS(torch.tensor(c["x"], dtype=torch.float64),
                                         [torch.tensor(n, dtype=torch.float64) for n in c["normals"]], c["faces"], c["vf"],
                                         2, its)
    errs = [np.abs(_np(out) - ref["x"]).max(), np.abs(_np(t) - ref["t"]).max()] + \
        [np.abs(_np(dx[s]) - ref["dx"][s]).max() for s in range(3)]
    err_free = np.abs(_np(free) - _np(free64)).max()
    print("forward %s %s truncate=%s: |gpu - f64| x %.2e t %.2e dx %.2e %.2e %.2e; the free update against its own f64 "
          "%.2e; max |t| %.3e" % ((its, kind, truncate) + tuple(errs) + (err_free, np.abs(ref["t"]).max())))
    assert max(errs) <= TOL_FWD, errs
    assert np.abs(ref["t"]).max() > 1e-3 and np.abs(_np(out) - _np(free)).max() > 1e-4      # the constraint matters


# ---------------------------------------------------------------------------------------------------------------------
# 2. on the ray
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", mc.DIR_SETS)
def test_vertices_stay_on_their_rays(kind):
    c = _case(kind, False)
    out, _, t = _gpu(c, (80, 20, 20), return_t=True)
    x, t = _np(out), _np(t)
    # x_out is fma(t, d, x0): the host's value (the product is exact in float64, one rounding of the sum, one to float32)
    host = (t.astype(np.float64)[:, None] * c["d"].astype(np.float64) + c["x"].astype(np.float64)).astype(np.float32)
    assert (np.abs(x - host) <= np.spacing(np.abs(host))).all()
    assert np.abs(t).max() > 1e-3


def test_view_along_z_keeps_x_and_y_bits():
    c = dict(_case("camera", False), d=utils.view_rays(_case("camera", False)["x"], view_dir=(0, 0, 1)))
    out, dx = _gpu(c, (80, 20, 20))
    x = _np(out)
    assert np.array_equal(_bits(x[:, :2]), _bits(c["x"][:, :2])) and np.abs(x[:, 2] - c["x"][:, 2]).max() > 1e-3
    assert not _np(dx)[:, :, :2].any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. edge forms
# ---------------------------------------------------------------------------------------------------------------------
def test_zero_iterations_return_the_input():
    c = _case("camera", False)
    out, dx, t = _gpu(c, (0, 0, 0), return_t=True)
    assert np.array_equal(_bits(_np(out)), _bits(c["x"])) and not _np(t).any() and not _np(dx).any()
    traj, t = ops.vertex_update_ms_dir_traj(_dev(c["x"]), [_dev(n) for n in c["normals"]], _dev(c["faces"]), _dev(c["vf"]),
                                            _dev(c["d"]), (0, 0, 0), return_t=True)
    assert traj.shape == (1,) + c["x"].shape and np.array_equal(_bits(_np(traj[0])), _bits(c["x"])) and not _np(t).any()


@pytest.mark.parametrize("its", mc.ITERS)
def test_one_row_equals_a_full_table_of_it(its):
    c = _case("view_dir", True)
    assert c["d"].shape == (1, 3)
    full = dict(c, d=np.ascontiguousarray(np.broadcast_to(c["d"], c["x"].shape)))
    a, b = _gpu(c, its, return_t=True), _gpu(full, its, return_t=True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    args = lambda k: (_dev(k["x"]), [_dev(n) for n in k["normals"]], _dev(k["faces"]), _dev(k["vf"]), _dev(k["d"]))  # noqa: E731
    ta, tb = ops.vertex_update_ms_dir_traj(*args(c), its), ops.vertex_update_ms_dir_traj(*args(full), its)
    g = _dev(c["g_out"])
    ga = ops.vertex_update_ms_dir_bwd(ta, *args(c)[1:], g, its)
    gb = ops.vertex_update_ms_dir_bwd(tb, *args(full)[1:], g, its)
    assert torch.equal(ta, tb) and torch.equal(ga[0], gb[0]) and all(torch.equal(p, q) for p, q in zip(ga[1], gb[1]))


@pytest.mark.parametrize("truncate", [False, True])
@pytest.mark.parametrize("its", mc.ITERS)
def test_trajectory_equals_the_plain_form_and_runs_repeat(its, truncate):
    c = _case("scaled", truncate)
    out, dx, t = _gpu(c, its, return_t=True)
    args = (_dev(c["x"]), [_dev(n) for n in c["normals"]], _dev(c["faces"]), _dev(c["vf"]), _dev(c["d"]))
    traj, tt = ops.vertex_update_ms_dir_traj(*args, its, return_t=True)
    assert traj.shape[0] == sum(its) + 1
    assert torch.equal(traj[0], args[0]) and torch.equal(traj[-1], out) and torch.equal(tt, t)
    T0, T1 = its[0], its[0] + its[1]
    assert torch.equal(dx[0], traj[T0] - traj[0]) and torch.equal(dx[1], traj[T1] - traj[T0])
    assert torch.equal(dx[2], traj[-1] - traj[T1])
    # two runs: the same bits, forward and adjoint
    out2, dx2, t2 = _gpu(c, its, return_t=True)
    g = _dev(c["g_out"])
    g1 = ops.vertex_update_ms_dir_bwd(traj, *args[1:], g, its)
    g2 = ops.vertex_update_ms_dir_bwd(ops.vertex_update_ms_dir_traj(*args, its), *args[1:], g, its)
    assert torch.equal(out, out2) and torch.equal(dx, dx2) and torch.equal(t, t2)
    assert torch.equal(g1[0], g2[0]) and all(torch.equal(p, q) for p, q in zip(g1[1], g2[1]))


def _ragged_mesh(name):
    """A ragged torus as the multi-scale update reads it: faces padded to a multiple of 16 with -1 rows, 25 face slots per
    vertex, face normals at level 0 and seeded rows of norm <= 1 at the two coarse levels."""
    V, F = dc.ragged(name)
    n0 = -(-F.shape[0] // 16) * 16
    faces = np.concatenate([F.astype(np.int64), -np.ones((n0 - F.shape[0], 3), dtype=np.int64)])
    vf = utils.getVerticesFaces(faces, 25, V.shape[0])
    fn = np.concatenate([utils.computeFacesNormals(V, F), np.zeros((n0 - F.shape[0], 3))]).astype(np.float32)
    rs = np.random.RandomState(3)
    coarse = []
    for n in (n0 // 4, n0 // 16):
        r = rs.standard_normal((n, 3))
        coarse.append((r / np.linalg.norm(r, axis=1, keepdims=True) * rs.uniform(0.3, 1.0, (n, 1))).astype(np.float32))
    V = (V + 0.02 * rs.standard_normal(V.shape)).astype(np.float32)
    return V, [fn] + coarse, faces, np.asarray(vf)


@pytest.mark.parametrize("name", ["t255", "t256", "t257"])
def test_ragged_sizes(name):
    V, normals, faces, vf = _ragged_mesh(name)
    assert V.shape[0] == {"t255": 255, "t256": 256, "t257": 257}[name] == vf.shape[0]
    its = (2, 1, 2)
    g_out = np.random.RandomState(8).standard_normal(V.shape).astype(np.float32)
    for d in (utils.view_rays(V, camera=mc.CAMERA), utils.view_rays(V, view_dir=(0, 0.6, 0.8))):
        args = (_dev(V), [_dev(n) for n in normals], _dev(faces), _dev(vf), _dev(d))
        out, dx, t = ops.vertex_update_ms_dir(*args, its, return_t=True)
        traj = ops.vertex_update_ms_dir_traj(*args, its)
        g_x, g_n = ops.vertex_update_ms_dir_bwd(traj, *args[1:], _dev(g_out), its)
        x64 = torch.tensor(V, dtype=torch.float64, requires_grad=True)
        n64 = [torch.tensor(n, dtype=torch.float64, requires_grad=True) for n in normals]
        want, tw, _ = mc.restate(x64, n64, faces, vf, d, its)
        (want * torch.tensor(g_out, dtype=torch.float64)).sum().backward()
        # (TOL_FWD was measured on coordinates of at most 0.29: scaled to this mesh's largest coordinate)
        tol = TOL_FWD * max(1.0, np.abs(V).max() / 0.29)
        err = max(np.abs(_np(out) - _np(want)).max(), np.abs(_np(t) - _np(tw)).max())
        print("ragged %s dirs %s: |gpu - f64| %.2e (bound %.2e)" % (name, d.shape, err, tol))
        assert err <= tol
        assert torch.equal(traj[-1], out) and np.abs(_np(out) - V).max() > 1e-3
        errs = [_rel(_np(g_x), _np(x64.grad))] + [_rel(_np(g), _np(n.grad)) for g, n in zip(g_n, n64)]
        assert max(errs) < 1e-5, (name, d.shape, errs)
        if name == "t257":      # the isolated vertex keeps its position, and its gradient passes through unchanged
            assert (vf[-1] < 0).all()
            assert np.array_equal(_bits(_np(out)[-1]), _bits(V[-1])) and _np(t)[-1] == 0
            assert np.array_equal(_bits(_np(g_x)[-1]), _bits(g_out[-1]))
    # the free forms run through the same driver: the same inputs, bit for bit among themselves and from run to run
    args = args[:4]
    out, dx = ops.vertex_update_ms(*args, its)
    traj = ops.vertex_update_ms_traj(*args, its)
    T0, T1 = its[0], its[0] + its[1]
    assert traj.shape[0] == sum(its) + 1 and torch.equal(traj[0], args[0]) and torch.equal(traj[-1], out)
    assert torch.equal(dx[0], traj[T0] - traj[0]) and torch.equal(dx[1], traj[T1] - traj[T0])
    assert torch.equal(dx[2], traj[-1] - traj[T1]) and np.abs(_np(out) - V).max() > 1e-3
    out2, dx2 = ops.vertex_update_ms(*args, its)
    assert torch.equal(out, out2) and torch.equal(dx, dx2) and torch.equal(ops.vertex_update_ms_traj(*args, its), traj)
    if name == "t257":      # the isolated vertex again: its position bits, and g_out's row through the free adjoint
        g_x, _ = ops.vertex_update_ms_bwd(traj, *args[1:], _dev(g_out), its)
        assert np.array_equal(_bits(_np(out)[-1]), _bits(V[-1])) and np.array_equal(_bits(_np(g_x)[-1]), _bits(g_out[-1]))


# ---------------------------------------------------------------------------------------------------------------------
# 4. one step from rest
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("truncate", [False, True])
@pytest.mark.parametrize("kind", mc.DIR_SETS)
def test_one_step_from_rest_is_the_projected_free_step(kind, truncate):
    c = _case(kind, truncate)
    its = (0, 0, 1)
    _, _, t = _gpu(c, its, return_t=True)
    free, _ = ops.vertex_update_ms(_dev(c["x"]), [_dev(n) for n in c["normals"]], _dev(c["faces"]), _dev(c["vf"]), its)
    want = ((_np(free).astype(np.float64) - c["x"].astype(np.float64)) * c["d"].astype(np.float64)).sum(1)
    err = np.abs(_np(t) - want).max()
    print("one step from rest %s truncate=%s: |t - d . (x_free - x0)| %.2e, max |t| %.3e" % (kind, truncate, err,
                                                                                          np.abs(want).max()))
    assert err <= TOL_FWD and np.abs(want).max() > 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# 5. adjoint against autograd of the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("truncate", [False, True])
@pytest.mark.parametrize("kind", mc.DIR_SETS)
@pytest.mark.parametrize("its", mc.ITERS)
def test_adjoint_matches_autograd(its, kind, truncate):
    c, ref = _case(kind, truncate), _ref(its, kind, truncate)
    args = (_dev(c["x"]), [_dev(n) for n in c["normals"]], _dev(c["faces"]), _dev(c["vf"]), _dev(c["d"]))
    traj = ops.vertex_update_ms_dir_traj(*args, its)
    g_x, g_n = ops.vertex_update_ms_dir_bwd(traj, *args[1:], _dev(c["g_out"]), its)
    torch.cuda.synchronize()
    errs = [_rel(_np(g_x), ref["g_x"])] + [_rel(_np(g), r) for g, r in zip(g_n, ref["g_n"])]
    print("adjoint %s %s truncate=%s: rel err x %.2e n0 %.2e n1 %.2e n2 %.2e" % ((its, kind, truncate) + tuple(errs)))
    assert max(errs) < 1e-5, errs


def test_update_position_ms_is_differentiable_along_rays():
    """train.update_position_MS(depth_dir=): the values of the plain call, the gradients of the adjoint entry point."""
    c = _case("camera", False)
    its = (2, 1, 1)
    x = _dev(c["x"])[None].requires_grad_(True)
    ns = [_dev(n)[None].requires_grad_(True) for n in c["normals"]]
    faces, vf = _dev(c["faces"])[None], _dev(c["vf"])[None]
    out, dxs = T.update_position_MS(x, ns, faces, vf, 2, list(its), depth_dir=c["d"])
    (out[0] * _dev(c["g_out"])).sum().backward()
    with torch.no_grad():
        plain, dxp = T.update_position_MS(x, ns, faces, vf, 2, list(its), depth_dir=_dev(c["d"]))
    want, dxw = _gpu(c, its)
    assert torch.equal(out.detach()[0], want) and torch.equal(plain[0], want)
    assert all(torch.equal(a.detach(), dxw[s]) and torch.equal(b, dxw[s]) for s, (a, b) in enumerate(zip(dxs, dxp)))
    ref = _ref(its, "camera", False)
    errs = [_rel(_np(x.grad[0]), ref["g_x"])] + [_rel(_np(n.grad[0]), r) for n, r in zip(ns, ref["g_n"])]
    assert max(errs) < 1e-5, errs
    free, _ = T.update_position_MS(x.detach(), [n.detach() for n in ns], faces, vf, 2, list(its))
    assert not torch.equal(free[0], want)
    with pytest.raises(ValueError, match="depth_dir"):
        T.update_position_MS(x.detach(), [n.detach() for n in ns], faces, vf, 2, list(its), depth_dir=c["d"][:5])


# ---------------------------------------------------------------------------------------------------------------------
# 6. step level
# ---------------------------------------------------------------------------------------------------------------------
def _bound_step(double, depth_dir):
    """test_gpu_points' small mesh set bound with a ray table: (ds, net, i0, i1, R, rays)."""
    from test_gpu_points import _mesh_set
    from facet_graph_convolution_amd.net import FacetDenoiser
    ds = _mesh_set("ico3")
    net = FacetDenoiser(DEV, multi_scale=True, seed=0)
    nv = ds.v_list[0].shape[1]
    rays = utils.view_rays(ds.v_list[0][0], camera=mc.CAMERA) if isinstance(depth_dir, str) else depth_dir
    net.bind_vertices(0, ds.in_list[0], ds.adj_list[0], ds.v_list[0][0], ds.faces_list[0][0], ds.v_faces_list[0][0],
                      ds.gtv_list[0][0], depth_dir=rays, **({"gt_normals": ds.gt_list[0][0]} if double else {}))
    rs = np.random.RandomState(5)
    i0, i1 = rs.randint(nv, size=500), rs.randint(ds.gtv_list[0].shape[1], size=500)
    Rm = utils.rand_rotation_matrix(randnums=rs.uniform(size=3))
    net.set_point_samples(i0, i1)
    net.set_rotation(Rm)
    return ds, net, i0, i1, Rm, rays


@pytest.mark.parametrize("double", [False, True])
def test_step_along_rays_matches_oracle(double):
    from oracle import model_ref as R
    from test_gpu_points import _full_loss_f64
    ds, net, i0, i1, Rm, rays = _bound_step(double, "camera")
    step = net.double_loss_forward_backward if double else net.pointset_forward_backward
    out = np.atleast_1d(step(rotate=True).cpu().numpy())
    grads = [g.detach().cpu().numpy().copy() for g in net.params.grads]
    theta_g = net.params.grad.clone()
    # the captured step: the eager step's bits
    out_c = np.atleast_1d(step(rotate=True, capture=True).cpu().numpy())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(out_c)) and torch.equal(theta_g, net.params.grad)
    out_c = np.atleast_1d(step(rotate=True, capture=True).cpu().numpy())      # (a replay)
    assert np.array_equal(_bits(out), _bits(out_c)) and torch.equal(theta_g, net.params.grad)
    params = [p.detach().cpu().double().requires_grad_(True) for p in net.params.values]
    R64 = torch.tensor(Rm, dtype=torch.float64)
    x = torch.tensor(ds.in_list[0], dtype=torch.float64)
    gt = torch.tensor(ds.gt_list[0].astype(np.float32), dtype=torch.float64)
    adjs = [torch.tensor(a.astype(np.int32)) for a in ds.adj_list[0]]
    xr, gtr = R.rotate_inputs(x, gt, R64)
    y0, y1, y2 = R.get_model_reg_multi_scale(xr, adjs, params, multiScale=True)
    n0 = R.normalizeTensor(y0)
    heads = [n0[0], R.normalizeTensor(y1)[0], R.normalizeTensor(y2)[0]] if double else [n0[0], y1[0], y2[0]]
    v = torch.tensor(ds.v_list[0][0], dtype=torch.float64) @ R64.t()
    gtv = torch.tensor(ds.gtv_list[0][0], dtype=torch.float64) @ R64.t()
    d = (torch.tensor(rays, dtype=torch.float64) @ R64.t()).numpy()
    moved = mc.restate(v, heads, ds.faces_list[0][0], ds.v_faces_list[0][0], d, (80, 20, 20))[0]
    pts = _full_loss_f64(moved, gtv, i0, i1)
    want = [pts]
    if double:
        nrm = R.faceNormalsLoss(n0, gtr)
        want = [pts + nrm, pts, nrm]
    want[0].backward()
    want = [w.item() for w in want]
    errs = [abs(float(a) - b) / abs(b) for a, b in zip(out, want)]
    # the refined vertices lie on the rotated rays, and the step is not the free one
    refined = net._mesh["verts"]["traj"].reshape(121, -1, 3)[-1].cpu().numpy().astype(np.float64)
    off = np.linalg.norm(np.cross(refined - v.numpy(), d), axis=1).max()
    err_x = np.abs(refined - moved.detach().numpy()).max()
    print("step along rays (double=%s): loss %s (oracle %s, rel err %s); refined max err %.2e, off the ray %.2e"
          % (double, out, want, ["%.2e" % e for e in errs], err_x, off))
    worst = 0.0
    for (name, shape), g, p in zip(net.params.spec, grads, params):
        e = _rel(g, p.grad)
        worst = max(worst, e)
        print("  %-24s %-16s max|g| %.3e  rel err %.2e" % (name, tuple(shape), p.grad.abs().max().item(), e))
        assert np.abs(p.grad.numpy()).max() > 0, name
    print("worst rel grad err %.2e" % worst)
    assert max(errs) < 1e-4 and worst < 1e-3 and err_x < 1e-5 and off < 1e-6


def test_bound_rays_are_kept_with_the_mesh():
    """A key is bound with its rays or without: a rebind with the same table is a lookup, another table is refused; the
    step without rotation reads the table as bound, and an unbound table leaves the free step's bits alone."""
    from test_gpu_points import _bind_step, _mesh_set
    ds, net, i0, i1, Rm, rays = _bound_step(False, utils.view_rays(np.zeros((1, 3)), view_dir=(0, 0, 1)))
    a = (ds.in_list[0], ds.adj_list[0], ds.v_list[0][0], ds.faces_list[0][0], ds.v_faces_list[0][0], ds.gtv_list[0][0])
    net.bind_vertices(0, *a, depth_dir=rays)
    net.bind_vertices(0, *a, depth_dir=rays.copy())
    for other in (None, utils.view_rays(np.zeros((1, 3)), view_dir=(0, 1, 0))):
        with pytest.raises(ValueError, match="rays"):
            net.bind_vertices(0, *a, depth_dir=other)
    with pytest.raises(ValueError, match="depth_dir"):
        net.bind_vertices(1, *a, depth_dir=np.ones((7, 3), dtype=np.float32))
    assert 1 not in net._mesh_cache and net._mesh is net._mesh_cache[0]
    loss = net.pointset_forward_backward(rotate=False).item()
    V = net._mesh["verts"]
    refined = V["traj"].reshape(121, -1, 3)[-1]
    assert torch.equal(refined[:, :2], V["x"][:, :2]) and not torch.equal(refined[:, 2], V["x"][:, 2])
    free_net, *_ = _bind_step(_mesh_set("ico3"))
    free_loss = free_net.pointset_forward_backward(rotate=False).item()
    assert np.isfinite(loss) and loss != free_loss
    net.bind_vertices(2, *a)                                     # the same network, no table: the free step's bits
    net.set_point_samples(i0, i1)
    assert net.pointset_forward_backward(rotate=False).item() == free_loss


def _clean_set(seeds, sub=2):
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    from facet_graph_convolution_amd.meshgen import icosphere
    V, F = icosphere(sub)
    ds = TrainingSet()
    for s in seeds:
        ds.addCleanMeshWithVertices(V, F, seed=s)
    return ds


@pytest.mark.parametrize("double", [False, True])
def test_trainer_with_ray_update_moves_vertices_along_the_view(double):
    """--synth-noise ... --noise-direction ray --view-dir 0,0,1 --ray-update, as the Python call: a few iterations, then on
    the last bound mesh without rotation the noisy vertices and the refined ones share their x and y columns; without
    ray_update they do not."""
    from facet_graph_convolution_amd.net import FacetDenoiser
    trainer = T.trainDoubleLossNet if double else T.trainAccuracyNet
    view = {"view_dir": (0, 0, 1)}
    logs = []
    net, arr, hist = trainer(_clean_set([1, 2]), 4, validSet=_clean_set([3]), log=logs.append, noise_levels=(0.1, 0.3),
                             noise_direction=view, ray_update=True, capture=True)
    assert np.isfinite(hist).all() and hist.shape[0] == 4 and any("validation loss" in s for s in logs)
    assert all(m["verts"]["dirs"] is not None for m in net._mesh_cache.values())
    net_f, _, hist_f = trainer(_clean_set([1, 2]), 4, validSet=_clean_set([3]), log=logs.append, noise_levels=(0.1, 0.3),
                               noise_direction=view)
    assert all(m["verts"]["dirs"] is None for m in net_f._mesh_cache.values()) and not np.array_equal(hist, hist_f)
    shared = []
    for n in (net, net_f):
        n.set_noise(17, 0.3)
        (n.double_loss_forward_backward if double else n.pointset_forward_backward)(rotate=False)
        Vs, S = n._mesh["verts"], n._mesh["synth"]
        noisy, refined = n.noisy_vertices(), Vs["traj"].reshape(121, -1, 3)[-1]
        # (the step reads the noisy vertices over the diagonal of the union box: xr; the clean mesh's x and y survive the noise)
        assert torch.equal(noisy[:, :2], S.v[:, :2]) and not torch.equal(noisy[:, 2], S.v[:, 2])
        scale = (noisy[:, :2] / Vs["xr"][:, :2])[Vs["xr"][:, :2].abs() > 1e-3]
        assert (scale.max() - scale.min()).item() < 1e-5 * scale.max().item()
        shared.append(torch.equal(refined[:, :2], Vs["xr"][:, :2]))
        assert not torch.equal(refined[:, 2], Vs["xr"][:, 2])
    assert shared == [True, False]
    with pytest.raises(ValueError, match="ray_update"):
        FacetDenoiser(DEV, multi_scale=True).bind_clean_vertices(
            0, *T._clean_vertex_meshes(_clean_set([1]), "training set")[0].args, direction="normal", ray_update=True)


# ---------------------------------------------------------------------------------------------------------------------
# 7. drivers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m, max_size", [(9, 10 ** 9), (13, 120)])
def test_infer_net_takes_rays(m, max_size):
    """inferNet(depth_dir=) on a height field seen along z, whole and in patches (a 13 x 13 grid in five patches of 120
    faces, vertices in up to five of them: patches under 100 faces are dropped): the three vertex sets keep the input's x
    and y (divided by the diagonal, as inferNet returns them); with a camera they lie on its rays."""
    from facet_graph_convolution_amd.dataClasses import InferenceMesh
    from facet_graph_convolution_amd.net import FacetDenoiser
    Vn, _, F = dc.height_field(m)
    np.random.seed(0)      # (patch seeds)
    mesh = InferenceMesh(maxSize=max_size)
    mesh.addMeshWithVertices(Vn, F, seed=0)
    assert len(mesh.in_list) == (5 if max_size == 120 else 1)
    if max_size == 120:
        assert np.bincount(np.concatenate(mesh.vOldInd_list), minlength=len(Vn)).min() >= 1
        assert np.bincount(np.concatenate(mesh.vOldInd_list), minlength=len(Vn)).max() >= 3
    net = FacetDenoiser(DEV, multi_scale=True, seed=0)
    x0 = utils.normalizePointSets(Vn, Vn)[0].astype(np.float32)
    res = T.inferNet(mesh, net, depth_dir=utils.view_rays(Vn, view_dir=(0, 0, 1)))
    free = T.inferNet(mesh, net)
    for k in range(3):
        assert res[k].shape == Vn.shape and np.array_equal(_bits(res[k][:, :2]), _bits(x0[:, :2])), k
        assert np.abs(res[k][:, 2] - x0[:, 2]).max() > 1e-4 and np.abs(free[k][:, :2] - x0[:, :2]).max() > 1e-5
    for k in range(3, 9):
        assert np.array_equal(res[k], free[k])
    cam = (0.4, 0.6, 3.0)
    rays = utils.view_rays(Vn, camera=cam)
    res = T.inferNet(mesh, net, depth_dir=rays)
    for k in range(3):
        off = np.linalg.norm(np.cross(res[k].astype(np.float64) - x0, rays.astype(np.float64)), axis=1).max()
        assert off <= 2.0 ** -21 * np.abs(x0).max() and np.abs(res[k] - x0).max() > 1e-4, (k, off)
    with pytest.raises(ValueError, match="depth_dir"):
        T.inferNet(mesh, net, depth_dir=rays[:7])


def test_commands_train_with_ray_update_and_infer_along_z(tmp_path, capsys, monkeypatch):
    """preprocess --clean --with-vertices, `train --with-vertices --synth-noise ... --noise-direction ray --view-dir 0,0,1
    --ray-update` for a few iterations (every bind asks for the constrained update), then `infer --with-vertices --view-dir
    0,0,1 --ray-update` with the saved network on a height field: three OBJ files whose x and y columns are the input's."""
    from facet_graph_convolution_amd import infer, preprocess
    from facet_graph_convolution_amd.meshgen import icosphere
    from facet_graph_convolution_amd.net import FacetDenoiser
    V, F = icosphere(2)
    clean, dump, path = (tmp_path / k for k in ("clean", "dump", "net"))
    clean.mkdir()
    utils.write_mesh(V, F, str(clean / "ball.obj"))
    preprocess.main([str(clean), str(dump), "--clean", "--with-vertices", "--valid", str(clean)])
    binds = []
    bind = FacetDenoiser.bind_clean_vertices

    def spy(self, *a, **k):
        binds.append(bool(k.get("ray_update")))
        return bind(self, *a, **k)
    monkeypatch.setattr(FacetDenoiser, "bind_clean_vertices", spy)
    capsys.readouterr()
    assert T.main([str(dump), str(path), "--with-vertices", "--synth-noise", "0.1,0.2", "--noise-direction", "ray",
                   "--view-dir", "0,0,1", "--ray-update", "--num-iterations", "3", "--net-name", "ray"]) == "trainAccuracyNet"
    out = capsys.readouterr().out
    assert "Iteration 0, validation loss" in out and "NAN" not in out and "nan" not in out
    assert len(binds) >= 4 and all(binds) and any(f.startswith("ray-3") for f in os.listdir(path))
    monkeypatch.undo()
    Vn, _, F = dc.height_field()
    noisy, res = tmp_path / "noisy", tmp_path / "res"
    noisy.mkdir()
    utils.write_mesh(Vn, F, str(noisy / "scan.obj"))
    infer.main([str(noisy), str(res), str(path), "--with-vertices", "--view-dir", "0,0,1", "--ray-update"])
    assert sorted(os.listdir(res)) == ["scan_d_coarse.obj", "scan_d_mid.obj", "scan_denoised.obj"]
    rows = lambda p: np.array([l.split()[1:4] for l in open(p) if l.startswith("v ")], dtype=np.float64)  # noqa: E731
    inp = rows(noisy / "scan.obj").astype(np.float32)             # what the command reads
    want = utils.normalizePointSets(inp, inp)[0].astype(np.float32)
    for name in os.listdir(res):
        got = rows(res / name)
        assert got.shape == Vn.shape
        assert np.array_equal(np.array(["%.6f" % v for v in want[:, :2].ravel()]),
                              np.array(["%.6f" % v for v in got[:, :2].ravel()])), name
        assert np.abs(got[:, 2] - want[:, 2]).max() > 1e-4, name
