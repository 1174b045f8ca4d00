"""GPU checks of the depth-scan mode: fgc_vertex_update_dir behind ops.vertex_update_dir and
train.update_position_with_depth, the drivers that take viewing rays, and noise synthesis along rays.  Nothing here
reads the reference: the yardsticks are the fixtures made by running its update_position_with_depth
(tests/golden/gen/make_golden_depth.py) and the float64 restatement of tests/depth_cases.py, which tests/test_depth_cpu.py
pins to those fixtures at 1e-12.

Bounds.  2e-6 absolute against float64 is what tests/test_gpu_ops.py holds the plain update to on the same meshes (the t
form in numpy float32 sits at 7e-8); against the reference's OWN float32 run 4e-6: the 2e-6 plus the reference's
float32-to-float64 gap, 1.5e-6 at most over the three cases, rounded up.  On the ray: x_out = fma(t, d, x0) rounds each
coordinate once, so |cross(x_out - x0, d)| <= sqrt(3) 2^-24 max|x| for unit d; the tests ask 2^-23 max|x|."""
import os
import sys

import numpy as np
import pytest
import torch

from facet_graph_convolution_amd import ops, utils
from facet_graph_convolution_amd import train as T
from facet_graph_convolution_amd.meshgen import icosphere

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAMERA = (0.3, -0.2, 4.0)
TOL64, TOL32 = 2e-6, 4e-6


def _dev(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)


def _run(V, normals, em, vem, dirs, iters, return_t=False, lmbd=dc.LAMBDA):
    out = ops.vertex_update_dir(_dev(V, np.float32), _dev(normals, np.float32), _dev(em, np.int32).reshape(-1, 4),
                                _dev(vem, np.int32), _dev(dirs, np.float32), iters, lmbd=lmbd, return_t=return_t)
    torch.cuda.synchronize()
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) if return_t else out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _off_ray(x_out, x0, d):
    """The largest |cross(x_out - x0, d)|, in float64 from the float32 values, d one row or one per vertex."""
    d = np.broadcast_to(np.asarray(d, dtype=np.float64).reshape(-1, 3), x0.shape)
    return np.linalg.norm(np.cross(x_out.astype(np.float64) - x0.astype(np.float64), d), axis=1).max()


@pytest.fixture(scope="module")
def ico3():
    """Noisy icosphere(3) of the ico3_rays fixture's making, with its clean normals, 20-slot tables and rays."""
    from facet_graph_convolution_amd.meshgen import add_noise
    V, F = icosphere(3)
    Vn = add_noise(V, F).astype(np.float32)
    em, vem = dc.edge_tables(F)
    return dict(V=V.astype(np.float32), Vn=Vn, F=F.astype(np.int32), n=utils.computeFacesNormals(V, F).astype(np.float32),
                em=em, vem=vem, rays=utils.view_rays(Vn, camera=CAMERA))


@pytest.mark.parametrize("tag", dc.CASES)
def test_fixtures(golden_dir, tag):
    z, z64 = dc.load(golden_dir, tag)
    x = _dev(z["verts"])[None]
    fn, em, vem, d = _dev(z["normals"])[None], _dev(z["edge_map"])[None], _dev(z["v_e_map"])[None], _dev(z["dirs"])
    for it in (0, 1, 2, 60):
        out, dx = T.update_position_with_depth(x, fn, em, vem, d, iter_num=it)
        assert out.shape == x.shape and dx.shape == x.shape and out.dtype == torch.float32
        assert torch.equal(dx, out - x)
        if it == 0:
            assert torch.equal(out, x) and not dx.any()
        if it in (1, 60):
            got = out[0].cpu().numpy()
            e64 = np.abs(got.astype(np.float64) - z64["x_%d" % it]).max()
            e32 = np.abs(got.astype(np.float64) - z["x_%d" % it].astype(np.float64)).max()
            ed = np.abs(dx[0].cpu().numpy().astype(np.float64) - z["dx_%d" % it].astype(np.float64)).max()
            print("%s, %d iterations: |gpu - f64| %.2e, |gpu - reference fp32| %.2e (dx %.2e)" % (tag, it, e64, e32, ed))
            assert e64 <= TOL64 and e32 <= TOL32 and ed <= TOL32


def test_vertices_stay_on_their_rays(ico3):
    m = ico3
    x, t = _run(m["Vn"], m["n"], m["em"], m["vem"], m["rays"], 60, return_t=True)
    off = _off_ray(x, m["Vn"], m["rays"])
    bound = 2.0 ** -23 * np.abs(m["Vn"]).max()
    print("off the ray after 60 iterations: %.2e (bound %.2e)" % (off, bound))
    assert off <= bound
    # x_out is fma(t, d, x0): the host's value (the product is exact in float64, one rounding of the sum, one to float32)
    host = (t.astype(np.float64)[:, None] * m["rays"].astype(np.float64) + m["Vn"].astype(np.float64)).astype(np.float32)
    assert (np.abs(x - host) <= np.spacing(np.abs(host))).all()
    assert np.abs(t).max() > 1e-3
    # along z the other two coordinates are not touched
    xz, tz = _run(m["Vn"], m["n"], m["em"], m["vem"], np.array([[0, 0, 1]], dtype=np.float32), 60, return_t=True)
    assert np.array_equal(_bits(xz[:, :2]), _bits(m["Vn"][:, :2]))
    assert np.abs(xz[:, 2] - m["Vn"][:, 2]).max() > 1e-3 and np.array_equal(_bits(xz[:, 2]), _bits(m["Vn"][:, 2] + tz))
    # iters = 0 through the op: the input bit for bit, t = 0
    x0, t0 = _run(m["Vn"], m["n"], m["em"], m["vem"], m["rays"], 0, return_t=True)
    assert np.array_equal(_bits(x0), _bits(m["Vn"])) and not t0.any()


@pytest.mark.parametrize("iters", [1, 5])
def test_directions_are_used_as_given(ico3, iters):
    """d of norm 0.5: the rule is (u . d) d, a quarter of the unit direction's step, nothing is normalised inside."""
    m = ico3
    d = (m["rays"] * np.float32(0.5)).astype(np.float32)
    got = _run(m["Vn"], m["n"], m["em"], m["vem"], d, iters)
    want, _ = dc.restate(m["Vn"], m["n"], m["em"], m["vem"], d, iters)
    unit, _ = dc.restate(m["Vn"], m["n"], m["em"], m["vem"], m["rays"], iters)
    err = np.abs(got - want).max()
    print("norm 0.5, %d iterations: |gpu - restatement| %.2e" % (iters, err))
    assert err <= TOL64 and np.abs(want - unit).max() > 1e-3


@pytest.mark.parametrize("name", ["t255", "t256", "t257", "single"])
def test_ragged_sizes(name):
    if name == "single":
        V = np.array([[0.1, 0.2, 0.3]], dtype=np.float32)
        n = np.array([[0, 0, 1]], dtype=np.float32)
        em, vem = np.zeros((0, 4), dtype=np.int32), np.full((1, 20), -1, dtype=np.int32)
    else:
        V, F = dc.ragged(name)
        n = utils.computeFacesNormals(V, F).astype(np.float32)
        V = (V + 0.02 * np.random.RandomState(1).standard_normal(V.shape)).astype(np.float32)
        em, vem = dc.tables_for(V, F)
    assert V.shape[0] == {"t255": 255, "t256": 256, "t257": 257, "single": 1}[name] == vem.shape[0]
    for dirs in (utils.view_rays(V, camera=CAMERA), utils.view_rays(V, view_dir=(0, 0.6, 0.8))):
        for iters in (1, 3, 20):
            got, t = _run(V, n, em, vem, dirs, iters, return_t=True)
            want, tw = dc.restate(V, n, em, vem, dirs, iters)
            assert np.abs(got - want).max() <= TOL64 and np.abs(t - tw).max() <= TOL64, (name, dirs.shape, iters)
            if name in ("t257", "single"):       # a vertex whose slots are all -1 comes back bit-equal
                assert np.array_equal(_bits(got[-1]), _bits(V[-1])) and t[-1] == 0
            if name != "single":
                assert np.abs(got - V).max() > 1e-3


def test_slots():
    """(lambda = 1/150 here: with 100 face terms at the hub the iteration of lambda = 1/18 diverges on this mesh.)"""
    lm = 1.0 / 150
    V, F = dc.fan(50)
    n = utils.computeFacesNormals(V, F).astype(np.float32)
    rs = np.random.RandomState(2)
    n = n + 0.2 * rs.standard_normal(n.shape).astype(np.float32)
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    em, vem = utils.getEdgeMap(F, maxEdges=50)
    assert em.shape == (100, 4) and (vem[0] >= 0).all() and vem.shape == (51, 50)
    rays = utils.view_rays(V, camera=(0.1, 0.2, 3.0))
    for iters in (1, 7):
        got = _run(V, n, em, vem, rays, iters, lmbd=lm)
        want, _ = dc.restate(V, n, em, vem, rays, iters, lm)
        assert np.abs(got - want).max() <= TOL64
    assert np.abs(got[0] - V[0]).max() > 1e-3 and np.abs(want).max() < 2
    with pytest.raises(RuntimeError):
        utils.getEdgeMap(F, maxEdges=20)
    # an unused slot BETWEEN used ones, and a slot value >= ne: the two `continue`s of the plain kernel
    gap = np.full((51, 50), -1, dtype=np.int32)
    gap[:, ::2] = vem[:, :25]                           # the rim's three edges at slots 0, 2, 4; half of the hub's
    big = vem.copy()
    big[1:, 3] = 100 + np.arange(50)                    # (the rim uses slots 0 .. 2)
    big[0, 49] = 2 ** 31 - 1
    for table in (gap, big):
        got = _run(V, n, em, table, rays, 3, lmbd=lm)
        want, _ = dc.restate(V, n, em, table, rays, 3, lm)
        assert np.abs(got - want).max() <= TOL64
    full, _ = dc.restate(V, n, em, vem, rays, 3, lm)
    wgap, _ = dc.restate(V, n, em, gap, rays, 3, lm)
    assert np.abs(full[0] - wgap[0]).max() > 1e-4       # the dropped hub edges matter: the case tests something


def test_it_denoises(ico3):
    """Noise of 0.3 mean edge lengths ALONG the rays, the clean normals, 20 iterations: the mean distance to the clean
    vertices falls below half (the float64 restatement gives 0.32 - 0.37 on this mesh).  A sanity check."""
    m = ico3
    rays = utils.view_rays(m["V"], camera=CAMERA)
    el = utils.getAverageEdgeLength(m["V"], m["F"])[0]
    g = np.random.RandomState(4).standard_normal(m["V"].shape[0])
    Vn = (m["V"].astype(np.float64) + 0.3 * el * g[:, None] * rays).astype(np.float32)
    got = _run(Vn, m["n"], m["em"], m["vem"], utils.view_rays(Vn, camera=CAMERA), 20)
    before = np.linalg.norm(Vn.astype(np.float64) - m["V"], axis=1).mean()
    after = np.linalg.norm(got.astype(np.float64) - m["V"], axis=1).mean()
    print("mean distance to the clean vertices: %.3e -> %.3e (x %.2f)" % (before, after, after / before))
    assert after < 0.5 * before


def test_bilateral_driver_takes_rays(ico3):
    from facet_graph_convolution_amd import bilateral
    from facet_graph_convolution_amd.settings import MAX_EDGES
    m = ico3
    pts, normals = bilateral.denoise_mesh(m["Vn"], m["F"], iterations=3, depth_dir=m["rays"])
    em, vem = utils.getEdgeMap(m["F"], maxEdges=MAX_EDGES)
    want = _run(m["Vn"], normals, em, vem, m["rays"], 60)
    assert np.array_equal(_bits(pts), _bits(want))
    plain, normals2 = bilateral.denoise_mesh(m["Vn"], m["F"], iterations=3)
    assert np.array_equal(_bits(normals), _bits(normals2)) and not np.array_equal(_bits(plain), _bits(pts))
    assert _off_ray(pts, m["Vn"], m["rays"]) <= 2.0 ** -23 * np.abs(m["Vn"]).max()
    assert _off_ray(plain, m["Vn"], m["rays"]) > 1e-4


def test_inference_driver_takes_rays(ico3):
    """inferNetOld on the mesh of the infer_ico3 fixture (noisy icosphere(3)), weights of seed 0."""
    from facet_graph_convolution_amd.dataClasses import InferenceMesh
    from facet_graph_convolution_amd.net import FacetDenoiser
    m = ico3
    mesh = InferenceMesh()
    mesh.addMesh(m["Vn"], m["F"], seed=0)
    net = FacetDenoiser(DEV, seed=0)
    pts, normals = T.inferNetOld(mesh, net, update_vertices=True, depth_dir=m["rays"])
    want = _run(m["Vn"], normals, mesh.edge_map[0], mesh.v_e_map[0], m["rays"], 60)
    assert pts.shape == m["Vn"].shape and np.array_equal(_bits(pts), _bits(want))
    plain, normals2 = T.inferNetOld(mesh, net, update_vertices=True)
    assert np.array_equal(_bits(normals), _bits(normals2)) and not np.array_equal(_bits(plain), _bits(pts))
    one, _ = T.inferNetOld(mesh, net, update_vertices=True, depth_dir=utils.view_rays(m["Vn"], view_dir=(0, 0, 1)))
    assert np.array_equal(_bits(one[:, :2]), _bits(m["Vn"][:, :2]))


def test_bilateral_cli_along_z_keeps_x_and_y(tmp_path):
    from facet_graph_convolution_amd import bilateral
    Vn, _, F = dc.height_field()
    noisy, res = tmp_path / "noisy", tmp_path / "res"
    noisy.mkdir()
    utils.write_mesh(Vn, F, str(noisy / "scan.obj"))
    bilateral.main([str(noisy), str(res), "--view-dir", "0,0,1", "--iterations", "2", "--vertex-iterations", "10"])
    rows = lambda p: [l.split() for l in open(p) if l.startswith("v ")]  # noqa: E731
    a, b = rows(noisy / "scan.obj"), rows(res / "scan_denoised.obj")
    assert len(a) == len(b) == Vn.shape[0]
    assert [r[1:3] for r in a] == [r[1:3] for r in b]
    assert sum(r[3] != s[3] for r, s in zip(a, b)) > len(a) // 2


def test_noise_along_rays(ico3):
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    from facet_graph_convolution_amd.makeNoisy import make_noisy
    from facet_graph_convolution_amd.net import FacetDenoiser
    m = ico3
    V, F = m["V"], m["F"]
    rays = utils.view_rays(V, camera=CAMERA)
    el = utils.getAverageEdgeLength(V, F)[0]
    got = make_noisy(V, F, 0.2, seed=3, stream=2, step=5, direction=rays)
    want = ops.synth_noise(_dev(V), np.float32(0.2) * np.float32(el), 5, seed=3, stream=2, normals=_dev(rays)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want)) and not np.array_equal(_bits(got), _bits(V))
    assert not np.array_equal(_bits(got), _bits(make_noisy(V, F, 0.2, seed=3, stream=2, step=5, direction="normal")))
    # bind_clean with a table of rays: the displacement is parallel to them
    ds = TrainingSet()
    ds.addCleanMesh(V, F, seed=0)
    args = (ds.in_list[0], ds.adj_list[0], ds.gt_list[0], ds.clean_vertices[0], ds.clean_faces_rows[0], ds.clean_edge_len[0])
    net = FacetDenoiser(DEV, seed=0)
    net.bind_clean("scan", *args, seed=3, stream=2, direction=rays)
    net.set_noise(5, 0.2)
    net.forward(rotate=False)
    torch.cuda.synchronize()
    vn = net.noisy_vertices().cpu().numpy()
    cv = np.asarray(ds.clean_vertices[0], dtype=np.float32).reshape(-1, 3)
    assert np.array_equal(_bits(vn), _bits(make_noisy(cv, F, 0.2, seed=3, stream=2, step=5, direction=rays)))
    off, bound = _off_ray(vn, cv, rays), 2.0 ** -23 * np.abs(vn).max()
    print("noise off the ray: %.2e (bound %.2e)" % (off, bound))
    assert off <= bound and np.abs(vn - cv).max() > 1e-3
    net.bind_clean("scan", *args, seed=3, stream=2, direction=rays.copy())           # the same rows: a lookup
    with pytest.raises(ValueError, match="another seed / stream / direction"):
        net.bind_clean("scan", *args, seed=3, stream=2, direction=utils.view_rays(V, camera=(0, 0, 6)))
    with pytest.raises(ValueError, match="another seed / stream / direction"):
        net.bind_clean("scan", *args, seed=3, stream=2, direction="normal")


def test_trainer_takes_a_view(ico3):
    """trainNet(noise_direction={'camera': ...}): every step's noise runs along the rays of the mesh's CLEAN vertices - the
    table make_noisy is given by `makeNoisy --direction ray` - and the run is finite; a wrong view name is refused."""
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    from facet_graph_convolution_amd.makeNoisy import make_noisy
    m = ico3
    ds = TrainingSet()
    ds.addCleanMesh(m["V"], m["F"], seed=0)
    net, loss = T.trainNet(ds, 3, seed=0, log=lambda s: None, noise_levels=(0.2,), noise_direction={"camera": CAMERA})
    torch.cuda.synchronize()
    assert np.isfinite(np.asarray(loss)).all()
    cv = np.asarray(ds.clean_vertices[0], dtype=np.float32).reshape(-1, 3)
    rays = utils.view_rays(cv, camera=CAMERA)
    vn = net.noisy_vertices().cpu().numpy()                      # the last step: counter 2, training stream 0
    assert np.array_equal(_bits(vn), _bits(make_noisy(cv, m["F"], 0.2, seed=0, stream=0, step=2, direction=rays)))
    assert _off_ray(vn, cv, rays) <= 2.0 ** -23 * np.abs(vn).max() and np.abs(vn - cv).max() > 1e-3
    with pytest.raises(ValueError, match="a view is"):
        T.trainNet(ds, 1, seed=0, log=lambda s: None, noise_levels=(0.2,), noise_direction={"eye": CAMERA})


def test_make_noisy_cli_along_rays(tmp_path):
    """`makeNoisy --direction ray --camera`: file k of mesh i is make_noisy with the rays of the CLEAN vertices, stream
    1 + i and step k - the validation mesh of a training run with the same seed and view."""
    from facet_graph_convolution_amd import makeNoisy
    V, F = icosphere(1)
    clean, out = tmp_path / "clean", tmp_path / "noisy"
    clean.mkdir()
    utils.write_mesh(V, F, str(clean / "ball.obj"))
    written = makeNoisy.main([str(clean), str(out), "--levels", "0.1,0.2", "--direction", "ray", "--camera", "0,0,5", "--seed", "4"])
    assert [os.path.basename(p) for p in written] == ["ball_n1.obj", "ball_n2.obj"]
    Vc, _, _, Fc, _ = utils.load_mesh(str(clean), "ball.obj", 0, False)
    rays = utils.view_rays(Vc, camera=(0, 0, 5))
    for k, level in enumerate((0.1, 0.2)):
        got = utils.load_mesh(str(out), "ball_n%d.obj" % (k + 1), 0, False)[0]
        want = makeNoisy.make_noisy(Vc, Fc, level, 4, 1, k, rays)
        assert np.abs(got - want).max() <= 1e-6                 # (the file keeps 6 decimals)
        assert _off_ray(want, Vc, rays) <= 2.0 ** -23 * np.abs(want).max() and np.abs(want - Vc).max() > 1e-3
