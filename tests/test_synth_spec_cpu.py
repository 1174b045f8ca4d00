"""synth.py without a GPU: the refusals and the key of a NoiseSpec, and the entry point a NoisePlan chooses - recorded from the
one dispatch that FacetDenoiser's steps and makeNoisy.make_noisy share."""
import numpy as np
import pytest
import torch

from facet_graph_convolution_amd import _lib, ops, synth, utils
from facet_graph_convolution_amd.meshgen import icosphere
from facet_graph_convolution_amd.synth import NoisePlan, NoiseSpec

CAMERA = (2.5, 0.4, 1.2)


@pytest.fixture(scope="module")
def mesh():
    V, F = icosphere(1)
    V = np.asarray(V, dtype=np.float32)
    rays = np.ascontiguousarray(np.broadcast_to(utils.view_rays(V, camera=CAMERA), V.shape)).astype(np.float32)
    edge_len = float(utils.getAverageEdgeLength(V, F)[0])
    return V, F, rays, edge_len, utils.sensor_model(V, CAMERA, edge_len, 2, 0.5)


def test_a_spec_makes_the_refusals_of_a_bind(mesh):
    V, F, rays, edge_len, model = mesh
    nv = V.shape[0]
    for d in ("sideways", ""):
        with pytest.raises(ValueError, match="direction must be 'random', 'normal' or a \\[V,3\\] array of unit rows"):
            NoiseSpec(direction=d).check(nv)
    nan, half = rays.copy(), rays.copy()
    nan[3, 1] = np.nan
    half[5] *= 0.5
    for d, msg in ((rays[:-1], "one row per vertex"), (nan, "finite"), (half, "unit vectors")):
        with pytest.raises(ValueError, match=msg):
            NoiseSpec(direction=d).check(nv)
    for d in ("random", "normal"):
        with pytest.raises(ValueError, match="sensor: the model works along viewing rays: direction must be the \\[V,3\\] table"):
            NoiseSpec(direction=d, sensor=model).check(nv)
    with pytest.raises(ValueError, match="sensor: a model \\(power, r_ref, q, camera\\)"):
        NoiseSpec(direction=rays, sensor=(2, 0.5)).check(nv)
    with pytest.raises(ValueError, match="sensor: quantisation after bumps along the normals \\(lf=\\) is not built; choose one"):
        NoiseSpec(direction=rays, lf=(3.0, None), sensor=model).check(nv)
    for stream in (1 << 31, (1 << 32) - 1, -1):
        with pytest.raises(ValueError, match="lf: stream must lie below 2\\^31"):
            NoiseSpec(stream=stream, lf=(3.0, None)).check(nv)
    # the same stream without bumps is fine, and every valid setting returns its table of rays (a copy) or None
    assert NoiseSpec(stream=1 << 31).check(nv) is None and NoiseSpec(direction="normal", lf=(3.0, 7)).check(nv) is None
    got = NoiseSpec(direction=rays, sensor=model).check(nv)
    assert got is not rays and got.dtype == np.float32 and got.tobytes() == rays.tobytes()
    with pytest.raises(ValueError, match="edge_len must be a positive length"):
        NoisePlan(NoiseSpec(), V, F, 0.0, "cpu")


def test_the_key_two_binds_are_compared_by(mesh):
    V, F, rays, edge_len, model = mesh
    base = NoiseSpec(7, 1, rays, None, model)
    k = base.key()
    assert hash(k) is not None and k == base._replace(direction=rays.copy()).key()
    assert k == base._replace(direction=rays.astype(np.float64)).key() and k == base._replace(ray_update=True).key()
    other = rays.copy()
    other[2] = other[3]
    changed = [base._replace(direction=other), base._replace(seed=8), base._replace(stream=2), base._replace(sensor=None),
               base._replace(sensor=model._replace(power=1)), base._replace(sensor=model._replace(q=model.q * 2)),
               base._replace(sensor=model._replace(r_ref=model.r_ref * 2)),
               base._replace(sensor=model._replace(camera=(2.5, 0.4, 1.25)))]
    assert all(c.key() != k for c in changed)
    lf = NoiseSpec(7, 1, "normal", (3.0, None))
    assert lf.key() == NoiseSpec(7, 1, "normal", (3, None)).key() and lf.key().direction == "normal"
    assert all(lf._replace(lf=pair).key() != lf.key() for pair in (None, (2.0, None), (3.0, 12)))
    assert lf._replace(direction="random").key() != lf.key()
    # the very same read-only table takes the bound key's digest; a writeable one is digested again
    ro = rays.copy()
    ro.setflags(write=False)
    bound = NoiseSpec(7, 1, ro)
    stale = bound.key()._replace(direction=("rays", "taken as it is"))
    assert NoiseSpec(7, 1, ro).key(bound=(bound, stale)) == stale
    assert NoiseSpec(7, 1, rays).key(bound=(NoiseSpec(7, 1, rays), stale)) == bound.key()


ENTRIES = ("fgc_synth_noise", "fgc_synth_noise_lf", "fgc_synth_noise_sensor")


def test_a_plan_chooses_the_entry_point_and_the_tables(mesh, monkeypatch):
    """The five settings: what make_noisy called before there was a plan - fgc_synth_noise for random / normal / rays (white
    table: none / the vertex normals / the rays), fgc_synth_noise_lf with the bumps along the vertex normals whatever the
    white table, fgc_synth_noise_sensor along the rays - through the three library calls replaced by recorders."""
    V, F, rays, edge_len, model = mesh
    nv = V.shape[0]
    L = _lib.lib()
    calls = []
    for name in ENTRIES:
        monkeypatch.setattr(L, name, lambda *a, _n=name: calls.append((_n, a)) or 0, raising=True)
    vn = utils.areaWeightedVertexNormals(V, F).astype(np.float32)

    def run(spec):
        plan = NoisePlan(spec, V, F, edge_len, "cpu")
        v = torch.from_numpy(V.copy())
        out, scratch = torch.empty_like(v), torch.zeros(max(plan.scratch_floats, 1))
        ctl = torch.from_numpy(plan.noise_words(3, 0.2))
        lf_ctl = None if plan.lf is None else torch.from_numpy(plan.lf_words(0.3))
        del calls[:]
        synth.enqueue(plan, v, out, scratch, ctl, lf_ctl, None)
        assert len(calls) == 1 and calls[0][0] == plan.entry
        return plan, calls[0][1], (v, out, scratch, ctl, lf_ctl)

    def table(t):
        return None if t is None else t.numpy().tobytes()

    ptr = lambda t: t.data_ptr()  # noqa: E731
    for direction, white in (("random", None), ("normal", vn), (rays, rays)):
        plan, a, (v, out, scratch, ctl, _) = run(NoiseSpec(7, 2, direction))
        assert plan.entry == "fgc_synth_noise" and table(plan.white) == (None if white is None else white.tobytes())
        assert plan.scratch_floats == L.fgc_synth_scratch_floats(nv) and plan.lf is None and plan.sensor_ctl is None
        assert [a[0].value, a[2], a[3].value, a[4], a[5], a[6].value, a[7].value, a[8], a[9]] == \
            [ptr(v), nv, ptr(ctl), 7, 2, ptr(out), ptr(scratch), scratch.numel(), None]
        assert (a[1] is None) if white is None else (a[1].value == ptr(plan.white))
        # bumps on top: along the vertex normals, whatever the white table
        plan, a, (v, out, scratch, ctl, lf_ctl) = run(NoiseSpec(7, 2, direction, (3.0, None)))
        assert plan.entry == "fgc_synth_noise_lf" and table(plan.white) == (None if white is None else white.tobytes())
        assert table(plan.bump_normals) == vn.tobytes() and plan.lf.K == -(-F.shape[0] // 6)
        assert plan.lf.width == 3.0 * edge_len and plan.scratch_floats == L.fgc_synth_lf_scratch_floats(nv, plan.lf.K)
        assert [a[0].value, a[1].value, a[3], a[4].value, a[5].value, a[6], a[7], a[8]] == \
            [ptr(v), ptr(plan.bump_normals), nv, ptr(ctl), ptr(lf_ctl), plan.lf.K, 7, 2]
        assert (a[2] is None) if white is None else (a[2].value == ptr(plan.white))
    plan, a, (v, out, scratch, ctl, _) = run(NoiseSpec(7, 2, rays, None, model))
    assert plan.entry == "fgc_synth_noise_sensor" and table(plan.white) == rays.tobytes()
    assert plan.scratch_floats == L.fgc_synth_scratch_floats(nv)
    assert plan.sensor_ctl.numpy().view(np.uint32).tolist() == [int(w) for w in ops.sensor_words(model.power, model.r_ref, model.q)]
    assert tuple(plan.camera) == tuple(float(np.float32(c)) for c in CAMERA)
    assert [a[0].value, a[1].value, a[2], a[3].value, a[4].value, a[5], a[6], a[7]] == \
        [ptr(v), ptr(plan.white), nv, ptr(ctl), ptr(plan.sensor_ctl), plan.camera, 7, 2]
    # the control words of a level are those of level x edge length in fp32, None switches off
    assert plan.noise_words(3, 0.2).tobytes() == ops.noise_words(3, np.float32(0.2) * np.float32(edge_len)).tobytes()
    assert not plan.noise_words(3, None).any()


def test_make_noisy_goes_through_the_same_dispatch(mesh, monkeypatch):
    """make_noisy on the five settings reaches the entry point it called before it was built on the plan."""
    from facet_graph_convolution_amd.makeNoisy import make_noisy
    V, F, rays, edge_len, model = mesh
    L = _lib.lib()
    calls = []
    for name in ENTRIES:
        monkeypatch.setattr(L, name, lambda *a, _n=name: calls.append(_n) or 0, raising=True)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(ops, "_req_cuda", lambda *t: None)      # (host tensors: nothing here dereferences them)
    for kw, entry in ((dict(direction="random"), "fgc_synth_noise"), (dict(direction="normal"), "fgc_synth_noise"),
                      (dict(direction=rays), "fgc_synth_noise"), (dict(direction="random", lf_level=0.3), "fgc_synth_noise_lf"),
                      (dict(direction=rays, lf_level=0.3), "fgc_synth_noise_lf"),
                      (dict(direction=rays, sensor=(2, 0.5), camera=CAMERA), "fgc_synth_noise_sensor")):
        del calls[:]
        out = make_noisy(V, F, 0.2, seed=7, stream=2, step=3, device="cpu", **kw)
        assert calls == [entry] and out.shape == V.shape and out.dtype == np.float32
