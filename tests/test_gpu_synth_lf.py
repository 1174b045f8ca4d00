"""Low-frequency noise synthesis on the GPU (include/fgc.h: fgc_synth_noise_lf; FacetDenoiser.bind_clean(lf=...),
set_noise(step, level, lf_level)) against the float64 oracle of its definition (tests/lf_noise_cases.py), the white path it
must reproduce when the bumps are off, the host routines downstream of it, and the offline loop from makeNoisy to
computeMetrics."""
import functools
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_cases as sc  # noqa: E402
import lf_noise_cases as lf  # noqa: E402

from facet_graph_convolution_amd import ops, utils
from facet_graph_convolution_amd.dataClasses import TrainingSet
from facet_graph_convolution_amd.meshgen import icosphere, torus, flip_edges

pytestmark = pytest.mark.gpu

SEED = 1234
STEPS = (0, 1, 7)
DEV = "cuda:0"
TAGS = ("ico3", "torus", "flipped")
# 1000 and 5000 are split into slices over blockIdx.y on these meshes (3 and 12 vertex blocks: 3 and 19 slices)
BUMPS = (1, 15, 17, 214, 1000, 5000)


@functools.lru_cache(maxsize=None)
def _mesh(tag):
    if tag == "ico3":
        return icosphere(3)
    if tag == "torus":
        return torus(60, 50)
    V, F = torus(24, 20)
    return V, flip_edges(F, 400, seed=1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _geom(tag):
    """(fp32 vertex normals the kernel is given, mean edge length)."""
    V, F = _mesh(tag)
    return utils.areaWeightedVertexNormals(V, F).astype(np.float32), float(utils.getAverageEdgeLength(V, F)[0])


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _run(V, vn, K, width, amplitude, step, sigma=0.0, seed=SEED, stream=0, white_normals=None, **kw):
    out = ops.synth_noise_lf(torch.as_tensor(V, device=DEV), torch.as_tensor(vn, device=DEV), sigma, step, amplitude, width, K,
                             seed=seed, stream=stream,
                             white_normals=None if white_normals is None else torch.as_tensor(white_normals, device=DEV), **kw)
    return out.cpu().numpy()


def _field_of(V, vn, out):
    """The field the kernel applied, read back from v_out = V + vn s (sigma 0): the displacement along the normal.  The
    final add's rounding, at most 2^-24 max|V| per coordinate, enters with sum |vn_t| <= sqrt(3): below 2^-23 max|V|."""
    d = out.astype(np.float64) - V.astype(np.float64)
    n = vn.astype(np.float64)
    return (d * n).sum(1) / (n * n).sum(1)


def _check_field(V, vn, K, width, amplitude, step, what, stream=0):
    """One call at white sigma 0 against float64, per vertex, with the issue's bound; returns error / bound."""
    nv = V.shape[0]
    out = _run(V, vn, K, width, amplitude, step, stream=stream)
    centres, amps = lf.bump_table(nv, K, step, SEED, stream, amplitude)
    s64, T = lf.field(V, centres, amps, width)
    bound = lf.field_bound(T, K, np.abs(V).max())
    err = np.abs(_field_of(V, vn, out) - s64)
    worst = float((err / bound).max())
    print("%s K %d width %.4f step %d: worst |s - s64| / bound = %.3f (max |s64| %.3e)" % (what, K, width, step, worst,
                                                                                          np.abs(s64).max()))
    assert np.isfinite(out).all() and (err <= bound).all(), (what, K, width, step, worst)
    if K == 1 and nv > 1:
        # the single bump peaks on its centre, the clean vertex mulhi32(x0, nv)
        x0 = int(lf.bump_words(1, step, SEED, stream)[0][0])
        assert int(np.abs(_field_of(V, vn, out)).argmax()) == lf.mulhi32(x0, nv), (what, step)
    return worst


@pytest.mark.parametrize("K", BUMPS)
@pytest.mark.parametrize("tag", TAGS)
def test_field_matches_the_float64_oracle(tag, K):
    """|s_gpu - s_64| <= (1e-5 + (K + 16) 2^-24) T_i + 2^-23 max|V|, T_i = sum_k |a_k| (1 + t_ik) e^-t_ik: 1e-5 for the fp32
    Gaussian (the allowance of test_gpu_synth.py), K 2^-24 for an fp32 sum of K terms in any order, 16 ulp for the rounded
    exponent argument and the hardware exponential (their error grows with t: the factor 1 + t), 2^-23 max|V| for the
    final add."""
    V, F = _mesh(tag)
    vn, edge = _geom(tag)
    worst = 0.0
    for width_rel in (1.0, 3.0):
        for step in STEPS:
            worst = max(worst, _check_field(V, vn, K, width_rel * edge, 0.3 * edge, step, tag))
    print("%s K %d: worst error / bound = %.3f" % (tag, K, worst))


@pytest.mark.parametrize("tag", TAGS)
def test_the_bump_table_holds_the_centres_and_amplitudes(tag):
    """The table the first launch leaves in the scratch (include/fgc.h: behind the box partials, at the next multiple of 4
    floats): row k is the clean vertex mulhi32(x0_k, nv) bit for bit and a_k = A z within the fp32 Gaussian's 1e-5."""
    V, F = _mesh(tag)
    vn, edge = _geom(tag)
    L = ops._lib.lib()
    amp = 0.3 * edge
    for K in (17, 1000):
        for step in STEPS:
            scratch = torch.zeros(L.fgc_synth_lf_scratch_floats(len(V), K), dtype=torch.float32, device=DEV)
            _run(V, vn, K, 3.0 * edge, amp, step, stream=2, scratch=scratch)
            at = -(-L.fgc_synth_scratch_floats(len(V)) // 4) * 4
            table = scratch[at:at + 4 * K].cpu().numpy().reshape(K, 4)
            words = lf.bump_words(K, step, SEED, 2)
            centres = np.array([lf.mulhi32(x, len(V)) for x in words[0]])
            _, amps = lf.bump_table(len(V), K, step, SEED, 2, amp)
            assert np.array_equal(_bits(table[:, :3]), _bits(V[centres])), (tag, K, step)
            assert np.abs(table[:, 3] - amps).max() <= 1e-5 * amp * max(1.0, np.abs(amps / amp).max()), (tag, K, step)
            assert len(set(centres.tolist())) > min(K, len(V)) // 2


@pytest.mark.parametrize("nv", [1, 257])
def test_field_on_vertex_prefixes(nv):
    V, F = _mesh("torus")
    vn, edge = _geom("torus")
    for K in (1, 17):
        for step in STEPS:
            _check_field(V[:nv].copy(), vn[:nv].copy(), K, 3.0 * edge, 0.3 * edge, step, "prefix %d" % nv)


@pytest.mark.parametrize("K", [17, 512])
def test_field_above_the_partial_box_cap(K):
    """262 145 = 1 024 x 256 + 1 vertices: the first size at which a workgroup owns more than one vertex (the stride of
    fgc_synth_noise's capped launch); 512 bumps there are two slices."""
    nv = 262145
    rs = np.random.RandomState(nv)
    V = (rs.uniform(-1, 1, (nv, 3)) * [3.0, 1.0, 0.5]).astype(np.float32)
    vn = rs.normal(size=(nv, 3))
    vn = (vn / np.linalg.norm(vn, axis=1, keepdims=True)).astype(np.float32)
    out = _run(V, vn, K, 0.4, 0.05, 3)
    centres, amps = lf.bump_table(nv, K, 3, SEED, 0, 0.05)
    s64, T = lf.field(V, centres, amps, 0.4, chunk=16)
    bound = lf.field_bound(T, K, np.abs(V).max())
    err = np.abs(_field_of(V, vn, out) - s64)
    print("262145 vertices, K %d: worst |s - s64| / bound = %.3f" % (K, (err / bound).max()))
    assert (err <= bound).all()
    # bumps off: vertices and boxes of the white path at this size too
    Vd, nd = torch.as_tensor(V, device=DEV), torch.as_tensor(vn, device=DEV)
    need = 6 * 1024
    s_lf = torch.zeros(ops._lib.lib().fgc_synth_lf_scratch_floats(nv, K), dtype=torch.float32, device=DEV)
    s_w = torch.zeros(need, dtype=torch.float32, device=DEV)
    off = torch.zeros(4, dtype=torch.int32, device=DEV)
    a = ops.synth_noise_lf(Vd, nd, 0.02, 5, None, None, K, seed=SEED, scratch=s_lf, lf_ctl=off)
    b = ops.synth_noise(Vd, 0.02, 5, seed=SEED, scratch=s_w)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(s_lf[:need].view(torch.int32), s_w.view(torch.int32))


@pytest.mark.parametrize("direction", ["random", "normal"])
@pytest.mark.parametrize("tag", TAGS)
def test_white_plus_bumps_matches_the_two_oracles(tag, direction):
    """v_out = the white oracle's displaced vertex + vn s: the bound is the white one of test_gpu_synth.py (1e-5 sigma +
    2^-23 max|V|) plus the field's."""
    V, F = _mesh(tag)
    vn, edge = _geom(tag)
    sigma, width, amp = np.float32(0.2) * np.float32(edge), 3.0 * edge, 0.3 * edge
    worst = 0.0
    for K in (17, 1000):
        for step in STEPS:
            out = _run(V, vn, K, width, amp, step, sigma=sigma, white_normals=vn if direction == "normal" else None)
            white = sc.oracle(V, F, sigma, step, SEED, 0, direction)
            centres, amps = lf.bump_table(len(V), K, step, SEED, 0, amp)
            s64, T = lf.field(V, centres, amps, width)
            want = white + vn.astype(np.float64) * s64[:, None]
            bound = (1e-5 * float(sigma) + 2.0 ** -23 * float(np.abs(V).max())) + lf.field_bound(T, K, np.abs(V).max())
            err = np.abs(out.astype(np.float64) - want).max(1)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (tag, direction, K, step, float((err / bound).max()))
            # ... and both parts are there
            assert np.abs(out - V).max() > 0.1 * float(sigma) and np.abs(out.astype(np.float64) - white).max() > 0.05 * amp
    print("%s %s: worst error / bound = %.3f" % (tag, direction, worst))


@pytest.mark.parametrize("direction", ["random", "normal"])
@pytest.mark.parametrize("tag", TAGS)
def test_bumps_off_is_the_white_path_bit_for_bit(tag, direction):
    V, F = _mesh(tag)
    vn, edge = _geom(tag)
    Vd, nd = torch.as_tensor(V, device=DEV), torch.as_tensor(vn, device=DEV)
    wn = nd if direction == "normal" else None
    L = ops._lib.lib()
    nbox = L.fgc_synth_scratch_floats(len(V))
    off = torch.zeros(4, dtype=torch.int32, device=DEV)
    for K in (17, 1000):
        for sigma in (0.0, 0.2 * edge):
            s_lf = torch.full((L.fgc_synth_lf_scratch_floats(len(V), K),), 7.0, dtype=torch.float32, device=DEV)
            s_w = torch.full((nbox,), 7.0, dtype=torch.float32, device=DEV)
            a = ops.synth_noise_lf(Vd, nd, sigma, 5, None, None, K, seed=SEED, stream=2, white_normals=wn, scratch=s_lf,
                                   lf_ctl=off)
            b = ops.synth_noise(Vd, sigma, 5, seed=SEED, stream=2, normals=wn, scratch=s_w)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (K, sigma)
            assert torch.equal(s_lf[:nbox].view(torch.int32), s_w.view(torch.int32)), (K, sigma)
            assert (s_lf[nbox:] == 7.0).all().item()          # table, slice sums and counters are not touched
            # ops.lf_words(None, ...) are those zeros
            c = ops.synth_noise_lf(Vd, nd, sigma, 5, None, 3.0 * edge, K, seed=SEED, stream=2, white_normals=wn)
            assert torch.equal(a, c)
    # ctl[2] = 0 switches everything off: nothing is written
    out = torch.full_like(Vd, 3.0)
    s_lf = torch.full((L.fgc_synth_lf_scratch_floats(len(V), 1000),), 7.0, dtype=torch.float32, device=DEV)
    on = torch.from_numpy(ops.lf_words(0.3 * edge, 3.0 * edge).view(np.int32)).to(DEV)
    ops.synth_noise_lf(Vd, nd, None, 5, None, None, 1000, seed=SEED, out=out, scratch=s_lf, lf_ctl=on,
                       ctl=torch.zeros(3, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert (out == 3.0).all().item() and (s_lf == 7.0).all().item()


def test_the_boxes_are_those_of_the_final_vertices():
    """The scratch's head after a call with bumps: per vertex block of 256 the bounding box of v_out."""
    V, F = _mesh("torus")
    vn, edge = _geom("torus")
    L = ops._lib.lib()
    for K in (17, 1000):
        scratch = torch.zeros(L.fgc_synth_lf_scratch_floats(len(V), K), dtype=torch.float32, device=DEV)
        out = _run(V, vn, K, 3.0 * edge, 0.5 * edge, 3, sigma=0.1 * edge, scratch=scratch)
        boxes = scratch[:L.fgc_synth_scratch_floats(len(V))].cpu().numpy().reshape(-1, 6)
        assert boxes.shape[0] == -(-len(V) // 256)
        for b in range(boxes.shape[0]):
            blk = out[256 * b:256 * (b + 1)]
            assert np.array_equal(boxes[b, :3], blk.min(0)) and np.array_equal(boxes[b, 3:], blk.max(0)), (K, b)
        assert not np.array_equal(boxes[:, :3].min(0), V.min(0))


def test_field_is_deterministic_and_moves_with_step_stream_and_seed():
    V, F = _mesh("torus")
    vn, edge = _geom("torus")
    for K in (214, 1000):
        run = lambda **kw: _run(V, vn, K, 3.0 * edge, 0.3 * edge, **{"step": 7, "stream": 2, **kw})  # noqa: E731
        a = run()
        for _ in range(3):
            assert np.array_equal(_bits(a), _bits(run()))
        for other in (run(step=8), run(stream=3), run(seed=SEED + 1), run(step=7 + (1 << 32)), run(seed=SEED + (1 << 32))):
            assert (np.abs(other - a).max(1) > 0).mean() > 0.9
    # the bump counters are not the per-vertex ones: with the amplitude of the white sigma the two displacements differ
    w = ops.synth_noise(torch.as_tensor(V, device=DEV), 0.3 * edge, 7, seed=SEED, stream=2,
                        normals=torch.as_tensor(vn, device=DEV)).cpu().numpy()
    assert not np.allclose(w, _run(V, vn, len(V), 3.0 * edge, 0.3 * edge, 7, stream=2), atol=1e-3 * edge)


# ---- the network ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _clean_set(tag, vertices=False):
    V, F = _mesh(tag)
    ds = TrainingSet()
    (ds.addCleanMeshWithVertices if vertices else ds.addCleanMesh)(V, F, seed=0)
    return ds


def _faces_of(ds):
    rows = ds.clean_faces_rows[0][0]
    return rows[np.asarray(ds.permutations[0])][:ds.num_faces[0]].astype(np.uint32)


def _host_rows(ds, V):
    nrm, ctr = utils.face_features(V, _faces_of(ds))
    per_face = np.concatenate([nrm.astype(np.float32), ctr.astype(np.float32)], axis=1)
    return sc.rows_in_node_order(per_face, ds.permutations[0], ds.in_list[0].shape[1])


def _bound_net(tag, lf_arg=(3.0, None), direction="random", stream=0, key="m", net=None):
    from facet_graph_convolution_amd.net import FacetDenoiser
    ds = _clean_set(tag)
    net = net or FacetDenoiser(DEV, seed=0)
    net.bind_clean(key, ds.in_list[0], ds.adj_list[0], ds.gt_list[0], ds.clean_vertices[0], ds.clean_faces_rows[0],
                   ds.clean_edge_len[0], seed=SEED, stream=stream, direction=direction, lf=lf_arg)
    return net, ds


def _bound_vertex_net(tag, lf_arg=(3.0, None), direction="random", key="m"):
    from facet_graph_convolution_amd.net import FacetDenoiser
    ds = _clean_set(tag, True)
    net = FacetDenoiser(DEV, multi_scale=True, seed=0)
    net.bind_clean_vertices(key, ds.in_list[0], ds.adj_list[0], ds.clean_vertices[0], ds.clean_faces_rows[0],
                            ds.v_faces_list[0], ds.clean_edge_len[0], seed=SEED, direction=direction, lf=lf_arg)
    return net, ds


def _rotation(seed=3):
    return utils.rand_rotation_matrix(randnums=np.random.RandomState(seed).uniform(size=3)).astype(np.float32)


@pytest.mark.parametrize("tag,direction", [("ico3", "random"), ("flipped", "normal")])
def test_a_network_bound_with_lf_and_no_lf_level_is_the_white_network(tag, direction):
    net, ds = _bound_net(tag, direction=direction)
    white, _ = _bound_net(tag, lf_arg=None, direction=direction)
    assert net._mesh["synth"].plan.lf.K == -(-ds.num_faces[0] // 6) and white._mesh["synth"].plan.lf is None
    for step, level in ((7, 0.2), (8, 0.0)):
        for n in (net, white):
            n.set_noise(step, level)
            n.forward(rotate=False)
        torch.cuda.synchronize()
        assert torch.equal(net.buffers["x"].view(torch.int32), white.buffers["x"].view(torch.int32))
        assert torch.equal(net.noisy_vertices().view(torch.int32), white.noisy_vertices().view(torch.int32))
    # a step with bumps, then without: the white rows again (set_noise without lf_level clears the bump words)
    net.set_noise(7, 0.2, 0.3)
    net.forward(rotate=False)
    assert not torch.equal(net.buffers["x"], white.buffers["x"])
    net.set_noise(8, 0.0)
    net.forward(rotate=False)
    torch.cuda.synchronize()
    assert torch.equal(net.buffers["x"].view(torch.int32), white.buffers["x"].view(torch.int32))
    assert np.array_equal(_bits(net.noisy_vertices().cpu().numpy()), _bits(_mesh(tag)[0]))


@pytest.mark.parametrize("tag,direction", [("ico3", "random"), ("flipped", "normal")])
def test_the_network_draws_what_make_noisy_draws_and_feeds_the_host_routine_rows(tag, direction):
    """After a synthesising step: noisy_vertices() are makeNoisy's for the same arguments, and the input rows equal
    utils.face_features of them in node order, bit for bit (the boxes the rows kernel read are the final ones)."""
    from facet_graph_convolution_amd.makeNoisy import make_noisy
    V, F = _mesh(tag)
    net, ds = _bound_net(tag, lf_arg=(3.0, None), direction=direction, stream=4)
    for step, level, lf_level in ((0, 0.0, 0.3), (7, 0.1, 0.2)):
        net.set_noise(step, level, lf_level)
        net.forward(rotate=False)
        torch.cuda.synchronize()
        Vn = net.noisy_vertices().cpu().numpy()
        want = make_noisy(V, F, level, seed=SEED, stream=4, step=step, direction=direction, lf_level=lf_level)
        assert np.abs(Vn - V).max() > 0.05 * ds.clean_edge_len[0]
        assert np.abs(Vn - want).max() <= 1e-6 * max(1.0, float(np.abs(V).max()))
        diff = _bits(net.buffers["x"].cpu().numpy()) != _bits(_host_rows(ds, Vn))
        print("%s step %d: %d of %d words of the rows differ" % (tag, step, int(diff.sum()), diff.size))
        assert not diff.any()


@pytest.mark.parametrize("tag,direction", [("ico3", "random"), ("flipped", "normal")])
def test_prepared_point_sets_are_those_of_the_final_vertices(tag, direction):
    net, ds = _bound_vertex_net(tag, direction=direction)
    V = ds.clean_vertices[0][0]
    rs = np.random.RandomState(2)
    net.set_point_samples(rs.randint(len(V), size=500), rs.randint(len(V), size=500))
    Rm = _rotation()
    net.set_rotation(Rm)
    net.set_noise(7, 0.1, 0.3)
    net.pointset_forward_backward(rotate=True)
    torch.cuda.synchronize()
    Vn = net.noisy_vertices().cpu().numpy()
    assert np.abs(Vn - V).max() > 0.05 * ds.clean_edge_len[0]
    qv, qg = utils.normalizePointSets(Vn, V)
    want = [ops.rotate_rows(torch.as_tensor(q, device=DEV), Rm) for q in (qv, qg)]
    S = net._mesh["verts"]
    assert torch.equal(S["xr"].view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(S["gtr"].view(torch.int32), want[1].view(torch.int32))
    assert torch.equal(net.buffers["x"].view(torch.int32),
                       torch.as_tensor(_host_rows(ds, Vn), device=DEV).view(torch.int32))
    assert np.isfinite(S["loss"].cpu().numpy()).all()


def _state(net):
    torch.cuda.synchronize()
    return (net.noisy_vertices().clone(), net.buffers["x"].clone(), net.buffers["loss"].clone(),
            [g.clone() for g in net.params.grads])


def _same(a, b, what):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), what
    for k, (p, q) in enumerate(zip(a[3], b[3])):
        assert torch.equal(p, q), (what, k)


def test_a_captured_step_replays_with_new_bump_words_and_has_one_launch_more():
    net, ds = _bound_net("ico3", lf_arg=(3.0, 1000))       # (1000 bumps on 642 vertices: the sliced form)
    white, _ = _bound_net("ico3", lf_arg=None)
    n0 = ds.in_list[0].shape[1]
    samp = np.random.RandomState(2).randint(n0, size=4000)
    for n in (net, white):
        n.set_samples(samp)
        n.set_rotation(_rotation())
    net.set_noise(7, 0.1, 0.3)
    net.forward_backward(rotate=True)
    eager7 = _state(net)
    assert np.isfinite(eager7[2][0].item())
    net.forward_backward(rotate=True, capture=True)          # records, then replays
    net.forward_backward(rotate=True, capture=True)
    _same(_state(net), eager7, "captured")
    net.set_noise(8, 0.1, 0.2)
    net.forward_backward(rotate=True, capture=True)
    replay8 = _state(net)
    assert not torch.equal(replay8[0], eager7[0])
    net.forward_backward(rotate=True)
    _same(_state(net), replay8, "eager at counter 8")
    # the same counter with another lf level alone moves the vertices: the graph reads the bump words from device memory
    net.set_noise(8, 0.1, 0.1)
    net.forward_backward(rotate=True, capture=True)
    assert not torch.equal(_state(net)[0], replay8[0])
    net.set_noise(8, 0.1, 0.2)
    net.forward_backward(rotate=True, capture=True)
    _same(_state(net), replay8, "replay, the words of counter 8 again")
    # launches of an eager step: one more than the white synthesis
    counts = []
    for n in (net, white):
        n.set_noise(7, 0.1, *((0.3,) if n is net else ()))
        n.forward_backward(rotate=True)
        torch.cuda.synchronize()
        n.profile_start()
        n.forward_backward(rotate=True)
        torch.cuda.synchronize()
        counts.append(n.profile_stop())
    total = lambda prof: sum(c for c, _ in prof.values())  # noqa: E731
    print("launches of an eager step: %d with bumps, %d white" % (total(counts[0]), total(counts[1])))
    assert total(counts[0]) == total(counts[1]) + 1
    assert sum(c for k, (c, _) in counts[0].items() if "lf_table_kernel" in k or "lf_field_kernel" in k) == 2
    assert not [k for k in counts[0] if "synth_noise_kernel" in k]


def test_bumps_are_smooth_where_white_noise_is_not():
    """What the feature exists for, on torus(60, 50), width 3 edge lengths, K = faces / 6: the field of edge-adjacent
    vertices is as correlated as the float64 oracle's, and bumps of RMS level 0.3 turn the face normals LESS than white
    noise of level 0.3 along the normals does.  Both sides of each comparison are computed here."""
    V, F = _mesh("torus")
    vn, edge = _geom("torus")
    K, width, area = ops.lf_plan(V, F, edge, 3.0, None)
    assert K == 1000
    amp = ops.lf_amplitude(0.3, edge, width, K, area)
    out = _run(V, vn, K, width, amp, 0)
    s = _field_of(V, vn, out)
    centres, amps = lf.bump_table(len(V), K, 0, SEED, 0, amp)
    s64, _ = lf.field(V, centres, amps, width)
    Fi = F.astype(np.int64)
    e = np.concatenate([Fi[:, [0, 1]], Fi[:, [1, 2]], Fi[:, [2, 0]]])
    corr = lambda f: float(np.corrcoef(f[e[:, 0]], f[e[:, 1]])[0, 1])  # noqa: E731
    z = sc.gaussians(len(V), 0, SEED, 0)[:, 3]
    print("correlation of the field across an edge: %.5f on the GPU, %.5f in float64; of the white draw %.5f; RMS of the "
          "field %.3f edge lengths" % (corr(s), corr(s64), corr(z), np.sqrt((s * s).mean()) / edge))
    assert corr(s) > corr(s64) - 1e-3
    assert corr(s) > corr(z) + 0.5
    clean = utils.computeFacesNormals(V, F)
    ang = lambda Vn: float(np.degrees(np.arccos(np.clip((clean * utils.computeFacesNormals(Vn, F)).sum(1), -1, 1))).mean())  # noqa: E731
    white = ops.synth_noise(torch.as_tensor(V, device=DEV), np.float32(0.3 * edge), 0, seed=SEED,
                            normals=torch.as_tensor(vn, device=DEV)).cpu().numpy()
    a_lf, a_white = ang(out), ang(white)
    print("mean angular error of the noisy face normals: %.2f degrees with bumps of RMS level 0.3, %.2f with white noise of "
          "level 0.3 along the normals" % (a_lf, a_white))
    assert 0 < a_lf < a_white


def test_offline_loop_with_bumps_end_to_end(tmp_path, capsys):
    """makeNoisy --lf-levels, preprocess --clean --with-vertices, train --with-vertices --synth-noise 0 --lf-noise 0.3,
    infer --with-vertices, computeMetrics: the files, finite losses, and the validation meshes of the run against the
    makeNoisy files."""
    from facet_graph_convolution_amd import train as T, preprocess, infer, makeNoisy, computeMetrics, bilateral
    from facet_graph_convolution_amd.net import FacetDenoiser
    V, F = icosphere(3)
    clean, noisy, dump, path, res = (tmp_path / k for k in ("clean", "noisy", "dump", "net", "res"))
    clean.mkdir()
    utils.write_mesh(V, F, str(clean / "ball.obj"))
    written = makeNoisy.main([str(clean), str(noisy), "--seed", "3", "--levels", "0,0.1", "--lf-levels", "0.3,0.2"])
    assert sorted(os.listdir(noisy)) == ["ball_n1.obj", "ball_n2.obj"] and len(written) == 2
    files = [utils.load_mesh(str(noisy), "ball_n%d.obj" % k)[0] for k in (1, 2)]
    edge = float(utils.getAverageEdgeLength(V, F)[0])
    assert all(f.shape == V.shape and 0.05 * edge < np.abs(f - V).max() < 3 * edge for f in files)
    preprocess.main([str(clean), str(dump), "--clean", "--with-vertices", "--valid", str(clean)])
    capsys.readouterr()
    assert T.main([str(dump), str(path), "--with-vertices", "--synth-noise", "0", "--lf-noise", "0.3", "--num-iterations", "4",
                   "--net-name", "lf", "--seed", "3"]) == "trainAccuracyNet"
    out = capsys.readouterr().out
    assert "Iteration 0, validation loss" in out and "Iteration 0, training loss" in out
    assert "NAN" not in out and "nan" not in out
    losses = [float(line.rsplit(" ", 1)[1]) for line in out.splitlines() if "loss" in line]
    assert losses and np.isfinite(losses).all()
    assert any(f.startswith("lf-4") for f in os.listdir(path))
    # the validation meshes of such a run are the makeNoisy files (stream 1 + mesh index, step = pair index), to the six
    # decimals an OBJ keeps
    import pickle
    with open(dump / "validSetCleanWithVertices.pkl", "rb") as fp:
        valid = T._clean_vertex_meshes(pickle.load(fp), "validation set")
    net = FacetDenoiser(DEV, multi_scale=True, seed=3)
    levels, lf_arg = (0.0, 0.1), ((0.3, 0.2), (3.0, None))
    T._validation_loss(net, "points", valid, np.eye(3), np.random.RandomState(0), levels, 3, "random", lf_arg)
    torch.cuda.synchronize()
    assert np.abs(net.noisy_vertices().cpu().numpy() - files[1]).max() <= 1e-6        # (the last pair scored)
    net.set_noise(0, 0.0, 0.3)
    net.pointset_loss(rotate=True)
    torch.cuda.synchronize()
    assert np.abs(net.noisy_vertices().cpu().numpy() - files[0]).max() <= 1e-6
    one = tmp_path / "one"
    one.mkdir()
    shutil.copy(str(noisy / "ball_n1.obj"), str(one / "ball_n1.obj"))
    infer.main([str(one), str(res), str(path), "--with-vertices"])
    assert "ball_n1_denoised.obj" in os.listdir(res)
    got = np.loadtxt(str(res / "ball_n1_denoised.obj"), usecols=(1, 2, 3), max_rows=len(V))
    assert got.shape == V.shape and np.isfinite(got).all()
    # Scoring.  computeMetrics cannot score what a network of a few iterations writes, in any units: the loss has not
    # moved (40 - 47 after 4, 30 and 100 iterations alike, measured on an MI355X) and the vertex update on its normals
    # pulls vertices to radius 0.02 ... 0.28 of a 0.289 sphere, where the reference's partition scan finds query cells
    # without candidates and raises - with --with-vertices also because infer writes the vertices divided by the noisy
    # mesh's bounding-box diagonal while CLEAN_DIR holds raw units (README).  The scoring of files with
    # bumps is held where it is defined whatever a network has learnt: the same makeNoisy files through the classical
    # filter (bilateral), scored against the clean folder.
    filt = tmp_path / "filtered"
    bilateral.main([str(noisy), str(filt), "--iterations", "3"])
    computeMetrics.main([str(clean), str(filt)])
    names = ["ball_n1_denoised.obj", "ball_n2_denoised.obj"]
    assert all(n in os.listdir(filt) for n in names + ["results_heat.csv", "ball_n1_heatmap.obj", "ball_n2_heatmap.obj"])
    rows = [ln.split() for ln in open(filt / "results_heat.csv").read().splitlines()]
    assert [r[0] for r in rows] == names
    for r in rows:
        vals = [float(t) for t in r[1:6]]
        print("computeMetrics %s: haus %.7f, mean distance %.7f, mean angle %.3f, std %.3f, faces %d" % ((r[0],) + tuple(vals)))
        assert np.isfinite(vals).all() and vals[4] == len(F) and 0 < vals[2] < 90


def test_refusals():
    from facet_graph_convolution_amd import train as T
    from facet_graph_convolution_amd.net import FacetDenoiser
    V, F = _mesh("ico3")
    vn, edge = _geom("ico3")
    Vd, nd = torch.as_tensor(V, device=DEV), torch.as_tensor(vn, device=DEV)
    ok = dict(sigma=0.0, step=0, amplitude=0.3 * edge, width=3.0 * edge, bumps=17)
    call = lambda **kw: ops.synth_noise_lf(Vd, kw.pop("normals", nd), **{**ok, **kw})  # noqa: E731
    call()
    with pytest.raises(RuntimeError, match="stream_id"):
        call(stream=1 << 31)
    for bumps in (0, ops._lib.SYNTH_LF_MAX_BUMPS + 1):
        with pytest.raises(RuntimeError, match="n_bumps"):
            call(bumps=bumps)
    with pytest.raises(ValueError):
        call(width=0.0)
    with pytest.raises(ValueError):
        call(amplitude=-1.0)
    with pytest.raises(ValueError):
        call(normals=None)
    with pytest.raises(ValueError):
        call(normals=nd[:-1])
    with pytest.raises(RuntimeError, match="scratch too small"):
        call(bumps=1000, scratch=torch.zeros(ops._lib.lib().fgc_synth_lf_scratch_floats(len(V), 1000) - 1, device=DEV))
    with pytest.raises(RuntimeError, match="distinct"):
        call(out=Vd)
    # the network
    ds = _clean_set("ico3")
    args = (ds.in_list[0], ds.adj_list[0], ds.gt_list[0], ds.clean_vertices[0], ds.clean_faces_rows[0], ds.clean_edge_len[0])
    net = FacetDenoiser(DEV, seed=0)
    for bad in ((0.0, None), (-1.0, None), (3.0, 0), (3.0, ops._lib.SYNTH_LF_MAX_BUMPS + 1)):
        with pytest.raises(ValueError):
            net.bind_clean("m", *args, lf=bad)
    with pytest.raises(ValueError):
        net.bind_clean("m", *args, lf=(3.0, None), stream=1 << 31)
    assert "m" not in net._mesh_cache
    net.bind_clean("m", *args, lf=(3.0, None))
    net.bind_clean("m", *args, lf=(3.0, None))               # a cached mesh: a lookup
    for other in (None, (2.0, None), (3.0, 100)):
        with pytest.raises(ValueError, match="another lf setting"):
            net.bind_clean("m", *args, lf=other)
    with pytest.raises(ValueError):
        net.set_noise(0, 0.1, -0.3)
    with pytest.raises(ValueError):
        net.set_noise(0, None, 0.3)
    net.bind_clean("w", *args)
    with pytest.raises(ValueError, match="another lf setting"):
        net.bind_clean("w", *args, lf=(3.0, None))
    with pytest.raises(ValueError, match="lf_level needs a mesh bound with lf"):
        net.set_noise(0, 0.1, 0.3)
    with pytest.raises(ValueError):
        net.train_step(np.arange(4000) % 1000, np.eye(3), noise=(0, 0.1, 0.3))
    # the trainers
    with pytest.raises(ValueError, match="lf_levels"):
        T.trainNet(ds, 1, noise_levels=(0.0, 0.1, 0.2), lf_levels=(0.3, 0.2), log=lambda s: None)
    plain = TrainingSet()
    plain.addMeshWithGT(V, F, V, seed=0)
    with pytest.raises(ValueError, match="lf_levels needs noise_levels"):
        T.trainNet(plain, 1, lf_levels=(0.3,), log=lambda s: None)
