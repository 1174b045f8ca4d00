"""Developer tool: the SIGNATURE of the noise synthesis - to hold a refactor of csrc/fgc_synth*.hip,
ops.synth_noise*, synth.py and their callers against its parent commit (tools/tree_signature.py does the same for the tree
walks, tools/step_signature.py for a plain training step).  It uses only what the public surface has had since the
depth-sensor model: ops.synth_noise / _lf / _sensor, ops.face_features_rows, ops.point_sets_prepare, makeNoisy.make_noisy
and FacetDenoiser's bind_clean / bind_clean_vertices / set_noise / noisy_vertices.

As JSON, SHA-256 over raw bytes:
  entry/<nv>/...      the three entry points on point clouds of nv = 1, 255, 256, 257 and 262144 + 300 vertices (the last: more
                      than SY_MAX_BLOCKS workgroups' worth, a thread takes two vertices): v_out and the first 6 x blocks floats
                      of the scratch - direction absent and a table of unit rows, sigma 0 and > 0; the sensor model off, with
                      words out of range, and on with power 0, 1, 2 and q = 0 and > 0; the bumps off and on with K = 40 (one
                      slice, a tail shorter than a chunk)
  entry/lf1000_K600   nv = 1000, K = 600: two slices and the last-arriver sum
  rows/<nv>/...       ops.face_features_rows and ops.point_sets_prepare on the boxes a noise call left (have_bbox) and without
  net/<setting>       a small mesh bound five ways with bind_clean (random, normal, a ray table, lf=, sensor=) and with
                      bind_clean_vertices(ray_update=True): after set_noise one step eager and one captured - noisy_vertices(),
                      the input rows, the loss and the flat gradient
  make_noisy/<setting>   makeNoisy.make_noisy for the same five settings
Nothing here is atomic on floats or depends on a launch order: two commits that compute the same print the same bytes.

  python tools/synth_signature.py [OUT.json]          (kept as profiles/synth_signature_parent.json and ..._after.json)
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))      # (the mesh and camera the sensor tests share)

import sensor_noise_cases as sn  # noqa: E402
from facet_graph_convolution_amd import _lib, ops, utils  # noqa: E402
from facet_graph_convolution_amd.dataClasses import TrainingSet  # noqa: E402
from facet_graph_convolution_amd.makeNoisy import make_noisy  # noqa: E402
from facet_graph_convolution_amd.net import FacetDenoiser  # noqa: E402

DEV = "cuda:0"
SEED, STREAM, STEP = 1234, 2, 3
SIZES = (1, 255, 256, 257, 262144 + 300)
SIGMAS = (0.0, 0.05)


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
        h.update(a.tobytes())
    return h.hexdigest()


def _blocks(nv):
    return min(-(-nv // 256), 1024)


def _i32(words):
    return torch.from_numpy(np.asarray(words, dtype=np.uint32).view(np.int32)).to(DEV)


def cloud(nv):
    """nv points of [-1, 1]^3 (the first x coordinate -0.0) and nv unit rows, float32 on the device."""
    rs = np.random.RandomState(nv % 65521)
    V = rs.uniform(-1, 1, size=(nv, 3)).astype(np.float32)
    V[0, 0] = -0.0
    d = rs.standard_normal((nv, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return torch.from_numpy(V).to(DEV), torch.from_numpy(d).to(DEV)


def sensor_settings():
    """{name: the four sensor words}: off, out of range (each falls back to plain ray noise), power x q."""
    f = lambda x: int(np.array([x], dtype=np.float32).view(np.uint32)[0])  # noqa: E731
    on = 0x80000000
    out = {"off": [0, 0, 0, 0], "bad_power": [on | 3, f(2.0), f(0.0), 0], "bad_ref": [on | 2, f(0.0), f(0.0), 0],
           "bad_q": [on | 1, f(2.0), f(float("nan")), 0]}
    for power in (0, 1, 2):
        for q in (0.0, 0.01):
            out["p%d_q%g" % (power, q)] = [int(w) for w in ops.sensor_words(power, 2.5, q)]
    return out


def entries(doc):
    L = _lib.lib()
    for nv in SIZES:
        V, rows = cloud(nv)
        nb = 6 * _blocks(nv)
        for sigma in SIGMAS:
            for dname, d in (("random", None), ("rows", rows)):
                tag = "entry/%d/sigma%g/%s" % (nv, sigma, dname)
                sc = torch.zeros(max(L.fgc_synth_scratch_floats(nv), 1), dtype=torch.float32, device=DEV)
                out = ops.synth_noise(V, sigma, STEP, seed=SEED, stream=STREAM, normals=d, scratch=sc)
                doc[tag + "/noise"] = _sha(out, sc[:nb])
                K = 40
                for lname, amp in (("off", None), ("on", 0.1)):
                    sc = torch.zeros(L.fgc_synth_lf_scratch_floats(nv, K), dtype=torch.float32, device=DEV)
                    out = ops.synth_noise_lf(V, rows, sigma, STEP, amp, 0.3, K, seed=SEED, stream=STREAM, white_normals=d,
                                             scratch=sc)
                    doc[tag + "/lf_" + lname] = _sha(out, sc[:nb])
            for sname, words in sensor_settings().items():
                sc = torch.zeros(max(L.fgc_synth_scratch_floats(nv), 1), dtype=torch.float32, device=DEV)
                out = ops.synth_noise_sensor(V, rows, sn.CAMERA, sigma, STEP, None, None, None, seed=SEED, stream=STREAM,
                                             scratch=sc, sensor_ctl=_i32(words))
                doc["entry/%d/sigma%g/sensor_%s" % (nv, sigma, sname)] = _sha(out, sc[:nb])
    nv, K = 1000, 600
    V, rows = cloud(nv)
    for sigma in SIGMAS:
        for dname, d in (("random", None), ("rows", rows)):
            for lname, amp in (("off", None), ("on", 0.1)):
                sc = torch.zeros(L.fgc_synth_lf_scratch_floats(nv, K), dtype=torch.float32, device=DEV)
                out = ops.synth_noise_lf(V, rows, sigma, STEP, amp, 0.3, K, seed=SEED, stream=STREAM, white_normals=d, scratch=sc)
                doc["entry/lf1000_K600/sigma%g/%s/lf_%s" % (sigma, dname, lname)] = _sha(out, sc[:6 * _blocks(nv)])


def rows_and_points(doc):
    L = _lib.lib()
    R = utils.rand_rotation_matrix(randnums=np.random.RandomState(3).uniform(size=3)).astype(np.float32)
    for nv in SIZES:
        V, rows = cloud(nv)
        rs = np.random.RandomState(7)
        nf = min(2 * nv + 3, 4099)
        faces = rs.randint(nv, size=(nf, 3)).astype(np.int32)
        faces[::17] = -1      # fake nodes
        faces = torch.from_numpy(faces).to(DEV)
        sc = torch.zeros(max(L.fgc_synth_scratch_floats(nv), 1), dtype=torch.float32, device=DEV)
        out = ops.synth_noise(V, 0.05, STEP, seed=SEED, stream=STREAM, normals=rows, scratch=sc)
        for have in (True, False):
            tag = "rows/%d/have_bbox%d" % (nv, have)
            doc[tag + "/face_features_rows"] = _sha(ops.face_features_rows(out, faces, scratch=sc if have else None,
                                                                           have_bbox=have))
            for rname, rot in (("R", R), ("noR", None)):
                doc[tag + "/point_sets_prepare_" + rname] = _sha(*ops.point_sets_prepare(out, V, R=rot, scratch=sc if have else None,
                                                                                         have_bbox=have))


def settings(V, edge_len):
    """{name: (bind keywords, set_noise's levels, make_noisy's keywords)} of the five settings."""
    rays = utils.view_rays(V, camera=sn.CAMERA)
    rays = np.ascontiguousarray(np.broadcast_to(rays, V.shape)).astype(np.float32)
    model = utils.sensor_model(V, sn.CAMERA, edge_len, 2, 0.5)
    return {"random": (dict(direction="random"), (0.2,), dict(direction="random")),
            "normal": (dict(direction="normal"), (0.2,), dict(direction="normal")),
            "rays": (dict(direction=rays), (0.2,), dict(direction=rays)),
            "lf": (dict(direction="random", lf=(3.0, None)), (0.2, 0.3), dict(direction="random", lf_level=0.3, lf_width=3.0)),
            "sensor": (dict(direction=rays, sensor=model), (0.2,), dict(direction=rays, sensor=(2, 0.5), camera=sn.CAMERA))}


def _steps(doc, tag, net, step):
    for mode, kw in (("eager", {}), ("captured", dict(capture=True)), ("replayed", dict(capture=True))):
        loss = step(rotate=True, **kw)
        torch.cuda.synchronize()
        doc["%s/%s" % (tag, mode)] = {"noisy_vertices": _sha(net.noisy_vertices()), "rows": _sha(net.buffers["x"]),
                                      "loss": _sha(loss), "grad": _sha(net.params.grad)}


def networks(doc):
    V, F = sn.mesh("ico3")
    V = np.asarray(V, dtype=np.float32)
    rs = np.random.RandomState(2)
    R = utils.rand_rotation_matrix(randnums=np.random.RandomState(3).uniform(size=3))
    ds = TrainingSet()
    ds.addCleanMesh(V, F, seed=0)
    edge_len = ds.clean_edge_len[0]
    samp = rs.randint(ds.in_list[0].shape[1], size=4000)
    for name, (bind_kw, levels, noisy_kw) in settings(V, edge_len).items():
        net = FacetDenoiser(DEV, seed=0)
        net.bind_clean(0, ds.in_list[0], ds.adj_list[0], ds.gt_list[0], ds.clean_vertices[0], ds.clean_faces_rows[0], edge_len,
                       seed=SEED, stream=1, **bind_kw)
        net.set_samples(samp)
        net.set_rotation(R)
        net.set_noise(5, *levels)
        _steps(doc, "net/" + name, net, net.forward_backward)
        doc["make_noisy/" + name] = _sha(make_noisy(V, F, levels[0], seed=SEED, stream=1, step=5, **noisy_kw))
        del net
    dv = TrainingSet()
    dv.addCleanMeshWithVertices(V, F, seed=0)
    nv = V.shape[0]
    rays = settings(V, edge_len)["rays"][0]["direction"]
    net = FacetDenoiser(DEV, multi_scale=True, seed=0)
    net.bind_clean_vertices(0, dv.in_list[0], dv.adj_list[0], dv.clean_vertices[0], dv.clean_faces_rows[0], dv.v_faces_list[0],
                            dv.clean_edge_len[0], seed=SEED, stream=1, direction=rays, ray_update=True)
    net.set_point_samples(rs.randint(nv, size=500), rs.randint(nv, size=500))
    net.set_rotation(R)
    net.set_noise(5, 0.2)
    _steps(doc, "net/vertices_ray_update", net, net.pointset_forward_backward)


def main(argv):
    doc = {}
    entries(doc)
    rows_and_points(doc)
    networks(doc)
    s = json.dumps(doc, indent=1, sort_keys=True)
    print(s)
    if argv:
        with open(argv[0], "w") as fh:
            fh.write(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
