"""Developer tool: the SIGNATURE of one training step per configuration, on the golden fixtures (ico3, torus640 with
their net_*.npz samples and rotation) - to hold a refactor of the step schedule against its parent commit.

Per configuration and mesh, as JSON: the profile table {tag/kernel: launches} of one eager step; for the facet-sharded
configurations (2 simulated shards) the request trace of both schedules of shard 0 as [kind, key or None, item kinds]
and the segment_nodes of a segment capture; SHA-256 digests of params.grad, the loss tensor and nconv after the step.
points_rays / double_rays: the points / double step bound with viewing rays (depth_dir), once with a per-vertex table and
once with one [1,3] row, with the digest of the vertex trajectory.  points_surface: the points step bound with the mesh's own
faces as ground-truth faces (gt_faces: the surface loss in the place of fullLoss).  vertex_ops: no step - the digests of every output of the
eight vertex-update ops (free and along rays, [V,3] and [1,3] rays) on the ico3 fixtures and the ragged tori of the tests,
and their launch table - to hold a refactor of csrc/fgc_vertex.hip and its callers against its parent.
The backward pass has a fixed order and no float atomics: two commits with the same library build must print the same
bytes.

  python tools/step_signature.py            every configuration, each in a fresh process -> one JSON document
  python tools/step_signature.py NAME       one configuration (the child of the above)
"""
import hashlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))      # (the cases the vertex-update tests share)
GOLDEN = os.path.join(REPO, "tests", "golden")

# name: (form, dtype, multi_scale, shards, FGC_SPLIT_MIN_TILES or None, meshes)
BOTH = ("ico3", "torus640")
CONFIGS = {
    "angular_f32": ("angular", "f32", False, 0, None, BOTH),
    "angular_bf16": ("angular", "bf16", False, 0, None, BOTH),
    "angular_ms_f32": ("angular", "f32", True, 0, None, BOTH),
    "points": ("points", "f32", True, 0, None, ("ico3",)),
    "double": ("double", "f32", True, 0, None, ("ico3",)),
    "points_rays": ("points", "f32", True, 0, None, ("ico3_table", "ico3_row")),
    "double_rays": ("double", "f32", True, 0, None, ("ico3_table", "ico3_row")),
    "points_surface": ("points", "f32", True, 0, None, ("ico3_surface",)),
    "vertex_ops": None,
    "shard2_f32": ("angular", "f32", False, 2, None, BOTH),
    "shard2_bf16": ("angular", "bf16", False, 2, None, BOTH),
    "shard2_f32_split0": ("angular", "f32", False, 2, "0", BOTH),
    "shard2_bf16_split0": ("angular", "bf16", False, 2, "0", BOTH),
}


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _digests(net, loss):
    return {"grad": _sha(net.params.grad), "loss": _sha(loss), "nconv": _sha(net.buffers["nconv"])}


def _launches(prof):
    return {k: v[0] for k, v in sorted(prof.items())}


def _unsharded(form, dtype, multi_scale, tag):
    import numpy as np
    from facet_graph_convolution_amd.net import FacetDenoiser
    net = FacetDenoiser("cuda:0", seed=0, dtype=dtype, multi_scale=multi_scale)
    if form == "angular":
        p, z = np.load(os.path.join(GOLDEN, "prep_%s.npz" % tag)), np.load(os.path.join(GOLDEN, "net_%s.npz" % tag))
        net.bind_mesh(p["x"], [p["adj0"], p["adj1"], p["adj2"]], gt=p["gt"])
        net.set_samples(z["sample_ind"])
        step = net.forward_backward
    else:
        p, z = np.load(os.path.join(GOLDEN, "points_ico3.npz")), np.load(os.path.join(GOLDEN, "double_ico3.npz"))
        rays = {}
        if tag == "ico3_surface":
            rays = {"gt_faces": p["faces"].astype(np.int32)}
        elif tag != "ico3":      # ico3_table: the camera's rays, one per vertex; ico3_row: one view direction
            import depth_ms_cases as mc
            from facet_graph_convolution_amd import utils
            view = {"camera": mc.CAMERA} if tag == "ico3_table" else {"view_dir": mc.VIEW_DIR}
            rays = {"depth_dir": utils.view_rays(p["verts"], **view)}
        net.bind_vertices(0, p["x"], [p["adj%d" % k].astype(np.int32) for k in range(3)], p["verts"], p["faces"],
                          p["v_faces"].astype(np.int32), p["gt_verts"], gt_normals=z["gt_normals"], **rays)
        net.set_point_samples(z["sample_ind0"], z["sample_ind1"])
        step = net.pointset_forward_backward if form == "points" else net.double_loss_forward_backward
    net.set_rotation(z["R"])
    net.profile_start()
    loss = step(rotate=True)
    out = dict(launches=_launches(net.profile_stop()), **_digests(net, loss))
    if tag not in BOTH:
        out["traj"] = _sha(net._mesh["verts"]["traj"])
    return out


def _vertex_ops():
    import ctypes
    import numpy as np
    import torch
    import depth_cases as dc
    import depth_ms_cases as mc
    from facet_graph_convolution_amd import _lib, ops, utils
    from test_gpu_depth_ms import _ragged_mesh
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")  # noqa: E731
    L = _lib.lib()
    L.fgc_profile_enable(1)
    out = {}
    # the single-scale pair on the fixtures of tests/depth_cases.py ([V,3] rays, one [1,3] row)
    for tag in ("ico3_rays", "ico3_dir"):
        z = dc.load(GOLDEN, tag)[0]
        a = (dev(z["verts"]), dev(z["normals"]), dev(z["edge_map"]), dev(z["v_e_map"]))
        for it in (0, 1, 60):
            x, t = ops.vertex_update_dir(*a, dev(z["dirs"]), it, return_t=True)
            out["%s/%d" % (tag, it)] = {"vertex_update": _sha(ops.vertex_update(*a, it)), "vertex_update_dir": _sha(x),
                                        "vertex_update_dir_t": _sha(t)}

    def ms(x, normals, faces, vf, rays, g_out, its):
        a = (dev(x), [dev(n) for n in normals], dev(faces), dev(vf))
        g = dev(g_out)
        o, dx = ops.vertex_update_ms(*a, its)
        traj = ops.vertex_update_ms_traj(*a, its)
        g_x, g_n = ops.vertex_update_ms_bwd(traj, *a[1:], g, its)
        r = {"out": _sha(o), "dx": _sha(dx), "traj": _sha(traj), "g_x": _sha(g_x), "g_n": [_sha(t) for t in g_n]}
        for name, d in rays.items():
            d = dev(d)
            o, dx, t = ops.vertex_update_ms_dir(*a, d, its, return_t=True)
            traj, tt = ops.vertex_update_ms_dir_traj(*a, d, its, return_t=True)
            g_x, g_n = ops.vertex_update_ms_dir_bwd(traj, *a[1:], d, g, its)
            r[name] = {"out": _sha(o), "dx": _sha(dx), "t": _sha(t), "traj": _sha(traj), "traj_t": _sha(tt), "g_x": _sha(g_x),
                       "g_n": [_sha(t) for t in g_n]}
        return r
    for truncate in (False, True):
        x, normals, faces, vf = mc.load(GOLDEN, truncate)
        rays = {kind: mc.directions(x, kind) for kind in mc.DIR_SETS}      # (view_dir: the [1,3] row)
        g_out = np.random.RandomState(7).standard_normal(x.shape).astype(np.float32)
        for its in ((80, 20, 20),) + tuple(i for i in mc.ITERS if i != (80, 20, 20)):
            out["ms_ico3%s/%d_%d_%d" % (("_4slots" if truncate else "",) + its)] = ms(x, normals, faces, vf, rays, g_out, its)
    for name in ("t255", "t256", "t257"):
        V, normals, faces, vf = _ragged_mesh(name)
        rays = {"camera": utils.view_rays(V, camera=mc.CAMERA), "view_dir": utils.view_rays(V, view_dir=(0, 0.6, 0.8))}
        g_out = np.random.RandomState(8).standard_normal(V.shape).astype(np.float32)
        out["ms_%s/2_1_2" % name] = ms(V, normals, faces, vf, rays, g_out, (2, 1, 2))
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    L.fgc_profile_collect(buf, len(buf))
    L.fgc_profile_enable(0)
    out["launches"] = {k: int(c) for k, c, _ in sorted(l.rsplit(" ", 2) for l in buf.value.decode().splitlines())}
    return out


def _sharded(dtype, tag):
    import numpy as np
    import torch
    from facet_graph_convolution_amd.shard import make_sim_shards, sim_run
    p, z = np.load(os.path.join(GOLDEN, "prep_%s.npz" % tag)), np.load(os.path.join(GOLDEN, "net_%s.npz" % tag))
    nets = make_sim_shards(p["x"], [p["adj0"], p["adj1"], p["adj2"]], p["gt"], 2, "cuda:0", 0, dtype=dtype)
    for n in nets:
        n.set_rotation(z["R"])
        n.set_samples(z["sample_ind"])
        n.profile = True
    trace = {"forward": [], "backward": []}

    def traced(n, gen, out):
        for r in gen:
            if n is nets[0]:
                # (a request keeps its kind in field 0; an exchange is (kind, items, key), a wait (kind, key))
                key = r[2] if r[0] == "xchg" else r[1] if r[0] == "wait" else None
                out.append([r[0], key, [it[0] for it in r[1]] if r[0] == "xchg" else []])
            yield r
    nets[0].L.fgc_profile_enable(1)
    sim_run(nets, lambda n: traced(n, n._forward_gen(True, n.fused_loss), trace["forward"]))
    sim_run(nets, lambda n: traced(n, n._loss_backward_gen(True), trace["backward"]))
    prof = nets[0].profile_stop()
    for n in nets:
        n.profile = False
    torch.cuda.synchronize()
    out = dict(launches=_launches(prof), requests=trace, **_digests(nets[0], nets[0].buffers["loss"]))
    n = nets[0]
    n._own_step_inputs()
    n.segment_nodes = []
    n._capture_segments(lambda: n._forward_gen(True, n.fused_loss))
    n._capture_segments(lambda: n._loss_backward_gen(True))
    out["segment_nodes"] = list(n.segment_nodes)
    return out


def run_config(name):
    if name == "vertex_ops":
        return _vertex_ops()
    form, dtype, multi_scale, shards, _, meshes = CONFIGS[name]
    return {tag: _sharded(dtype, tag) if shards else _unsharded(form, dtype, multi_scale, tag) for tag in meshes}


def main(argv):
    if argv:
        print("SIGNATURE " + json.dumps(run_config(argv[0]), sort_keys=True))
        return 0
    doc = {}
    for name, cfg in CONFIGS.items():
        env = {k: v for k, v in os.environ.items() if k != "FGC_SPLIT_MIN_TILES"}
        if cfg is not None and cfg[4] is not None:
            env["FGC_SPLIT_MIN_TILES"] = cfg[4]
        out = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=env, capture_output=True, text=True,
                             timeout=300)
        lines = [l for l in out.stdout.splitlines() if l.startswith("SIGNATURE ")]
        if out.returncode != 0 or len(lines) != 1:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
            return out.returncode or 1        # (nothing more is started on the device behind a failed configuration)
        doc[name] = json.loads(lines[0][len("SIGNATURE "):])
        sys.stderr.write("%s: done\n" % name)
    print(json.dumps(doc, indent=1, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
