"""Developer tool: the SIGNATURE of one training step per configuration, on the golden fixtures (ico3, torus640 with
their net_*.npz samples and rotation) - to hold a refactor of the step schedule against its parent commit.

Per configuration and mesh, as JSON: the profile table {tag/kernel: launches} of one eager step; for the facet-sharded
configurations (2 simulated shards) the request trace of both schedules of shard 0 as [kind, key or None, item kinds]
and the segment_nodes of a segment capture; SHA-256 digests of params.grad, the loss tensor and nconv after the step.
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
GOLDEN = os.path.join(REPO, "tests", "golden")

# name: (form, dtype, multi_scale, shards, FGC_SPLIT_MIN_TILES or None, meshes)
BOTH = ("ico3", "torus640")
CONFIGS = {
    "angular_f32": ("angular", "f32", False, 0, None, BOTH),
    "angular_bf16": ("angular", "bf16", False, 0, None, BOTH),
    "angular_ms_f32": ("angular", "f32", True, 0, None, BOTH),
    "points": ("points", "f32", True, 0, None, ("ico3",)),
    "double": ("double", "f32", True, 0, None, ("ico3",)),
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
        net.bind_vertices(0, p["x"], [p["adj%d" % k].astype(np.int32) for k in range(3)], p["verts"], p["faces"],
                          p["v_faces"].astype(np.int32), p["gt_verts"], gt_normals=z["gt_normals"])
        net.set_point_samples(z["sample_ind0"], z["sample_ind1"])
        step = net.pointset_forward_backward if form == "points" else net.double_loss_forward_backward
    net.set_rotation(z["R"])
    net.profile_start()
    loss = step(rotate=True)
    return dict(launches=_launches(net.profile_stop()), **_digests(net, loss))


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
    form, dtype, multi_scale, shards, _, meshes = CONFIGS[name]
    return {tag: _sharded(dtype, tag) if shards else _unsharded(form, dtype, multi_scale, tag) for tag in meshes}


def main(argv):
    if argv:
        print("SIGNATURE " + json.dumps(run_config(argv[0]), sort_keys=True))
        return 0
    doc = {}
    for name, cfg in CONFIGS.items():
        env = {k: v for k, v in os.environ.items() if k != "FGC_SPLIT_MIN_TILES"}
        if cfg[4] is not None:
            env["FGC_SPLIT_MIN_TILES"] = cfg[4]
        out = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=env, capture_output=True, text=True,
                             timeout=300)
        lines = [l for l in out.stdout.splitlines() if l.startswith("SIGNATURE ")]
        if out.returncode != 0 or len(lines) != 1:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
            return out.returncode or 1        # (nothing more is started on the device behind a failed configuration)
        doc[name] = json.loads(lines[0][len("SIGNATURE "):])
    print(json.dumps(doc, indent=1, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
