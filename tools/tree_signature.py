"""Developer tool: the SIGNATURE of the ray casts and the closest-point query on the scenes of the tests - to hold a refactor of
csrc/fgc_raycast.hip, fgc_raytree.hip, fgc_closest.hip and their callers against its parent commit (tools/step_signature.py
does the same for a training step).

As JSON, SHA-256 over the raw bytes of the three outputs of one call:
  rays/<scene>/<view>      every scene of tests/scan_cases.py - the pixel rays of its image and, for the visibility scenes, the
                           rays to its vertices from the camera and along VIEW_DIR: (t, face, bary) of ops.ray_cast and of
                           ops.ray_cast_tree with sort_rays on and off
  points/<scene>           every scene of tests/closest_cases.py on all its point sets: (dist, face, bary) of
                           ops.closest_point_tree with sort_points on and off and with exhaustive=True
Nothing here is atomic on floats or depends on a launch order: two commits that compute the same print the same bytes.

  python tools/tree_signature.py [OUT.json]          (kept as profiles/tree_signature_parent.json and ..._after.json)
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))      # (the scenes the tests share)

import closest_cases as cc  # noqa: E402
import scan_cases as sc  # noqa: E402
from facet_graph_convolution_amd import ops  # noqa: E402


def _sha(outputs):
    h = hashlib.sha256()
    for t in outputs:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _dev(a, dt):
    return torch.from_numpy(np.array(a, dtype=dt)).cuda()          # (a copy: the scenes are read-only)


def ray_sets(name):
    """{view: (origins, dirs)} of a scene, float32 on the host."""
    V, F, camera = sc.scene(name)
    V64 = V.astype(np.float64)
    sets = {"image": (np.asarray(camera).reshape(1, 3), sc.pixel_rays(camera, 0.5 * (V64.min(0) + V64.max(0))).reshape(-1, 3))}
    if name in sc.VISIBILITY_SCENES:
        sets["camera"] = sc.perspective_rays(V, camera)
        sets["dir"] = sc.orthographic_rays(V, sc.VIEW_DIR)
    return sets


def main(argv):
    doc = {}
    for name in sc.SCENES:
        V, F, _ = sc.scene(name)
        Vd, Fd = _dev(V, np.float32), _dev(F, np.int32)
        tree = ops.ray_tree(Vd, Fd)
        for view, (o, d) in ray_sets(name).items():
            o, d = _dev(o, np.float32), _dev(d, np.float32)
            doc["rays/%s/%s" % (name, view)] = {
                "rays": int(d.shape[0]),
                "ray_cast": _sha(ops.ray_cast(Vd, Fd, o, d, want_bary=True)),
                "ray_cast_tree_sort_on": _sha(ops.ray_cast_tree(tree, o, d, want_bary=True, sort_rays=True)),
                "ray_cast_tree_sort_off": _sha(ops.ray_cast_tree(tree, o, d, want_bary=True, sort_rays=False))}
    for name in cc.SCENES:
        V, F = cc.mesh(name)
        tree = ops.ray_tree(_dev(V, np.float32), _dev(F, np.int32))
        P = _dev(cc.all_points(name)[0], np.float32)
        doc["points/%s" % name] = {
            "points": int(P.shape[0]),
            "closest_point_tree_sort_on": _sha(ops.closest_point_tree(tree, P, want_bary=True, sort_points=True)),
            "closest_point_tree_sort_off": _sha(ops.closest_point_tree(tree, P, want_bary=True, sort_points=False)),
            "closest_point_tree_exhaustive": _sha(ops.closest_point_tree(tree, P, want_bary=True, exhaustive=True))}
    s = json.dumps(doc, indent=1, sort_keys=True)
    print(s)
    if argv:
        with open(argv[0], "w") as fh:
            fh.write(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
