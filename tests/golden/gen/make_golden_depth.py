#!/usr/bin/env python3
"""Generate tests/golden/vertex_dir_<tag>*.npz by EXECUTING THE REFERENCE'S update_position_with_depth
(train.py:1561-1665) with getEdgeMap(F, maxEdges=50) (the function hard-codes 50 slots per vertex), imported through
tf_shim as make_golden.py does:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_depth.py
    PYTHONDONTWRITEBYTECODE=1 TF_SHIM_DTYPE=float64 python tests/golden/gen/make_golden_depth.py

The meshes are those of make_golden.py's vertex_case (noisy icosphere(3); the first 450 faces of torus(20,16), an open
mesh with boundary edges), the target normals those of the clean mesh, the directions float32 rows of this package's
utils.view_rays.  The float64 run feeds the same float32 values as float64 arrays.  Every file holds the inputs and
x_1, x_60, dx_1, dx_60 (the function's two return values after 1 and 60 iterations).  Only arrays are written.  Needs the
built library (getEdgeMap's host routine, no GPU).
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
OUT = os.path.abspath(os.path.join(HERE, ".."))
REF = "/root/reference/Code"

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "tf_shim"))
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
if not hasattr(time, "clock"):
    time.clock = time.perf_counter

import warnings  # noqa: E402

warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tensorflow  # noqa: E402,F401  (the shim)
import utils as ref_utils  # noqa: E402
import train as ref_train  # noqa: E402

from facet_graph_convolution_amd import utils as pkg  # noqa: E402
from facet_graph_convolution_amd.meshgen import icosphere, torus, add_noise  # noqa: E402

F64 = os.environ.get("TF_SHIM_DTYPE", "float32") == "float64"
FDT = torch.float64 if F64 else torch.float32
SLOTS = 50     # train.py:1566


def cases():
    V, F = icosphere(3)
    ico = (add_noise(V, F).astype(np.float32), F.astype(np.int32), ref_utils.computeFacesNormals(V, F))
    Vt, Ft = torus(20, 16)
    used, Fo = np.unique(Ft[:450], return_inverse=True)
    Fo = Fo.reshape(-1, 3).astype(np.int32)
    Vo = Vt[used]
    opn = (add_noise(Vo, Fo).astype(np.float32), Fo, ref_utils.computeFacesNormals(Vo, Fo))
    return [("ico3_rays", ico, dict(camera=(0.3, -0.2, 4.0))),
            ("ico3_dir", ico, dict(view_dir=(0.0, 0.6, 0.8))),
            ("torus_open_rays", opn, dict(camera=(0.0, 0.0, 5.0)))]


def main():
    for tag, (Vn, F, normals), view in cases():
        dirs = pkg.view_rays(Vn, **view)
        e_map, v_e_map = ref_utils.getEdgeMap(F, maxEdges=SLOTS)
        x = torch.tensor(Vn, dtype=FDT)[None]
        fn = torch.tensor(normals.astype(np.float32), dtype=FDT)[None]
        d = torch.tensor(dirs, dtype=FDT)
        em = torch.tensor(e_map[None].astype(np.int32))
        vem = torch.tensor(v_e_map[None].astype(np.int32))
        out = {}
        for it in (1, 60):
            xo, dx = ref_train.update_position_with_depth(x, fn, em, vem, d, iter_num=it)
            out["x_%d" % it], out["dx_%d" % it] = xo.detach().numpy()[0], dx.detach().numpy()[0]
            assert out["x_%d" % it].dtype == (np.float64 if F64 else np.float32)
        name = "vertex_dir_%s%s.npz" % (tag, "_f64" if F64 else "")
        path = os.path.join(OUT, name)
        np.savez_compressed(path, verts=Vn, faces=F, normals=normals.astype(np.float32), edge_map=e_map.astype(np.int32),
                            v_e_map=v_e_map.astype(np.int32), dirs=dirs, **out)
        assert os.path.getsize(path) < 1 << 20
        print("wrote %-36s %7.1f KB  max|dx_60| %.3e" % (name, os.path.getsize(path) / 1024.0, np.abs(out["dx_60"]).max()))


if __name__ == "__main__":
    main()
