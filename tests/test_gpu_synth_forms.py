"""The three noise entry points are one per-vertex step: with the extra model off they return the same bytes and leave the
same bounding-box partials, the partials reduce to the exact box of the vertices, and the step is the float64 oracle's."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_cases as sc  # noqa: E402

from facet_graph_convolution_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED, STREAM, STEP, SIGMA = 1234, 2, 7, 0.05
CAMERA = (2.5, 0.4, 1.2)
K = 40      # bumps of the lf call (off): one slice


def _cloud(nv):
    rs = np.random.RandomState(nv % 65521)
    V = rs.uniform(-1, 1, size=(nv, 3)).astype(np.float32)
    d = rs.standard_normal((nv, 3))
    return V, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _blocks(nv):
    return min(-(-nv // 256), 1024)      # (SY_THREADS, SY_MAX_BLOCKS of csrc/fgc_synth.h)


# 1: one workgroup, one lane; 257: two workgroups, the second with one vertex; 262144 + 300: more vertices than the 1024 x 256
# threads of the largest launch - a thread takes two
@pytest.mark.parametrize("nv", [1, 257, 262144 + 300])
def test_the_three_entry_points_are_one_white_step(nv):
    L = _lib.lib()
    V, rows = _cloud(nv)
    Vd, rd = torch.from_numpy(V).to(DEV), torch.from_numpy(rows).to(DEV)
    nb = 6 * _blocks(nv)
    assert L.fgc_synth_scratch_floats(nv) == nb
    got = {}
    sc0 = torch.zeros(nb, dtype=torch.float32, device=DEV)
    got["noise"] = (ops.synth_noise(Vd, SIGMA, STEP, seed=SEED, stream=STREAM, normals=rd, scratch=sc0), sc0)
    sc1 = torch.zeros(nb, dtype=torch.float32, device=DEV)
    got["sensor"] = (ops.synth_noise_sensor(Vd, rd, CAMERA, SIGMA, STEP, None, None, None, seed=SEED, stream=STREAM, scratch=sc1), sc1)
    sc2 = torch.zeros(L.fgc_synth_lf_scratch_floats(nv, K), dtype=torch.float32, device=DEV)
    got["lf"] = (ops.synth_noise_lf(Vd, rd, SIGMA, STEP, None, 0.3, K, seed=SEED, stream=STREAM, white_normals=rd, scratch=sc2), sc2)
    torch.cuda.synchronize()
    out = got["noise"][0].cpu().numpy()
    assert np.isfinite(out).all() and not np.array_equal(out, V)
    for name in ("sensor", "lf"):
        assert np.array_equal(got[name][0].cpu().numpy().view(np.uint32), out.view(np.uint32)), name
        assert np.array_equal(got[name][1][:nb].cpu().numpy().view(np.uint32), sc0.cpu().numpy().view(np.uint32)), name
    # the partials reduce to the box of v_out, exactly (min and max round nothing)
    part = sc0.cpu().numpy().reshape(-1, 6)
    assert np.array_equal(part[:, :3].min(0), out.min(0)) and np.array_equal(part[:, 3:].max(0), out.max(0))
    if nv == 257:
        # the tolerance of test_gpu_synth.py::test_noise_matches_the_float64_oracle, with the rows as the "normals"
        bound = 1e-5 * float(SIGMA) + 2.0 ** -23 * float(np.abs(V).max())
        z = sc.gaussians(nv, STEP, SEED, STREAM)
        want = V.astype(np.float64) + rows.astype(np.float64) * (float(np.float32(SIGMA)) * z[:, 3:4])
        err = np.abs(out.astype(np.float64) - want).max()
        print("nv 257 along rows: max |V' - oracle| = %.3e (bound %.3e)" % (err, bound))
        assert err <= bound
        rnd = ops.synth_noise(Vd, SIGMA, STEP, seed=SEED, stream=STREAM).cpu().numpy().astype(np.float64)
        want = sc.oracle(V, None, np.float32(SIGMA), STEP, SEED, STREAM, "random")
        err = np.abs(rnd - want).max()
        print("nv 257 random: max |V' - oracle| = %.3e (bound %.3e)" % (err, bound))
        assert err <= bound
