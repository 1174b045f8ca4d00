"""Shared by the depth-sensor noise tests: a float64 oracle of the definition in include/fgc.h (fgc_synth_noise_sensor),
written from that text alone, on synth_cases.gaussians for z3; the meshes, camera and cases of the tests."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_cases as sc  # noqa: E402

CAMERA = (2.5, 0.4, 1.2)
SEED = 1234
STEPS = (0, 1, 7)
LEVELS = (0.1, 0.3)
POWERS = (0, 1, 2)
QUANTS = (0.5, 2.0)
K_MAX = 2.0 ** 24


@functools.lru_cache(maxsize=None)
def mesh(tag):
    from facet_graph_convolution_amd.meshgen import icosphere, torus, flip_edges
    if tag == "ico3":
        return icosphere(3)
    V, F = torus(24, 20)
    return V, flip_edges(F, 400, seed=1).astype(np.uint32)


def ranges(V, camera):
    w = np.asarray(V, dtype=np.float64) - np.asarray(camera, dtype=np.float64)
    return np.sqrt((w * w).sum(1))


def oracle(V, rays, camera, sigma, step, seed, stream, power, r_ref, q):
    """The definition in float64.  Returns (v' [V,3], k [V] or None, x [V] = 1 / (rt q) before the rounding or None,
    rt <= 0 flags [V])."""
    V = np.asarray(V, dtype=np.float64)
    d = np.asarray(rays, dtype=np.float64)
    z3 = sc.gaussians(V.shape[0], step, seed, stream)[:, 3]
    r = ranges(V, camera)
    s = float(sigma) * (r / float(r_ref)) ** int(power)
    length = s * z3
    through = np.zeros(V.shape[0], dtype=bool)
    if q == 0:
        return V + d * length[:, None], None, None, through
    rt = r + length
    through = rt <= 0
    rt = np.where(through, r, rt)
    x = 1.0 / (rt * float(q))
    k = np.clip(np.rint(x), 1.0, K_MAX)
    length = 1.0 / (k * float(q)) - r
    return V + d * length[:, None], k, x, through


def position_bound(sigma, power, V, camera, r_ref):
    """1e-5 s_max + 2^-23 max|v|: the bound of test_noise_matches_the_float64_oracle with s_max = sigma max(rho)^power."""
    rho = ranges(V, camera) / float(r_ref)
    return 1e-5 * float(sigma) * rho.max() ** int(power) + 2.0 ** -23 * float(np.abs(V).max())


def disparity_margin(bound, k_max, r_min):
    """m = 4 k_max bound / r_min: the position bound turned into disparity steps, times 4 for the two divisions and r."""
    return 4.0 * k_max * bound / r_min
