"""Shared by the guided-filter tests: the case meshes and a numpy oracle written from the definition in include/fgc.h
(fgc_guided_normals, fgc_bilateral_filter_guided) alone.  Every oracle function takes a dtype: the float64 run is the
yardstick, the float32 run of the SAME code defines dev32 per case and quantity - the largest float32-against-float64
difference of the oracle itself, the convention of tests/test_gpu_bilateral.py."""
import functools

import numpy as np

from facet_graph_convolution_amd import bilateral, utils
from facet_graph_convolution_amd.meshgen import add_noise, cube, icosphere, torus

MARGIN = 8.0
CASES = ("cube4", "ico2", "open", "fan18", "fans36", "one", "torus65", "torus257", "zeros", "cube12")
LEVEL, SEED = 0.3, 1          # cube12: the quality conditions' noise (meshgen.add_noise)


def submesh(V, F, nfaces):
    """The first faces of a mesh, vertices re-indexed."""
    used, Fo = np.unique(np.asarray(F)[:nfaces], return_inverse=True)
    return np.asarray(V)[used].astype(np.float32), Fo.reshape(-1, 3).astype(np.int32)


def fan(k, seed=0):
    """k faces around one vertex (a closed fan, a low cone with a little noise): every ring is the whole mesh."""
    rs = np.random.RandomState(seed)
    t = 2 * np.pi * np.arange(k) / k
    V = np.concatenate([[[0, 0, 0.3]], np.stack([np.cos(t), np.sin(t), np.zeros(k)], -1)])
    V = V + rs.normal(scale=0.03, size=V.shape)
    F = np.stack([np.zeros(k, dtype=np.int64), 1 + np.arange(k), 1 + (np.arange(k) + 1) % k], -1)
    return V.astype(np.float32), F.astype(np.int32)


def two_fans(seed=0):
    """Two fan vertices A and B of valence 19 that share the edge AB: 19 + 19 - 2 = 36 faces, the two faces on AB lie in
    both fans and have rings of 36."""
    rs = np.random.RandomState(seed)
    ang = np.deg2rad(np.linspace(100, 260, 16))
    A, B, T, U = (-0.5, 0, 0), (0.5, 0, 0), (0, 0.6, 0), (0, -0.6, 0)
    a = np.stack([-0.5 + np.cos(ang), np.sin(ang), 0 * ang], -1)          # round A from above T to below U
    b = np.stack([0.5 - np.cos(ang), -np.sin(ang), 0 * ang], -1)          # round B from below U to above T
    V = np.concatenate([[A, B, T, U], a, b]) + rs.normal(scale=0.03, size=(36, 3))
    ia, ib = 4 + np.arange(16), 20 + np.arange(16)
    rim_a = [1, 2] + list(ia) + [3]                                       # B, T, a.., U  (counter-clockwise round A)
    rim_b = [0, 3] + list(ib) + [2]                                       # A, U, b.., T  (counter-clockwise round B)
    F = [(0, rim_a[i], rim_a[(i + 1) % 19]) for i in range(19)]
    F += [(1, rim_b[i], rim_b[(i + 1) % 19]) for i in range(1, 18)]       # (B, A, U) and (B, T, A) are already there
    return V.astype(np.float32), np.asarray(F, dtype=np.int32)


def _mesh(name):
    if name == "cube4":
        V, F = cube(4)
        return add_noise(V, F, sigma_rel=0.3, seed=2), F
    if name == "cube12":
        V, F = cube(12)
        return add_noise(V, F, sigma_rel=LEVEL, seed=SEED), F
    if name in ("ico2", "zeros"):
        V, F = icosphere(2)
        return add_noise(V, F, sigma_rel=0.2, seed=3), F
    if name == "open":
        V, F = submesh(*torus(20, 16), 450)
        return add_noise(V, F, sigma_rel=0.2, seed=3), F
    if name in ("torus65", "torus257"):
        V, F = submesh(*torus(20, 16), int(name[5:]))
        return add_noise(V, F, sigma_rel=0.2, seed=4), F
    if name == "fan18":
        return fan(18)
    if name == "fans36":
        return two_fans()
    if name == "one":
        return np.array([[0, 0, 0], [1, 0, 0], [0.2, 0.9, 0.3]], np.float32), np.array([[0, 1, 2]], np.int32)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: V, F, Fc (device centres), Fn, Fa float32, ring, ld, fe, el (mean edge length), grid and cell (the partition
    bilateral.denoise_mesh takes for sigma_s = 1 edge length)."""
    V, F = _mesh(name)
    V, F = np.asarray(V, dtype=np.float32), np.asarray(F).astype(np.int32)
    Fc = utils.getTrianglesBarycenter(V, F, normalize=False)
    Fn = utils.computeFacesNormals(V, F).astype(np.float32)
    Fa = utils.getTrianglesArea(V, F).astype(np.float32)
    if name == "zeros":                               # faces of zero area and rows with a zero normal
        Fa, Fn = Fa.copy(), Fn.copy()
        Fa[::3] = 0
        Fn[::5] = 0
    ring, ld = utils.face_rings(F)
    el = float(utils.getAverageEdgeLength(V, F)[0])
    grid = bilateral.auto_slices(Fc, el)
    return dict(name=name, V=V, F=F, Fc=utils.bilateral_device_centres(Fc), Fn=Fn, Fa=Fa, ring=ring, ld=ld,
                fe=utils.face_edge_neighbours(F), el=el, grid=grid,
                cell=utils.bilateral_cells(Fc, grid, flat_axis_one_cell=True))


# ---------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------
def patches(N, A, ring, fe, dtype=np.float64):
    """(H [n], M [n,3]) of every face's patch, vectorised over the padded rings."""
    N, A = np.asarray(N, dtype=dtype), np.asarray(A, dtype=dtype)
    n = N.shape[0]
    valid = (ring >= 0) & (ring < n)
    idx = np.where(valid, ring, 0)
    Np = N[idx]                                                            # [n, ld, 3]
    d = Np[:, :, None, :] - Np[:, None, :, :]
    dist = np.sqrt((d * d).sum(-1))
    Phi = np.where(valid[:, :, None] & valid[:, None, :], dist, 0).max((1, 2))
    b = fe[idx]                                                            # [n, ld, 3]: across each edge of each member
    inside = ((b[:, :, :, None] == ring[:, None, None, :]) & valid[:, None, None, :]).any(-1)
    edge = inside & valid[:, :, None] & (b > idx[:, :, None])              # every edge once: from its lower face
    e = Np[:, :, None, :] - N[np.clip(b, 0, n - 1)]
    phi = np.where(edge, np.sqrt((e * e).sum(-1)), 0).astype(dtype)
    R = phi.max((1, 2)) / (dtype(1e-9) + phi.sum((1, 2)))
    M = np.zeros((n, 3), dtype=dtype)
    for s in range(ring.shape[1]):                                         # slot order
        M = M + np.where(valid[:, s, None], A[idx[:, s], None] * Np[:, s], 0).astype(dtype)
    return (Phi * R).astype(dtype), M


def pick_of(H, ring):
    """The face of ring[i] with the smallest H, the first such slot on a tie (-1 for a row without a valid slot)."""
    valid = (ring >= 0) & (ring < H.shape[0])
    Hr = np.where(valid, H[np.where(valid, ring, 0)], np.inf)
    slot = np.argmin(Hr, axis=1)
    return np.where(valid.any(1), ring[np.arange(ring.shape[0]), slot], -1)


def guidance(N, A, ring, fe, dtype=np.float64, pick=None):
    """(G, pick, H, M) in `dtype`; a given pick replaces the oracle's own."""
    H, M = patches(N, A, ring, fe, dtype)
    if pick is None:
        pick = pick_of(H, ring)
    pick = np.asarray(pick)
    G = utils.normalize(np.where(pick[:, None] >= 0, M[np.clip(pick, 0, None)], 0).astype(dtype))
    return G.astype(dtype), pick, H, M


def guided_pass(Fc, Fn, Fa, G, sigma_s, sigma_r, cell, dtype=np.float64):
    """Rows of fgc_bilateral_filter_guided for one (sigma_s, sigma_r): the range term on the guide G."""
    Fc, Fn, Fa, G = (np.asarray(a, dtype=dtype) for a in (Fc, Fn, Fa, G))
    n = Fc.shape[0]
    out = np.zeros((n, 3), dtype=dtype)
    ok = (cell >= 0).all(1)
    dense = bool(ok.all() and ((cell.max(0) - cell.min(0)) <= 1).all())      # every face in every window

    def dist2(X, r):
        return sum((X[r, k][:, None] - X[None, :, k]) ** 2 for k in range(3))
    step = max(8, min(256, 3000000 // n))
    for s in range(0, n, step):
        r = slice(s, s + step)
        w = np.exp(-dist2(Fc, r) / dtype(2 * sigma_s ** 2)) * Fa[None, :]
        if sigma_r != -1:
            w = w * np.exp(-dist2(G, r) / dtype(2 * sigma_r ** 2))
        if not dense:
            near = (np.abs(cell[r][:, None, :] - cell[None, :, :]) <= 1).all(-1) & ok[None, :] & ok[r][:, None]
            w = np.where(near, w, 0).astype(dtype)
        out[r] = w @ Fn
    return utils.normalize(out).astype(dtype)


def full_pass(c, N, sigma_s, sigma_r, dtype=np.float64, pick=None):
    """One pass of denoise_mesh(guided=True) on the normals N of case c: (normals out, pick, H)."""
    G, pick, H, _ = guidance(N, c["Fa"], c["ring"], c["fe"], dtype, pick)
    return guided_pass(c["Fc"], N, c["Fa"], G, sigma_s * c["el"], sigma_r, c["cell"], dtype), pick, H


def dev(a32, a64):
    return float(np.abs(np.asarray(a32, dtype=np.float64) - np.asarray(a64, dtype=np.float64)).max())


@functools.lru_cache(maxsize=None)
def reference(name):
    """The two oracle runs of a case's guidance and what they lose against each other: dict with H, M, G, pick (float64),
    G32 (the float32 run's guide, with the float64 pick) and dev32 of H, M and G."""
    c = case(name)
    G, pick, H, M = guidance(c["Fn"], c["Fa"], c["ring"], c["fe"], np.float64)
    G32, _, H32, M32 = guidance(c["Fn"], c["Fa"], c["ring"], c["fe"], np.float32, pick)
    return dict(H=H, M=M, G=G, pick=pick, G32=G32.astype(np.float32), dev_H=dev(H32, H), dev_M=dev(M32, M),
                dev_G=dev(G32, G))


def angular_error(N, clean):
    """Mean angle in degrees between rows of N and the clean unit normals."""
    N, clean = np.asarray(N, dtype=np.float64), np.asarray(clean, dtype=np.float64)
    cos = (N * clean).sum(1) / np.maximum(np.linalg.norm(N, axis=1) * np.linalg.norm(clean, axis=1), 1e-30)
    return float(np.degrees(np.arccos(np.clip(cos, -1, 1))).mean())


def clean_cube12_normals():
    V, F = cube(12)
    return utils.computeFacesNormals(V, F)
