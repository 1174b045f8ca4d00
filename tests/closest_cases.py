"""Scenes, point sets and the oracle of the closest-point query (include/fgc.h: fgc_closest_point_tree).

The oracle runs the definition of include/fgc.h - the region walk of Ericson 5.1.5 on the record (a, e1, e2), the first region
that applies wins, the clamp of the last region - in numpy over ALL pairs: in float64 it is the reference, the same code in
float32 is the "restatement" whose distance to the float64 result says what fp32 costs (numpy has no fma and sums a dot
product in another order than the kernel, so the kernel gets a wider bound: TOL_UNITS).

The unit of every tolerance is 2^-24 x (max|q| + max|V|), per scene and point set."""
import concurrent.futures
import functools

import numpy as np

from facet_graph_convolution_amd import meshgen

SMALL = ("icosphere", "torus", "cube", "torus64")
SCENES = SMALL + ("icosphere5",)          # icosphere5: tree against exhaustive only
RESTATED = ("icosphere", "torus", "cube")          # the three scenes the restatement figure was measured on
_MESH = {"icosphere": lambda: meshgen.icosphere(3),        # 1 280 faces
         "torus": lambda: meshgen.torus(32, 16),            # 1 024
         "cube": lambda: meshgen.cube(5),                   # 300
         "torus64": lambda: meshgen.torus(64, 32),          # 4 096
         "icosphere5": lambda: meshgen.icosphere(5)}        # 20 480: a tree of depth 5, ragged upper levels
TOL_UNITS = 16.0          # the GPU bound
RESTATEMENT_UNITS = 2.0   # what the float32 numpy restatement must stay within (measured: 1.19)
N_BOX = 600
WORKERS = 8             # threads of the oracle over chunks of points


@functools.lru_cache(maxsize=None)
def mesh(name):
    V, F = _MESH[name]()
    V, F = np.ascontiguousarray(V, dtype=np.float32), np.ascontiguousarray(F).astype(np.int32)
    V.setflags(write=False)
    F.setflags(write=False)
    return V, F


def unit(V, P):
    return 2.0 ** -24 * (float(np.abs(np.asarray(P, dtype=np.float64)).max()) + float(np.abs(np.asarray(V, dtype=np.float64)).max()))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _xyz(a):
    """[..., 3] -> three contiguous component arrays (numpy is several times faster on them than on a stride of 3)."""
    return [np.ascontiguousarray(a[..., k]) for k in range(3)]


def pair(q, a, e1, e2):
    """The per-pair function on broadcastable arrays [..., 3] of one dtype: (dist2, u, v, region 0 .. 6).  A record with
    e1 = e2 = 0 takes no part: dist2 = nan."""
    dt = q.dtype
    one, zero = dt.type(1), dt.type(0)
    q, a, e1, e2 = _xyz(q), _xyz(a), _xyz(e1), _xyz(e2)
    with np.errstate(all="ignore"):
        ap = [q[k] - a[k] for k in range(3)]
        d1, d2 = _dot(e1, ap), _dot(e2, ap)
        bp = [ap[k] - e1[k] for k in range(3)]
        d3, d4 = _dot(e1, bp), _dot(e2, bp)
        cp = [ap[k] - e2[k] for k in range(3)]
        d5, d6 = _dot(e1, cp), _dot(e2, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        d43, d56 = d4 - d3, d5 - d6
        w = d43 / (d43 + d56)
        den = one / ((va + vb) + vc)
        ui, vi = vb * den, vc * den
        ui = np.where(ui < 0, zero, ui)
        ui = np.where(ui > 1, one, ui)
        rest = one - ui
        vi = np.where(vi < 0, zero, vi)
        vi = np.where(vi > rest, rest, vi)
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d43 >= 0) & (d56 >= 0)]
        # the first region that applies wins: written from the last to the first, each overriding the later ones
        u, v, region = ui, vi, np.full(d1.shape, 6, dtype=np.int8)
        for k, uk, vk in ((5, one - w, w), (4, zero, d2 / (d2 - d6)), (3, zero, one), (2, d1 / (d1 - d3), zero),
                          (1, one, zero), (0, zero, zero)):
            u, v, region = np.where(conds[k], uk, u), np.where(conds[k], vk, v), np.where(conds[k], np.int8(k), region)
        r = [ap[k] - u * e1[k] - v * e2[k] for k in range(3)]
        dist2 = _dot(r, r)
        dead = ~(e1[0].astype(bool) | e1[1].astype(bool) | e1[2].astype(bool) |
                 e2[0].astype(bool) | e2[1].astype(bool) | e2[2].astype(bool))
        dist2 = np.where(np.broadcast_to(dead, dist2.shape), dt.type(np.nan), dist2)
    return dist2.astype(dt), u.astype(dt), v.astype(dt), region


def records(V, F, dtype):
    """(a, e1, e2) [F,3] as the tree makes them of the fp32 vertices: in float32 the subtraction rounds, in float64 it is
    exact.  A row with an id out of range is a zero record."""
    V = np.asarray(V, dtype=np.float32)
    F = np.asarray(F).astype(np.int64).reshape(-1, 3)
    ok = ((F >= 0) & (F < V.shape[0])).all(1)
    T = V[np.where(ok[:, None], F, 0)].astype(dtype)
    a, e1, e2 = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    a[~ok], e1[~ok], e2[~ok] = 0, 0, 0
    return a, e1, e2


def closest(V, F, P, dtype=np.float64, chunk=256):
    """Over all pairs: dict of dist (= sqrt(dist2)), dist2, face (-1 where no record takes part; ties to the lower index),
    u, v."""
    a, e1, e2 = records(V, F, dtype)
    P = np.asarray(P, dtype=np.float32).reshape(-1, 3).astype(dtype)
    a, e1, e2 = a[None], e1[None], e2[None]

    def one_chunk(s):
        d2, u, v, _ = pair(P[s:s + chunk, None, :], a, e1, e2)
        key = np.where(np.isfinite(d2), d2, np.inf)
        f = key.argmin(1)
        rows = np.arange(f.size)
        none = ~np.isfinite(key[rows, f])
        return (np.where(none, np.inf, d2[rows, f]), np.where(none, -1, f), np.where(none, 0, u[rows, f]),
                np.where(none, 0, v[rows, f]))
    # (numpy releases the interpreter lock inside its loops: the chunks of a large point set run side by side)
    with concurrent.futures.ThreadPoolExecutor(max_workers=WORKERS) as pool:
        parts = list(pool.map(one_chunk, range(0, P.shape[0], chunk)))
    out = {k: [p[j] for p in parts] for j, k in enumerate(("dist2", "face", "u", "v"))}
    res = {k: np.concatenate(x) for k, x in out.items()}
    res["dist"] = np.sqrt(res["dist2"])
    res["face"] = res["face"].astype(np.int32)
    return res


def dist_to_face(V, F, P, face):
    """float64 distance of every point to the triangle face[q] (inf where face[q] < 0)."""
    a, e1, e2 = records(V, F, np.float64)
    f = np.where(face >= 0, face, 0)
    d2 = pair(np.asarray(P, dtype=np.float32).astype(np.float64), a[f], e1[f], e2[f])[0]
    return np.where(face >= 0, np.sqrt(d2), np.inf)


def rebuilt(V, F, face, u, v):
    """The closest point in float64 from (u, v) and the vertices."""
    T = np.asarray(V, dtype=np.float64)[np.asarray(F).astype(np.int64)[face]]
    u, v = np.asarray(u, dtype=np.float64)[:, None], np.asarray(v, dtype=np.float64)[:, None]
    return (1 - u - v) * T[:, 0] + u * T[:, 1] + v * T[:, 2]


def cube_diagonal_points(V, F, height=0.1):
    """One point straight above the middle of every face's longest edge - on the cube the diagonal its quad was split
    along, shared by two faces: a tie."""
    T = np.asarray(V, dtype=np.float64)[np.asarray(F).astype(np.int64)]
    E = np.stack([T[:, 1] - T[:, 0], T[:, 2] - T[:, 1], T[:, 0] - T[:, 2]], 1)
    k = (E * E).sum(2).argmax(1)
    rows = np.arange(T.shape[0])
    mid = 0.5 * (T[rows, k] + T[rows, (k + 1) % 3])
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return (mid + height * n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def point_sets(name):
    """dict: name of the set -> float32 [Q,3] (read-only)."""
    V, F = mesh(name)
    V64, F64 = V.astype(np.float64), F.astype(np.int64)
    sets = {"noisy": meshgen.add_noise(V, F64, 0.2, seed=7), "verts": V.copy(),
            "centroids": V64[F64].mean(1).astype(np.float32)}
    E = np.sort(np.concatenate([F64[:, [0, 1]], F64[:, [1, 2]], F64[:, [2, 0]]]), axis=1)
    E = np.unique(E, axis=0)
    sets["midpoints"] = (0.5 * (V64[E[:, 0]] + V64[E[:, 1]])).astype(np.float32)
    lo, hi = V64.min(0), V64.max(0)
    pad = 0.25 * np.linalg.norm(hi - lo)
    sets["box"] = np.random.RandomState(11).uniform(lo - pad, hi + pad, size=(N_BOX, 3)).astype(np.float32)
    if name.startswith("icosphere"):
        sets["centre"] = np.zeros((1, 3), dtype=np.float32)          # nearly every face ties
    if name.startswith("torus"):
        t = 2 * np.pi * np.arange(16) / 16 + 0.05
        sets["centre"] = np.stack([np.cos(t), np.sin(t), 0 * t], 1).astype(np.float32)          # the middle of the tube
    if name == "cube":
        sets["diagonals"] = cube_diagonal_points(V, F)
    for p in sets.values():
        p.setflags(write=False)
    return sets


@functools.lru_cache(maxsize=None)
def all_points(name):
    """Every point set of a scene in one array, and the slices: (P float32 [Q,3], {set: slice})."""
    sets = point_sets(name)
    where, s = {}, 0
    for k, p in sets.items():
        where[k] = slice(s, s + p.shape[0])
        s += p.shape[0]
    P = np.concatenate(list(sets.values()))
    P.setflags(write=False)
    return P, where


@functools.lru_cache(maxsize=None)
def oracle(name):
    """closest() in float64 on all_points(name): computed once, shared, read-only."""
    V, F = mesh(name)
    res = closest(V, F, all_points(name)[0])
    for x in res.values():
        x.setflags(write=False)
    return res
