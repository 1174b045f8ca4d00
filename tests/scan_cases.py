"""Float64 oracle and scenes of the virtual depth scans (numpy only, no GPU): Moeller-Trumbore over all pairs of rays and
triangles, the three views (perspective rays to the vertices, orthographic rays to the vertices, pixel rays of a pinhole),
the visible cut and the range mesh, written from the definitions in include/fgc.h and the docstrings of utils.py, not from
their code.  fp32 Moeller-Trumbore is not watertight, so the GPU tests compare ROBUST cases only; which those are is decided
here, in float64, and every test asserts that at most 2 % of a scene's cases were skipped (CAP)."""
import functools

import numpy as np

from facet_graph_convolution_amd.meshgen import cube, icosphere, torus

IMAGE = (50, 37)          # W, H: 1 850 rays, not a multiple of 64
FOV = 40.0
CAP = 0.02                # share of a scene's cases a test may skip
EDGE = 1e-4               # a barycentric closer to 0 than this: the hit may flip in fp32
GRAZE = 1e-4              # |n . d| below this: the triangle is seen edge-on

SCENES = {
    "icosphere": (lambda: icosphere(3), (0.3, -0.2, 3.0)),       # 642 vertices, 1 280 faces
    "torus": (lambda: torus(32, 16), (2.5, 0.4, 1.2)),           # 512 vertices, 1 024 faces; occludes itself through the hole
    "cube": (lambda: cube(5), (1.7, 1.1, 2.3)),                  # 300 faces, not a multiple of 8; an image scene only
}
VISIBILITY_SCENES = ("icosphere", "torus")
# (straight down, (0, 0, -1), is no test view: both meshes are mirror symmetric in z, so the ray of every lower vertex runs
#  through its mirror vertex - 305 of the icosphere's 642 vertices and 224 of the torus' 512 are ambiguous, far over the cap)
VIEW_DIR = (0.2, -0.3, -1.0)


@functools.lru_cache(maxsize=None)
def scene(name):
    make, camera = SCENES[name]
    V, F = make()
    V = np.ascontiguousarray(V, dtype=np.float32)
    F = np.ascontiguousarray(np.asarray(F).astype(np.int32))
    V.setflags(write=False)
    F.setflags(write=False)
    return V, F, camera


def _dot(a, b):
    return (a * b).sum(-1)


def moller_trumbore(V, F, origins, dirs):
    """All pairs in float64: dict of [Q, F] arrays t, u, v, w = 1 - u - v and nd = n . d / |d| (n the unit face normal; 0
    for a face without area).  A pair with det == 0 has non-finite entries."""
    V = np.asarray(V, dtype=np.float64)
    F = np.asarray(F).astype(np.int64)
    o = np.broadcast_to(np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(dirs).reshape(-1, 3).shape)[:, None]
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)[:, None]
    a, b, c = V[F[:, 0]][None], V[F[:, 1]][None], V[F[:, 2]][None]
    e1, e2 = b - a, c - a
    p = np.cross(d, e2)
    det = _dot(e1, p)
    s = o - a
    qv = np.cross(s, e1)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = _dot(s, p) / det
        v = _dot(d, qv) / det
        t = _dot(e2, qv) / det
        w = 1.0 - u - v
    n = np.cross(e1, e2)
    nn = np.sqrt(_dot(n, n))
    n = n / np.where(nn > 0, nn, 1.0)[..., None]
    nd = _dot(n, d / np.sqrt(_dot(d, d))[..., None])
    return {"t": t, "u": u, "v": v, "w": w, "nd": nd}


def first_hit(V, F, origins, dirs, t_min=0.0, mt=None):
    """(t [Q], face [Q], u [Q], v [Q]): the smallest t > t_min over the hits, the smallest face among equal t; a miss is
    (inf, -1, 0, 0)."""
    mt = moller_trumbore(V, F, origins, dirs) if mt is None else mt
    with np.errstate(invalid="ignore"):
        hit = (mt["u"] >= 0) & (mt["v"] >= 0) & (mt["u"] + mt["v"] <= 1) & (mt["t"] > t_min) & np.isfinite(mt["t"])
    t = np.where(hit, mt["t"], np.inf)
    face = np.argmin(t, axis=1)                  # (the first of equal minima: the smallest face index)
    rows = np.arange(t.shape[0])
    miss = ~hit[rows, face]
    tt = t[rows, face]
    return (tt, np.where(miss, -1, face).astype(np.int32), np.where(miss, 0.0, mt["u"][rows, face]),
            np.where(miss, 0.0, mt["v"][rows, face]))


def robust_rays(mt):
    """bool [Q]: no triangle in front of the ray is met within EDGE of its border, none is grazed."""
    with np.errstate(invalid="ignore"):
        m = np.minimum(np.minimum(mt["u"], mt["v"]), mt["w"])
        edge = (mt["t"] > 0) & (np.abs(m) < EDGE)
        graze = (np.abs(mt["nd"]) < GRAZE) & (m > -0.1)
    return ~(edge | graze).any(1)


# ---- the three views ------------------------------------------------------------------------------------------------
def perspective_rays(V, camera):
    """origin [1,3], dirs [V,3]: the vertex sits at t = 1."""
    c = np.asarray(camera, dtype=np.float64).reshape(1, 3)
    return c, np.asarray(V, dtype=np.float64) - c


def orthographic_rays(V, view_dir):
    V = np.asarray(V, dtype=np.float64)
    d = np.asarray(view_dir, dtype=np.float64)
    step = d / np.linalg.norm(d) * 2.0 * np.linalg.norm(V.max(0) - V.min(0))
    return V - step[None], np.broadcast_to(step[None], V.shape)


def pixel_rays(camera, look_at, size=IMAGE, fov=FOV, up=(0.0, 0.0, 1.0)):
    """float32 [H,W,3]: row 0 on top, column 0 on the left, fov horizontal, square pixels."""
    W, H = size
    c = np.asarray(camera, dtype=np.float64)
    f = np.asarray(look_at, dtype=np.float64) - c
    f /= np.linalg.norm(f)
    up = np.asarray(up, dtype=np.float64) / np.linalg.norm(up)
    if abs(f @ up) > 0.99:
        up = np.array([0.0, 1.0, 0.0])
    right = np.cross(f, up)
    right /= np.linalg.norm(right)
    top = np.cross(right, f)
    half = np.tan(np.radians(fov) / 2)
    out = np.empty((H, W, 3))
    for j in range(H):
        for i in range(W):
            x = (2 * (i + 0.5) / W - 1) * half
            y = (1 - 2 * (j + 0.5) / H) * half * H / W
            r = f + x * right + y * top
            out[j, i] = r / np.linalg.norm(r)
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def image_case(name):
    """The image of a scene in float64: dict with rays float32 [Q,3], t, face, u, v of the first hit, robust [Q] and
    bound_scale [Q] = t / |n . d| of the hit face (0 for a miss)."""
    V, F, camera = scene(name)
    V64 = V.astype(np.float64)
    rays = pixel_rays(camera, 0.5 * (V64.min(0) + V64.max(0))).reshape(-1, 3)
    mt = moller_trumbore(V, F, np.asarray(camera).reshape(1, 3), rays)
    t, face, u, v = first_hit(V, F, None, None, mt=mt)
    rows = np.arange(rays.shape[0])
    nd = np.abs(mt["nd"][rows, np.maximum(face, 0)])
    scale = np.where(face >= 0, t / np.where(nd > 0, nd, 1.0), 0.0)
    return {"rays": rays, "t": t, "face": face, "u": u, "v": v, "robust": robust_rays(mt), "scale": scale}


def classify_vertices(V, F, origins, dirs, eps=1e-3):
    """int8 [V]: 1 strictly visible, 0 strictly hidden, -1 ambiguous, for rays on which vertex i sits at t = 1.  Only
    triangles that do not hold the vertex count."""
    mt = moller_trumbore(V, F, origins, dirs)
    F = np.asarray(F).astype(np.int64)
    other = (F[None, :, :] != np.arange(mt["t"].shape[0])[:, None, None]).all(-1)
    with np.errstate(invalid="ignore"):
        m = np.minimum(np.minimum(mt["u"], mt["v"]), mt["w"])
        hidden = (other & (m >= EDGE) & (mt["t"] > 0) & (mt["t"] <= 1 - 2 * eps)).any(1)
        maybe = (other & (m >= -EDGE) & (mt["t"] > 0) & (mt["t"] <= 1 - eps / 2)).any(1)
    return np.where(hidden, 0, np.where(~maybe, 1, -1)).astype(np.int8)


@functools.lru_cache(maxsize=None)
def visibility_case(name, view):
    """view: "camera" (the scene's) or "dir" (VIEW_DIR).  The classification of every vertex."""
    V, F, camera = scene(name)
    o, d = perspective_rays(V, camera) if view == "camera" else orthographic_rays(V, VIEW_DIR)
    return classify_vertices(V, F, o, d)


def view_kwargs(name, view):
    return {"camera": scene(name)[2]} if view == "camera" else {"view_dir": VIEW_DIR}


def cut(V, F, visible, camera=None, view_dir=None, max_angle=80.0):
    """(V_cut, faces_cut, vertex_ids, kept faces bool [F]) for a given visibility mask."""
    V64 = np.asarray(V, dtype=np.float64)
    F = np.asarray(F).astype(np.int64)
    keep = np.zeros(F.shape[0], dtype=bool)
    for k, (a, b, c) in enumerate(F):
        n = np.cross(V64[b] - V64[a], V64[c] - V64[a])
        if not visible[[a, b, c]].all() or not np.linalg.norm(n) > 0:
            continue
        n = n / np.linalg.norm(n)
        r = (V64[a] + V64[b] + V64[c]) / 3 - np.asarray(camera, dtype=np.float64) if camera is not None \
            else np.asarray(view_dir, dtype=np.float64)
        keep[k] = -(n @ (r / np.linalg.norm(r))) >= np.cos(np.radians(max_angle))
    ids = np.array(sorted(set(F[keep].ravel().tolist())), dtype=np.int64)
    new = {int(o): k for k, o in enumerate(ids)}
    faces = np.array([[new[int(i)] for i in row] for row in F[keep]], dtype=np.int32).reshape(-1, 3)
    return np.asarray(V)[ids], faces, ids, keep


def range_mesh(depth, rays, camera, jump=0.05):
    """(V float64 [v,3], faces as PIXEL triples [f,3], pixel index of every vertex [v], block of every face [f,2]) of a
    depth image: p00 = (r, c), p10 = (r + 1, c), p01 = (r, c + 1), p11 = (r + 1, c + 1); triangles (p00, p10, p01) and
    (p10, p11, p01)."""
    H, W = depth.shape
    faces, blocks = [], []
    for r in range(H - 1):
        for c in range(W - 1):
            d = np.array([depth[r, c], depth[r + 1, c], depth[r, c + 1], depth[r + 1, c + 1]])
            if not np.isfinite(d).all() or d.max() - d.min() > jump * d.min():
                continue
            p00, p10, p01, p11 = r * W + c, (r + 1) * W + c, r * W + c + 1, (r + 1) * W + c + 1
            faces += [(p00, p10, p01), (p10, p11, p01)]
            blocks += [(r, c), (r, c)]
    faces = np.array(faces, dtype=np.int64).reshape(-1, 3)
    ids = np.unique(faces)
    P = np.asarray(camera, dtype=np.float64)[None] + depth.reshape(-1)[ids, None] * rays.reshape(-1, 3)[ids].astype(np.float64)
    return P, faces, ids, np.array(blocks, dtype=np.int64).reshape(-1, 2)


def jump_margin(depth, jump=0.05):
    """[H-1, W-1]: |(max - min) / min - jump| of every block (inf where a depth is not finite)."""
    d = np.stack([depth[:-1, :-1], depth[1:, :-1], depth[:-1, 1:], depth[1:, 1:]])
    with np.errstate(invalid="ignore"):
        m = np.abs((d.max(0) - d.min(0)) / d.min(0) - jump)
    return np.where(np.isfinite(d).all(0), m, np.inf)
