"""Host-side helpers that keep the names of the reference's ``utils.py`` where a counterpart exists."""
import collections
import math

import numpy as np


def rand_rotation_matrix(deflection=1.0, randnums=None):
    """Uniform random rotation (Arvo's method), same parametrisation as the reference
    (utils.py:2034-2074): theta/phi/z from three uniforms, M = (V V^T - I) Rz(theta)."""
    if randnums is None:
        randnums = np.random.uniform(size=(3,))
    t, p, z = randnums
    t = t * 2.0 * deflection * np.pi
    p = p * 2.0 * np.pi
    z = z * 2.0 * deflection
    r = np.sqrt(z)
    V = np.array([np.sin(p) * r, np.cos(p) * r, np.sqrt(2.0 - z)])
    st, ct = np.sin(t), np.cos(t)
    Rz = np.array(((ct, st, 0.0), (-st, ct, 0.0), (0.0, 0.0, 1.0)))
    return (np.outer(V, V) - np.eye(3)).dot(Rz)


def normalizeOnce(a):
    """utils.py:26-31: row-wise a / (|a| + 1e-8)."""
    a = np.asarray(a)
    flat = a.reshape(-1, a.shape[-1])
    norms = np.sqrt((flat * flat).sum(1))[:, None] + 0.00000001
    return (flat * (1 / norms)).reshape(a.shape)


def normalize(a):
    """utils.py:33-35 (applied twice, as the reference does)."""
    return normalizeOnce(normalizeOnce(a))


def inv_perm(perm):
    """utils.py:1830-1835."""
    perm = np.asarray(perm)
    inv = np.zeros(max(len(perm), int(perm.max()) + 1), dtype=np.int64)
    inv[perm] = np.arange(len(perm))
    return inv


# ------------------------------------------------------------------------------------------------
# native preprocessing (libfgc host routines), same names / argument meaning as the reference utils.py
# ------------------------------------------------------------------------------------------------
def _faces_u32(faces):
    f = np.ascontiguousarray(np.asarray(faces).astype(np.uint32))
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("faces must be [F,3] (triangular faces only)")
    return f


def face_features(verts, faces):
    """(normals float32 [F,3], barycentres/bbox-diagonal float64 [F,3]) in one native pass."""
    from . import _lib
    V = np.ascontiguousarray(np.asarray(verts, dtype=np.float32))
    F = _faces_u32(faces)
    normals = np.empty((F.shape[0], 3), dtype=np.float32)
    centres = np.empty((F.shape[0], 3), dtype=np.float64)
    _lib.check(_lib.lib().fgc_face_features(V.ctypes.data, V.shape[0], F.ctypes.data, F.shape[0],
                                            normals.ctypes.data, centres.ctypes.data), "fgc_face_features")
    return normals, centres


def computeFacesNormals(verts, faces):
    """utils.py:63-68."""
    return face_features(verts, faces)[0]


def getTrianglesBarycenter(vl, fl, normalize=True):
    """utils.py:1264-1294.  normalize=True: positions divided by the bbox diagonal, not centred (natively);
    normalize=False: the plain barycentres (v0 + v1 + v2) / 3 in the vertices' dtype, returned as float64 like the
    reference's array (what the bilateral filter works on)."""
    if not normalize:
        vl, fl = np.asarray(vl), np.asarray(fl).astype(np.int64)
        return ((vl[fl[:, 0]] + vl[fl[:, 1]] + vl[fl[:, 2]]) / 3).astype(np.float64)
    return face_features(vl, fl)[1]


def getFacesLargeAdj(faces, K):
    """utils.py:243-295: vertex-sharing facet adjacency as a K-list (one-indexed, slot 0 = self), bit-exact."""
    from . import _lib
    import ctypes as C
    F = _faces_u32(faces)
    nv = int(F.max()) + 1
    adj = np.empty((F.shape[0], K), dtype=np.int32)
    unreg = C.c_int64(0)
    _lib.check(_lib.lib().fgc_faces_large_adj(F.ctypes.data, F.shape[0], nv, K, adj.ctypes.data, C.byref(unreg)),
               "fgc_faces_large_adj")
    if unreg.value > 0:
        print("unregistered connections (faces): " + str(unreg.value / 2))
    return adj


def getVerticesFaces(faces, k_v, vnum=0):
    """utils.py:370-395: faces incident to every vertex (row indices of `faces`, -1 padded to k_v; rows starting with
    -1 are fake faces and skipped), natively and bit-exact."""
    from . import _lib
    F = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3), dtype=np.int32)
    if vnum == 0:
        vnum = int(F.max()) + 1
    out = np.empty((int(vnum), int(k_v)), dtype=np.int32)
    _lib.check(_lib.lib().fgc_vertices_faces(F.ctypes.data, F.shape[0], int(vnum), int(k_v), out.ctypes.data),
               "fgc_vertices_faces")
    return out


def normalizePointSets(vl1, vl2):
    """utils.py:2077-2104: both point sets divided by the bounding-box diagonal of their union (not centred)."""
    vl1, vl2 = np.asarray(vl1), np.asarray(vl2)
    lo = np.minimum(vl1.min(0), vl2.min(0))
    hi = np.maximum(vl1.max(0), vl2.max(0))
    diag = float(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))
    return vl1 / diag, vl2 / diag


def getEdgeMap(faces, maxEdges=50):
    """utils.py:91-183: (e_map [E,4] = [v1, v2, f1, f2 or -1], v_e_map [V, maxEdges] edge ids per vertex, -1 padded),
    bit-exact (same visiting order), natively."""
    from . import _lib
    import ctypes as C
    F = _faces_u32(faces)
    nv = int(F.max()) + 1
    e_map = np.empty((F.shape[0] * 3, 4), dtype=np.int32)
    v_e_map = np.empty((nv, maxEdges), dtype=np.int32)
    ne = C.c_int32(0)
    _lib.check(_lib.lib().fgc_edge_map(F.ctypes.data, F.shape[0], nv, int(maxEdges), e_map.ctypes.data, C.byref(ne),
                                       v_e_map.ctypes.data), "fgc_edge_map")
    return e_map[:ne.value].copy(), v_e_map


def getGraphPatch_wMask(fAdjIn, nodesNum, seed, mask, minPatchSize):
    """utils.py:1508-1696: (patch K-list one-indexed [n, K], old index of every patch node [n], nextSeed), natively and
    bit-exact (same breadth-first queue discipline)."""
    from . import _lib
    import ctypes as C
    adj = np.ascontiguousarray(np.asarray(fAdjIn), dtype=np.int32)
    n, K = adj.shape
    m = np.ascontiguousarray(np.asarray(mask) == 1, dtype=np.int8)
    out = np.empty((int(nodesNum) + K, K), dtype=np.int32)
    old = np.empty(int(nodesNum) + K, dtype=np.int32)
    cnt, nxt = C.c_int32(0), C.c_int32(-1)
    _lib.check(_lib.lib().fgc_graph_patch(adj.ctypes.data, n, K, int(nodesNum), int(seed), m.ctypes.data,
                                          int(minPatchSize), out.ctypes.data, old.ctypes.data, C.byref(cnt),
                                          C.byref(nxt)), "fgc_graph_patch")
    return out[:cnt.value].copy(), old[:cnt.value].copy(), int(nxt.value)


def getMeshPatch(vIn, fIn, fAdjIn, faceNum, seed):
    """utils.py:1298-1410: (vOut [nv',3] float32, fOut [nf',3] in patch vertex ids, fAdjOut [nf',K] one-indexed, vOldInd,
    fOldInd), natively and bit-exact (same breadth-first queue discipline; the reference's vertex buffer of
    int(0.6 * faceNum) + K rows is kept, overflowing it raises like the reference's IndexError)."""
    from . import _lib
    import ctypes as C
    V = np.ascontiguousarray(np.asarray(vIn), dtype=np.float32)
    F = np.ascontiguousarray(np.asarray(fIn), dtype=np.int32)
    adj = np.ascontiguousarray(np.asarray(fAdjIn), dtype=np.int32)
    K = adj.shape[1]
    faceNum = int(faceNum)
    v_cap = int(faceNum * 0.6) + K
    v_out = np.empty((v_cap, 3), dtype=np.float32)
    f_out = np.empty((faceNum + K, 3), dtype=np.int32)
    adj_out = np.empty((faceNum + K, K), dtype=np.int32)
    v_old = np.empty(v_cap, dtype=np.int32)
    f_old = np.empty(faceNum + K, dtype=np.int32)
    n_v, n_f = C.c_int32(0), C.c_int32(0)
    rc = _lib.lib().fgc_mesh_patch(V.ctypes.data, V.shape[0], F.ctypes.data, F.shape[0], adj.ctypes.data, K, faceNum,
                                   int(seed), v_out.ctypes.data, v_cap, f_out.ctypes.data, adj_out.ctypes.data,
                                   v_old.ctypes.data, f_old.ctypes.data, C.byref(n_v), C.byref(n_f))
    if rc:
        raise IndexError(_lib.lib().fgc_last_error().decode())
    nv, nf = n_v.value, n_f.value
    return (v_out[:nv].copy(), f_out[:nf].astype(np.int64), adj_out[:nf].astype(np.int64), v_old[:nv].astype(np.int64),
            f_old[:nf].astype(np.int64))


def getBoundingBox(points):
    """utils.py:2130-2137: [[xmin, xmax], [ymin, ymax], [zmin, zmax]]."""
    points = np.asarray(points)
    return np.stack([points.min(axis=0), points.max(axis=0)], axis=1)


def takePointSetSlice(points, boundBox):
    """utils.py:2109-2125: the points inside the (closed) box."""
    points = np.asarray(points)
    boundBox = np.asarray(boundBox)
    return points[np.all((points >= boundBox[:, 0]) & (points <= boundBox[:, 1]), axis=1)]


def coarsen_klists(adj, pos, normals, levels=4, K=23, seed=0, parents=None, keep=(0, 2, 4)):
    """listToSparseWNormals + coarsen + sparseToList (utils.py:1753-1827, lib/coarsening.py:5-31).

    Returns (klists for the graph levels in `keep`, newToOld, parents, has_saturated).  With `parents`
    (recorded cluster assignments of a reference run) the result replays that run bit-exactly."""
    from . import _lib
    import ctypes as C
    L = _lib.lib()
    adj = np.ascontiguousarray(np.asarray(adj, dtype=np.int32))
    pos = np.ascontiguousarray(np.asarray(pos, dtype=np.float64))
    nrm = np.ascontiguousarray(np.asarray(normals, dtype=np.float32))
    n, Kin = adj.shape
    h = C.c_void_p(0)
    if parents is not None:
        arrs = [np.ascontiguousarray(np.asarray(p, dtype=np.int32)) for p in parents]
        if len(arrs) != levels:
            raise ValueError("need %d recorded parent arrays" % levels)
        ptrs = (C.c_void_p * levels)(*[a.ctypes.data for a in arrs])
        lens = np.asarray([len(a) for a in arrs], dtype=np.int32)
        pp, pl = C.cast(ptrs, C.c_void_p), lens.ctypes.data
    else:
        pp, pl = None, None
    _lib.check(L.fgc_hierarchy_build(adj.ctypes.data, n, Kin, pos.ctypes.data, nrm.ctypes.data, levels,
                                     C.c_uint64(seed), pp, pl, C.byref(h)), "fgc_hierarchy_build")
    try:
        klists, sat_any = [], False
        for lvl in keep:
            m = L.fgc_hierarchy_size(h, lvl)
            out = np.empty((m, K), dtype=np.int32)
            sat = C.c_int32(0)
            _lib.check(L.fgc_hierarchy_klist(h, lvl, K, out.ctypes.data, C.byref(sat)), "fgc_hierarchy_klist")
            sat_any = sat_any or bool(sat.value)
            klists.append(out)
        n0 = L.fgc_hierarchy_size(h, 0)
        new_to_old = np.empty(n0, dtype=np.int32)
        _lib.check(L.fgc_hierarchy_new_to_old(h, 0, new_to_old.ctypes.data), "fgc_hierarchy_new_to_old")
        par = []
        for lvl in range(levels):
            p = np.empty(L.fgc_hierarchy_real_size(h, lvl), dtype=np.int32)
            _lib.check(L.fgc_hierarchy_parents(h, lvl, p.ctypes.data), "fgc_hierarchy_parents")
            par.append(p)
    finally:
        L.fgc_hierarchy_free(h)
    return klists, new_to_old, par, sat_any


def metis_one_level(rr, cc, vv, rid, weights):
    """lib/coarsening.py:135-192 (native, bit-exact given its arguments). Returns (cluster_id, totalAssoc)."""
    from . import _lib
    import ctypes as C
    rr = np.ascontiguousarray(rr, dtype=np.int32)
    cc = np.ascontiguousarray(cc, dtype=np.int32)
    vv = np.ascontiguousarray(vv, dtype=np.float32)
    rid = np.ascontiguousarray(rid, dtype=np.int64)
    weights = np.ascontiguousarray(weights, dtype=np.float32)
    N = int(rr[-1]) + 1
    cid = np.empty(N, dtype=np.int32)
    assoc = C.c_double(0)
    _lib.check(_lib.lib().fgc_metis_one_level(rr.ctypes.data, cc.ctypes.data, vv.ctypes.data, len(rr),
                                              rid.ctypes.data, weights.ctypes.data, N, cid.ctypes.data,
                                              C.byref(assoc)), "fgc_metis_one_level")
    return cid, assoc.value


# ---------------------------------------------------------------------------------------------------
# OBJ input / output (utils.py:476-640, 659-697): what infer.py reads and writes
# ---------------------------------------------------------------------------------------------------
def load_mesh(path, filename, K=0, bGetAdj=False):
    """utils.py:476-640 for bGetAdj=False (the only mode the denoising path uses, dataClasses.py:513): reads 'v' and
    'f' records of a Wavefront OBJ (vertex/texture/normal triplets accepted, polygons fan-triangulated around their
    first vertex, everything else ignored).  Returns (vertices float32 [V,3], adj, free_ind, faces [F,3] zero-indexed
    uint16 when V < 65536 else uint32, per-vertex normals) with adj / free_ind empty as in the reference."""
    import os
    if bGetAdj:
        raise NotImplementedError("vertex adjacency (bGetAdj=True) is not on the facet denoising path")
    verts, faces = [], []
    with open(os.path.join(path, filename), "r") as fh:
        for line in fh:
            if line.startswith("#"):
                continue
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
            elif tok[0] == "f":
                idx = [int(t.split("/")[0]) - 1 for t in tok[1:]]
                for k in range(1, len(idx) - 1):
                    faces.append((idx[0], idx[k], idx[k + 1]))
    V = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    F = np.asarray(faces, dtype=np.int64).reshape(-1, 3).astype(np.uint16 if V.shape[0] < 65536 else np.uint32)
    return V, [], [], F, computeNormals(V, F)


def computeNormals(verts, faces):
    """utils.py:44-60: per-vertex normals from the unit face normals.  `normals[faces[:, i]] += Nn` is a buffered
    fancy-index add: for each corner i a vertex keeps the contribution of the LAST face listing it there, not the sum
    over faces.  Kept as the reference has it (the denoising path never reads this output, dataClasses.py:513)."""
    verts = np.asarray(verts, dtype=np.float32)
    F = np.asarray(faces).astype(np.int64)
    T = verts[F]
    Nn = normalize(np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]))
    out = np.zeros(verts.shape, dtype=np.float32)
    for k in range(3):
        out[F[:, k]] += Nn
    return normalize(out)


def areaWeightedVertexNormals(verts, faces):
    """Unit vertex normals as the area-weighted SUM of the incident faces' normals (the cross products (v1 - v0) x
    (v2 - v0), whose length is twice the area, added over all faces around a vertex), float64 [V,3]; a vertex without a
    face gets a zero row.  Build extension for the noise synthesis along the normal (ops.synth_noise); not
    computeNormals, which keeps the reference's last-face-wins quirk."""
    V = np.asarray(verts, dtype=np.float64)
    F = np.asarray(faces).astype(np.int64)
    T = V[F]
    cp = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    out = np.zeros(V.shape, dtype=np.float64)
    for k in range(3):
        np.add.at(out, F[:, k], cp)
    nrm = np.sqrt((out * out).sum(1, keepdims=True))
    return np.where(nrm > 0, out / np.where(nrm > 0, nrm, 1.0), 0.0)


def view_rays(V, camera=None, view_dir=None):
    """Viewing rays of a depth scan (build extension), float32 unit rows.  camera: a point in the mesh's raw units, the
    rows are normalize(V - camera), [V,3]; view_dir: one direction for every vertex (an orthographic sensor), normalised,
    [1,3].  Exactly one of the two.  Computed in float64 and rounded once, so a second call gives the same bits; a vertex
    at the camera has no ray: ValueError."""
    if (camera is None) == (view_dir is None):
        raise ValueError("view_rays takes exactly one of camera and view_dir")
    if view_dir is not None:
        d = np.asarray(view_dir, dtype=np.float64).reshape(-1)
        if d.shape != (3,) or not np.isfinite(d).all() or not np.linalg.norm(d) > 0:
            raise ValueError("view_dir must be three finite numbers, not all zero (got %r)" % (view_dir,))
        return (d / np.linalg.norm(d)).astype(np.float32).reshape(1, 3)
    c = np.asarray(camera, dtype=np.float64).reshape(-1)
    if c.shape != (3,) or not np.isfinite(c).all():
        raise ValueError("camera must be three finite numbers (got %r)" % (camera,))
    r = np.asarray(V, dtype=np.float64).reshape(-1, 3) - c
    n = np.sqrt((r * r).sum(1, keepdims=True))
    if not (n > 0).all():
        raise ValueError("vertex %d lies at the camera: it has no viewing ray" % int(np.argmin(n)))
    return (r / n).astype(np.float32)


SensorModel = collections.namedtuple("SensorModel", "power r_ref q camera")


def sensor_model(V, camera, edge_len, power=2, quant=0.0, ref_range=None):
    """The depth-sensor noise model (build extension; include/fgc.h: fgc_synth_noise_sensor) of one clean mesh as
    SensorModel(power, r_ref, q, camera) - what FacetDenoiser.bind_clean(sensor=), makeNoisy and the trainers hand to
    ops.synth_noise_sensor, so that training, validation and the files cannot disagree.
    camera: the sensor's position in the mesh's raw units (a perspective view: an orthographic one has no range).
    power 0, 1, 2: sigma grows with (range / r_ref)^power; a noise level keeps its meaning, multiples of the mean edge length
    edge_len, now AT THE REFERENCE RANGE.  quant = S >= 0: the depth step at the reference range in mean edge lengths; the step
    at range r is r^2 q, so q = S edge_len / r_ref^2 (0: no quantisation).  ref_range (None: the distance from the camera to
    the centre of V's bounding box; the centre in float64 from the fp32 extents, the distance rounded to fp32 once)."""
    power, quant = check_sensor((power, quant))
    if camera is None:
        raise ValueError("sensor: the model needs a camera (a view_dir view has no range)")
    c = np.asarray(camera, dtype=np.float64).reshape(-1)
    if c.shape != (3,) or not np.isfinite(c).all():
        raise ValueError("sensor: camera must be three finite numbers (got %r)" % (camera,))
    if not (np.isfinite(edge_len) and edge_len > 0):
        raise ValueError("sensor: edge_len must be a positive length")
    if ref_range is None:
        v = np.asarray(V, dtype=np.float32).reshape(-1, 3)
        centre = (v.min(0).astype(np.float64) + v.max(0).astype(np.float64)) / 2.0
        ref_range = np.sqrt(((centre - c) ** 2).sum())
    r_ref = np.float32(ref_range)
    if not (np.isfinite(r_ref) and r_ref >= np.finfo(np.float32).tiny):
        raise ValueError("sensor: the reference range must be finite and > 0 (got %r; is the camera at the centre of the "
                         "mesh's bounding box?)" % (float(ref_range),))
    q = np.float32(float(quant) * float(edge_len) / float(r_ref) ** 2)
    if not np.isfinite(q) or (quant > 0 and q < np.finfo(np.float32).tiny):
        raise ValueError("sensor: quant %r gives a disparity step outside fp32 at reference range %g" % (quant, float(r_ref)))
    return SensorModel(int(power), float(r_ref), float(q), tuple(float(np.float32(t)) for t in c))


def parse_sensor(text):
    """'POWER[:QUANT]' of --sensor as (power, quant); ValueError otherwise."""
    parts = text.split(":")
    if len(parts) not in (1, 2) or not all(parts):
        raise ValueError("POWER[:QUANT]")
    try:
        power = int(parts[0])
    except ValueError:
        raise ValueError("POWER is 0, 1 or 2") from None
    quant = float(parts[1]) if len(parts) == 2 else 0.0
    if power not in (0, 1, 2):
        raise ValueError("POWER is 0, 1 or 2")
    if not (np.isfinite(quant) and quant >= 0):
        raise ValueError("QUANT must be >= 0")
    return power, quant


def check_sensor(sensor):
    """sensor=(power, quant) of the trainers and make_noisy as a checked (int, float) pair; ValueError names `sensor`."""
    try:
        power, quant = sensor
    except (TypeError, ValueError):
        raise ValueError("sensor: a pair (power, quant) (got %r)" % (sensor,)) from None
    if isinstance(power, (bool, np.bool_)) or not isinstance(power, (int, np.integer)) or int(power) not in (0, 1, 2):
        raise ValueError("sensor: power must be 0, 1 or 2 (got %r)" % (power,))
    if not (np.isfinite(quant) and quant >= 0):
        raise ValueError("sensor: quant must be finite and >= 0 (got %r)" % (quant,))
    return int(power), float(quant)


def parse_xyz(text):
    """'X,Y,Z' of --view-dir / --camera as three floats; ValueError otherwise."""
    vals = [float(t) for t in text.split(",")]
    if len(vals) != 3 or not np.isfinite(vals).all():
        raise ValueError("X,Y,Z: three finite numbers")
    return tuple(vals)


def view_options(ap):
    """The options --view-dir / --camera every depth-scan CLI has (mutually exclusive)."""
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--view-dir", default=None, metavar="X,Y,Z",
                   help="depth-scan mode: one viewing direction for every vertex (an orthographic sensor)")
    g.add_argument("--camera", default=None, metavar="X,Y,Z",
                   help="depth-scan mode: the camera position in the mesh's raw units; the rays run from it to the vertices")


def view_spec(ap, args):
    """The parsed pair of view_options as keywords of view_rays: {}, {'view_dir': xyz} or {'camera': xyz}."""
    out = {}
    for name in ("view_dir", "camera"):
        text = getattr(args, name)
        if text is not None:
            try:
                out[name] = parse_xyz(text)
            except ValueError as e:
                ap.error("--%s: %s (got %r)" % (name.replace("_", "-"), e, text))
    if "view_dir" in out and not np.linalg.norm(out["view_dir"]) > 0:
        ap.error("--view-dir must not be the zero vector")
    return out


def noise_view_spec(ap, args, direction_opt, lf_opt):
    """view_spec for the two programs that make noise along the view (train, makeNoisy), with their --sensor: the refusals of
    a --sensor that has no camera to range from and of a ray direction without a view (or a view without it).  direction_opt
    / lf_opt: the names of the program's direction and low-frequency options (their values: args.<name>).
    Returns (view, sensor = (power, quant) | None)."""
    view = view_spec(ap, args)
    attr = lambda opt: getattr(args, opt[2:].replace("-", "_"))  # noqa: E731
    sensor = None
    if args.sensor is not None:
        try:
            sensor = parse_sensor(args.sensor)
        except ValueError as e:
            ap.error("--sensor POWER[:QUANT], e.g. 2:0.5 - %s (got %r)" % (e, args.sensor))
        if args.view_dir is not None:
            ap.error("--sensor needs a perspective view: --view-dir has no range, use --camera")
        if attr(direction_opt) != "ray":
            ap.error("--sensor needs %s ray (got %s %s)" % (direction_opt, direction_opt, attr(direction_opt)))
        if args.camera is None:
            ap.error("--sensor needs --camera X,Y,Z (with %s ray)" % direction_opt)
        if attr(lf_opt) is not None:
            ap.error("--sensor does not combine with %s: quantisation after bumps along the normals is not built" % lf_opt)
    if (attr(direction_opt) == "ray") != bool(view):
        ap.error("%s ray needs --view-dir or --camera, and the two go with %s ray only" % (direction_opt, direction_opt))
    return view, sensor


def check_directions(direction, nv):
    """A [V,3] table of unit noise directions (rays) as a contiguous float32 copy (the caller's may be read-only): nv rows,
    finite, every row norm within 1e-3 of 1; ValueError otherwise."""
    d = np.asarray(direction)
    if d.ndim != 2 or d.shape != (nv, 3):
        raise ValueError("direction: an array must be [V,3] with one row per vertex (%d), got shape %r" % (nv, d.shape))
    d = np.array(d, dtype=np.float32, order="C")
    if not np.isfinite(d).all():
        raise ValueError("direction: the rows must be finite")
    n = np.sqrt((d.astype(np.float64) ** 2).sum(1))
    if np.abs(n - 1.0).max() > 1e-3:
        raise ValueError("direction: the rows must be unit vectors (row %d has norm %g)"
                         % (int(np.argmax(np.abs(n - 1.0))), n[int(np.argmax(np.abs(n - 1.0)))]))
    return d


def direction_key(direction):
    """What two binds compare a noise direction by: the mode name, or ('rays', digest of the rows) for an array."""
    if isinstance(direction, str):
        return direction
    import hashlib
    d = np.ascontiguousarray(direction, dtype=np.float32)
    return ("rays", hashlib.sha1(d.tobytes()).hexdigest())


# ---------------------------------------------------------------------------------------------------
# virtual depth scans (build extension; README "Depth scans"): what one sensor sees of a clean mesh.  The ray casting is
# ops.ray_cast (include/fgc.h: fgc_ray_cast) or, with accel=, ops.ray_cast_tree; everything around it is host code, numpy
# in and out.
# ---------------------------------------------------------------------------------------------------
def _put(a, dt):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)


def ray_tree(V, faces):
    """The bounding-box tree of a mesh on the current GPU (ops.ray_tree, include/fgc.h: fgc_ray_tree_build), numpy in, a
    handle out: pass it as accel= to visible_vertices, scan_cut and depth_image so that several views of ONE mesh share a
    build (the handle remembers the sizes of the mesh, not the mesh: give it the arrays it was built of)."""
    from . import ops
    return ops.ray_tree(_put(np.array(V, dtype=np.float32).reshape(-1, 3), np.float32),
                        _put(np.asarray(faces).astype(np.int64).reshape(-1, 3), np.int32))


def _tree_for(accel, V, faces, build):
    """The tree a call with accel= goes through: one built for this call if `build`, else accel itself if it is a handle of
    ray_tree - which must have been built of a mesh of these sizes - else None: the caller says what it accepts."""
    from . import ops
    if build:
        return ray_tree(V, faces)
    if not isinstance(accel, ops.RayTree):
        return None
    nv, nf = np.asarray(V).reshape(-1, 3).shape[0], np.asarray(faces).reshape(-1, 3).shape[0]
    if (accel.nv, accel.nf) != (nv, nf):
        raise ValueError("the tree was built of a mesh of %d vertices and %d faces, this one has %d and %d"
                         % (accel.nv, accel.nf, nv, nf))
    return accel


def _ray_cast_host(V, faces, origins, dirs, t_min=0.0, accel="none"):
    """ops.ray_cast on host arrays: (t float32 [Q], face int32 [Q]).  accel: "none" - rays x faces, brute force; "tree" -
    build a bounding-box tree for this call and cast through it (ops.ray_cast_tree); a handle of utils.ray_tree - cast
    through that tree."""
    from . import ops
    if isinstance(accel, str) and accel == "none":
        t, face = ops.ray_cast(_put(V, np.float32), _put(np.asarray(faces).astype(np.int64), np.int32),
                               _put(origins, np.float32), _put(dirs, np.float32), t_min)
        return t.cpu().numpy(), face.cpu().numpy()
    tree = _tree_for(accel, V, faces, isinstance(accel, str) and accel == "tree")
    if tree is None:
        raise ValueError('accel must be "none", "tree" or a handle of utils.ray_tree (got %r)' % (accel,))
    t, face = ops.ray_cast_tree(tree, _put(origins, np.float32), _put(dirs, np.float32), t_min)
    return t.cpu().numpy(), face.cpu().numpy()


def _bbox_diagonal(V):
    V = np.asarray(V, dtype=np.float64).reshape(-1, 3)
    return float(np.linalg.norm(V.max(0) - V.min(0)))


def visible_vertices(V, faces, camera=None, view_dir=None, eps=1e-3, accel="none"):
    """Which vertices of a mesh one sensor sees: bool [V].  Exactly one of camera (a point, perspective) and view_dir (one
    direction for every vertex, orthographic), checked as view_rays checks them.  One ray per vertex, built so that the
    vertex itself sits at t = 1: from the camera, origin = camera and d = v - camera (unnormalised); along a direction,
    origin = v - L dhat and d = L dhat with L twice the bounding-box diagonal, so that every origin lies outside the mesh.
    A vertex is visible iff the first hit of its ray (ops.ray_cast over ALL faces, its own included - they are hit at t
    close to 1) has t >= 1 - eps; a ray that hits nothing counts as visible.  accel="none": rays x faces pairs, no spatial
    culling; "tree" or a handle of utils.ray_tree: through a bounding-box tree (_ray_cast_host)."""
    view_rays(V, camera=camera, view_dir=view_dir)          # (the checks: exactly one view, finite, no vertex at the camera)
    if not (np.isfinite(eps) and 0 <= eps < 1):
        raise ValueError("eps must lie in [0, 1) (got %r)" % (eps,))
    V64 = np.asarray(V, dtype=np.float64).reshape(-1, 3)
    if camera is not None:
        c = np.asarray(camera, dtype=np.float64).reshape(1, 3)
        origins, dirs = c, V64 - c
    else:
        d = np.asarray(view_dir, dtype=np.float64).reshape(1, 3)
        step = d / np.linalg.norm(d) * (2.0 * _bbox_diagonal(V64))
        origins, dirs = V64 - step, np.broadcast_to(step, V64.shape)
    t, _ = _ray_cast_host(V64, faces, origins, dirs, accel=accel)
    return t >= np.float32(1.0 - eps)


def scan_cut(V, faces, camera=None, view_dir=None, eps=1e-3, max_angle=80.0, accel="none"):
    """The part of a mesh one sensor sees, as an open mesh: (V_cut float32 [v,3], faces_cut int32 [f,3], vertex_ids int64
    [v]).  A face stays iff its three vertices are visible (visible_vertices) and it is turned towards the sensor by less
    than max_angle degrees: -n . r >= cos(max_angle), n the unit face normal and r the unit ray to the face centre (from
    the camera, or view_dir), both in float64 on the host.  The vertices are those of the kept faces in their old order,
    vertex_ids maps them to the old ones; the faces keep their order and are re-indexed.  Nothing left: ValueError.
    max_angle = 80 is this build's choice (a sensor returns little from a surface it grazes); nobody has tuned it.
    accel: as in visible_vertices."""
    if not (np.isfinite(max_angle) and 0 < max_angle <= 180):
        raise ValueError("max_angle must lie in (0, 180] degrees (got %r)" % (max_angle,))
    vis = visible_vertices(V, faces, camera=camera, view_dir=view_dir, eps=eps, accel=accel)
    V = np.asarray(V)
    F = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    T = V.astype(np.float64).reshape(-1, 3)[F]
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    nn = np.sqrt((n * n).sum(1, keepdims=True))
    n = np.where(nn > 0, n / np.where(nn > 0, nn, 1.0), 0.0)
    if camera is not None:
        r = T.mean(1) - np.asarray(camera, dtype=np.float64).reshape(1, 3)
        r = r / np.sqrt((r * r).sum(1, keepdims=True))
    else:
        r = np.asarray(view_dir, dtype=np.float64).reshape(1, 3)
        r = r / np.linalg.norm(r)
    keep = vis[F].all(1) & (-(n * r).sum(1) >= math.cos(math.radians(max_angle)))
    if not keep.any():
        raise ValueError("scan_cut: the view sees no face of the mesh")
    Fk = F[keep]
    ids = np.unique(Fk)
    new = np.full(V.reshape(-1, 3).shape[0], -1, dtype=np.int64)
    new[ids] = np.arange(ids.size)
    return np.ascontiguousarray(V.reshape(-1, 3)[ids], dtype=np.float32), new[Fk].astype(np.int32), ids


def pixel_rays(camera, look_at, size, fov=40.0, up=(0, 0, 1)):
    """Unit pixel-centre rays of a pinhole camera, float32 [H,W,3] (built in float64, rounded once).  The camera sits at
    `camera` and looks at `look_at`; fov is the HORIZONTAL field of view in degrees, size = (W, H), square pixels; row 0 is
    the top of the image, column 0 its left.  up falls back to (0, 1, 0) when the view is within |f . up| > 0.99 of it."""
    W, H = (int(s) for s in size)
    if W < 1 or H < 1:
        raise ValueError("size = (W, H), both >= 1 (got %r)" % (size,))
    if not (np.isfinite(fov) and 0 < fov < 180):
        raise ValueError("fov must lie in (0, 180) degrees (got %r)" % (fov,))
    c = np.asarray(camera, dtype=np.float64).reshape(-1)
    f = np.asarray(look_at, dtype=np.float64).reshape(-1) - c
    if c.shape != (3,) or f.shape != (3,) or not np.isfinite(c).all() or not np.isfinite(f).all() or not np.linalg.norm(f) > 0:
        raise ValueError("camera and look_at must be two different finite points")
    f = f / np.linalg.norm(f)
    u = np.asarray(up, dtype=np.float64).reshape(-1)
    if u.shape != (3,) or not np.isfinite(u).all() or not np.linalg.norm(u) > 0:
        raise ValueError("up must be three finite numbers, not all zero (got %r)" % (up,))
    u = u / np.linalg.norm(u)
    if abs(f @ u) > 0.99:
        u = np.array([0.0, 1.0, 0.0])
    right = np.cross(f, u)
    right = right / np.linalg.norm(right)
    top = np.cross(right, f)
    half = math.tan(math.radians(fov) / 2.0)
    x = (2.0 * (np.arange(W) + 0.5) / W - 1.0) * half
    y = (1.0 - 2.0 * (np.arange(H) + 0.5) / H) * half * H / W
    r = f[None, None] + x[None, :, None] * right[None, None] + y[:, None, None] * top[None, None]
    return (r / np.sqrt((r * r).sum(-1, keepdims=True))).astype(np.float32)


def depth_image(V, faces, camera, size=(640, 480), fov=40.0, look_at=None, up=(0, 0, 1), accel="none"):
    """A depth image of a mesh: (depth float32 [H,W], face int32 [H,W], rays float32 [H,W,3]).  A pinhole at `camera`
    looking at look_at (default: the centre of the bounding box), the rays of pixel_rays; depth is the distance t along the
    unit ray to the first hit (ops.ray_cast), +inf for background, face the triangle hit or -1.  fov = 40 degrees is this
    build's choice; nobody has tuned it.  accel="none": W x H x faces pairs, no spatial culling; "tree" or a handle of
    utils.ray_tree: through a bounding-box tree (_ray_cast_host)."""
    V64 = np.asarray(V, dtype=np.float64).reshape(-1, 3)
    if look_at is None:
        look_at = 0.5 * (V64.min(0) + V64.max(0))
    rays = pixel_rays(camera, look_at, size, fov, up)
    H, W = rays.shape[:2]
    t, face = _ray_cast_host(V64, faces, np.asarray(camera, dtype=np.float64).reshape(1, 3), rays.reshape(-1, 3), accel=accel)
    return t.reshape(H, W), face.reshape(H, W), rays


def range_mesh(depth, rays, camera, jump=0.05, return_pixels=False):
    """The mesh a sensor driver would make of a depth image: (V float32 [v,3], faces int32 [f,3]).  One vertex
    camera + t r per pixel (float64, rounded once); every 2 x 2 block of pixels p[row][col] gives the two triangles
    (p00, p10, p01) and (p10, p11, p01), p10 the pixel below p00 and p01 the one to its right, which are oriented towards
    the camera; a block is kept only if its four depths are finite and max - min <= jump x min (a larger step is a
    silhouette, not a surface).  Pixels no triangle uses are dropped; the vertices are in row-major order.
    utils.view_rays(V, camera=camera) then gives the pixel rays back to one rounding.  Nothing left: ValueError.
    return_pixels: also the flat pixel index row * W + col of every vertex, int64 [v].
    jump = 0.05 is this build's choice; nobody has tuned it."""
    depth = np.asarray(depth, dtype=np.float64)
    rays = np.asarray(rays, dtype=np.float64)
    if depth.ndim != 2 or rays.shape != depth.shape + (3,):
        raise ValueError("depth [H,W] and rays [H,W,3] (got %r and %r)" % (depth.shape, rays.shape))
    if not (np.isfinite(jump) and jump >= 0):
        raise ValueError("jump must be finite and >= 0 (got %r)" % (jump,))
    H, W = depth.shape
    c = np.asarray(camera, dtype=np.float64).reshape(1, 1, 3)
    d = np.stack([depth[:-1, :-1], depth[1:, :-1], depth[:-1, 1:], depth[1:, 1:]])          # p00, p10, p01, p11
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(d).all(0) & (d.max(0) - d.min(0) <= jump * d.min(0))
    idx = np.arange(H * W).reshape(H, W)
    p00, p10, p01, p11 = idx[:-1, :-1][ok], idx[1:, :-1][ok], idx[:-1, 1:][ok], idx[1:, 1:][ok]
    faces = np.stack([np.stack([p00, p10, p01], 1), np.stack([p10, p11, p01], 1)], 1).reshape(-1, 3)
    if faces.shape[0] == 0:
        raise ValueError("range_mesh: no 2 x 2 block of the image holds a surface")
    ids = np.unique(faces)
    new = np.full(H * W, -1, dtype=np.int64)
    new[ids] = np.arange(ids.size)
    t = depth.reshape(-1)[ids]
    P = c.reshape(1, 3) + t[:, None] * rays.reshape(-1, 3)[ids]
    out = (P.astype(np.float32), new[faces].astype(np.int32))
    return out + (ids,) if return_pixels else out


def write_mesh(vl, fl, strFileName, fmt="%.6f"):
    """utils.py:659-697: 'v x y z' (6 decimals, extra per-vertex columns such as colours written as they are), then
    'f a b c' one-indexed; a face (0,0,..) ends the list and a face (-1,-1,..) is skipped, as in the reference.
    fmt (build extension): the format of a coordinate; "%.9g" keeps every float32 bit (the scan tool: a range mesh's
    vertices lie on their pixel rays to one rounding, which six decimals would undo)."""
    vl = np.asarray(vl)
    fl = np.asarray(fl).astype(np.int64) + 1
    with open(strFileName, "w") as fh:
        for row in vl:
            fh.write("v " + " ".join(fmt % x for x in row) + " \n")
        for row in fl:
            if row[0] == 1 and row[1] == 1:
                break
            if row[0] == 0 and row[1] == 0:
                continue
            fh.write("f " + " ".join(str(int(t)) for t in row) + " \n")


# ---------------------------------------------------------------------------------------------------
# evaluation metrics (what computeMetrics.py calls, utils.py:227-240, 816-1006, 1168-1239, 1973-2031, 2322-2342)
# ---------------------------------------------------------------------------------------------------
def _nn_gpu(q, p, q_cell=None, p_cell=None):
    """fgc_nn_query on host arrays: (dist float32 [nq], idx int64 [nq]) of the nearest point of p for every row of q."""
    import torch
    from . import ops
    dev = torch.device("cuda", torch.cuda.current_device())

    def put(a, dt):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    dist, idx = ops.nn_query(put(q, np.float32), put(p, np.float32), put(q_cell, np.int32), put(p_cell, np.int32))
    return dist.cpu().numpy(), idx.cpu().numpy().astype(np.int64)


def _slice_cells(pts, bounds, slices):
    """Cell coordinates of every point in the reference's partition (utils.py:876-930): along each axis slice i holds
    the points with i*max/slices < c < (i+1)*max/slices, the same numpy expressions as the reference; -1 on an axis
    where a point lies on a bound or outside [0, max]."""
    cell = np.full((pts.shape[0], 3), -1, dtype=np.int64)
    for axis, m in enumerate(bounds):
        c = pts[:, axis]
        for i in range(slices):
            cm = i * m / slices
            cM = (i + 1) * m / slices
            cell[(c > cm) & (c < cM), axis] = i
    return cell


def _one_side_over_cells(Q, S, bounds):
    """Distances of the query points Q that lie in a cell of the 5^3 partition to their nearest point of S among the
    2x2x2 cells of the 6^3 partition that the reference concatenates for that query cell (utils.py:951-965), in the
    reference's order: query cells (i, j, k) in lexicographic order, points in row order inside a cell."""
    from .ops import pack_cells
    qc = _slice_cells(Q, bounds, 5)
    sc = _slice_cells(S, bounds, 6)
    inside = np.flatnonzero((qc >= 0).all(1))
    if inside.size == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity (no point in any cell)")
    flat = (qc[inside] * np.array([25, 5, 1])).sum(1)
    order = inside[np.argsort(flat, kind="stable")]
    dist, idx = _nn_gpu(Q, S, pack_cells(qc), pack_cells(sc))
    if (idx[order] < 0).any():
        raise ValueError("zero-size array to reduction operation minimum which has no identity "
                         "(a query cell with points has no candidate point in its 2x2x2 cells)")
    return dist[order]


def hausdorffOverSampled(V0, V1, sV0, sV1, accuracyOnly=False):
    """utils.py:816-1006: (min_acc, min_comp, avg_acc, avg_comp) over the reference's spatial partition.

    Normalisation as the reference: every set is translated by the float32 corner of V0 u V1 and divided by the
    bounding-box diagonal of V0 u V1; the partition's upper bounds are the maxima of the normalised V0 u V1.  Accuracy:
    every point of V0 that lies in one of the 5^3 query cells, to its nearest point of sV1 among the 2x2x2 cells of the
    6^3 candidate partition above that query cell; completeness: V1 against sV0 the same way (skipped with accuracyOnly,
    which returns 0 for both completeness values, as the reference).  The distance scan is fgc_nn_query (libfgc) with
    the cells as masks; distances are float32 in the reference's arithmetic, so the values match the reference's.

    Quirks of the reference, kept:
      * the first two values are the MINIMUM of the per-point distances (np.amin, utils.py:997), although
        computeMetrics stores the first as its Hausdorff distance;
      * a query whose true nearest point lies outside its 2x2x2 candidate cells gets the larger, approximate distance;
      * points in no cell (on a slice bound, or outside [0, max] on an axis) are left out, of the minimum and the mean;
      * no point in any query cell, or an empty candidate set for a query cell that holds points, raises ValueError
        where the reference's np.amin over a zero-size axis raises.
    Queries and candidates are float32 on the device whatever the input dtype."""
    V0, V1, sV0, sV1 = (np.asarray(a) for a in (V0, V1, sV0, sV1))
    xmin = min(np.amin(V0[:, 0]), np.amin(V1[:, 0]))
    ymin = min(np.amin(V0[:, 1]), np.amin(V1[:, 1]))
    zmin = min(np.amin(V0[:, 2]), np.amin(V1[:, 2]))
    xmax = max(np.amax(V0[:, 0]), np.amax(V1[:, 0]))
    ymax = max(np.amax(V0[:, 1]), np.amax(V1[:, 1]))
    zmax = max(np.amax(V0[:, 2]), np.amax(V1[:, 2]))
    diag = math.sqrt(math.pow(xmax - xmin, 2) + math.pow(ymax - ymin, 2) + math.pow(zmax - zmin, 2))
    transVec = np.array(([[xmin, ymin, zmin]]), dtype=np.float32)
    V0 = (V0 - transVec) / diag
    V1 = (V1 - transVec) / diag
    sV0 = (sV0 - transVec) / diag
    sV1 = (sV1 - transVec) / diag
    bounds = (max(np.amax(V0[:, 0]), np.amax(V1[:, 0])), max(np.amax(V0[:, 1]), np.amax(V1[:, 1])),
              max(np.amax(V0[:, 2]), np.amax(V1[:, 2])))
    total_acc = _one_side_over_cells(V0, sV1, bounds)
    min_acc, avg_acc = np.amin(total_acc), np.mean(total_acc)
    if accuracyOnly:
        return min_acc, 0, avg_acc, 0
    total_comp = _one_side_over_cells(V1, sV0, bounds)
    return min_acc, np.amin(total_comp), avg_acc, np.mean(total_comp)


def mesh_distances(V0, V1):
    """Exact point-set distances between V0 (e.g. a denoised mesh) and V1 (its ground truth).  NOT a reference function:
    the reference's 'Hausdorff' column is a minimum of approximate distances (hausdorffOverSampled); this is what a user
    comparing methods wants.  Both sets are normalised as in hausdorffOverSampled (float32 corner translation, division
    by the bounding-box diagonal of V0 u V1); two unmasked fgc_nn_query scans give, over ALL points,
      acc_max, acc_mean    max / mean over V0 of the distance to the nearest point of V1,
      comp_max, comp_mean  max / mean over V1 of the distance to the nearest point of V0,
      hausdorff            max(acc_max, comp_max), the two-sided Hausdorff distance of the vertex sets.
    Returns a dict with these five float32 values."""
    V0, V1 = np.asarray(V0), np.asarray(V1)
    lo = np.minimum(V0.min(0), V1.min(0))
    hi = np.maximum(V0.max(0), V1.max(0))
    diag = math.sqrt(sum(math.pow(float(h) - float(l), 2) for l, h in zip(lo, hi)))
    transVec = lo.astype(np.float32)[None]
    A = (V0 - transVec) / diag
    B = (V1 - transVec) / diag
    acc, _ = _nn_gpu(A, B)
    comp, _ = _nn_gpu(B, A)
    out = {"acc_max": np.amax(acc), "acc_mean": np.mean(acc), "comp_max": np.amax(comp), "comp_mean": np.mean(comp)}
    out["hausdorff"] = max(out["acc_max"], out["comp_max"])
    return out


def closest_points(P, V, faces, accel=None):
    """The closest point of the mesh (V, faces) to every row of P (ops.closest_point_tree, include/fgc.h:
    fgc_closest_point_tree), numpy in and out: (dist float32 [Q], face int32 [Q], point float64 [Q,3]).  accel: a handle of
    utils.ray_tree built of these very arrays, so that several point sets share a build; None builds one for this call.
    The point is rebuilt in float64 from the kernel's (u, v) and the vertices: (1 - u - v) a + u b + v c.  A mesh without a
    face that takes part gives (inf, -1, nan)."""
    from . import ops
    V32 = np.array(V, dtype=np.float32).reshape(-1, 3)
    F = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    tree = _tree_for(accel, V32, F, accel is None)
    if tree is None:
        raise ValueError("accel must be None or a handle of utils.ray_tree (got %r)" % (accel,))
    dist, face, bary = (x.cpu().numpy() for x in ops.closest_point_tree(tree, _put(P, np.float32), want_bary=True))
    T = V32.astype(np.float64)[F[np.maximum(face, 0)].clip(0, V32.shape[0] - 1)]
    u, v = bary[:, :1].astype(np.float64), bary[:, 1:].astype(np.float64)
    point = (1.0 - u - v) * T[:, 0] + u * T[:, 1] + v * T[:, 2]
    point[face < 0] = np.nan
    return dist, face, point


class SurfaceTree:
    """What surface_tree returns: the float32 shift, the shifted vertices, the faces and the tree built of them."""

    def __init__(self, shift, V, faces, tree):
        self.shift, self.V, self.faces, self.tree = shift, V, faces, tree


def surface_tree(V, faces, shift=None):
    """A mesh prepared as the SURFACE of surface_distances: translated by `shift` (float32 [1,3]; None: its own float32
    corner) and put under a bounding-box tree on the current GPU.  Pass it as accel= so that several meshes scored against
    one ground truth share its build."""
    V = np.asarray(V).reshape(-1, 3)
    shift = V.min(0).astype(np.float32)[None] if shift is None else np.asarray(shift, dtype=np.float32).reshape(1, 3)
    Vt = (V - shift).astype(np.float32)
    F = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    return SurfaceTree(shift, Vt, F, ray_tree(Vt, F))


def surface_distances(V0, V1, F1, F0=None, accel=None):
    """Distances between a mesh and a SURFACE: the counterpart of mesh_distances, which measures to the nearest vertex.
    Normalised like it - float32 corner translation, division by the bounding-box diagonal of V0 u V1 - with the division
    applied to the distances (a distance scales with the coordinates, so this is the same number up to rounding, and the
    tree of the surface does not depend on V0); the translation takes the coordinates' magnitude out of the fp32 error.
      ev_max, ev_mean, ev_rms   max / mean / root mean square over the vertices V0 of the distance to the surface (V1, F1):
                                E_v of the denoising papers,
      comp_max, comp_mean       (with F0) max / mean over the vertices V1 of the distance to the surface (V0, F0),
      hausdorff                 (with F0) max(ev_max, comp_max);
    without F0 the last three are nan.  V0 and V1 need not have the same number of vertices.  accel: surface_tree(V1, F1),
    to share the build of one surface among several V0 (the translation is then that surface's own corner instead of the
    corner of V0 u V1).  Returns a dict of float32 values.  The distances are ops.closest_point_tree's."""
    V0, V1 = np.asarray(V0).reshape(-1, 3), np.asarray(V1).reshape(-1, 3)
    lo = np.minimum(V0.min(0), V1.min(0))
    hi = np.maximum(V0.max(0), V1.max(0))
    diag = math.sqrt(sum(math.pow(float(h) - float(l), 2) for l, h in zip(lo, hi)))
    if accel is None:
        accel = surface_tree(V1, F1, lo.astype(np.float32)[None])
    elif not isinstance(accel, SurfaceTree):
        raise ValueError("accel must be None or a handle of utils.surface_tree (got %r)" % (accel,))
    A = (V0 - accel.shift).astype(np.float32)
    ev = closest_points(A, accel.V, accel.faces, accel.tree)[0].astype(np.float64) / diag
    out = {"ev_max": ev.max(), "ev_mean": ev.mean(), "ev_rms": math.sqrt(float((ev * ev).mean())),
           "comp_max": np.nan, "comp_mean": np.nan, "hausdorff": np.nan}
    if F0 is not None:
        comp = closest_points(accel.V, A, F0)[0].astype(np.float64) / diag
        out.update(comp_max=comp.max(), comp_mean=comp.mean(), hausdorff=max(ev.max(), comp.max()))
    return {k: np.float32(v) for k, v in out.items()}


def angularDiffVec(n0, n1):
    """utils.py:1218-1239: per-row angle in degrees between n0 and n1, arccos(0.999999 * <normalize(n0), normalize(n1)>)
    with the reference's double normalisation (1e-8 in the norm); fake nodes (rows of n1 with every |entry| <= 1e-3)
    are NOT excluded here."""
    n0 = normalize(np.asarray(n0))
    n1 = normalize(np.asarray(n1))
    dotP = np.sum(np.multiply(n0, n1), axis=1)
    angDiff = np.arccos(0.999999 * dotP)
    return angDiff * 180 / math.pi


def fakeNodes(n1):
    """The fake-node mask of angularDiff (utils.py:1171-1172): every |entry| of the row <= 1e-3."""
    return np.all(np.less_equal(np.absolute(np.asarray(n1)), 10e-4), axis=-1)


def angularDiff(n0, n1):
    """utils.py:1168-1213: (mean, std) of angularDiffVec over the rows that are not fake nodes of n1."""
    fake = fakeNodes(n1)
    angDiff = np.extract(fake == False, angularDiffVec(n0, n1))  # noqa: E712  (the reference's expression)
    return np.mean(angDiff), np.std(angDiff)


def getBorderFaces(faces):
    """utils.py:227-240: int8 [F], 1 for a face with an edge that has no second face (getEdgeMap, maxEdges = 50)."""
    faces = np.asarray(faces)
    fborder = np.zeros([faces.shape[0]], dtype=np.int8)
    e_map, _ = getEdgeMap(faces)
    fborder[e_map[e_map[:, 3] < 0, 2]] = 1
    return fborder


def getDensePC(V, F, res=4):
    """utils.py:2322-2342: V followed by the barycentric samples (b0 V1 + b1 V2 + (res-b0-b1) V3) / res of every face,
    0 < b0 + b1, b0 < res, b1 < res; with res = 1 there are none and the result is V."""
    V, F = np.asarray(V), np.asarray(F)
    V1, V2, V3 = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    listV = [V]
    for b0 in range(res):
        for b1 in range(res - b0 + 1):
            if b0 < res and b1 < res and b1 + b0 > 0:
                listV.append((b0 * V1 + b1 * V2 + (res - b0 - b1) * V3) / res)
    return np.concatenate(listV, axis=0)


def getHeatMapColor(myVec):
    """utils.py:2002-2031, vectorised: float64 [n,3] colours on the ramp blue - cyan - green - yellow - red, four linear
    pieces on [0, 0.25), [0.25, 0.5), [0.5, 0.75) and the rest (NaN included).  The coefficient 4*e - k is formed in the
    input's dtype and the blend in float64, as the reference's per-element code does."""
    myVec = np.asarray(myVec)
    ramp = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 1.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    piece = np.full(myVec.shape[0], 3, dtype=np.int64)
    for k, lim in reversed(list(enumerate((0.25, 0.5, 0.75)))):
        piece[myVec < lim] = k
    heatmap = np.empty((myVec.shape[0], 3))
    for k in range(4):
        sel = piece == k
        coef = 4 * myVec[sel] - k if k else 4 * myVec[sel]
        heatmap[sel] = coef[:, None] * ramp[k + 1] + (1 - coef)[:, None] * ramp[k]
    return heatmap


def getColoredMesh(V, F, faceColors):
    """utils.py:1973-2000: a mesh with three vertices of its own per face, rows [x, y, z, r, g, b] (a face index -1
    reads the zero vertex), faces [F,3] = 0 .. 3F-1."""
    F = np.asarray(F) + 1
    V = np.concatenate((np.array([[0, 0, 0]], dtype=np.float32), np.asarray(V)), axis=0)
    Vl = V[F]
    faceColors = np.tile(np.expand_dims(np.asarray(faceColors), axis=1), (1, 3, 1))
    facesNum = F.shape[0]
    newV = np.reshape(np.concatenate((Vl, faceColors), axis=-1), (3 * facesNum, 6))
    newF = np.reshape(np.arange(3 * facesNum), (facesNum, 3))
    return newV, newF


# ---------------------------------------------------------------------------------------------------
# bilateral normal filtering, the classical baseline (utils.py:1242-1260, 2344-2526)
# ---------------------------------------------------------------------------------------------------
BILATERAL_MAX_SLICES = 64     # cells per axis of the filter's grid (FGC_BILATERAL_MAX_SLICES, include/fgc.h)


def getTrianglesArea(vl, fl, normalize=False):
    """utils.py:1242-1260, vectorised: 0.5 |(v1 - v0) x (v2 - v0)| per face in the vertices' dtype, returned as float64
    like the reference's array; normalize=True divides the vertices by twice the average edge length first."""
    vl, fl = np.asarray(vl), np.asarray(fl).astype(np.int64)
    if normalize:
        el, _ = getAverageEdgeLength(vl, fl)
        vl = vl / (2 * el)
    v0 = vl[fl[:, 0]]
    cp = np.cross(vl[fl[:, 1]] - v0, vl[fl[:, 2]] - v0)
    return (0.5 * np.sqrt((cp * cp).sum(-1))).astype(np.float64)


def getAverageEdgeLength(vl, fl, normalize=False):
    """utils.py:2501-2526: (mean edge length, number of edges), every edge counted once per adjacent triangle;
    normalize=True divides the vertices by the bounding-box diagonal first."""
    vl, fl = np.asarray(vl), np.asarray(fl).astype(np.int64)
    if normalize:
        lo, hi = vl.min(0), vl.max(0)
        vl = vl / math.sqrt(sum(math.pow(h - l, 2) for l, h in zip(lo, hi)))
    tri = vl[fl]
    lt = np.concatenate([np.linalg.norm(tri[:, 1] - tri[:, 0], axis=-1), np.linalg.norm(tri[:, 2] - tri[:, 1], axis=-1),
                         np.linalg.norm(tri[:, 0] - tri[:, 2], axis=-1)], axis=0)
    return np.mean(lt), lt.shape[0]


def bilateral_grid(slices):
    """(sx, sy, sz) of a `slices` argument: an int (the same count on every axis; the reference's grid is 10) or a
    3-tuple.  1 .. BILATERAL_MAX_SLICES per axis, ValueError otherwise."""
    if isinstance(slices, (int, np.integer)):
        grid = (int(slices),) * 3
    else:
        grid = tuple(int(s) for s in slices)
        if len(grid) != 3 or any(g != s for g, s in zip(grid, slices)):
            raise ValueError("slices must be an int or three ints, not %r" % (slices,))
    if min(grid) < 1 or max(grid) > BILATERAL_MAX_SLICES:
        raise ValueError("slices %r: 1 .. %d cells per axis are supported" % (slices, BILATERAL_MAX_SLICES))
    return grid


def bilateral_cells(Fc, slices=10, flat_axis_one_cell=False):
    """Cell coordinates int64 [n,3] of every face centre in the partition of the reference's bilateralFilter
    (utils.py:2351-2399), with the reference's own numpy expressions: the centres minus their float32 corner, bounds
    max * 1.01 in the centres' dtype, slice i of an axis holds i * max / slices <= c < (i + 1) * max / slices.  -1 on an
    axis where no slice takes the centre: on an axis of zero extent that is every face (the reference then filters
    nothing), unless flat_axis_one_cell, which gives such an axis one slice that holds every face."""
    grid = bilateral_grid(slices)
    Fc = np.asarray(Fc)
    transVec = np.array(([[np.amin(Fc[:, 0]), np.amin(Fc[:, 1]), np.amin(Fc[:, 2])]]), dtype=np.float32)
    Fc = Fc - transVec
    cell = np.full((Fc.shape[0], 3), -1, dtype=np.int64)
    for axis, s in enumerate(grid):
        c = Fc[:, axis]
        m = np.amax(c)
        if flat_axis_one_cell and not m > 0:
            cell[:, axis] = 0
            continue
        m *= 1.01
        for i in range(s):
            cm = i * m / s
            cM = (i + 1) * m / s
            cell[(c >= cm) & (c < cM), axis] = i
    return cell


def bilateral_order(cell, slices):
    """The filter's two tables (include/fgc.h: fgc_bilateral_filter) from bilateral_cells' coordinates: (order int32 [n],
    ptr int32 [sx sy sz + 1]).  order lists the faces that lie in a cell by flattened cell (i * sy + j) * sz + k, in face
    order inside a cell (a stable counting sort), then the faces in no cell; ptr is the range table over it."""
    sx, sy, sz = bilateral_grid(slices)
    cell = np.asarray(cell, dtype=np.int64).reshape(-1, 3)
    if (cell >= np.array([sx, sy, sz])).any():
        raise ValueError("cell coordinates outside the %d x %d x %d grid" % (sx, sy, sz))
    ncell = sx * sy * sz
    flat = np.where((cell < 0).any(1), ncell, (cell[:, 0] * sy + cell[:, 1]) * sz + cell[:, 2])
    order = np.argsort(flat, kind="stable").astype(np.int32)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=ncell + 1)[:ncell])]).astype(np.int32)
    return order, ptr


def bilateral_device_centres(Fc):
    """float32 centres for the device.  The filter sees only differences of centres: float32 input goes as it is, wider
    input is moved to its corner first so that the cast keeps the differences."""
    Fc = np.asarray(Fc)
    if Fc.dtype == np.float32:
        return Fc
    return (Fc - Fc.min(0)).astype(np.float32)


def FND(Fc, Fn, Fa, sigma_s_list, sigma_r_list, K=1, slices=10):
    """utils.py:2480-2496: the filtered normal descriptors, float32 [n, 3 S R]: bilateralFilter for every sigma_s (outer)
    and sigma_r (inner), concatenated; all pairs come from ONE pass over the candidates (fgc_bilateral_filter), and each
    equals the single-pair call bit for bit.  K is unused, as in the reference.  `slices` as in bilateralFilter."""
    import torch
    from . import ops
    grid = bilateral_grid(slices)
    Fc, Fn, Fa = np.asarray(Fc), np.asarray(Fn), np.asarray(Fa)
    order, ptr = bilateral_order(bilateral_cells(Fc, grid), grid)
    dev = torch.device("cuda", torch.cuda.current_device())

    def put(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    out = ops.bilateral_filter(put(bilateral_device_centres(Fc), np.float32), put(Fn, np.float32),
                               put(Fa.reshape(-1), np.float32), sigma_s_list, sigma_r_list, put(order, np.int32),
                               put(ptr, np.int32), grid)
    return out.cpu().numpy()


def bilateralFilter(Fc, Fn, Fa, sigma_s, sigma_r, slices=10):
    """utils.py:2344-2477 ("bilateral filter on list of triangles, as defined in Wang et al."): float32 [n,3],

        normalize( sum over j in window(i) of Fa_j exp(-|Fc_i - Fc_j|^2 / (2 sigma_s^2))
                                                    exp(-|Fn_i - Fn_j|^2 / (2 sigma_r^2)) Fn_j ),

    sigma_r = -1: no range term.  window(i) is the 3 x 3 x 3 block of cells around face i's cell in a grid of `slices`
    cells per axis over the centres' bounding box (bilateral_cells).  With the default slices = 10 this is the
    reference's partition and the reference's result, including what follows from it: on a coarse mesh the window cuts
    the Gaussian off early, a face in no cell gets a zero row, and a mesh with an axis of zero extent is all zeros.
    `slices` may also be a 3-tuple (not in the reference); at most BILATERAL_MAX_SLICES per axis, ValueError above.
    The sum runs on the GPU in float32 (fgc_bilateral_filter), the binning on the host."""
    return FND(Fc, Fn, Fa, [sigma_s], [sigma_r], slices=slices)


# ---------------------------------------------------------------------------------------------------
# guided normal filtering (BUILD EXTENSION: the reference stops at the bilateral filter; include/fgc.h: fgc_guided_normals)
# ---------------------------------------------------------------------------------------------------
GUIDED_MAX_RING = 64          # FGC_GUIDED_MAX_RING, include/fgc.h


def face_rings(faces):
    """(ring int32 [n, ld], ld): the patch of every face for fgc_guided_normals, zero-based and -1 padded: slot 0 the face
    itself, then the faces that share at least one vertex with it, each once, in the order of getFacesLargeAdj's row (which
    names an edge neighbour twice) with the repeats dropped.  ld is the longest ring rounded up to a multiple of 4.  A ring
    that does not fit GUIDED_MAX_RING slots raises RuntimeError(bilateral.NO_EDGE_TABLES), the message of a mesh the
    bilateral tool skips."""
    from .bilateral import NO_EDGE_TABLES
    adj = getFacesLargeAdj(faces, GUIDED_MAX_RING).astype(np.int64) - 1
    if (adj[:, -1] >= 0).any():                       # a full row: the list was cut (or the next entry would have been)
        raise RuntimeError(NO_EDGE_TABLES)
    width = int((adj >= 0).sum(1).max())
    adj = adj[:, :width]
    bad = adj < 0
    for j in range(1, width):
        bad[:, j] |= (adj[:, :j] == adj[:, j:j + 1]).any(1)
    order = np.argsort(bad, axis=1, kind="stable")    # the kept entries first, in their order
    ring = np.where(np.take_along_axis(bad, order, 1), -1, np.take_along_axis(adj, order, 1))
    ld = max(4, -(-int((ring >= 0).sum(1).max()) // 4) * 4)
    out = np.full((adj.shape[0], ld), -1, dtype=np.int32)
    out[:, :min(ld, width)] = ring[:, :ld]
    return out, ld


def face_edge_neighbours(faces, e_map=None):
    """int32 [n,3]: the face across edge t = (corner t, corner t + 1) of every face, from getEdgeMap's table (e_map, computed
    here with maxEdges = MAX_EDGES when not given), -1 at a border edge."""
    F = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    if e_map is None:
        from .settings import MAX_EDGES
        e_map, _ = getEdgeMap(F, maxEdges=MAX_EDGES)
    e_map = np.asarray(e_map, dtype=np.int64).reshape(-1, 4)
    fe = np.full(F.shape, -1, dtype=np.int32)
    e = e_map[e_map[:, 3] >= 0]
    lo, hi = np.minimum(e[:, 0], e[:, 1]), np.maximum(e[:, 0], e[:, 1])
    for mine, other in ((e[:, 2], e[:, 3]), (e[:, 3], e[:, 2])):
        for t in range(3):
            a, b = F[mine, t], F[mine, (t + 1) % 3]
            hit = (np.minimum(a, b) == lo) & (np.maximum(a, b) == hi)
            fe[mine[hit], t] = other[hit]
    return fe


def guidedFilter(Fc, Fn, Fa, faces, sigma_s, sigma_r, slices=10):
    """One pass of guided normal filtering (Zhang et al. 2015; not in the reference): float32 [n,3], bilateralFilter with
    the range term exp(-|G_i - G_j|^2 / (2 sigma_r^2)) on the guidance normals G of fgc_guided_normals (computed from Fn,
    Fa and the face rings of `faces` on the GPU) instead of on Fn.  Window, `slices` and sigma_r = -1 as in
    bilateralFilter."""
    import torch
    from . import ops
    grid = bilateral_grid(slices)
    Fc, Fn, Fa = np.asarray(Fc), np.asarray(Fn), np.asarray(Fa)
    ring, _ = face_rings(faces)
    fe = face_edge_neighbours(faces)
    order, ptr = bilateral_order(bilateral_cells(Fc, grid), grid)
    dev = torch.device("cuda", torch.cuda.current_device())

    def put(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    n, a = put(Fn, np.float32), put(Fa.reshape(-1), np.float32)
    guide = ops.guidance_normals(n, a, put(ring, np.int32), put(fe, np.int32))
    out = ops.bilateral_filter(put(bilateral_device_centres(Fc), np.float32), n, a, sigma_s, sigma_r, put(order, np.int32),
                               put(ptr, np.int32), grid, guide=guide)
    return out.cpu().numpy()
