"""Denoise every OBJ of a folder WITHOUT a network: bilateral normal filtering (the reference's utils.bilateralFilter,
"as defined in Wang et al.", iterated) followed by the vertex update the network path uses:

    python -m facet_graph_convolution_amd.bilateral NOISY_DIR RESULTS_DIR
           [--iterations 10] [--sigma-s 1.0] [--sigma-r 0.35] [--vertex-iterations 60] [--slices auto|N] [--overwrite]
           [--guided] [--view-dir X,Y,Z | --camera X,Y,Z]

For each `name.obj`: face centres and areas of the noisy mesh (kept fixed), `--iterations` passes of the filter over
the face normals (fgc_bilateral_filter; centres, areas and cells stay on the device between passes), then
`--vertex-iterations` iterations of update_position2 on the filtered normals, and `name_denoised.obj` with the input's
faces - the file computeMetrics scores, so the baseline and a network's result differ only in where the normals came
from.  Existing results are skipped unless --overwrite, as in infer.

--sigma-s is in units of the mesh's mean edge length, --sigma-r is the width of the range term on |n_i - n_j| (-1: no
range term).  --slices N (or X,Y,Z) is the filter's grid; 10 is the reference's.  --slices auto (the default) takes per
axis the largest count (1 .. 64) whose cell edge is still >= 4 sigma_s: everything outside a face's 3 x 3 x 3 window then
carries a spatial weight below exp(-8) of a face at distance 0, the work per face does not grow with the mesh, and an
axis of zero extent is one slice that holds every face (the reference's partition puts such a mesh in no cell).

--guided (a build extension, not in the reference) turns every pass into guided normal filtering (Zhang et al. 2015): the
range term reads a guidance normal G instead of the noisy normal, G_i being the area-weighted mean normal of the most
consistent patch (a face and the faces that share a vertex with it) among the patches that contain face i
(include/fgc.h: fgc_guided_normals).  The guidance is recomputed from the current normals before every pass, on the
device.  It pays at high noise and loses to the plain filter at low noise (README); the other defaults stay as they are,
and nobody has tuned --sigma-s, --sigma-r or --iterations for this mode either.

--view-dir / --camera (depth-scan mode, README "Depth scans"): the mesh is a depth scan seen along one direction, or from a
camera position given in the mesh's raw units.  The viewing rays are built from the NOISY input's vertices
(utils.view_rays) and the vertex iterations become update_position_with_depth's: every vertex moves along its ray only.
"""
import argparse
import os
import time

import numpy as np

NO_EDGE_TABLES = "the mesh has a vertex with more than MAX_EDGES edges: no edge tables, no vertex update"


def auto_slices(Fc, sigma_s):
    """Per axis the largest slice count, 1 .. BILATERAL_MAX_SLICES, whose cell edge (extent * 1.01 / count, the
    partition of utils.bilateral_cells) is still >= 4 sigma_s."""
    from .utils import BILATERAL_MAX_SLICES
    Fc = np.asarray(Fc, dtype=np.float64)
    extent = (Fc.max(0) - Fc.min(0)) * 1.01
    return tuple(int(min(BILATERAL_MAX_SLICES, max(1.0, np.floor(e / (4.0 * sigma_s))))) for e in extent)


def denoise_mesh(V, faces, iterations=10, sigma_s=1.0, sigma_r=0.35, vertex_iterations=60, slices="auto", timings=None,
                 guided=False, depth_dir=None):
    """(V_out float32 [V,3], normals float32 [F,3]): `iterations` bilateral passes over the face normals of the mesh
    (sigma_s in mean edge lengths), then `vertex_iterations` iterations of update_position2.  slices: "auto", an int or
    a 3-tuple (module docstring).  Raises RuntimeError for a mesh with a vertex of more than MAX_EDGES edges.
    guided: guided normal filtering (module docstring): the face rings and edge neighbours go to the device once, every
    pass computes its guidance from the current normals there, nothing is read back between passes.  A ring of more than
    utils.GUIDED_MAX_RING faces raises the same RuntimeError.
    timings (a dict, optional) receives the wall seconds of 'host', 'filter' (all passes, guidance included) and 'vertex',
    and 'guidance', the device time of the guidance launches alone (0 without guided).
    depth_dir ([V,3] or [1,3] viewing rays, utils.view_rays): the vertex iterations are update_position_with_depth's, every
    vertex moves along its ray only."""
    import torch
    from . import ops, utils
    from .settings import MAX_EDGES
    from .train import update_position2, depth_update
    if iterations < 0 or vertex_iterations < 0:
        raise ValueError("iterations and vertex_iterations must be >= 0")
    if not sigma_s > 0 or not (sigma_r > 0 or sigma_r == -1):
        raise ValueError("sigma_s must be > 0, sigma_r > 0 or -1")
    t0 = time.time()
    V = np.ascontiguousarray(V, dtype=np.float32)
    faces = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3), dtype=np.int32)
    try:
        e_map, v_e_map = utils.getEdgeMap(faces, maxEdges=MAX_EDGES)
    except RuntimeError as e:
        raise RuntimeError(NO_EDGE_TABLES) from e
    Fc = utils.getTrianglesBarycenter(V, faces, normalize=False)
    Fa = utils.getTrianglesArea(V, faces)
    Fn = utils.computeFacesNormals(V, faces)
    el, _ = utils.getAverageEdgeLength(V, faces)
    sig = float(sigma_s) * float(el)
    auto = isinstance(slices, str)
    if auto and slices != "auto":
        raise ValueError("slices must be 'auto', an int or three ints")
    grid = auto_slices(Fc, sig) if auto else utils.bilateral_grid(slices)
    order, ptr = utils.bilateral_order(utils.bilateral_cells(Fc, grid, flat_axis_one_cell=auto), grid)
    dev = torch.device("cuda", torch.cuda.current_device())

    def put(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    c, a, n = put(utils.bilateral_device_centres(Fc), np.float32), put(Fa, np.float32), put(Fn, np.float32)
    order, ptr = put(order, np.int32), put(ptr, np.int32)
    if guided:
        ring, fe = put(utils.face_rings(faces)[0], np.int32), put(utils.face_edge_neighbours(faces, e_map), np.int32)
    torch.cuda.synchronize()
    t1 = time.time()
    marks = []
    for _ in range(iterations):
        if guided:
            marks.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            marks[-1][0].record()
            g = ops.guidance_normals(n, a, ring, fe)
            marks[-1][1].record()
            n = ops.bilateral_filter(c, n, a, sig, sigma_r, order, ptr, grid, guide=g)
        else:
            n = ops.bilateral_filter(c, n, a, sig, sigma_r, order, ptr, grid)
    torch.cuda.synchronize()
    t2 = time.time()
    guidance = sum(b.elapsed_time(e) for b, e in marks) / 1000.0
    if depth_dir is not None:
        pts = depth_update(put(V, np.float32), n, put(e_map, np.int32).unsqueeze(0), put(v_e_map, np.int32).unsqueeze(0),
                           depth_dir, vertex_iterations).unsqueeze(0)
    else:
        pts = update_position2(put(V, np.float32).unsqueeze(0), n.unsqueeze(0), put(e_map, np.int32).unsqueeze(0),
                               put(v_e_map, np.int32).unsqueeze(0), iter_num=vertex_iterations, max_edges=MAX_EDGES)
    out = pts[0].cpu().numpy(), n.cpu().numpy()
    if timings is not None:
        timings.update(host=t1 - t0, filter=t2 - t1, vertex=time.time() - t2, grid=grid, guidance=guidance)
    return out


def denoise_file(noisy_dir, filename, results_dir, overwrite=False, log=print, view=None, **params):
    """view: {} / None, or the keywords of utils.view_rays ({'view_dir': xyz} or {'camera': xyz}): depth-scan mode."""
    from .utils import load_mesh, write_mesh, view_rays
    out_name = filename[:-4] + "_denoised.obj"
    out_path = os.path.join(results_dir, out_name)
    if os.path.isfile(out_path) and not overwrite:
        log("Skipping %s. File already exists." % out_name)
        return None
    V, _, _, faces, _ = load_mesh(noisy_dir, filename, 0, False)
    faces = np.array(faces).astype(np.int32)
    tm = {}
    if view:
        params["depth_dir"] = view_rays(V, **view)
    try:
        points, _ = denoise_mesh(V, faces, timings=tm, **params)
    except RuntimeError as e:
        if str(e) != NO_EDGE_TABLES:
            raise
        log("Skipping %s: %s" % (filename, e))
        return None
    log("%s: %d faces, grid %s, host %.0f ms, filter %.0f ms%s, vertex update %.0f ms" %
        (filename, faces.shape[0], "x".join(str(g) for g in tm["grid"]), 1000 * tm["host"], 1000 * tm["filter"],
         " (guidance %.1f ms)" % (1000 * tm["guidance"]) if params.get("guided") else "", 1000 * tm["vertex"]))
    write_mesh(points, faces, out_path)
    return out_path


def _slices_arg(text):
    if text == "auto":
        return text
    try:
        vals = [int(t) for t in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("'auto', N or X,Y,Z")
    if len(vals) not in (1, 3):
        raise argparse.ArgumentTypeError("'auto', N or X,Y,Z")
    return vals[0] if len(vals) == 1 else tuple(vals)


def main(argv=None):
    from .utils import BILATERAL_MAX_SLICES, bilateral_grid, view_options, view_spec
    ap = argparse.ArgumentParser(prog="python -m facet_graph_convolution_amd.bilateral",
                                 description=__doc__.split("\n")[0])
    ap.add_argument("noisy_dir")
    ap.add_argument("results_dir")
    ap.add_argument("--iterations", type=int, default=10, help="passes of the filter over the normals")
    ap.add_argument("--sigma-s", type=float, default=1.0, help="spatial width, in mean edge lengths of the mesh")
    ap.add_argument("--sigma-r", type=float, default=0.35, help="range width on |n_i - n_j|; -1: no range term")
    ap.add_argument("--vertex-iterations", type=int, default=60, help="iterations of update_position2")
    ap.add_argument("--slices", type=_slices_arg, default="auto",
                    help="the filter's grid: auto (cell edge >= 4 sigma_s), N or X,Y,Z (1 .. %d; 10 is the reference's)"
                    % BILATERAL_MAX_SLICES)
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--guided", action="store_true",
                    help="guided normal filtering: the range term reads a guidance normal (a build extension; untuned)")
    view_options(ap)
    args = ap.parse_args(argv)
    view = view_spec(ap, args)
    if not args.sigma_s > 0:
        ap.error("--sigma-s must be > 0")
    if not (args.sigma_r > 0 or args.sigma_r == -1):
        ap.error("--sigma-r must be > 0, or -1 for no range term")
    if args.iterations < 0 or args.vertex_iterations < 0:
        ap.error("--iterations and --vertex-iterations must be >= 0")
    if args.slices != "auto":
        try:
            bilateral_grid(args.slices)
        except ValueError as e:
            ap.error("--slices: %s" % e)
    os.makedirs(args.results_dir, exist_ok=True)
    for f in sorted(os.listdir(args.noisy_dir)):
        if f.endswith(".obj"):
            print("processing noisy file: " + f)
            denoise_file(args.noisy_dir, f, args.results_dir, args.overwrite, iterations=args.iterations,
                         sigma_s=args.sigma_s, sigma_r=args.sigma_r, vertex_iterations=args.vertex_iterations,
                         slices=args.slices, guided=args.guided, view=view)


if __name__ == "__main__":
    main()
