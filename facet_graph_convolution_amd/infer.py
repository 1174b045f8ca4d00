"""Denoise every OBJ of a folder (the reference's infer.py:40-100 for the face-normal network, withVerts = False):

    python -m facet_graph_convolution_amd.infer NOISY_DIR RESULTS_DIR NETWORK.pt [--view-dir X,Y,Z | --camera X,Y,Z]
        [--with-vertices [--ray-update]]

For each `name.obj`: preprocess (native adjacency + coarsening), predict the facet normals, move the vertices with 60
iterations of update_position2, write `name_denoised.obj` (same faces) and, like the reference,
`name_inferred_normals.obj` is replaced by a plain `name_normals.txt` (one predicted unit normal per face).
Existing results are skipped unless --overwrite (B_OVERWRITE_RESULT, settings.py).

With --with-vertices (the reference's withVerts branch) the network is the multi-scale one (trainAccuracyNet's): inferNet
moves the vertices with update_position_MS and writes `name_denoised.obj`, `name_d_mid.obj` and `name_d_coarse.obj`
(the positions after the fine, the middle and the coarse stage).

--view-dir / --camera (depth-scan mode, README "Depth scans"): the mesh is a depth scan seen along one direction, or from a
camera position given in the mesh's raw units.  The viewing rays are built from the NOISY input's vertices
(utils.view_rays) and the 60 iterations are update_position_with_depth's: every vertex moves along its ray only.  With
--with-vertices the two options need --ray-update (as `train --ray-update`; without it they are refused as before: the
multi-scale update of the reference has no ray-constrained form): the 80 / 20 / 20 iterations of update_position_MS are then
the ray-constrained ones (a build extension, include/fgc.h: fgc_vertex_update_ms_dir), the vertices of all three files lie
on their rays.
"""
import argparse
import os
import time

import numpy as np


def denoise_file(net, noisy_dir, filename, results_dir, overwrite=False, log=print, view=None):
    """view: {} / None, or the keywords of utils.view_rays ({'view_dir': xyz} or {'camera': xyz}): depth-scan mode."""
    from .dataClasses import InferenceMesh
    from .train import inferNetOld
    from .utils import write_mesh, view_rays
    out_name = filename[:-4] + "_denoised.obj"
    out_path = os.path.join(results_dir, out_name)
    if os.path.isfile(out_path) and not overwrite:
        log("Skipping %s. File already exists." % out_name)
        return None
    t0 = time.time()
    mesh = InferenceMesh()
    mesh.addMesh(noisy_dir, filename)
    log("mesh added (%.0f ms): %d faces" % (1000 * (time.time() - t0), mesh.faces.shape[0]))
    t0 = time.time()
    rays = view_rays(np.asarray(mesh.vertices).reshape(-1, 3), **view) if view else None
    points, normals = inferNetOld(mesh, net, update_vertices=True, depth_dir=rays)
    log("Inference complete (%.0f ms)" % (1000 * (time.time() - t0)))
    write_mesh(points, mesh.faces, out_path)
    np.savetxt(os.path.join(results_dir, filename[:-4] + "_normals.txt"), normals, fmt="%.6f")
    return out_path


def denoise_file_with_vertices(net, noisy_dir, filename, results_dir, overwrite=False, log=print, view=None):
    """infer.py:82-101 withVerts: the three vertex sets of inferNet as OBJ files with the input's faces.  view: as in
    denoise_file - the rays of the noisy input's raw vertices go to inferNet(depth_dir=)."""
    from .dataClasses import InferenceMesh
    from .train import inferNet
    from .utils import write_mesh, view_rays
    out_path = os.path.join(results_dir, filename[:-4] + "_denoised.obj")
    if os.path.isfile(out_path) and not overwrite:
        log("Skipping %s. File already exists." % os.path.basename(out_path))
        return None
    t0 = time.time()
    mesh = InferenceMesh()
    mesh.addMeshWithVertices(noisy_dir, filename)
    log("mesh added (%.0f ms): %d faces" % (1000 * (time.time() - t0), mesh.faces.shape[0]))
    t0 = time.time()
    rays = view_rays(np.asarray(mesh.vertices).reshape(-1, 3), **view) if view else None
    res = inferNet(mesh, net, depth_dir=rays)
    log("Inference complete (%.0f ms)" % (1000 * (time.time() - t0)))
    write_mesh(res[0], mesh.faces, out_path)
    write_mesh(res[1], mesh.faces, os.path.join(results_dir, filename[:-4] + "_d_mid.obj"))
    write_mesh(res[2], mesh.faces, os.path.join(results_dir, filename[:-4] + "_d_coarse.obj"))
    return out_path


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("noisy_dir")
    ap.add_argument("results_dir")
    ap.add_argument("network", help="TensorFlow checkpoint directory / prefix (as the reference writes them) or a .pt file")
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--with-vertices", action="store_true",
                    help="multi-scale network + update_position_MS (a network trained by trainAccuracyNet)")
    from .utils import view_options, view_spec
    view_options(ap)
    ap.add_argument("--ray-update", action="store_true",
                    help="with --with-vertices and --view-dir / --camera: update_position_MS moves every vertex along its "
                    "viewing ray only (a build extension)")
    args = ap.parse_args(argv)
    view = view_spec(ap, args)
    if view and args.with_vertices and not args.ray_update:
        ap.error("--view-dir / --camera go with the single-scale vertex update: the multi-scale update of --with-vertices "
                 "has no ray-constrained form unless --ray-update asks for this build's (fgc_vertex_update_ms_dir)")
    if args.ray_update and not (view and args.with_vertices):
        ap.error("--ray-update constrains the multi-scale vertex update to the viewing rays: it needs --with-vertices and "
                 "--view-dir or --camera")
    from .net import FacetDenoiser
    from .train import load_checkpoint
    net = FacetDenoiser("cuda:0", multi_scale=args.with_vertices)
    load_checkpoint(args.network, net)
    run = denoise_file_with_vertices if args.with_vertices else denoise_file
    os.makedirs(args.results_dir, exist_ok=True)
    for f in sorted(os.listdir(args.noisy_dir)):
        if f.endswith(".obj"):
            print("processing noisy file: " + f)
            run(net, args.noisy_dir, f, args.results_dir, args.overwrite, **({"view": view} if view else {}))


if __name__ == "__main__":
    main()
