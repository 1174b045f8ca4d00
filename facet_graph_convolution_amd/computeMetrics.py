"""Score denoised meshes against their ground truth (the reference's computeMetrics.py:12-139):

    python -m facet_graph_convolution_amd.computeMetrics GT_DIR RESULTS_DIR [--overwrite] [--surface | --surface-only]

GT_DIR stands for TEST_GT_DATA_PATH, RESULTS_DIR for RESULTS_PATH.  For every ground truth `<name>.obj` (sorted) and
k = 1, 2, 3, the denoised `<name>_n<k>_denoised.obj` of RESULTS_DIR (what the infer CLI writes for `<name>_n<k>.obj`)
is scored with its vertices on the ground truth's faces:
  * hausdorffOverSampled(V0, GT, V0, getDensePC(GT, F, res=1), accuracyOnly=True): the reference's 'Hausdorff' (the
    MINIMUM of the per-vertex distances over its spatial partition) and mean distance;
  * per-face angular error (angularDiffVec), its mean / std without fake faces (angularDiff), and mean / std over the
    interior and the border faces (getBorderFaces);
  * `<name>_n<k>_heatmap.obj`: one coloured triangle per face, red at HEATMAP_MAX_ANGLE degrees and above;
  * one line appended to RESULTS_DIR/results_heat.csv per ground truth and k: the file name, then haus, mean distance,
    mean angle, std angle, face count, mean / std interior, mean / std border, each '%.7f' of the float32 value and
    followed by one space (a closed mesh has no border faces: its last two columns are nan, as in the reference);
  * RESULTS_DIR/angDiffFinal.mat (per-face angles of the files scored in this run) rewritten after every ground truth,
    if scipy imports.
A file whose heat map exists is skipped unless --overwrite (the reference always skips).

Deviations from the reference, nothing else: a missing `_n<k>_denoised.obj` is logged and skipped (the reference
raises); a denoised mesh whose vertex count differs from the ground truth's raises ValueError (the reference indexes out
of bounds or scores garbage); the unused getFacesLargeAdj call (computeMetrics.py:48) is not made; without scipy the
.mat file is skipped with a message (the reference fails at savemat); only `.obj` files of GT_DIR are ground truths.
Not in the reference: RESULTS_DIR/results_exact.csv gets, per scored file, the name and the five exact distances of
utils.mesh_distances (acc_max, acc_mean, comp_max, comp_mean, hausdorff) in the same format.
Not in the reference either, and only on request (without the two options nothing below happens: no file, no launch):
  --surface       every scored file also gets a line in RESULTS_DIR/results_surface.csv, same format: the name, then
                  ev_max ev_mean ev_rms comp_max comp_mean hausdorff of utils.surface_distances - distances to the ground
                  truth's SURFACE (E_v), and of the ground truth's vertices to the result's surface.  The ground truth's tree
                  is built once per ground truth.
  --surface-only  for results of another topology (a cut scan scored against the whole clean mesh): no vertex-count check,
                  no heat map; results_heat.csv, results_exact.csv and the .mat file are not written; only the three ev_*
                  columns are computed, the other three are nan.  A name that already has a line in results_surface.csv
                  is skipped unless --overwrite.
"""
import argparse
import os
import time
import warnings

import numpy as np

EXACT_KEYS = ("acc_max", "acc_mean", "comp_max", "comp_mean", "hausdorff")
SURFACE_KEYS = ("ev_max", "ev_mean", "ev_rms", "comp_max", "comp_mean", "hausdorff")


def _csv_lines(names, rows):
    """computeMetrics.py:117-132: name, then every value as '%.7f' of its float32, each followed by one space."""
    arr = np.array(rows, dtype=np.float32)
    return ["".join(w + " " for w in [n] + ["%.7f" % v for v in r]) + "\n" for n, r in zip(names, arr)]


def score_file(V0, GT, faces_gt, GTf_normals, denseGT, borderF):
    """The metrics of one denoised mesh (computeMetrics.py:71-114): (row of results_heat.csv, per-face angles,
    heat-map vertices, heat-map faces)."""
    from .settings import HEATMAP_MAX_ANGLE
    from .utils import (angularDiff, angularDiffVec, computeFacesNormals, getColoredMesh, getHeatMapColor,
                        hausdorffOverSampled)
    f_normals0 = computeFacesNormals(V0, faces_gt)
    haus_dist0, _, avg_dist0, _ = hausdorffOverSampled(V0, GT, V0, denseGT, accuracyOnly=True)
    angDistVec = angularDiffVec(f_normals0, GTf_normals)
    angDistIn = angDistVec[borderF == 0]
    angDistOut = angDistVec[borderF == 1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)    # no border faces: mean / std of nothing are nan
        angDistIn0, angStdIn0 = np.mean(angDistIn), np.std(angDistIn)
        angDistOut0, angStdOut0 = np.mean(angDistOut), np.std(angDistOut)
    angDist0, angStd0 = angularDiff(f_normals0, GTf_normals)
    angColor = np.maximum(1 - angDistVec / HEATMAP_MAX_ANGLE, np.zeros_like(angDistVec))
    newV, newF = getColoredMesh(V0, faces_gt, getHeatMapColor(1 - angColor))
    row = [haus_dist0, avg_dist0, angDist0, angStd0, faces_gt.shape[0], angDistIn0, angStdIn0, angDistOut0, angStdOut0]
    return row, angDistVec, newV, newF


def _surface_names(csv_path):
    """The names that have a line in a results_surface.csv (the first word of every line); none if there is no file."""
    if not os.path.isfile(csv_path):
        return set()
    with open(csv_path) as fh:
        return {line.split(" ", 1)[0] for line in fh if line.strip()}


def _score_surface_only(gt_dir, results_dir, overwrite, log):
    """--surface-only: E_v of every result against the surface of its ground truth, nothing else (module docstring)."""
    from .utils import load_mesh, surface_distances, surface_tree
    csv_surface = os.path.join(results_dir, "results_surface.csv")
    done = set() if overwrite else _surface_names(csv_surface)
    for gtFileName in sorted(os.listdir(gt_dir)):
        if not gtFileName.endswith(".obj"):
            continue
        base = gtFileName[:-4]
        todo = []
        for k in (1, 2, 3):
            denoizedFile = "%s_n%d_denoised.obj" % (base, k)
            if denoizedFile in done:
                log("Skipping %s: it has a line in results_surface.csv" % denoizedFile)
            elif not os.path.isfile(os.path.join(results_dir, denoizedFile)):
                log("Skipping %s: file not found" % denoizedFile)
            else:
                todo.append(denoizedFile)
        if not todo:
            continue
        GT, _, _, faces_gt, _ = load_mesh(gt_dir, gtFileName, 0, False)
        gt_tree = surface_tree(GT, np.array(faces_gt).astype(np.int32))          # once per ground truth
        rows = []
        for denoizedFile in todo:
            V0, _, _, _, _ = load_mesh(results_dir, denoizedFile, 0, False)
            t0 = time.time()
            s = surface_distances(V0, GT, gt_tree.faces, accel=gt_tree)
            log("%s: %d vertices against %d faces, E_v max %.7f mean %.7f rms %.7f (%.0f ms)" %
                (denoizedFile, V0.shape[0], gt_tree.faces.shape[0], s["ev_max"], s["ev_mean"], s["ev_rms"],
                 1000 * (time.time() - t0)))
            rows.append([s[key] for key in SURFACE_KEYS])
        with open(csv_surface, "a") as fh:
            fh.writelines(_csv_lines(todo, rows))


def computeMetrics(gt_dir, results_dir, overwrite=False, log=print, surface=False, surface_only=False):
    """Score every ground truth of gt_dir against its three denoised versions in results_dir (module docstring)."""
    from .utils import (computeFacesNormals, getBorderFaces, getDensePC, load_mesh, mesh_distances, write_mesh)
    if surface and surface_only:
        raise ValueError("surface and surface_only exclude each other")
    if surface_only:
        return _score_surface_only(gt_dir, results_dir, overwrite, log)
    try:
        import scipy.io
    except ImportError:
        scipy = None
        log("scipy not found: angDiffFinal.mat will not be written")
    csv_heat = os.path.join(results_dir, "results_heat.csv")
    csv_exact = os.path.join(results_dir, "results_exact.csv")
    csv_surface = os.path.join(results_dir, "results_surface.csv")
    angDict = {}
    for gtFileName in sorted(os.listdir(gt_dir)):
        if not gtFileName.endswith(".obj"):
            continue
        base = gtFileName[:-4]
        GT, _, _, faces_gt, _ = load_mesh(gt_dir, gtFileName, 0, False)
        GTf_normals = computeFacesNormals(GT, faces_gt)
        denseGT = getDensePC(GT, faces_gt, res=1)
        faces_gt = np.array(faces_gt).astype(np.int32)
        borderF = getBorderFaces(faces_gt)
        names, rows, exact, surf = [], [], [], []
        gt_tree = None          # --surface: the ground truth's tree, built when its first file is scored
        for k in (1, 2, 3):
            denoizedFile = "%s_n%d_denoised.obj" % (base, k)
            heatFile = "%s_n%d_heatmap.obj" % (base, k)
            if os.path.isfile(os.path.join(results_dir, heatFile)) and not overwrite:
                log("Skipping %s: %s exists" % (denoizedFile, heatFile))
                continue
            if not os.path.isfile(os.path.join(results_dir, denoizedFile)):
                log("Skipping %s: file not found" % denoizedFile)
                continue
            V0, _, _, _, _ = load_mesh(results_dir, denoizedFile, 0, False)
            if V0.shape[0] != GT.shape[0]:
                raise ValueError("%s has %d vertices, its ground truth %s has %d" %
                                 (denoizedFile, V0.shape[0], gtFileName, GT.shape[0]))
            t0 = time.time()
            row, angDistVec, newV, newF = score_file(V0, GT, faces_gt, GTf_normals, denseGT, borderF)
            d = mesh_distances(V0, GT)
            if surface:
                from .utils import surface_distances, surface_tree
                gt_tree = surface_tree(GT, faces_gt) if gt_tree is None else gt_tree
                sd = surface_distances(V0, GT, faces_gt, F0=faces_gt, accel=gt_tree)
                surf.append([sd[key] for key in SURFACE_KEYS])
            write_mesh(newV, newF, os.path.join(results_dir, heatFile))
            log("%s: haus %.7f, mean dist %.7f, angle %.4f +- %.4f deg, exact Hausdorff %.7f (%.0f ms)" %
                (denoizedFile, row[0], row[1], row[2], row[3], d["hausdorff"], 1000 * (time.time() - t0)))
            angDict[denoizedFile[:-4].replace("-", "_")] = angDistVec
            names.append(denoizedFile)
            rows.append(row)
            exact.append([d[key] for key in EXACT_KEYS])
        if not names:
            continue
        with open(csv_heat, "a") as fh:
            fh.writelines(_csv_lines(names, rows))
        with open(csv_exact, "a") as fh:
            fh.writelines(_csv_lines(names, exact))
        if surface:
            with open(csv_surface, "a") as fh:
                fh.writelines(_csv_lines(names, surf))
        if scipy is not None:
            scipy.io.savemat(os.path.join(results_dir, "angDiffFinal.mat"), mdict=angDict)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("gt_dir", help="ground-truth meshes <name>.obj (TEST_GT_DATA_PATH)")
    ap.add_argument("results_dir", help="denoised meshes <name>_n<k>_denoised.obj; results are written here (RESULTS_PATH)")
    ap.add_argument("--overwrite", action="store_true", help="score files whose heat map exists again")
    group = ap.add_mutually_exclusive_group()
    group.add_argument("--surface", action="store_true",
                       help="also write results_surface.csv: distances to the ground truth's SURFACE (E_v) and back")
    group.add_argument("--surface-only", action="store_true",
                       help="only E_v into results_surface.csv; the results may have another topology than the ground truth")
    args = ap.parse_args(argv)
    computeMetrics(args.gt_dir, args.results_dir, args.overwrite, surface=args.surface, surface_only=args.surface_only)


if __name__ == "__main__":
    main()
