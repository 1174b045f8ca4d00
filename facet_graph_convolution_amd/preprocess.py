"""Build the pickled training / validation sets from folders of OBJ files (the reference's preprocess.py:8-52):

    python -m facet_graph_convolution_amd.preprocess TRAINING_DIR GT_DIR DUMP_DIR [--valid VALID_DIR] [--redundancy R]

Every `name.obj` of TRAINING_DIR is paired with its ground truth through `gt_name` (default: the reference's
`getGTFilename`, settings.py:44-47, `<model>_n<k>.obj` -> `<model>.obj`; `gt_filename` below is a laxer variant), preprocessed
natively (adjacency, coarsening, padding) `redundancy` times (each pass draws a different coarsening: the reference
uses this as data augmentation, settings.py:24) and pickled as `trainingSet.pkl` / `validSet.pkl`.  With --with-vertices
(the reference's INCLUDE_VERTICES) every mesh also keeps its vertices, faces in node order, vertex-face slots and
ground-truth vertices (addMeshWithVerticesAndGT) for trainAccuracyNet, pickled as `trainingSetWithVertices.pkl` /
`validSetWithVertices.pkl`.  With --gt-surface on top (a build extension) every ground-truth OBJ is read with its OWN faces
(addMeshWithVerticesAndGTMesh): a pair may differ in vertex and face count, nothing pairs their facets; the same two file
names, for `train --with-vertices` with or without `--surface-loss`.

Build extension - training from clean meshes, the noise synthesised per step on the GPU (train --synth-noise):

    python -m facet_graph_convolution_amd.preprocess CLEAN_DIR DUMP_DIR --clean [--valid CLEAN_VALID_DIR] [--redundancy R]

takes every OBJ of CLEAN_DIR as its own ground truth (TrainingSet.addCleanMesh) and writes `trainingSetClean.pkl` /
`validSetClean.pkl`.  With --with-vertices every mesh also keeps its vertex data (TrainingSet.addCleanMeshWithVertices) for
`train --with-vertices --synth-noise`, pickled as `trainingSetCleanWithVertices.pkl` / `validSetCleanWithVertices.pkl`.
"""
import argparse
import os
import pickle
import re

from .dataClasses import TrainingSet
from .settings import getGTFilename


def gt_filename(noisy_name):
    """`bunny_n1.obj`, `bunny_noisy.obj`, `bunny_n.obj` -> `bunny.obj`; names without such a suffix map to themselves."""
    stem = noisy_name[:-4]
    stem = re.sub(r"(_n\d*|_noisy\d*)$", "", stem)
    return stem + ".obj"


def pickleData(training_dir, gt_dir, dump_dir, valid_dir=None, redundancy=1, gt_name=getGTFilename, log=print,
               withVerts=False, gtSurface=False):
    if gtSurface and not withVerts:
        raise ValueError("gtSurface (a ground-truth mesh of its own topology) needs withVerts: only the vertex networks "
                         "train without face correspondence")
    os.makedirs(dump_dir, exist_ok=True)
    out = {}
    names = ("trainingSetWithVertices.pkl", "validSetWithVertices.pkl") if withVerts else ("trainingSet.pkl", "validSet.pkl")
    for tag, folder, rep in ((names[0], training_dir, redundancy), (names[1], valid_dir, 1)):
        if not folder or not os.path.isdir(folder):
            continue
        ds = TrainingSet()
        for f in sorted(os.listdir(folder)):
            if not f.endswith(".obj"):
                continue
            log("Adding %s (%i)" % (f, ds.mesh_count))
            for _ in range(rep):
                if gtSurface:
                    ds.addMeshWithVerticesAndGTMesh(folder, f, gt_dir, gt_name(f))
                elif withVerts:
                    ds.addMeshWithVerticesAndGT(folder, f, gt_dir, gt_name(f))
                else:
                    ds.addMeshWithGT(folder, f, gt_dir, gt_name(f))
        if ds.mesh_count:
            with open(os.path.join(dump_dir, tag), "wb") as fp:
                pickle.dump(ds, fp)
            out[tag] = ds
    return out


def pickleCleanData(clean_dir, dump_dir, valid_dir=None, redundancy=1, log=print, withVerts=False):
    """Build extension: `trainingSetClean.pkl` / `validSetClean.pkl` from folders of CLEAN OBJ files
    (TrainingSet.addCleanMesh), `redundancy` coarsenings per training mesh.  withVerts: with the vertex data
    (addCleanMeshWithVertices), as `trainingSetCleanWithVertices.pkl` / `validSetCleanWithVertices.pkl`."""
    os.makedirs(dump_dir, exist_ok=True)
    out = {}
    names = (("trainingSetCleanWithVertices.pkl", "validSetCleanWithVertices.pkl") if withVerts
             else ("trainingSetClean.pkl", "validSetClean.pkl"))
    for tag, folder, rep in ((names[0], clean_dir, redundancy), (names[1], valid_dir, 1)):
        if not folder or not os.path.isdir(folder):
            continue
        ds = TrainingSet()
        for f in sorted(os.listdir(folder)):
            if not f.endswith(".obj"):
                continue
            log("Adding %s (%i)" % (f, ds.mesh_count))
            for _ in range(rep):
                if withVerts:
                    ds.addCleanMeshWithVertices(folder, f)
                else:
                    ds.addCleanMesh(folder, f)
        if ds.mesh_count:
            with open(os.path.join(dump_dir, tag), "wb") as fp:
                pickle.dump(ds, fp)
            out[tag] = ds
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("training_dir", help="noisy training meshes (with --clean: the clean meshes)")
    ap.add_argument("gt_dir", help="their ground truth (with --clean: the dump folder)")
    ap.add_argument("dump_dir", nargs="?", default=None, help="where the pickles go (not with --clean)")
    ap.add_argument("--valid", default=None)
    ap.add_argument("--redundancy", type=int, default=1)
    ap.add_argument("--with-vertices", action="store_true",
                    help="keep the vertex data trainAccuracyNet needs (with --clean: trainingSetCleanWithVertices.pkl)")
    ap.add_argument("--clean", action="store_true",
                    help="build extension: CLEAN_DIR DUMP_DIR - clean meshes for training on synthesised noise")
    ap.add_argument("--gt-surface", action="store_true",
                    help="build extension, with --with-vertices: read every ground-truth OBJ with its own faces - a ground "
                         "truth of another topology (train --surface-loss)")
    args = ap.parse_args(argv)
    if args.gt_surface and (args.clean or not args.with_vertices):
        ap.error("--gt-surface needs --with-vertices and does not go with --clean (a clean mesh is its own ground truth)")
    if args.clean:
        if args.dump_dir is not None:
            ap.error("--clean takes two folders: CLEAN_DIR DUMP_DIR (a clean mesh is its own ground truth)")
        dump = args.gt_dir
        if not pickleCleanData(args.training_dir, dump, args.valid, args.redundancy, withVerts=args.with_vertices):
            ap.error("no OBJ file in %s" % args.training_dir)
    else:
        if args.dump_dir is None:
            ap.error("three folders are needed: TRAINING_DIR GT_DIR DUMP_DIR (or CLEAN_DIR DUMP_DIR --clean)")
        dump = args.dump_dir
        pickleData(args.training_dir, args.gt_dir, dump, args.valid, args.redundancy, withVerts=args.with_vertices,
                   gtSurface=args.gt_surface)
    print("Preprocessing complete. Dump files saved to " + dump)


if __name__ == "__main__":
    main()
