"""Write noisy test files from a folder of clean OBJ files (build extension; the reference's data sets are external
downloads that ship their noisy meshes):

    python -m facet_graph_convolution_amd.makeNoisy CLEAN_DIR OUT_DIR [--levels 0.1,0.2,0.3] [--seed S]
        [--direction random|normal] [--overwrite]

For every `name.obj` of CLEAN_DIR (sorted) and level k = 1, 2, ... the file `name_n<k>.obj` with the input's faces and
its vertices displaced by Gaussian noise of standard deviation level x mean edge length - the names getGTFilename,
`infer` and `computeMetrics` expect.  The noise comes from the kernel the training steps use (ops.synth_noise,
include/fgc.h: fgc_synth_noise) with stream = 1 + file index and step = level index: for the same seed these are the
meshes trainNet(noise_levels=...) validates on when the same folder was preprocessed as its validation set.
Existing files are skipped unless --overwrite.
"""
import argparse
import os

import numpy as np

DEFAULT_LEVELS = (0.1, 0.2, 0.3)


def make_noisy(V, faces, level, seed=0, stream=0, step=0, direction="random", device="cuda"):
    """The vertices V [V,3] of a clean mesh displaced at `level` x its mean edge length: float32 numpy [V,3]."""
    import torch
    from . import ops
    from .utils import getAverageEdgeLength, areaWeightedVertexNormals
    V = np.ascontiguousarray(np.asarray(V, dtype=np.float32))
    if direction not in ("random", "normal"):
        raise ValueError("direction must be 'random' or 'normal'")
    sigma = np.float32(level) * np.float32(getAverageEdgeLength(V, faces)[0])
    normals = None
    if direction == "normal":
        normals = torch.as_tensor(areaWeightedVertexNormals(V, faces).astype(np.float32), device=device)
    out = ops.synth_noise(torch.as_tensor(V, device=device), sigma, step, seed=seed, stream=stream, normals=normals)
    return out.cpu().numpy()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("clean_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--levels", default=",".join(str(l) for l in DEFAULT_LEVELS),
                    help="comma-separated multiples of the mean edge length, at most 9 (default %(default)s)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--direction", choices=("random", "normal"), default="random")
    ap.add_argument("--overwrite", action="store_true")
    args = ap.parse_args(argv)
    try:
        levels = [float(t) for t in args.levels.split(",")]
    except ValueError:
        ap.error("--levels takes comma-separated numbers (got %r)" % args.levels)
    if not levels or len(levels) > 9 or not all(np.isfinite(l) and l >= 0 for l in levels):
        ap.error("--levels: 1 to 9 levels >= 0 (the ground truth of <name>_n<k>.obj is found by dropping 7 characters)")
    if not os.path.isdir(args.clean_dir):
        ap.error("no folder %s" % args.clean_dir)
    from .utils import load_mesh, write_mesh
    os.makedirs(args.out_dir, exist_ok=True)
    written = []
    for i, f in enumerate(sorted(n for n in os.listdir(args.clean_dir) if n.endswith(".obj"))):
        V, _, _, faces, _ = load_mesh(args.clean_dir, f, 0, False)
        for k, level in enumerate(levels):
            out = os.path.join(args.out_dir, "%s_n%d.obj" % (f[:-4], k + 1))
            if os.path.isfile(out) and not args.overwrite:
                print("Skipping %s. File already exists." % os.path.basename(out))
                continue
            write_mesh(make_noisy(V, faces, level, args.seed, 1 + i, k, args.direction), faces, out)
            written.append(out)
    return written


if __name__ == "__main__":
    main()
