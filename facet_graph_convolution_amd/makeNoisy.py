"""Write noisy test files from a folder of clean OBJ files (build extension; the reference's data sets are external
downloads that ship their noisy meshes):

    python -m facet_graph_convolution_amd.makeNoisy CLEAN_DIR OUT_DIR [--levels 0.1,0.2,0.3] [--seed S]
        [--direction random|normal|ray] [--view-dir X,Y,Z | --camera X,Y,Z]
        [--lf-levels 0.3,0.2,0.1] [--lf-width 3] [--lf-bumps K] [--sensor POWER[:QUANT]] [--overwrite]

For every `name.obj` of CLEAN_DIR (sorted) and level k = 1, 2, ... the file `name_n<k>.obj` with the input's faces and
its vertices displaced by Gaussian noise of standard deviation level x mean edge length - the names getGTFilename,
`infer` and `computeMetrics` expect.  The noise comes from the kernel the training steps use (ops.synth_noise,
include/fgc.h: fgc_synth_noise) with stream = 1 + file index and step = level index: for the same seed these are the
meshes trainNet(noise_levels=...) validates on when the same folder was preprocessed as its validation set.
--lf-levels (one value, or one per level; level 0 in --levels gives bumps alone) adds the low-frequency field of
ops.synth_noise_lf (include/fgc.h: fgc_synth_noise_lf): file `_n<k>` is the pair (level k, lf level k), what
trainNet(noise_levels=..., lf_levels=...) validates on.  Existing files are skipped unless --overwrite.
--direction ray (with --view-dir or --camera; README "Depth scans") displaces every vertex along its viewing ray, the
noise of a depth sensor.  The rays are built from the CLEAN vertices (utils.view_rays), as `train --noise-direction ray`
builds them, so the files stay the validation meshes of a training run with the same seed and view.  The low-frequency
bumps keep going along the clean vertex normals.
--sensor POWER[:QUANT] (with --direction ray --camera; not with --view-dir or --lf-levels) makes that noise the one of a
triangulating depth sensor (utils.sensor_model, include/fgc.h: fgc_synth_noise_sensor): a level is the sigma at the
camera's distance to the mesh's centre and grows with range^POWER; QUANT > 0 quantises the depth in disparity, QUANT mean
edge lengths per step at that distance - the validation meshes of `train --sensor POWER:QUANT` with the same seed and camera.
"""
import argparse
import os

import numpy as np

DEFAULT_LEVELS = (0.1, 0.2, 0.3)


def make_noisy(V, faces, level, seed=0, stream=0, step=0, direction="random", device="cuda", lf_level=None, lf_width=3.0,
               lf_bumps=None, sensor=None, camera=None):
    """The vertices V [V,3] of a clean mesh displaced at `level` x its mean edge length: float32 numpy [V,3].  lf_level
    (None: white noise only): plus the low-frequency field of RMS lf_level mean edge lengths, bumps of width lf_width mean
    edge lengths, lf_bumps of them (None: ceil(faces / 6)) - what FacetDenoiser.set_noise(step, level, lf_level) makes on
    a mesh bound with lf=(lf_width, lf_bumps).  direction: "random", "normal" (the area-weighted vertex normals) or a
    [V,3] array of unit rows, e.g. the viewing rays of utils.view_rays (finite, every norm within 1e-3 of 1): the white
    noise goes along them.  The low-frequency bumps go along the clean vertex normals whatever the white direction.
    sensor = (power, quant) with camera = xyz (direction: the table of viewing rays from that camera; not with lf_level):
    the depth-sensor model utils.sensor_model(V, camera, edge length, power, quant) - what a step makes on a mesh bound
    with bind_clean(sensor=that model)."""
    import torch
    from . import _lib, ops, synth
    from .utils import getAverageEdgeLength
    V = np.ascontiguousarray(np.asarray(V, dtype=np.float32))
    edge_len = getAverageEdgeLength(V, faces)[0]
    if sensor is not None:
        from .utils import check_sensor, sensor_model
        sensor = check_sensor(sensor)
        if isinstance(direction, str) or camera is None:
            raise ValueError("sensor: the model works along viewing rays from a camera: direction must be the [V,3] table of "
                             "rays and camera its position")
        if lf_level is not None:
            raise ValueError("sensor does not combine with lf_level: quantisation after bumps along the normals is not built")
        sensor = sensor_model(V, camera, edge_len, *sensor)
    if lf_level is not None and not (np.isfinite(lf_level) and lf_level >= 0):
        raise ValueError("lf_level must be finite and >= 0 (got %r)" % (lf_level,))
    # the spec, plan and launch of a training step (synth.py): one copy of which table and which entry point
    spec = synth.NoiseSpec(seed, stream, direction, None if lf_level is None else (lf_width, lf_bumps), sensor)
    plan = synth.NoisePlan(spec, V, faces, edge_len, device)
    Vd = torch.as_tensor(V.reshape(-1, 3), device=device)
    ops._req_cuda(Vd)      # (a missing kernel is an error: no CPU fallback)
    out = torch.empty_like(Vd)
    scratch = torch.empty(max(plan.scratch_floats, 1), dtype=torch.float32, device=device)
    ctl = torch.from_numpy(plan.noise_words(step, level)).to(device)
    lf_ctl = None if plan.lf is None else torch.from_numpy(plan.lf_words(lf_level)).to(device)
    synth.enqueue(plan, Vd, out, scratch, ctl, lf_ctl, _lib.stream_ptr())
    return out.cpu().numpy()


def pair_lf_levels(lf_levels, n_levels):
    """The lf levels that go with n_levels noise levels (level index k pairs with lf level k; a single lf level goes with
    every noise level) as a tuple of floats >= 0 - the one check of --lf-levels here and of lf_levels in train.py."""
    lf = tuple(float(l) for l in lf_levels)
    if len(lf) == 1:
        lf = lf * n_levels
    if len(lf) != n_levels or not all(np.isfinite(l) and l >= 0 for l in lf):
        raise ValueError("lf_levels: one level >= 0, or one per noise level (%d)" % n_levels)
    return lf


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("clean_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--levels", default=",".join(str(l) for l in DEFAULT_LEVELS),
                    help="comma-separated multiples of the mean edge length, at most 9 (default %(default)s)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--direction", choices=("random", "normal", "ray"), default="random",
                    help="ray: along the viewing rays of --view-dir / --camera, built from the clean vertices")
    from .utils import view_options, noise_view_spec, view_rays
    view_options(ap)
    ap.add_argument("--lf-levels", default=None, help="low-frequency noise on top: comma-separated RMS levels in mean "
                    "edge lengths, one or one per --levels entry (pair k = level k with lf level k)")
    ap.add_argument("--lf-width", type=float, default=3.0, help="bump width in mean edge lengths (default %(default)s)")
    ap.add_argument("--lf-bumps", type=int, default=None, help="bumps per mesh (default: faces / 6, rounded up)")
    ap.add_argument("--sensor", default=None, metavar="POWER[:QUANT]",
                    help="with --direction ray --camera: depth-sensor noise - sigma grows with (range / reference range)^POWER "
                    "(0, 1 or 2), depth quantised in steps of QUANT mean edge lengths at the reference range (default 0: off)")
    ap.add_argument("--overwrite", action="store_true")
    args = ap.parse_args(argv)
    view, sensor = noise_view_spec(ap, args, "--direction", "--lf-levels")
    try:
        levels = [float(t) for t in args.levels.split(",")]
    except ValueError:
        ap.error("--levels takes comma-separated numbers (got %r)" % args.levels)
    if not levels or len(levels) > 9 or not all(np.isfinite(l) and l >= 0 for l in levels):
        ap.error("--levels: 1 to 9 levels >= 0 (the ground truth of <name>_n<k>.obj is found by dropping 7 characters)")
    lf_levels = [None] * len(levels)
    if args.lf_levels is not None:
        try:
            lf_levels = pair_lf_levels(args.lf_levels.split(","), len(levels))
        except ValueError as e:
            ap.error("--lf-levels: %s (got %r)" % (e, args.lf_levels))
        if not (np.isfinite(args.lf_width) and args.lf_width > 0):
            ap.error("--lf-width must be > 0")
        if args.lf_bumps is not None and args.lf_bumps < 1:
            ap.error("--lf-bumps must be >= 1")
    if not os.path.isdir(args.clean_dir):
        ap.error("no folder %s" % args.clean_dir)
    from .utils import load_mesh, write_mesh
    os.makedirs(args.out_dir, exist_ok=True)
    written = []
    for i, f in enumerate(sorted(n for n in os.listdir(args.clean_dir) if n.endswith(".obj"))):
        V, _, _, faces, _ = load_mesh(args.clean_dir, f, 0, False)
        direction = args.direction
        if view:        # (one ray per vertex: the synthesis kernel reads a [V,3] table)
            direction = np.ascontiguousarray(np.broadcast_to(view_rays(V, **view), np.asarray(V).shape))
        for k, level in enumerate(levels):
            out = os.path.join(args.out_dir, "%s_n%d.obj" % (f[:-4], k + 1))
            if os.path.isfile(out) and not args.overwrite:
                print("Skipping %s. File already exists." % os.path.basename(out))
                continue
            write_mesh(make_noisy(V, faces, level, args.seed, 1 + i, k, direction, lf_level=lf_levels[k],
                                  lf_width=args.lf_width, lf_bumps=args.lf_bumps, sensor=sensor,
                                  camera=view.get("camera")), faces, out)
            written.append(out)
    return written


if __name__ == "__main__":
    main()
