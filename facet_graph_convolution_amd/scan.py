"""Virtual depth scans of a folder of clean OBJ files (build extension; README "Depth scans"):

    python -m facet_graph_convolution_amd.scan CLEAN_DIR SCAN_DIR (--camera X,Y,Z | --view-dir X,Y,Z)
        [--image W,H [--fov DEG] [--jump R]] [--max-angle DEG] [--eps E] [--accel none|tree] [--overwrite]

For every `name.obj` of CLEAN_DIR (sorted) the file `SCAN_DIR/name.obj`: the part of the mesh that ONE sensor sees, an
open sheet that ends at silhouettes and occlusions.  Without --image it is the visible cut of the mesh itself
(utils.scan_cut: the faces whose three vertices the sensor sees and that are turned towards it by less than --max-angle),
with the mesh's own vertices.  With --image W,H (needs --camera) it is the range mesh of a depth image of that size
(utils.depth_image, utils.range_mesh): one vertex per pixel that hit the surface, 2 x 2 blocks of pixels triangulated unless
their depths jump by more than --jump.  The names are kept, so SCAN_DIR serves as the clean folder and the ground-truth
folder of everything downstream (makeNoisy --direction ray, preprocess --clean, train --noise-direction ray,
computeMetrics) with the same --camera / --view-dir.  Existing files are skipped unless --overwrite; a mesh of which the
view sees nothing is reported and skipped.

The visibility test is ops.ray_cast (include/fgc.h: fgc_ray_cast): rays x faces pairs, brute force, once per mesh; with
--accel tree it is ops.ray_cast_tree through a bounding-box tree built once per mesh (fgc_ray_cast_tree), whose cost does
not grow with rays x faces.
--max-angle 80, --fov 40 and --jump 0.05 are this build's choices; nobody has tuned them.
"""
import argparse
import os

import numpy as np


def scan_mesh(V, faces, camera=None, view_dir=None, image=None, fov=40.0, jump=0.05, max_angle=80.0, eps=1e-3, accel="none"):
    """One virtual scan of a mesh: (V float32 [v,3], faces int32 [f,3]).  image=None: utils.scan_cut (camera or view_dir);
    image=(W, H): utils.range_mesh of utils.depth_image (camera only; the camera looks at the centre of the bounding box).
    accel: "none", "tree" or a handle of utils.ray_tree, as in utils.visible_vertices.  ValueError when the view sees nothing."""
    from . import utils
    if image is None:
        Vc, Fc, _ = utils.scan_cut(V, faces, camera=camera, view_dir=view_dir, eps=eps, max_angle=max_angle, accel=accel)
        return Vc, Fc
    if camera is None or view_dir is not None:
        raise ValueError("a depth image needs a camera (and takes no view_dir)")
    depth, _, rays = utils.depth_image(V, faces, camera, size=image, fov=fov, accel=accel)
    return utils.range_mesh(depth, rays, camera, jump=jump)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("clean_dir")
    ap.add_argument("scan_dir")
    from .utils import view_options, view_spec, load_mesh, write_mesh
    view_options(ap)
    ap.add_argument("--image", default=None, metavar="W,H", help="write the range mesh of a W x H depth image (needs --camera)")
    ap.add_argument("--fov", type=float, default=40.0, help="horizontal field of view of --image in degrees (default %(default)s)")
    ap.add_argument("--jump", type=float, default=0.05,
                    help="--image: drop a 2 x 2 block whose depths differ by more than this share of the nearest (default %(default)s)")
    ap.add_argument("--max-angle", type=float, default=80.0,
                    help="the cut: drop faces turned away from the sensor by more than this many degrees (default %(default)s)")
    ap.add_argument("--eps", type=float, default=1e-3,
                    help="the cut: a vertex is visible when nothing is hit before t = 1 - eps on its ray (default %(default)s)")
    ap.add_argument("--accel", choices=("none", "tree"), default="none",
                    help="none: every ray against every face; tree: through a bounding-box tree built per mesh (default %(default)s)")
    ap.add_argument("--overwrite", action="store_true")
    args = ap.parse_args(argv)
    view = view_spec(ap, args)
    if not view:
        ap.error("a scan needs --view-dir or --camera")
    image = None
    if args.image is not None:
        try:
            image = tuple(int(t) for t in args.image.split(","))
        except ValueError:
            image = ()
        if len(image) != 2 or min(image) < 2:
            ap.error("--image takes W,H, two integers >= 2 (got %r)" % args.image)
        if "camera" not in view:
            ap.error("--image needs --camera (a depth image has a pinhole)")
        if not (np.isfinite(args.fov) and 0 < args.fov < 180):
            ap.error("--fov must lie in (0, 180) degrees")
        if not (np.isfinite(args.jump) and args.jump >= 0):
            ap.error("--jump must be >= 0")
    if not (np.isfinite(args.max_angle) and 0 < args.max_angle <= 180):
        ap.error("--max-angle must lie in (0, 180] degrees")
    if not (np.isfinite(args.eps) and 0 <= args.eps < 1):
        ap.error("--eps must lie in [0, 1)")
    if not os.path.isdir(args.clean_dir):
        ap.error("no folder %s" % args.clean_dir)
    os.makedirs(args.scan_dir, exist_ok=True)
    written = []
    for f in sorted(n for n in os.listdir(args.clean_dir) if n.endswith(".obj")):
        out = os.path.join(args.scan_dir, f)
        if os.path.isfile(out) and not args.overwrite:
            print("Skipping %s. File already exists." % f)
            continue
        V, _, _, faces, _ = load_mesh(args.clean_dir, f, 0, False)
        try:
            Vs, Fs = scan_mesh(V, faces, image=image, fov=args.fov, jump=args.jump, max_angle=args.max_angle, eps=args.eps,
                               accel=args.accel, **view)
        except ValueError as e:
            print("Skipping %s. %s" % (f, e))
            continue
        write_mesh(Vs, Fs, out, fmt="%.9g")         # every float32 bit: the vertices stay on their rays
        print("%s: %d of %d vertices, %d of %d faces" % (f, Vs.shape[0], V.shape[0], Fs.shape[0], faces.shape[0])
              if image is None else "%s: range mesh of %d vertices, %d faces" % (f, Vs.shape[0], Fs.shape[0]))
        written.append(out)
    return written


if __name__ == "__main__":
    main()
