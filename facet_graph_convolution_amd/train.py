"""Training / inference drivers: the behaviour of the reference's ``trainNet`` and ``inferNetOld``
(train.py:380-632, 29-144) on the MI355X kernels.  The TensorFlow session plumbing is not reproduced; what is:

  * one iteration = random patch (here: random mesh), 4000 random loss rows (fake rows included), a fresh random
    rotation applied to inputs and ground truth, ONE forward + backward + TF1-Adam update (the reference runs the
    forward three times per iteration, train.py:577,619,620: an artefact, not a contract);
  * the NaN watchdog (train.py:505-506,620-623), the smoothed loss every 50 iterations and the CSV of losses
    (train.py:580-586,629-632), checkpoints every SAVEITER iterations (train.py:551-552) with resume;
  * inference: forward without rotation, un-permute, drop fake rows, normalise twice (train.py:115-121,136).

Training command (the reference's ``train(withVerts)``, train.py:1894-1921):

    python -m facet_graph_convolution_amd.train DUMP_DIR NETWORK_DIR [--num-iterations N] [--net-name NAME]
        [--with-vertices] [--double-loss] [--capture] [--seed S]
        [--synth-noise 0.1,0.2,0.3] [--noise-direction random|normal|ray] [--view-dir X,Y,Z | --camera X,Y,Z] [--ray-update]
        [--lf-noise 0.3,0.2,0.1[:WIDTH[:BUMPS]]] [--sensor POWER[:QUANT]] [--surface-loss]

loads the pickles `preprocess` wrote and runs trainNet, trainAccuracyNet (--with-vertices) or trainDoubleLossNet
(--with-vertices --double-loss).  --synth-noise (build extension) loads the CLEAN pickles of `preprocess --clean`
(with --with-vertices: of `preprocess --clean --with-vertices`) and runs the same trainer on noise synthesised per step
on the GPU.
"""
import argparse
import collections
import os
import pickle

import numpy as np
import torch

from . import ops, tfckpt
from .makeNoisy import pair_lf_levels
from .net import FacetDenoiser, COST_SAMPLES, POINT_SAMPLES, POINT_LOSS_THRESHOLD
from .settings import SAVEITER, NUM_ITERATIONS
from .synth import NoiseSpec
from .utils import rand_rotation_matrix


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fn, gt):
        idx = torch.arange(fn.shape[0], dtype=torch.int32, device=fn.device)
        out = ops.angular_loss_fwd(fn, gt, idx)
        ctx.save_for_backward(fn, gt, idx, out)
        return out[0]

    @staticmethod
    def backward(ctx, dloss):
        fn, gt, idx, out = ctx.saved_tensors
        return ops.angular_loss_bwd(fn, gt, idx, out, 1.0) * dloss, None


def faceNormalsLoss(fn, gt_fn):
    """train.py:1272-1294: mean angle in degrees over the rows whose ground truth is not a fake (all-zero) row."""
    return _LossFn.apply(fn.reshape(-1, 3).contiguous(), gt_fn.reshape(-1, 3).contiguous().float())


class _FullLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p0, p1, i0, i1, threshold):
        loss, g = ops.point_loss(p0, p1, i0, i1, threshold, want_grad=True)
        ctx.save_for_backward(g)
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        g, = ctx.saved_tensors
        return g * dloss, None, None, None, None


def fullLoss(P0, P1, sample_ind0, sample_ind1, threshold=POINT_LOSS_THRESHOLD):
    """train.py:1373-1424: 1000 (mean distance of the sampled rows of P0 to P1 + mean distance of the sampled rows of P1
    to P0), distances above `threshold` counted as 0.  P0 [1,n0,3] / [n0,3] (differentiable), P1 the ground-truth
    points; sample_ind0 / sample_ind1 rows of P0 / P1 (int tensors on the GPU or arrays).  Gradient departures from
    TensorFlow: 0 at distance 0, and an exact tie sends the gradient to the lowest index (include/fgc.h)."""
    dev = P0.device
    i0 = torch.as_tensor(np.asarray(sample_ind0.cpu() if isinstance(sample_ind0, torch.Tensor) else sample_ind0),
                         dtype=torch.int32).to(dev)
    i1 = torch.as_tensor(np.asarray(sample_ind1.cpu() if isinstance(sample_ind1, torch.Tensor) else sample_ind1),
                         dtype=torch.int32).to(dev)
    return _FullLossFn.apply(P0.reshape(-1, 3), P1.reshape(-1, 3).detach(), i0, i1, float(threshold))


class _SurfaceLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p0, faces0, p1, faces1, i0, i1, threshold):
        loss, g = ops.surface_loss(p0, faces0, p1, faces1, i0, i1, threshold, want_grad=True)
        ctx.save_for_backward(g)
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        g, = ctx.saved_tensors
        return g * dloss, None, None, None, None, None, None


def surfaceLoss(P0, faces0, P1, faces1, sample_ind0, sample_ind1, threshold=POINT_LOSS_THRESHOLD):
    """fullLoss with distances to a SURFACE (a build extension; include/fgc.h: fgc_surface_loss): 1000 (mean distance of
    the sampled rows of P0 to the mesh (P1, faces1) + mean distance of the sampled rows of P1 to the mesh (P0, faces0)),
    distances above `threshold` counted as 0.  P0 [1,n0,3] / [n0,3] (differentiable, through the sampled rows and through
    the vertices of the faces the P1 samples land on), faces0 int [F0,3] (-1 rows allowed); P1, faces1 the ground-truth
    mesh, of any topology.  The gradient is 0 at distance 0."""
    dev = P0.device

    def ints(a):
        return torch.as_tensor(np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a), dtype=torch.int32).to(dev)
    return _SurfaceLossFn.apply(P0.reshape(-1, 3), ints(faces0).reshape(-1, 3), P1.reshape(-1, 3).detach(),
                                ints(faces1).reshape(-1, 3), ints(sample_ind0), ints(sample_ind1), float(threshold))


def save_checkpoint(path, net, iteration):
    """saver.save(sess, path, global_step=iteration) (train.py:551-552,626): weights + Adam moments + step as the
    TensorFlow bundle `<path>-<iteration>.index/.data-00000-of-00001` plus the `checkpoint` state file (tfckpt.py).
    A path ending in ".pt" keeps the same state as one torch file instead."""
    os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
    if not path.endswith(".pt"):
        return tfckpt.save_network(path, net, global_step=iteration)
    P = net.params
    torch.save({"theta": P.theta.cpu(), "m": P.m.cpu(), "v": P.v.cpu(), "step": P.step, "iteration": iteration,
                "multi_scale": net.multi_scale}, path)
    return path


def load_checkpoint(path, net):
    """saver.restore (train.py:79-87,522-534).  path: a TensorFlow checkpoint prefix, its .index file or a directory
    with a `checkpoint` state file - written by the reference or by save_checkpoint - or a ".pt" file.  Returns the
    iteration the checkpoint was taken at."""
    if tfckpt.is_tf_checkpoint(path):
        return tfckpt.load_network(path, net)
    if not os.path.isfile(path):
        raise FileNotFoundError("no checkpoint at %s" % path)
    ck = torch.load(path, map_location="cpu")
    P = net.params
    if ck["theta"].numel() != P.theta.numel():
        raise RuntimeError("checkpoint has %d parameters, network has %d" % (ck["theta"].numel(), P.theta.numel()))
    P.theta.copy_(ck["theta"])
    P.m.copy_(ck["m"])
    P.v.copy_(ck["v"])
    P.step = int(ck["step"])
    return int(ck["iteration"])


DEFAULT_NOISE_LEVELS = (0.1, 0.2, 0.3)      # --synth-noise without a value: a choice of this build (README)

# One mesh of a trainer's input: `args` follow the key in the bind call, `gt_normals` go with them (a keyword) for the
# double loss only, rows = the number of rows each sample set of a step is drawn from: (N0,), or (V, Vgt).
# verts: the raw clean vertices of a clean mesh, what the viewing rays of a depth-scan noise direction are built from.
_Mesh = collections.namedtuple("_Mesh", "args gt_normals rows verts bind_kw", defaults=(None, None))
_VALID_LOG = {1: "Iteration %d, validation loss %g", 3: "Iteration %d, validation loss = %g (points %g, normals %g)"}


def _rows(a):
    return np.asarray(a).reshape(-1, 3).shape[0]


def _meshes(ds):
    """The meshes of a TrainingSet (addMeshWithGT): bind_cached(key, x, adjs, gt)."""
    return [_Mesh((ds.in_list[i], ds.adj_list[i], ds.gt_list[i]), None, (ds.in_list[i].shape[1],))
            for i in range(len(ds.in_list))]


def _clean_meshes(ds, what):
    """The meshes of a clean TrainingSet (addCleanMesh): bind_clean(key, x, adjs, gt, vertices, faces_rows, edge_len)."""
    if not (hasattr(ds, "is_clean") and ds.is_clean()):
        raise ValueError("noise_levels needs a %s of clean meshes (TrainingSet.addCleanMesh, preprocess --clean)" % what)
    return [_Mesh((ds.in_list[i], ds.adj_list[i], ds.gt_list[i], ds.clean_vertices[i], ds.clean_faces_rows[i],
                   ds.clean_edge_len[i]), None, (np.asarray(ds.in_list[i]).shape[1],), ds.clean_vertices[i])
            for i in range(len(ds.in_list))]


def _vertex_meshes(ds, double, surface_loss=False):
    """The meshes of a TrainingSet that have ground-truth vertices: bind_vertices(key, features, adjacency, vertices,
    faces, v_faces, gt vertices[, gt_normals=gt normals][, gt_faces=gt faces]).  surface_loss: the ground-truth faces are
    the set's own (gtf_list, addMeshWithVerticesAndGTMesh) where it has them, otherwise - a paired set of one topology - the
    mesh's faces_list rows."""
    gtv, gtn, gtf = getattr(ds, "gtv_list", []), getattr(ds, "gt_list", []), getattr(ds, "gtf_list", [])
    out = []
    for i in range(len(ds.in_list)):
        if i >= len(gtv) or _rows(gtv[i]) == 0:
            continue        # train.py:792-796 draws again when a mesh has no ground-truth vertices
        if double and (i >= len(gtn) or _rows(gtn[i]) == 0):
            raise ValueError("mesh %d has no ground-truth face normals (gt_list) for the double loss" % i)
        kw = None
        if surface_loss:
            own = i < len(gtf) and _rows(gtf[i]) > 0
            if not own and _rows(gtv[i]) != _rows(ds.v_list[i]):
                raise ValueError("mesh %d has %d ground-truth vertices for %d vertices and no ground-truth faces (gtf_list: "
                                 "addMeshWithVerticesAndGTMesh, preprocess --gt-surface)"
                                 % (i, _rows(gtv[i]), _rows(ds.v_list[i])))
            kw = {"gt_faces": np.asarray(gtf[i] if own else ds.faces_list[i]).reshape(-1, 3).astype(np.int32)}
        out.append(_Mesh((ds.in_list[i], ds.adj_list[i], ds.v_list[i], ds.faces_list[i], ds.v_faces_list[i], gtv[i]),
                         gtn[i] if double else None, (_rows(ds.v_list[i]), _rows(gtv[i])), None, kw))
    return out


def _clean_vertex_meshes(ds, what, surface_loss=False):
    """The meshes of a clean vertex TrainingSet (addCleanMeshWithVertices): bind_clean_vertices(key, x, adjs, raw clean
    vertices, faces_rows, v_faces, edge_len[, gt_normals=clean normals][, surface_loss=True]); the clean vertices are the
    ground truth too, and - surface_loss - the clean faces the ground-truth faces."""
    n = len(getattr(ds, "in_list", ()))
    if not (hasattr(ds, "is_clean") and ds.is_clean() and len(ds.v_faces_list) == n and len(ds.gt_list) == n):
        raise ValueError("noise_levels needs a %s of clean meshes with their vertex data (TrainingSet."
                         "addCleanMeshWithVertices, preprocess --clean --with-vertices)" % what)
    return [_Mesh((ds.in_list[i], ds.adj_list[i], ds.clean_vertices[i], ds.clean_faces_rows[i], ds.v_faces_list[i],
                   ds.clean_edge_len[i]), ds.gt_list[i], (_rows(ds.clean_vertices[i]),) * 2, ds.clean_vertices[i],
                  {"surface_loss": True} if surface_loss else None)
            for i in range(n)]


def _trainer_inputs(form, trainSet, validSet, noise_levels, noise_direction, surface_loss=False):
    """The checked noise levels (None: the plain mode) and the training and validation meshes of a trainer.  surface_loss
    (the vertex trainers): the mesh records carry the ground-truth faces to bind."""
    if noise_levels is None:
        plain = _meshes if form == "angular" else lambda ds: _vertex_meshes(ds, form == "double", surface_loss)
        sets = [plain(ds) if ds is not None else [] for ds in (trainSet, validSet)]
        if form != "angular" and not sets[0]:
            raise ValueError("no training mesh has ground-truth vertices (addMeshWithVerticesAndGT)")
        return None, sets[0], sets[1]
    levels = tuple(float(l) for l in noise_levels)
    if not levels or not all(np.isfinite(l) and l >= 0 for l in levels):
        raise ValueError("noise_levels: a non-empty list of levels >= 0")
    if isinstance(noise_direction, dict):
        if len(noise_direction) != 1 or next(iter(noise_direction)) not in ("camera", "view_dir"):
            raise ValueError("noise_direction: a view is {'camera': xyz} or {'view_dir': xyz}")
    elif isinstance(noise_direction, str) and noise_direction not in ("random", "normal"):
        raise ValueError("noise_direction must be 'random' or 'normal', a [V,3] array of unit rows or a view "
                         "({'camera': xyz} / {'view_dir': xyz})")
    clean = _clean_meshes if form == "angular" else lambda ds, what: _clean_vertex_meshes(ds, what, surface_loss)
    return levels, clean(trainSet, "training set"), clean(validSet, "validation set") if validSet is not None else []


def _lf_inputs(levels, lf_levels, lf_width, lf_bumps):
    """The checked low-frequency setting of a trainer: (None, None), or (one lf level per noise level, (width, bumps)) -
    level index k pairs levels[k] with lf_levels[k]; a single lf level goes with every noise level."""
    if lf_levels is None:
        return None, None
    if levels is None:
        raise ValueError("lf_levels needs noise_levels (noise_levels=(0,) for bumps alone)")
    lf = pair_lf_levels(lf_levels, len(levels))
    if not (np.isfinite(lf_width) and lf_width > 0):
        raise ValueError("lf_width must be a positive number of mean edge lengths")
    if lf_bumps is not None and int(lf_bumps) < 1:
        raise ValueError("lf_bumps must be >= 1")
    return lf, (float(lf_width), None if lf_bumps is None else int(lf_bumps))


def _sensor_inputs(levels, sensor, noise_direction, lf):
    """The checked depth-sensor setting of a trainer: None, or (power, quant) - resolved per mesh by _mesh_sensor."""
    if sensor is None:
        return None
    from .utils import check_sensor
    sensor = check_sensor(sensor)
    if levels is None:
        raise ValueError("sensor needs noise_levels (noise_levels=(0,) for the quantisation alone)")
    if not (isinstance(noise_direction, dict) and "camera" in noise_direction):
        raise ValueError("sensor needs a noise_direction of viewing rays from a camera, {'camera': xyz}: a view_dir view has "
                         "no range, and 'random' / 'normal' noise no sensor")
    if lf is not None:
        raise ValueError("sensor does not combine with lf_levels: quantisation after bumps along the normals is not built")
    return sensor


def _mesh_sensor(sensor, direction, m):
    """sensor = (power, quant) of a trainer as the model of mesh record m seen from the view's camera (utils.sensor_model):
    the reference range is the camera's distance to the centre of the mesh's bounding box, so per mesh."""
    from .utils import sensor_model
    key = (id(m.verts), tuple(direction["camera"]), sensor)
    hit = _SENSORS.get(key)
    if hit is None or hit[0] is not m.verts:
        hit = _SENSORS[key] = (m.verts, sensor_model(m.verts, direction["camera"], m.args[-1], *sensor))
    return hit[1]


_SENSORS = {}


def _mesh_direction(direction, m):
    """The noise direction of mesh record m: a mode name or a [V,3] array as given, a view ({'camera': xyz} / {'view_dir':
    xyz}) as the viewing rays of the mesh's CLEAN vertices - one row per vertex, what makeNoisy --direction ray makes."""
    if not isinstance(direction, dict):
        return direction
    from .utils import view_rays
    key = (id(m.verts), tuple(sorted((k, tuple(v)) for k, v in direction.items())))
    hit = _RAYS.get(key)
    if hit is None or hit[0] is not m.verts:        # (built once per mesh and view: a loop binds its meshes every step)
        v = np.asarray(m.verts, dtype=np.float32).reshape(-1, 3)
        rays = np.ascontiguousarray(np.broadcast_to(view_rays(v, **direction), v.shape))
        rays.setflags(write=False)
        hit = _RAYS[key] = (m.verts, rays)
    return hit[1]


_RAYS = {}


def _run_noise(levels, seed, direction, lf_shape, ray_update, sensor):
    """The per-run part of a trainer's noise setting as a NoiseSpec (None: a plain run): stream 0, direction as given - a
    view is resolved per mesh - lf_shape = (width, bumps) of _lf_inputs, sensor = (power, quant) of _sensor_inputs."""
    if levels is None:
        return None
    return NoiseSpec(seed, 0, direction, lf_shape, sensor, bool(ray_update))


def _bind(F, key, m, noise=None):
    """Bind mesh record m under `key` through F = net.trainer_form(form): plain, or - noise: the run's NoiseSpec with the
    stream to bind under - clean for noise synthesis, direction and sensor filled per mesh.  (A cached mesh returns at once;
    the bind methods reshape the [1, ...] arrays.)"""
    kw = {"gt_normals": m.gt_normals} if F.gt_normals else {}
    kw.update(m.bind_kw or {})      # (the surface loss: the ground-truth faces, or the clean mesh's own)
    if noise is not None:
        spec = noise._replace(direction=_mesh_direction(noise.direction, m),
                              sensor=None if noise.sensor is None else _mesh_sensor(noise.sensor, noise.direction, m))
        # (the settings a run does not use stay out: bind_clean has no ray_update)
        kw.update({k: v for k, v in spec._asdict().items() if k in ("seed", "stream", "direction") or v})
    (F.bind if noise is None else F.bind_clean)(key, *m.args, **kw)


def _draw_samples(rs, F, m):
    """A step's sample sets: COST_SAMPLES rows of N0, or POINT_SAMPLES of V, then POINT_SAMPLES of Vgt."""
    return tuple(rs.randint(n, size=F.samples) for n in m.rows)


def _draw_step(rs, F, m, levels, counter, lf_levels=None):
    """A training step's draws, in their order: the sample sets, three uniforms for the rotation and - in synthesis mode
    only: the random stream of a plain run is what it was - the level of noise = (counter, level).  lf_levels (one per
    level): the same draw picks the pair, noise = (counter, level, lf level) - no draw of its own."""
    samples, R = _draw_samples(rs, F, m), rand_rotation_matrix(randnums=rs.uniform(size=3))
    if levels is None:
        return samples, R, None
    k = rs.randint(len(levels))
    return samples, R, (counter, levels[k]) if lf_levels is None else (counter, levels[k], lf_levels[k])


def _validate(net, form, valid, R, rs, levels=None, noise=None, lf_levels=None):
    """The mean {total, points, normals} (entries a form does not have stay 0) of the loss alone over the validation mesh
    records, with rotation R and fresh rows from rs: one pass per mesh, or - levels given - per clean mesh and noise level
    with stream = 1 + mesh index and step = level index: the SAME noisy meshes at every call (and what makeNoisy writes for
    the same seed), so the validation curve is comparable along a run.  noise: the run's NoiseSpec (_run_noise), bound as
    in training but for the stream; lf_levels: level k goes with lf level k."""
    F, vsum = net.trainer_form(form), np.zeros(3)
    for vbm, m in enumerate(valid):
        _bind(F, ("valid", vbm), m, None if levels is None else noise._replace(stream=1 + vbm))
        for k, level in enumerate((None,) if levels is None else levels):
            F.set_samples(*_draw_samples(rs, F, m))
            net.set_rotation(R)
            if level is not None:
                net.set_noise(k, level, *((lf_levels[k],) if lf_levels else ()))
            vsum[:F.outputs] += F.loss(rotate=True)[:F.outputs].cpu().numpy()
    return vsum / (len(valid) * (1 if levels is None else len(levels)))


def _validation_loss(net, form, valid, R, rs, levels=None, seed=0, direction="random", lf=None, ray_update=False,
                     sensor=None):
    """_validate with the noise setting as loose arguments: lf = (lf levels, (width, bumps)) of _lf_inputs; ray_update: the
    vertex update along the noise's rays, as in training; sensor = (power, quant): the depth-sensor model, resolved per
    mesh as in training."""
    lf_levels, lf_shape = lf or (None, None)
    return _validate(net, form, valid, R, rs, levels, _run_noise(levels, seed, direction, lf_shape, ray_update, sensor),
                     lf_levels)


def synthValidationLoss(net, valid, noise_levels, R, rs, seed=0, direction="random", lf=None, sensor=None):
    """Build extension: the mean loss over every clean validation mesh (records of _clean_meshes) at every noise level
    (_validation_loss).  R: the rotation; rs: the RandomState the loss rows are drawn from."""
    return float(_validation_loss(net, "angular", valid, R, rs, noise_levels, seed, direction, lf, sensor=sensor)[0])


def synthVertexValidationLoss(net, valid, noise_levels, R, rs, seed=0, direction="random", double=False, lf=None,
                              ray_update=False, sensor=None):
    """Build extension: {total, points, normals} (double) or {points, 0, 0} - the mean loss over every clean validation mesh
    (records of _clean_vertex_meshes) at every noise level (_validation_loss).  R: rotation; rs draws the 500 + 500 rows."""
    return _validation_loss(net, "double" if double else "points", valid, R, rs, noise_levels, seed, direction, lf,
                            ray_update, sensor)


def _resume(net, network_path, net_name):
    """Restore the directory's latest checkpoint if it belongs to this network (train.py:525-533); the iteration."""
    st = tfckpt.get_checkpoint_state(network_path)
    if st and st.model_checkpoint_path:
        split = os.path.basename(st.model_checkpoint_path).split('-')
        if split[0] == net_name:
            load_checkpoint(st.model_checkpoint_path, net)
            return int(split[1]) if len(split) > 1 and split[1].isdigit() else 0
    elif os.path.exists(os.path.join(network_path, net_name) + ".pt"):
        return load_checkpoint(os.path.join(network_path, net_name) + ".pt", net)
    return 0


def trainNet(trainSet, num_iterations, network_path=None, net_name="net", device="cuda", seed=0, log=print,
             capture=False, validSet=None, noise_levels=None, noise_direction="random", lf_levels=None, lf_width=3.0,
             lf_bumps=None, sensor=None):
    """train.py:380-632.  trainSet / validSet: dataClasses.TrainingSet.  Returns (net, lossArray [iters/50, 2]).

    noise_levels (build extension; None = the reference's loop, untouched): trainSet / validSet hold CLEAN meshes
    (TrainingSet.addCleanMesh, otherwise ValueError) and every iteration trains on fresh Gaussian vertex noise made on
    the GPU (FacetDenoiser.bind_clean): a level drawn from the list x the mesh's mean edge length, along
    noise_direction ("random" / "normal"; or a [V,3] array of unit rows for every mesh, or a view {'camera': xyz} /
    {'view_dir': xyz}: along the viewing rays of each mesh's clean vertices, the noise of a depth scan - the low-frequency
    bumps keep going along the clean vertex normals), with the global iteration as the noise counter - a resumed run goes on with
    new noise.  Validation: synthValidationLoss.

    lf_levels (build extension; needs noise_levels, length 1 or that of noise_levels): low-frequency noise on top
    (FacetDenoiser.bind_clean(lf=(lf_width, lf_bumps)), set_noise(step, level, lf_level)): level index k pairs
    noise_levels[k] with lf_levels[k] - RMS displacements in mean edge lengths of bumps lf_width mean edge lengths wide,
    lf_bumps per mesh (None: faces / 6).  The one draw that picks the level picks the pair.

    sensor = (power, quant) (build extension; needs noise_levels and noise_direction={'camera': xyz}; refused with a
    view_dir view, any other direction and lf_levels): the depth-sensor model (utils.sensor_model, FacetDenoiser.bind_clean(
    sensor=)), resolved per mesh - a level is the sigma at the camera's distance to the mesh's centre and grows with
    range^power; quant > 0 is the depth step there in mean edge lengths.  Validation scores its fixed meshes with the same model."""
    form = "angular"
    levels, meshes, valid = _trainer_inputs(form, trainSet, validSet, noise_levels, noise_direction)
    lf_levels, lf_shape = _lf_inputs(levels, lf_levels, lf_width, lf_bumps)
    sensor = _sensor_inputs(levels, sensor, noise_direction, lf_levels)
    train_noise = _run_noise(levels, seed, noise_direction, lf_shape, False, sensor)
    net = FacetDenoiser(device, seed=seed)
    F = net.trainer_form(form)
    ckpt = os.path.join(network_path, net_name) if network_path else None
    start = _resume(net, network_path, net_name) if ckpt else 0
    rs = np.random.RandomState(seed + 1)
    evalStepNum = 50
    lossArray = np.zeros([max(num_iterations // evalStepNum, 1), 2])
    bound, train_loss, train_samp, last_loss = -1, 0.0, 0, 0.0
    for it in range(num_iterations):
        if ckpt and it % SAVEITER == 0 and it > 0:
            save_checkpoint(ckpt, net, start + it)
        b = rs.randint(len(meshes))
        if b != bound:       # the reference feeds a new patch through feed_dict; here every mesh stays bound in HBM
            _bind(F, b, meshes[b], train_noise)
            bound = b
        samp_it, R_it, noise_it = _draw_step(rs, F, meshes[b], levels, start + it, lf_levels)
        if valid and it % (evalStepNum * 2) == 0:
            # train.py:588-617: every 100 iterations the loss alone on every validation mesh, with this iteration's
            # rotation and fresh random rows, BEFORE the training step; the previous row of the CSV gets the mean of
            # this and the last value
            valid_loss = _validate(net, form, valid, R_it, rs, levels, train_noise, lf_levels)[0]
            log("Iteration %d, validation loss %g" % (it, valid_loss))
            row = min(it // evalStepNum, len(lossArray) - 1)
            lossArray[row, 1] = valid_loss
            if it > 0:
                lossArray[row - 1, 1] = (valid_loss + last_loss) / 2
                last_loss = valid_loss
            _bind(F, b, meshes[b], train_noise)
        loss = F.step(*samp_it, R_it, capture=capture, noise=noise_it)
        if it % evalStepNum == 0 or it == num_iterations - 1:
            lv = loss[0].item()      # the only host sync of the loop
            if not np.isfinite(lv):  # NaN watchdog (train.py:620-623)
                log("WARNING! NAN FOUND AFTER TRAINING!!!! training example %d/%d" % (b, len(meshes)))
            train_loss += lv
            train_samp += 1
            if it % evalStepNum == 0:
                log("Iteration %d, training loss %g" % (it, train_loss / train_samp))
                lossArray[min(it // evalStepNum, len(lossArray) - 1), 0] = train_loss / train_samp
                train_loss, train_samp = 0.0, 0
    if ckpt:
        save_checkpoint(ckpt, net, start + num_iterations)
        with open(os.path.join(network_path, net_name + ".csv"), "ab") as fh:
            np.savetxt(fh, lossArray, delimiter=",")
    return net, lossArray


def trainAccuracyNet(trainSet, num_iterations, network_path=None, net_name="net", device="cuda", seed=0, log=print,
                     capture=False, validSet=None, noise_levels=None, noise_direction="random", lf_levels=None,
                     lf_width=3.0, lf_bumps=None, ray_update=False, sensor=None, surface_loss=False):
    """train.py:636-916: the multi-scale network trained through update_position_MS on the point-set loss fullLoss.
    trainSet / validSet: dataClasses.TrainingSet filled by addMeshWithVerticesAndGT.  One iteration = a random mesh
    (meshes without ground-truth vertices are skipped), SAMP_NUM = 500 random rows of the vertices and of the
    ground-truth vertices, a fresh random rotation of the input rows, the vertices and the ground truth, ONE network
    forward (normalizeTensor on head 0 only) + vertex update (80, 20, 20) + fullLoss + backward + TF1-Adam update
    (FacetDenoiser.pointset_step).  The smoothed training loss is logged every 10 iterations, the validation loss
    (every validation mesh, keep_prob 1 - this network has no dropout -, the iteration's rotation, fresh rows) every 20
    iterations before the training step; checkpoint and loss CSV every 500 iterations and at the end; resumes from the
    directory's latest checkpoint of `net_name`.

    Departure from the reference's CSV bookkeeping (train.py:846-913): the reference writes the smoothed training loss
    of iteration i to row lossArrayIter/10 - 1 (row -1, the last row, at the start of every 500-iteration block) and
    re-zeroes a 50-row array after each save.  Here iteration i writes row (i mod 500) / 10 of a 50-row block (training
    loss in column 0, validation loss in column 1, the previous row's validation entry set to the mean of its two
    neighbours as the reference does), and the block is appended to `<net_name>.csv` at every save.

    noise_levels (build extension; None = the loop above, untouched, with its random stream): trainSet / validSet hold
    CLEAN meshes (TrainingSet.addCleanMeshWithVertices, otherwise ValueError) and every iteration trains on fresh
    Gaussian vertex noise made on the GPU (FacetDenoiser.bind_clean_vertices): a level drawn from the list (after the
    rotation) x the mesh's mean edge length, along noise_direction, with the global iteration as the noise counter; the
    ground truth is the clean mesh.  Validation: synthVertexValidationLoss, every 20 iterations and - in this mode
    only - at iteration 0 as well.  lf_levels / lf_width / lf_bumps: low-frequency noise on top, as in trainNet.
    ray_update (with noise_levels and a noise_direction of rays - a view or a [V,3] table; otherwise ValueError): the
    vertex update of every training and validation step is the ray-constrained one along those rays
    (update_position_MS(depth_dir=), FacetDenoiser.bind_clean_vertices(ray_update=True)): the network learns what
    `infer --with-vertices --camera / --view-dir` will ask of it.  False: the free update, as before.
    sensor = (power, quant): the depth-sensor model, as in trainNet; ray_update composes with it unchanged.

    surface_loss (build extension; False = fullLoss as above, the same launches): the loss of every training and
    validation step is surfaceLoss, distances to SURFACES on both sides (include/fgc.h: fgc_surface_loss) - the refined
    mesh on its own faces against the ground-truth mesh on ITS faces: the set's gtf_list where it has one
    (TrainingSet.addMeshWithVerticesAndGTMesh: a ground truth of any topology), otherwise the mesh's own faces (a paired
    set of one topology), the clean faces with noise_levels.  The same scale as fullLoss, so curves compare; a vertex of a
    sparser ground truth no longer pulls the refined vertices sideways.  A gtf_list set also trains with
    surface_loss=False: fullLoss against ground-truth vertices of another count.

    Returns (net, lossArray of the last block, per-iteration training losses [num_iterations])."""
    return _train_with_vertices("points", trainSet, num_iterations, network_path, net_name, device, seed, log, capture,
                                validSet, noise_levels, noise_direction, lf_levels, lf_width, lf_bumps, ray_update, sensor,
                                surface_loss)


def trainDoubleLossNet(trainSet, num_iterations, network_path=None, net_name="net", device="cuda", seed=0, log=print,
                       capture=False, validSet=None, noise_levels=None, noise_direction="random", lf_levels=None,
                       lf_width=3.0, lf_bumps=None, ray_update=False, sensor=None, surface_loss=False):
    """train.py:919-1268: the multi-scale network trained on the point-set loss fullLoss PLUS the dense face-normal loss
    faceNormalsLoss of head 0 against the rotated ground-truth face normals (customLoss = pointsLoss + normalsLoss,
    unweighted, train.py:1100-1102).  trainSet / validSet: dataClasses.TrainingSet filled by addMeshWithVerticesAndGT
    (both gtv_list and gt_list).  One iteration is trainAccuracyNet's, except that all three heads go through
    normalizeTensor before the vertex update (train.py:1079-1081) and the normal loss joins the loss
    (FacetDenoiser.double_loss_step).  Same mesh selection, cadence (training loss every 10 iterations, validation every
    20 - logged with its points / normals split, train.py:1237 -, checkpoint and CSV every 500 and at the end), resume
    and NaN warning as trainAccuracyNet.  A mesh with ground-truth vertices but no ground-truth normals is an error.

    Departure from the reference's CSV bookkeeping (train.py:1199-1257), the same as trainAccuracyNet's: iteration i
    writes row (i mod 500) / 10 of a 50-row block (training loss - the total - in column 0, validation total in column
    1, the previous row's validation entry set to the mean of its two neighbours), and the block is appended to
    `<net_name>.csv` at every save.

    noise_levels / noise_direction / lf_levels / lf_width / lf_bumps / ray_update / sensor (build extension): as in
    trainAccuracyNet; the ground-truth normals are the clean ones.  surface_loss: the points part is surfaceLoss, as in
    trainAccuracyNet; the normals part still needs ground-truth normals of the mesh's own topology (gt_list), so a set made by
    addMeshWithVerticesAndGTMesh is refused here.

    Returns (net, lossArray of the last block, per-iteration {total, points, normals} [num_iterations, 3])."""
    return _train_with_vertices("double", trainSet, num_iterations, network_path, net_name, device, seed, log, capture,
                                validSet, noise_levels, noise_direction, lf_levels, lf_width, lf_bumps, ray_update, sensor,
                                surface_loss)


def _train_with_vertices(form, trainSet, num_iterations, network_path, net_name, device, seed, log, capture, validSet,
                         noise_levels=None, noise_direction="random", lf_levels=None, lf_width=3.0, lf_bumps=None,
                         ray_update=False, sensor=None, surface_loss=False):
    """The loop of trainAccuracyNet (form "points") and trainDoubleLossNet ("double")."""
    surface_loss = bool(surface_loss)
    levels, meshes, valid = _trainer_inputs(form, trainSet, validSet, noise_levels, noise_direction, surface_loss)
    # (said without the lower-case word the numeric log lines carry: readers of the log parse those by it)
    log("Point sets are scored by %s" % ("surfaceLoss: vertices to surfaces, both sides" if surface_loss
                                         else "fullLoss: vertices to nearest vertices"))
    lf_levels, lf_shape = _lf_inputs(levels, lf_levels, lf_width, lf_bumps)
    sensor = _sensor_inputs(levels, sensor, noise_direction, lf_levels)
    ray_update = bool(ray_update)
    if ray_update and (levels is None or isinstance(noise_direction, str)):
        raise ValueError("ray_update moves the vertices along the noise's rays: it needs noise_levels and a noise_direction "
                         "of rays (a view {'camera': xyz} / {'view_dir': xyz} or a [V,3] table)")
    train_noise = _run_noise(levels, seed, noise_direction, lf_shape, ray_update, sensor)
    net = FacetDenoiser(device, multi_scale=True, seed=seed)
    F = net.trainer_form(form)
    ckpt = os.path.join(network_path, net_name) if network_path else None
    start = _resume(net, network_path, net_name) if ckpt else 0
    rs = np.random.RandomState(seed + 1)
    evalStepNum, validStepNum, block = 10, 20, 500
    # (synthesis mode scores its fixed noisy validation meshes at iteration 0 too, as trainNet does: the curve starts at the
    #  restored weights, before this run's first step; the plain mode's first pass is iteration 20)
    first_valid = validStepNum if levels is None else 0
    lossArray = np.zeros([block // evalStepNum, 2])
    hist = torch.zeros(max(num_iterations, 1), F.outputs, dtype=torch.float32, device=net.device)
    acc = torch.zeros(1, dtype=torch.float32, device=net.device)
    acc_n, last_loss = 0, 0.0

    def save(iteration):
        save_checkpoint(ckpt, net, iteration)
        with open(os.path.join(network_path, net_name + ".csv"), "ab") as fh:
            np.savetxt(fh, lossArray, delimiter=",")

    for it in range(num_iterations):
        b = rs.randint(len(meshes))
        samp_it, R_it, noise_it = _draw_step(rs, F, meshes[b], levels, start + it, lf_levels)
        row = (it % block) // evalStepNum
        if valid and it % validStepNum == 0 and it >= first_valid:
            vsum = _validate(net, form, valid, R_it, rs, levels, train_noise, lf_levels)
            log(_VALID_LOG[F.outputs] % ((it,) + tuple(vsum[:F.outputs])))      # (the double loss with its points / normals split)
            lossArray[row, 1] = vsum[0]
            if row > 0:
                lossArray[row - 1, 1] = (vsum[0] + last_loss) / 2
            last_loss = vsum[0]
        _bind(F, b, meshes[b], train_noise)
        out = F.step(*samp_it, R_it, capture=capture, noise=noise_it)
        hist[it].copy_(out)
        acc += out[0:1]
        acc_n += 1
        if it % evalStepNum == 0:
            lv = acc.item() / acc_n           # the only host sync of a training iteration, every 10 iterations
            if not np.isfinite(lv):
                log("WARNING! NAN FOUND AFTER TRAINING!!!! training example %d/%d" % (b, len(meshes)))
            log("Iteration %d, training loss %g" % (it, lv))
            lossArray[row, 0] = lv
            acc.zero_()
            acc_n = 0
        if ckpt and it % block == 0 and it > 0:
            save(start + it)
            lossArray = np.zeros_like(lossArray)
    if ckpt:
        save(start + num_iterations)
    hist = hist[:num_iterations].cpu().numpy()
    return net, lossArray, hist if F.outputs > 1 else hist[:, 0]


def update_position2(x, face_normals, edge_map, v_edges, iter_num=20, max_edges=20):
    """train.py:1467-1557, same argument layout on torch GPU tensors: x [1,V,3], face_normals [1,F,3], edge_map
    int [1,E,4], v_edges int [1,V,max_edges] (-1 = unused slot); returns the updated positions [1,V,3].
    lambda = 1/18 as in the reference (:1469)."""
    if v_edges.shape[-1] != max_edges:
        raise ValueError("v_edges has %d slots per vertex, max_edges says %d" % (v_edges.shape[-1], max_edges))
    out = ops.vertex_update(x.reshape(-1, 3), face_normals.reshape(-1, 3), edge_map.reshape(-1, 4),
                            v_edges.reshape(-1, max_edges), iter_num)
    return out.unsqueeze(0)


def update_position_with_depth(x, face_normals, edge_map, v_edges, depth_dir, iter_num=20):
    """train.py:1561-1665, same argument layout on torch GPU tensors: update_position2 with every contribution projected
    onto a per-vertex direction, so that a vertex of a depth scan moves along its viewing ray only.  x [1,V,3],
    face_normals [1,F,3], edge_map int [1,E,4], v_edges int [1,V,slots] (-1 = unused; any width - the reference hard-codes
    50), depth_dir [1,3] or [V,3] (the reference's reshape(depth_dir, [1,-1,1,1,3]); used as given, not normalised).
    Returns the reference's pair (x [1,V,3], x - x_init [1,V,3]).  lambda = 1/18 (:1563).  The positions are fma(t,
    depth_dir, x_init) of the accumulated step t (include/fgc.h: fgc_vertex_update_dir), not a chain of additions."""
    x = x.reshape(-1, 3)
    out = ops.vertex_update_dir(x, face_normals.reshape(-1, 3), edge_map.reshape(-1, 4),
                                v_edges.reshape(x.shape[0], -1), depth_dir.reshape(-1, 3), iter_num)
    return out.unsqueeze(0), (out - x.float()).unsqueeze(0)


def depth_update(V, normals, e_map, v_e_map, depth_dir, iters):
    """What the single-scale drivers (inferNetOld, bilateral.denoise_mesh) run in the place of update_position2 when they are
    given viewing rays: update_position_with_depth on device tensors V [V,3], normals [F,3], e_map [1,E,4], v_e_map
    [1,V,slots] and depth_dir [V,3] / [1,3] (array-like or tensor).  Returns the positions [V,3]."""
    d = ops.ray_rows(depth_dir, V.shape[0], V.device, "depth_dir")
    return update_position_with_depth(V.unsqueeze(0), normals.unsqueeze(0), e_map, v_e_map, d, iter_num=iters)[0][0]


def updateFacesCenter(vertices, faces, coarsening_steps):
    """train.py:1768-1798: node centres of the three levels, [fpos0 [1,N0,3], fpos1 [1,N0/4,3], fpos2 [1,N0/16,3]]."""
    if coarsening_steps != 2:
        raise NotImplementedError("libfgc pools 4:1 (coarsening_steps = 2, settings.py:31)")
    f0 = ops.face_centers(vertices.reshape(-1, 3), faces.reshape(-1, 3))
    f1 = ops.pool4_avg_iz(f0)
    f2 = ops.pool4_avg_iz(f1)
    return [f0.unsqueeze(0), f1.unsqueeze(0), f2.unsqueeze(0)]


class _UpdatePositionMSFn(torch.autograd.Function):
    """The multi-scale update with its adjoint, free (dirs None) or along the rays `dirs` (no gradient with respect to them)."""
    @staticmethod
    def forward(ctx, x, n0, n1, n2, faces, v_faces, dirs, iters, tables):
        traj = ops._ms_forward(x, [n0, n1, n2], faces, v_faces, iters, dirs, traj=True)
        ctx.save_for_backward(traj, n0, n1, n2, faces, v_faces, dirs)
        ctx.iters, ctx.tables = iters, tables
        ctx.set_materialize_grads(False)      # (unused outputs: None, not zero tensors)
        T0, T1 = iters[0], iters[0] + iters[1]
        out = traj[-1].clone()
        # dx of each stage = end - start, the same fp32 subtraction as fgc_vertex_update_ms's dx_out
        return out, traj[T0] - traj[0], traj[T1] - traj[T0], traj[-1] - traj[T1]

    @staticmethod
    def backward(ctx, g_out, g_dx0, g_dx1, g_dx2):
        traj, n0, n1, n2, faces, v_faces, dirs = ctx.saved_tensors
        if g_out is None or any(g is not None for g in (g_dx0, g_dx1, g_dx2)):
            raise NotImplementedError("update_position_MS differentiates its positions, not the stage displacements")
        g_x, g_n = ops._ms_backward(traj, [n0, n1, n2], faces, v_faces, g_out, ctx.iters, ctx.tables, dirs)
        return g_x, g_n[0], g_n[1], g_n[2], None, None, None, None, None


def update_position_MS(x, face_normals_list, faces, v_faces0, coarsening_steps, iter_num_list=[80, 20, 20], tables=None,
                       depth_dir=None):
    """train.py:1668-1764, same arguments on torch GPU tensors: x [1,V,3], face_normals_list = [n0 [1,N0,3],
    n1 [1,N0/4,3], n2 [1,N0/16,3]], faces int [1,N0,3] (fake nodes = -1 rows), v_faces0 int [1,V,K].  Returns
    (x [1,V,3], [dx of the coarse, the middle and the fine stage, each [V,3]]).  Differentiable with respect to x and
    the three normal fields when one of them requires grad (the adjoint kernels of fgc_vertex_update_ms_bwd; the
    forward keeps its trajectory, 12 bytes per vertex and iteration); the values are the same bits either way.
    tables: the mesh's inverse tables (ops.vertex_ms_tables, as device tensors) for the backward; without them every
    backward copies faces and v_faces to the host and rebuilds them there (a host synchronisation per call) - pass them
    when the same mesh is differentiated repeatedly.  (FacetDenoiser.pointset_step keeps them per bound mesh.)
    depth_dir (build extension; [V,3] or [1,3] viewing rays, utils.view_rays; None: the free update above): every
    iteration's step is projected onto the vertex' ray (include/fgc.h: fgc_vertex_update_ms_dir), a vertex moves along
    its ray only; differentiable in the same arguments, not in the rays.  Rows are used as given: longer than 1 can
    diverge."""
    if coarsening_steps != 2 or len(face_normals_list) != 3:
        raise NotImplementedError("three levels pooled 4:1, as the network has them (settings.py:31-32)")
    xr = x.reshape(-1, 3)
    nv = xr.shape[0]
    d = None if depth_dir is None else ops.ray_rows(depth_dir, nv, xr.device, "depth_dir")
    ns = [t.reshape(-1, 3) for t in face_normals_list]
    faces, vf, it = faces.reshape(-1, 3), v_faces0.reshape(nv, -1), tuple(int(i) for i in iter_num_list)
    if torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in face_normals_list)):
        out, d0, d1, d2 = _UpdatePositionMSFn.apply(xr, *ns, faces, vf, d, it, tables)
        return out.unsqueeze(0), [d0, d1, d2]
    out, dx = ops._ms_forward(xr, ns, faces, vf, it, d)
    return out.unsqueeze(0), [dx[0], dx[1], dx[2]]


def inferNet(inputMesh, net_or_checkpoint, device="cuda", depth_dir=None):
    """train.py:147-376: the multi-scale network (three heads), its three normal fields normalised, update_position_MS
    with [80, 20, 20] iterations - on the whole mesh, or patch by patch when addMeshWithVertices cut it (maxSize).
    inputMesh: InferenceMesh filled by addMeshWithVertices; the network must have been built with multi_scale=True.
    Returns the reference's 9-tuple
    (points, points_mid, points_coarse, fine / mid / coarse normals [F,3] in face order, fine / mid / coarse positions
    [F,3]; as in the reference the three position arrays are the input barycentre channels).
    depth_dir (build extension): [V,3] or [1,3] viewing rays of the WHOLE mesh (utils.view_rays of the raw vertices: the
    vertices divided by the bounding-box diagonal have the same rays) - the update is the ray-constrained one
    (update_position_MS(depth_dir=)), every vertex of the three sets lies on its ray; a patch takes its rows through
    vOldInd_list."""
    if isinstance(net_or_checkpoint, FacetDenoiser):
        net = net_or_checkpoint
    else:
        net = FacetDenoiser(device, multi_scale=True)
        load_checkpoint(net_or_checkpoint, net)
    if not net.multi_scale:
        raise ValueError("inferNet needs a network with the multi-scale heads (multi_scale=True)")
    if not inputMesh.v_list or len(inputMesh.v_list) != len(inputMesh.in_list):
        raise ValueError("inferNet needs a mesh prepared by addMeshWithVertices")
    dev = net.device
    c = lambda t: t.cpu().numpy()
    n_patches = len(inputMesh.in_list)
    rays = None if depth_dir is None else ops.ray_rows(depth_dir, inputMesh.vNum, dev, "depth_dir")
    if n_patches > 1:
        # train.py:255-330: the vertex positions of the patches are averaged over the patches that hold a vertex, the
        # normals of a face are those of the last patch that holds it, and (as in the reference) the three position
        # arrays are the last patch's input barycentre channels, padded and in node order
        vnum, fnum = inputMesh.vNum, inputMesh.fNum
        acc = [torch.zeros(vnum, 3, dtype=torch.float32, device=dev) for _ in range(3)]
        weights = torch.zeros(vnum, 3, dtype=torch.float32, device=dev)
        normals = [torch.zeros(fnum, 3, dtype=torch.float32, device=dev) for _ in range(3)]
        pos = None
        if rays is not None:      # (the input positions, patch by patch)
            x0_all = torch.zeros(vnum, 3, dtype=torch.float32, device=dev)
    for i in range(n_patches):
        x, adjs = inputMesh.in_list[i], inputMesh.adj_list[i]
        net.bind_mesh(x, adjs)
        net.forward(rotate=False)
        B = net.buffers
        n0 = B["nconv"]                                              # normalizeTensor(y0), done by forward()
        n1 = _normalize_rows_like_reference(B["y1"])                 # train.py:192-193
        n2 = _normalize_rows_like_reference(B["y2"])
        xp = torch.as_tensor(inputMesh.v_list[i][0], dtype=torch.float32, device=dev)
        faces = torch.as_tensor(np.asarray(inputMesh.faces_list[i][0]).astype(np.int32), device=dev)
        vf = torch.as_tensor(np.asarray(inputMesh.v_faces_list[i][0]).astype(np.int32), device=dev)
        d = rays
        if rays is not None and len(inputMesh.vOldInd_list[i]) and rays.shape[0] > 1:      # a patch: the rows of its own vertices
            d = rays[torch.as_tensor(np.asarray(inputMesh.vOldInd_list[i]).astype(np.int64), device=dev)]
        pts, dx = ops._ms_forward(xp, [n0, n1, n2], faces, vf, (80, 20, 20), d)
        pts_mid = pts - dx[2]                                        # train.py:249-250
        pts_coarse = pts_mid - dx[1]
        perm = torch.as_tensor(np.asarray(inputMesh.permutations[i]).astype(np.int64), device=dev)
        nf = inputMesh.num_faces[i]
        up1 = n1.repeat_interleave(4, dim=0)                         # custom_upsampling, train.py:222-223
        up2 = n2.repeat_interleave(16, dim=0)
        fine = n0[perm][:nf]
        mid = _normalize_rows_like_reference(up1)[perm][:nf]
        coarse = _normalize_rows_like_reference(up2)[perm][:nf]
        pos_nodes = torch.as_tensor(np.asarray(x)[0, :, 3:].astype(np.float32), device=dev)
        if n_patches == 1:
            pos = pos_nodes[perm][:nf]                               # train.py:288,296-297
            torch.cuda.synchronize()
            return c(pts), c(pts_mid), c(pts_coarse), c(fine), c(mid), c(coarse), c(pos), c(pos), c(pos)
        vold = torch.as_tensor(np.asarray(inputMesh.vOldInd_list[i]).astype(np.int64), device=dev)
        fold = torch.as_tensor(np.asarray(inputMesh.fOldInd_list[i]).astype(np.int64), device=dev)
        if rays is not None:
            # along rays the patches are averaged in the ray's own coordinate, s = d . (p - x0) / d . d, and the vertex is
            # rebuilt from the input position: the mean lies on the ray as every patch's vertex does
            x0_all[vold] = xp
            dd = (d * d).sum(1, keepdim=True)
            for a, p_ in zip(acc, (pts, pts_mid, pts_coarse)):
                a.index_add_(0, vold, (((p_ - xp) * d).sum(1, keepdim=True) / dd).expand(-1, 3).contiguous())
        else:
            for a, p_ in zip(acc, (pts, pts_mid, pts_coarse)):
                a.index_add_(0, vold, p_)
        weights.index_add_(0, vold, torch.ones_like(pts))
        for nrm, v in zip(normals, (fine, mid, coarse)):
            nrm[fold] = v
        pos = pos_nodes
    w = torch.clamp(weights, min=1.0)
    if rays is not None:
        acc = [x0_all + (a / w) * rays for a in acc]
        w = torch.ones_like(w)
    torch.cuda.synchronize()
    return (c(acc[0] / w), c(acc[1] / w), c(acc[2] / w), c(normals[0]), c(normals[1]), c(normals[2]), c(pos), c(pos),
            c(pos))


def _normalize_rows_like_reference(t):
    """utils.normalizeTensor (utils.py:1700-1715) on [n,3] rows through the library's kernels."""
    from .model import normalizeTensor
    return normalizeTensor(t.unsqueeze(0))[0]


def inferNetOld(inputMesh, net_or_checkpoint, device="cuda", update_vertices=False, depth_dir=None):
    """train.py:29-144.  inputMesh: dataClasses.InferenceMesh.  Returns the predicted unit normals [F, 3] (numpy, face
    order); with update_vertices=True the reference's full return value (outPoints [V,3], predicted_normals): the
    vertex positions after 60 iterations of update_position2 on those normals (train.py:129-139).  depth_dir ([V,3] or
    [1,3] viewing rays, utils.view_rays): the 60 iterations are update_position_with_depth's instead, every vertex moves
    along its ray only (the commented call at train.py:131)."""
    if isinstance(net_or_checkpoint, FacetDenoiser):
        net = net_or_checkpoint
    else:
        net = FacetDenoiser(device)
        load_checkpoint(net_or_checkpoint, net)
    n_patches = len(inputMesh.in_list)
    if n_patches == 1:
        net.bind_mesh(inputMesh.in_list[0], inputMesh.adj_list[0])
        out = net.infer_normals(inputMesh.permutations[0], inputMesh.num_faces[0])
    else:
        # train.py:92-126,136: every patch predicts its own faces (context faces included); predictions of faces
        # covered by several patches are summed in the original face order, then normalised
        F = inputMesh.faces.shape[0]
        acc = torch.zeros(F, 3, dtype=torch.float32, device=net.device)
        for i in range(n_patches):
            net.bind_mesh(inputMesh.in_list[i], inputMesh.adj_list[i])
            n_conv = net.forward(rotate=False)
            perm = torch.as_tensor(np.asarray(inputMesh.permutations[i]).astype(np.int64), device=net.device)
            outN = n_conv[perm][:inputMesh.num_faces[i]]
            idx = torch.as_tensor(np.asarray(inputMesh.patch_indices[i]).astype(np.int64), device=net.device)
            acc.index_add_(0, idx, outN)
        out = acc
        for _ in range(2):          # utils.normalize = normalizeOnce twice
            out = out * (1.0 / (out.norm(dim=1, keepdim=True) + 1e-8))
    if update_vertices:
        if getattr(inputMesh, "edge_map", None) is None:
            raise RuntimeError("the mesh has a vertex with more than MAX_EDGES edges: no edge tables, no vertex update")
        dev = out.device
        xp = torch.as_tensor(inputMesh.vertices, dtype=torch.float32, device=dev)
        if depth_dir is not None:
            pts = depth_update(xp.reshape(-1, 3), out, torch.as_tensor(inputMesh.edge_map, device=dev),
                               torch.as_tensor(inputMesh.v_e_map, device=dev), depth_dir, 60)
            torch.cuda.synchronize()
            return pts.cpu().numpy(), out.cpu().numpy()
        pts = update_position2(xp, out.unsqueeze(0), torch.as_tensor(inputMesh.edge_map, device=dev),
                               torch.as_tensor(inputMesh.v_e_map, device=dev), iter_num=60,
                               max_edges=inputMesh.v_e_map.shape[2])
        torch.cuda.synchronize()
        return pts[0].cpu().numpy(), out.cpu().numpy()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def parse_lf_noise(text, n_levels):
    """--lf-noise LEVELS[:WIDTH[:BUMPS]] -> the keywords lf_levels, lf_width, lf_bumps of the trainers; ValueError with
    the reason otherwise."""
    parts = text.split(":")
    if not 1 <= len(parts) <= 3:
        raise ValueError("at most LEVELS:WIDTH:BUMPS")
    out = dict(lf_levels=tuple(float(t) for t in parts[0].split(",")), lf_width=3.0, lf_bumps=None)
    if len(parts) > 1:
        out["lf_width"] = float(parts[1])
    if len(parts) > 2:
        out["lf_bumps"] = int(parts[2])
    lf, _ = _lf_inputs((0.0,) * n_levels, out["lf_levels"], out["lf_width"], out["lf_bumps"])
    out["lf_levels"] = lf
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="Train the network on the pickles of `preprocess` (the reference's train()).")
    ap.add_argument("dump_dir", help="folder of trainingSet.pkl / validSet.pkl (or the ...WithVertices.pkl / ...Clean.pkl / "
                    "...CleanWithVertices.pkl pair)")
    ap.add_argument("network_dir", help="checkpoint folder (created; a checkpoint of --net-name there is resumed)")
    ap.add_argument("--num-iterations", type=int, default=NUM_ITERATIONS)
    ap.add_argument("--net-name", default="net")
    ap.add_argument("--with-vertices", action="store_true",
                    help="the multi-scale network through update_position_MS on the point-set loss (trainAccuracyNet)")
    ap.add_argument("--double-loss", action="store_true",
                    help="with --with-vertices: the point-set loss plus the face-normal loss (trainDoubleLossNet)")
    ap.add_argument("--capture", action="store_true", help="replay every training step from a hipGraph")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--synth-noise", nargs="?", const=",".join(str(l) for l in DEFAULT_NOISE_LEVELS), default=None,
                    metavar="LEVELS", help="build extension: train on the clean pickles of `preprocess --clean` (with "
                    "--with-vertices: of `preprocess --clean --with-vertices`), Gaussian "
                    "vertex noise made on the GPU every step; LEVELS = comma-separated multiples of the mean edge length "
                    "(default %(const)s; the value is optional, so write the option BEHIND the two folders or as --synth-noise=LEVELS)")
    ap.add_argument("--noise-direction", choices=("random", "normal", "ray"), default="random",
                    help="with --synth-noise: displace along a random direction, along the vertex normal, or (ray) along the "
                    "viewing rays of --view-dir / --camera, built from each mesh's clean vertices (depth scans)")
    from .utils import view_options, noise_view_spec
    view_options(ap)
    ap.add_argument("--ray-update", action="store_true",
                    help="with --with-vertices --noise-direction ray: the vertex update of every step moves the vertices along "
                    "the same viewing rays only (what `infer --with-vertices --view-dir / --camera` runs)")
    ap.add_argument("--surface-loss", action="store_true",
                    help="build extension, with --with-vertices: measure to SURFACES in the point loss - the ground-truth mesh "
                    "of `preprocess --gt-surface` (any topology), else the mesh's own faces; with --synth-noise the clean faces")
    ap.add_argument("--lf-noise", default=None, metavar="LEVELS[:WIDTH[:BUMPS]]",
                    help="with --synth-noise: low-frequency noise on top - LEVELS = comma-separated RMS displacements in mean "
                    "edge lengths, one or one per --synth-noise level (level k pairs with lf level k); WIDTH = bump width "
                    "in mean edge lengths (default 3); BUMPS per mesh (default faces / 6).  E.g. --synth-noise 0,0.1,0.2 "
                    "--lf-noise 0.3,0.2,0.1:3")
    ap.add_argument("--sensor", default=None, metavar="POWER[:QUANT]",
                    help="with --synth-noise --noise-direction ray --camera: the noise of a triangulating depth sensor - sigma "
                    "grows with (range / reference range)^POWER, POWER 0, 1 or 2; QUANT (default 0: off) is the depth step at "
                    "the reference range in mean edge lengths, depth quantised in disparity.  The reference range is the "
                    "camera's distance to each mesh's centre.  E.g. --sensor 2:0.5 (nobody has tuned these values)")
    args = ap.parse_args(argv)
    view, sensor = noise_view_spec(ap, args, "--noise-direction", "--lf-noise")
    if view and args.synth_noise is None:
        ap.error("--noise-direction ray needs --synth-noise")
    if args.double_loss and not args.with_vertices:
        ap.error("--double-loss trains on the vertex data: it needs --with-vertices")
    if args.ray_update and not (view and args.with_vertices):
        ap.error("--ray-update constrains the multi-scale vertex update to the noise's rays: it needs --with-vertices and "
                 "--noise-direction ray with --view-dir or --camera")
    if args.surface_loss and not args.with_vertices:
        ap.error("--surface-loss is the point loss of the vertex networks: it needs --with-vertices")
    if args.num_iterations < 0:
        ap.error("--num-iterations must be >= 0")
    levels = None
    if args.synth_noise is not None:
        try:
            levels = tuple(float(t) for t in args.synth_noise.split(","))
        except ValueError:
            ap.error("--synth-noise takes comma-separated numbers, e.g. 0.1,0.2,0.3 (got %r)" % args.synth_noise)
        if not all(np.isfinite(l) and l >= 0 for l in levels):
            ap.error("--synth-noise levels must be >= 0 (got %r)" % args.synth_noise)
    lf_extra = {}
    if args.lf_noise is not None:
        if levels is None:
            ap.error("--lf-noise needs --synth-noise: pass --synth-noise 0 for bumps alone")
        try:
            lf_extra = parse_lf_noise(args.lf_noise, len(levels))
        except ValueError as e:
            ap.error("--lf-noise LEVELS[:WIDTH[:BUMPS]], e.g. 0.3,0.2,0.1:3 - %s (got %r)" % (e, args.lf_noise))
    names = (("trainingSetCleanWithVertices.pkl", "validSetCleanWithVertices.pkl") if args.with_vertices and levels is not None
             else ("trainingSetWithVertices.pkl", "validSetWithVertices.pkl") if args.with_vertices
             else ("trainingSetClean.pkl", "validSetClean.pkl") if levels is not None
             else ("trainingSet.pkl", "validSet.pkl"))
    ts_path, vs_path = (os.path.join(args.dump_dir, n) for n in names)
    if not os.path.isfile(ts_path) and levels is not None:
        ap.error("no clean training set at %s: run `python -m facet_graph_convolution_amd.preprocess CLEAN_DIR %s --clean%s` "
                 "first" % (ts_path, args.dump_dir, " --with-vertices" if args.with_vertices else ""))
    if not os.path.isfile(ts_path):
        ap.error("no training set at %s: run `python -m facet_graph_convolution_amd.preprocess TRAINING_DIR GT_DIR %s%s` "
                 "first" % (ts_path, args.dump_dir, " --with-vertices" if args.with_vertices else ""))
    with open(ts_path, "rb") as fp:
        train_set = pickle.load(fp)
    valid_set = None
    if os.path.isfile(vs_path):
        with open(vs_path, "rb") as fp:
            valid_set = pickle.load(fp)
    os.makedirs(args.network_dir, exist_ok=True)
    trainer = (trainDoubleLossNet if args.double_loss else trainAccuracyNet) if args.with_vertices else trainNet
    extra = dict(noise_levels=levels, noise_direction=view or args.noise_direction, **lf_extra) if levels is not None else {}
    if args.ray_update:
        extra["ray_update"] = True
    if sensor is not None:
        extra["sensor"] = sensor
    if args.surface_loss:
        extra["surface_loss"] = True
    trainer(train_set, args.num_iterations, network_path=args.network_dir, net_name=args.net_name, seed=args.seed,
            capture=args.capture, validSet=valid_set, **extra)
    return trainer.__name__


if __name__ == "__main__":
    main()
