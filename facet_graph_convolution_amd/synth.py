"""Noise synthesis for training from clean meshes (build extension): what a noise setting is, what it
means for one clean mesh, and the one call that enqueues it.

  NoiseSpec    the setting: seed, stream, direction, lf, sensor, ray_update - its refusals (check) and the value two binds
               under one cache key are compared by (key)
  NoisePlan    a spec on one clean mesh (vertices, real faces, mean edge length): the table the white noise goes along, the
               normals and (K, width, area) of the bumps, the sensor words and camera, the scratch size, the control words of
               a level - and which library entry point all that means
  enqueue      the one launch sequence of a plan on device buffers and control words: nothing else, no allocation
  SynthState   the plan with its device buffers, kept with a bound mesh (FacetDenoiser: M["synth"])

FacetDenoiser's steps and makeNoisy.make_noisy both go spec -> plan -> enqueue: the files makeNoisy writes are the meshes a
training run validates on because there is one copy of every rule, not two that agree."""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .utils import areaWeightedVertexNormals, check_directions, direction_key

SpecKey = collections.namedtuple("SpecKey", "seed stream direction lf sensor")
LfPlan = collections.namedtuple("LfPlan", "K width area")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class NoiseSpec(collections.namedtuple("NoiseSpec", "seed stream direction lf sensor ray_update",
                                       defaults=(0, 0, "random", None, None, False))):
    """A noise setting.  seed, stream: the Philox key and stream id (training 0, validation mesh i 1 + i); direction:
    "random", "normal" or a [V,3] array of unit rows; lf = (width_rel, bumps) | None; sensor = (power, r_ref, q, camera)
    (utils.sensor_model) | None; ray_update: the vertex update goes along the same rays (the vertex networks).
    A trainer keeps the per-run part - direction possibly a view, sensor (power, quant) - and fills stream, direction and
    sensor per mesh with _replace."""
    __slots__ = ()

    def lf_key(self):
        if self.lf is None:
            return None
        width_rel, bumps = self.lf
        return (float(width_rel), None if bumps is None else int(bumps))

    def sensor_key(self):
        """The words the kernel reads and the camera in fp32."""
        if self.sensor is None:
            return None
        try:
            power, r_ref, q, camera = self.sensor
        except (TypeError, ValueError):
            raise ValueError("sensor: a model (power, r_ref, q, camera), as utils.sensor_model returns it") from None
        return (tuple(int(w) for w in ops.sensor_words(power, r_ref, q)), tuple(float(t) for t in ops.sensor_camera(camera)))

    def check(self, nv):
        """Every refusal of a setting for a mesh of nv vertices.  Returns the checked table of rays (a float32 copy) or None."""
        rays = None
        if not isinstance(self.direction, str):
            rays = check_directions(self.direction, nv)
        elif self.direction not in ("random", "normal"):
            raise ValueError("direction must be 'random', 'normal' or a [V,3] array of unit rows")
        lf_key, sensor_key = self.lf_key(), self.sensor_key()
        if sensor_key is not None:
            if rays is None:
                raise ValueError("sensor: the model works along viewing rays: direction must be the [V,3] table of rays "
                                 "from its camera")
            if lf_key is not None:
                raise ValueError("sensor: quantisation after bumps along the normals (lf=) is not built; choose one")
        if lf_key is not None and not 0 <= int(self.stream) < 1 << 31:
            raise ValueError("lf: stream must lie below 2^31 (the top bit marks the bump counters)")
        return rays

    def key(self, bound=None):
        """What two binds under one cache key are compared by: SpecKey(seed, stream, direction name or ('rays', digest of the
        rows), lf, sensor).  bound = (spec, key) of an earlier bind: the very same read-only table needs no digest (a training
        loop rebinds its meshes every step)."""
        d = self.direction
        if bound is not None and isinstance(d, np.ndarray) and d is bound[0].direction and not d.flags.writeable:
            dk = bound[1].direction
        else:
            dk = direction_key(d)
        return SpecKey(int(self.seed), int(self.stream), dk, self.lf_key(), self.sensor_key())


class NoisePlan:
    """spec on the clean mesh (verts [V,3], faces: the REAL faces, edge_len: the mean edge length), tables on `device`.
      entry          the library entry point: fgc_synth_noise, fgc_synth_noise_lf (lf) or fgc_synth_noise_sensor (sensor)
      white          the [V,3] table the white noise goes along: the rays if given, else the clean mesh's area-weighted vertex
                     normals if direction is 'normal', else None (a random direction)
      bump_normals   lf: the clean vertex normals - the bumps go along them whatever the white direction
      lf             LfPlan(K, width, area) of ops.lf_plan, or None
      sensor_ctl, camera   the model's four words on the device and its camera as three C floats, or None
      scratch_floats what the entry point asks for (its head: the bounding-box partials in every case)"""

    def __init__(self, spec, verts, faces, edge_len, device):
        vx = np.ascontiguousarray(np.asarray(verts, dtype=np.float32).reshape(-1, 3))
        rays = spec.check(vx.shape[0])
        if not (np.isfinite(edge_len) and edge_len > 0):
            raise ValueError("edge_len must be a positive length")
        lf_key, sensor_key = spec.lf_key(), spec.sensor_key()
        L = _lib.lib()
        self.spec, self.nv, self.edge_len = spec, vx.shape[0], float(edge_len)
        self.white = self.bump_normals = self.lf = self.sensor_ctl = self.camera = None
        self.entry, self.scratch_floats = "fgc_synth_noise", L.fgc_synth_scratch_floats(self.nv)
        normal = rays is None and spec.direction == "normal"
        if normal or lf_key is not None:
            vn = torch.as_tensor(areaWeightedVertexNormals(vx, faces).astype(np.float32), device=device)
            if normal:
                self.white = vn
        if rays is not None:
            self.white = torch.as_tensor(rays, device=device)      # (the kernel reads rows as given)
        if lf_key is not None:
            self.lf = LfPlan(*ops.lf_plan(vx, faces, edge_len, *lf_key))
            self.bump_normals = vn
            self.entry, self.scratch_floats = "fgc_synth_noise_lf", L.fgc_synth_lf_scratch_floats(self.nv, self.lf.K)
        if sensor_key is not None:
            words, cam = sensor_key
            self.sensor_ctl = torch.as_tensor(np.array(words, dtype=np.uint32).view(np.int32), device=device)
            self.camera = (C.c_float * 3)(*cam)
            self.entry = "fgc_synth_noise_sensor"

    def noise_words(self, step, level):
        """The white control words of counter `step` at `level` x the mean edge length (None: off), int32 numpy [3]."""
        sigma = None if level is None else np.float32(level) * np.float32(self.edge_len)
        return ops.noise_words(step, sigma).view(np.int32)

    def lf_words(self, lf_level):
        """The bump control words for a target RMS of lf_level mean edge lengths (None: bumps off), int32 numpy [4]."""
        amp = None if lf_level is None else ops.lf_amplitude(lf_level, self.edge_len, self.lf.width, self.lf.K, self.lf.area)
        return ops.lf_words(amp, self.lf.width).view(np.int32)


def enqueue(plan, v, v_out, scratch, ctl, lf_ctl, stream):
    """The plan's noise launch(es) on `stream`: v [V,3] -> v_out, the bounding-box partials into the head of scratch.  ctl: the
    white control words on the device, lf_ctl: the bump words (a plan with lf).  Enqueues nothing else and allocates nothing:
    safe under capture."""
    L, spec = _lib.lib(), plan.spec
    seed, sid = int(spec.seed) & 0xFFFFFFFFFFFFFFFF, int(spec.stream) & 0xFFFFFFFF
    tail = (seed, sid, _p(v_out), _p(scratch), scratch.numel(), stream)
    if plan.entry == "fgc_synth_noise_lf":
        rc = L.fgc_synth_noise_lf(_p(v), _p(plan.bump_normals), _p(plan.white), plan.nv, _p(ctl), _p(lf_ctl), plan.lf.K, *tail)
    elif plan.entry == "fgc_synth_noise_sensor":
        rc = L.fgc_synth_noise_sensor(_p(v), _p(plan.white), plan.nv, _p(ctl), _p(plan.sensor_ctl), plan.camera, *tail)
    else:
        rc = L.fgc_synth_noise(_p(v), _p(plan.white), plan.nv, _p(ctl), *tail)
    _lib.check(rc, plan.entry)


class SynthState:
    """The synthesis state kept with a bound mesh: the plan of its spec, the key it is compared by, and the device buffers -
    v: the clean vertices, faces: the faces in node order (-1 rows = fake nodes), v_out: the displaced vertices, scratch,
    lf_ctl: the bump words (a plan with lf), gt_box: the clean vertices' box (bind_clean_vertices)."""

    def __init__(self, spec, x, verts, faces_rows, edge_len, device):
        vx = np.ascontiguousarray(np.asarray(verts, dtype=np.float32).reshape(-1, 3))
        fr =np.ascontiguousarray(np.asarray(faces_rows).reshape(-1, 3).astype(np.int32))
        xa = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)
        n0 = xa.size // xa.shape[-1]
        if fr.shape[0] != n0:
            raise ValueError("faces_rows has %d rows, the graph %d nodes" % (fr.shape[0], n0))
        if fr.max() >= vx.shape[0]:
            raise ValueError("faces_rows names vertex %d of %d" % (fr.max(), vx.shape[0]))
        self.plan = NoisePlan(spec, vx, fr[fr[:, 0] >= 0], edge_len, device)
        self.spec, self.key = spec, spec.key()
        self.v, self.faces = torch.as_tensor(vx, device=device), torch.as_tensor(fr, device=device)
        self.v_out = self.v.clone()
        self.lf_ctl = torch.zeros(4, dtype=torch.int32, device=device) if self.plan.lf is not None else None
        self.scratch = torch.zeros(max(self.plan.scratch_floats, 1), dtype=torch.float32, device=device)
        self.gt_box = None

    def same_setting(self, spec, mesh_key):
        """Refuse another setting for the mesh cached under mesh_key."""
        k, b = spec.key(bound=(self.spec, self.key)), self.key
        if (k.seed, k.stream, k.direction) != (b.seed, b.stream, b.direction):
            raise ValueError("mesh %r is bound with another seed / stream / direction" % (mesh_key,))
        if k.lf != self.key.lf:
            raise ValueError("mesh %r is bound with another lf setting (%r)" % (mesh_key, self.key.lf))
        if k.sensor != self.key.sensor:
            raise ValueError("mesh %r is bound with another sensor model (%r)" % (mesh_key, self.key.sensor))
