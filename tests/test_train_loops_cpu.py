"""The three training loops against a recording stub of FacetDenoiser, without a GPU: the sequence of bind / set / step /
loss calls of a run - sample arrays, rotations, (noise counter, level) pairs, validation streams and step ids - must be the
one rebuilt here from np.random.RandomState(seed + 1) in the documented order of draws: mesh index; samples (COST_SAMPLES
rows of N0, or POINT_SAMPLES of V, then POINT_SAMPLES of Vgt); three uniforms for the rotation; in synthesis mode only the
noise-level index; then - before the training step - the validation draws, one sample set per validation mesh (plain) or
per mesh and level (synthesis, stream 1 + mesh index, step = level index)."""
import types

import numpy as np
import pytest
import torch

from facet_graph_convolution_amd import train as T
from facet_graph_convolution_amd.net import COST_SAMPLES, POINT_SAMPLES, FacetDenoiser
from facet_graph_convolution_amd.utils import rand_rotation_matrix

SEED = 5
LEVELS = (0.1, 0.3)
RESULT = {"train_step": 2, "eval_loss": 2, "pointset_step": 1, "pointset_loss": 1, "double_loss_step": 3, "double_loss": 3}
N0 = (64, 128, 32)              # input rows of the two training meshes and of the validation mesh
NV = (30, 50, 20)               # their vertices ...
NVGT = (25, 45, 15)             # ... and ground-truth vertices (plain mode; a clean mesh is its own ground truth)


def _frozen(v):
    """A call argument as something == compares: arrays by dtype, shape and bytes."""
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.shape, v.tobytes())
    if isinstance(v, (tuple, list)):
        return tuple(_frozen(t) for t in v)
    return v


STEP_ARGS = {"train_step": ("sample_ind", "R"), "pointset_step": ("sample_ind0", "sample_ind1", "R"),
             "double_loss_step": ("sample_ind0", "sample_ind1", "R")}


class StubNet:
    """Logs (method, frozen arguments, frozen keywords) - a step's leading arguments as positional ones however they were
    passed; a bind logs (method, key, number of mesh arguments, keywords) with gt_normals as a flag.  trainer_form is the
    network's own: the loops reach the logging methods through the real table of forms."""
    made = []
    _STEP_FORMS, _TrainerForm, trainer_form = FacetDenoiser._STEP_FORMS, FacetDenoiser._TrainerForm, FacetDenoiser.trainer_form

    def __init__(self, device, multi_scale=False, seed=0):
        self.device, self.multi_scale, self.calls = "cpu", multi_scale, []
        StubNet.made.append(self)

    def __getattr__(self, name):
        if name.startswith("bind"):
            def bind(key, *args, **kw):
                if kw.pop("gt_normals", None) is not None:
                    kw["gt_normals"] = True
                self.calls.append((name, key, len(args) + (kw.pop("gt", None) is not None), _frozen(sorted(kw.items()))))
            return bind
        if name.startswith("set_") or name in RESULT:
            def call(*args, **kw):
                args += tuple(kw.pop(k) for k in STEP_ARGS.get(name, ())[len(args):])
                self.calls.append((name, _frozen(args), _frozen(sorted(kw.items()))))
                if name in RESULT:
                    return torch.arange(1, 1 + RESULT[name], dtype=torch.float32)
            return call
        raise AttributeError(name)


def _set(indices, clean, vertices):
    """A TrainingSet's lists, as far as the trainers read them, with recognisable sizes."""
    ds = types.SimpleNamespace(in_list=[np.zeros((1, N0[i], 6)) for i in indices], adj_list=[None for _ in indices],
                               gt_list=[np.ones((1, N0[i], 3)) for i in indices])
    if vertices:
        ds.v_list = [np.zeros((1, NV[i], 3)) for i in indices]
        ds.faces_list = ds.v_faces_list = [None for _ in indices]
        ds.gtv_list = [np.zeros((1, NVGT[i], 3)) for i in indices]
    if clean:
        ds.is_clean = lambda: True
        ds.clean_vertices = [np.zeros((1, NV[i], 3)) for i in indices]
        ds.clean_faces_rows = [None for _ in indices]
        ds.clean_edge_len = [1.0 for _ in indices]
        ds.v_faces_list = [None for _ in indices]
    return ds


# per trainer: (function, bind, clean bind, arguments behind the key: plain / clean, set samples, step, loss, cadence of the
# validation, whether the plain mode skips iteration 0, whether the training mesh is bound every iteration)
TRAINERS = {
    "trainNet": ("bind_cached", "bind_clean", 3, 6, "set_samples", "train_step", "eval_loss", 100, False, False),
    "trainAccuracyNet": ("bind_vertices", "bind_clean_vertices", 6, 6, "set_point_samples", "pointset_step", "pointset_loss",
                         20, True, True),
    "trainDoubleLossNet": ("bind_vertices", "bind_clean_vertices", 6, 6, "set_point_samples", "double_loss_step",
                           "double_loss", 20, True, True),
}


def _expected(trainer, iterations, synth, direction, start=0):
    bind_plain, bind_clean, nargs_plain, nargs_clean, set_samples, step, loss, every, skip0, bind_always = TRAINERS[trainer]
    vertices, double = trainer != "trainNet", trainer == "trainDoubleLossNet"
    rs = np.random.RandomState(SEED + 1)
    calls = []

    def bind(key, stream):
        kw = {"gt_normals": True} if double else {}
        if synth:
            kw.update(seed=SEED, stream=stream, direction=direction)
        calls.append((bind_clean if synth else bind_plain, key, nargs_clean if synth else nargs_plain, _frozen(sorted(kw.items()))))

    def samples(i):
        if not vertices:
            return (rs.randint(N0[i], size=COST_SAMPLES),)
        return (rs.randint(NV[i], size=POINT_SAMPLES), rs.randint(NV[i] if synth else NVGT[i], size=POINT_SAMPLES))

    bound = -1
    for it in range(iterations):
        b = rs.randint(2)
        if b != bound and not bind_always:
            bind(b, 0)
            bound = b
        samp = samples(b)
        R = rand_rotation_matrix(randnums=rs.uniform(size=3))
        noise = (start + it, LEVELS[rs.randint(len(LEVELS))]) if synth else None
        if it % every == 0 and (it > 0 or synth or not skip0):
            bind(("valid", 0), 1)
            for k, level in enumerate(LEVELS if synth else (None,)):
                calls.append((set_samples, _frozen(samples(2)), ()))
                calls.append(("set_rotation", _frozen((R,)), ()))
                if synth:
                    calls.append(("set_noise", (k, level), ()))
                calls.append((loss, (), _frozen([("rotate", True)])))
            if not bind_always:
                bind(b, 0)
        if bind_always:
            bind(b, 0)
        calls.append((step, _frozen(samp + (R,)), _frozen([("capture", False), ("noise", noise)])))
    return calls


@pytest.mark.parametrize("synth,direction", [(False, "random"), (True, "random"), (True, "normal")])
@pytest.mark.parametrize("trainer,iterations", [("trainNet", 3), ("trainAccuracyNet", 3), ("trainDoubleLossNet", 3),
                                                ("trainAccuracyNet", 21), ("trainDoubleLossNet", 21)])
def test_a_run_calls_the_network_in_the_documented_order(monkeypatch, trainer, iterations, synth, direction):
    monkeypatch.setattr(T, "FacetDenoiser", StubNet)
    StubNet.made.clear()
    vertices = trainer != "trainNet"
    lines = []
    extra = dict(noise_levels=LEVELS, noise_direction=direction) if synth else {}
    out = getattr(T, trainer)(_set((0, 1), synth, vertices), iterations, seed=SEED, log=lines.append,
                              validSet=_set((2,), synth, vertices), **extra)
    net, = StubNet.made
    assert out[0] is net and net.multi_scale == vertices
    want = _expected(trainer, iterations, synth, direction)
    assert len(net.calls) == len(want), (len(net.calls), len(want))
    for k, (got, exp) in enumerate(zip(net.calls, want)):
        assert got == exp, (k, got[0], exp[0])
    names = {c[0] for c in net.calls}
    if not synth:
        assert "set_noise" not in names and not [n for n in names if n.startswith("bind_clean")]
    else:
        assert {c[1] for c in net.calls if c[0] == "set_noise"} == set(enumerate(LEVELS))
    # every validation pass logs one line; the vertex trainers' plain mode skips iteration 0, the synthesis mode does not
    passes = sum(1 for c in want if c[1] == ("valid", 0))
    assert sum("validation loss" in s for s in lines) == passes
    assert passes == (2 if iterations == 21 and synth else 0 if vertices and not synth and iterations == 3 else 1)
    if trainer == "trainDoubleLossNet" and passes:
        assert "validation loss = 1 (points 2, normals 3)" in "".join(lines)
    if vertices:
        assert out[2].shape == ((iterations, 3) if trainer == "trainDoubleLossNet" else (iterations,))
        assert (out[2].reshape(iterations, -1) == np.arange(1, 1 + RESULT[TRAINERS[trainer][5]])).all()


def test_noise_arguments_are_checked_once_for_every_trainer(monkeypatch):
    monkeypatch.setattr(T, "FacetDenoiser", StubNet)
    for trainer in TRAINERS:
        ds = _set((0, 1), True, trainer != "trainNet")
        for bad in ((), (0.1, -1.0), (float("nan"),)):
            with pytest.raises(ValueError, match="noise_levels: a non-empty list of levels >= 0"):
                getattr(T, trainer)(ds, 1, noise_levels=bad)
        with pytest.raises(ValueError, match="noise_direction must be 'random' or 'normal'"):
            getattr(T, trainer)(ds, 1, noise_levels=LEVELS, noise_direction="sideways")
        with pytest.raises(ValueError, match="noise_levels needs a training set of clean meshes"):
            getattr(T, trainer)(_set((0, 1), False, trainer != "trainNet"), 1, noise_levels=LEVELS)


@pytest.mark.parametrize("trainer", sorted(TRAINERS))
def test_the_noise_counter_goes_on_from_the_restored_iteration(monkeypatch, tmp_path, trainer):
    """Noise counter = start + it, start being what _resume restored from the network folder - in all three trainers."""
    resumed, saved = [], []
    monkeypatch.setattr(T, "FacetDenoiser", StubNet)
    monkeypatch.setattr(T, "_resume", lambda net, path, name: resumed.append((net, path, name)) or 1000)
    monkeypatch.setattr(T, "save_checkpoint", lambda path, net, iteration: saved.append((path, iteration)))
    StubNet.made.clear()
    vertices = trainer != "trainNet"
    getattr(T, trainer)(_set((0, 1), True, vertices), 3, network_path=str(tmp_path), net_name="n", seed=SEED,
                        log=lambda s: None, validSet=_set((2,), True, vertices), noise_levels=LEVELS)
    net, = StubNet.made
    assert resumed == [(net, str(tmp_path), "n")] and saved == [(str(tmp_path / "n"), 1003)]
    assert net.calls == _expected(trainer, 3, True, "random", start=1000)
    steps = [dict(c[2])["noise"][0] for c in net.calls if c[0] == TRAINERS[trainer][5]]
    assert steps == [1000, 1001, 1002]
