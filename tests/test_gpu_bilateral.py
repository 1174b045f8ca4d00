"""GPU checks of the bilateral normal filter (fgc_bilateral_filter, utils.bilateralFilter / FND, the bilateral CLI).
Nothing here reads the reference: the yardsticks are the fixtures made by running it
(tests/golden/gen/make_golden_bilateral.py) and a float64 brute force on the package's own host binning, which
tests/test_bilateral_cpu.py pins to the reference's partition.

Bound: the largest absolute difference of a normal component to the FLOAT64 result is at most 8 x dev32, dev32 being
what the reference's own float32 run loses against its float64 run on the same inputs (stored per case).  The kernel
differs from numpy's float32 run in the hardware exp2 with a pre-scaled argument, |c_i - c_j|^2 without the square root
and re-squaring, and the order of the sum; each is worth a few ulps of a weight and the common scale divides out in the
normalisation.  Every test prints the ratio it measured (DESIGN 8c records them)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from facet_graph_convolution_amd import bilateral, ops, utils
from facet_graph_convolution_amd.meshgen import icosphere, add_noise

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bilateral_cases as bc  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 8.0


@pytest.fixture(scope="module")
def fx(golden_dir):
    return bc.load(golden_dir)


def _report(what, err, dev32):
    print("bilateral %-28s max |diff| %.3e  dev32 %.3e  ratio %.2f" % (what, err, dev32, err / dev32 if dev32 else 0.0))


@pytest.mark.parametrize("name", bc.CASES)
def test_filter_matches_the_reference(fx, name):
    z32, z64 = fx
    Fc, Fn, Fa = bc.case_inputs(z32, name)
    ss, sr, dev32 = z32[name + "_sigma_s"], z32[name + "_sigma_r"], float(z32[name + "_dev32"])
    if name == "fnd":
        got = utils.FND(Fc, Fn, Fa, list(ss), list(sr))
    else:
        got = utils.bilateralFilter(Fc, Fn, Fa, float(ss[0]), float(sr[0]))
    want = z64[name + "_out"]
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    err = float(np.abs(got.astype(np.float64) - want).max())
    _report(name, err, dev32)
    if name == "flat":
        assert dev32 == 0 and not got.any()          # a zero-extent axis: every row exactly zero, as the reference
    assert err <= MARGIN * dev32


def test_fnd_equals_the_single_pair_calls(fx):
    """One pass for all pairs, and every pair bit-identical to its single-pair call (the instantiations run the same
    per-pair arithmetic in the same order); so also for more pairs than one launch takes (5 x 4 > 4 x 3)."""
    z32, _ = fx
    Fc, Fn, Fa = bc.case_inputs(z32, "fnd")
    ss, sr = list(z32["fnd_sigma_s"]), list(z32["fnd_sigma_r"])
    got = utils.FND(Fc, Fn, Fa, ss, sr)
    single = np.concatenate([utils.bilateralFilter(Fc, Fn, Fa, s, r) for s in ss for r in sr], axis=-1)
    assert got.shape == (1280, 18)
    _report("fnd vs single-pair calls", float(np.abs(got - single).max()), float(z32["fnd_dev32"]))
    assert np.array_equal(got, single)
    ss5, sr4 = [ss[0] * k for k in (1, 2, 3, 4, 5)], [0.2, -1, 0.5, 0.35]
    got = utils.FND(Fc, Fn, Fa, ss5, sr4)
    single = np.concatenate([utils.bilateralFilter(Fc, Fn, Fa, s, r) for s in ss5 for r in sr4], axis=-1)
    assert got.shape == (1280, 60) and np.array_equal(got, single)


def test_two_calls_are_bit_identical(fx):
    z32, _ = fx
    Fc, Fn, Fa = bc.case_inputs(z32, "ico5")
    ss, sr = float(z32["ico5_sigma_s"][0]), float(z32["ico5_sigma_r"][0])
    a = utils.bilateralFilter(Fc, Fn, Fa, ss, sr)
    b = utils.bilateralFilter(Fc, Fn, Fa, ss, sr)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("slices", [(4, 7, 13), 32, utils.BILATERAL_MAX_SLICES], ids=str)
def test_other_grids_against_brute_force(fx, slices):
    z32, _ = fx
    dev32 = float(z32["ico5_dev32"])
    V, F = bc.noisy_mesh("ico4")
    Fc, Fn, Fa = bc.mesh_inputs(V, F)
    ss, sr = float(utils.getAverageEdgeLength(V, F)[0]), 0.35
    got = utils.bilateralFilter(Fc, Fn, Fa, ss, sr, slices=slices)
    want = bc.brute(Fc, Fn, Fa, ss, sr, utils.bilateral_cells(Fc, slices))
    err = float(np.abs(got - want).max())
    _report("ico4 slices %s" % (slices,), err, dev32)
    assert err <= MARGIN * dev32


def _edge_case(fx, what, Fc, Fn, Fa, ss, sr, slices, rows=None):
    z32, _ = fx
    dev32 = float(z32["ico5_dev32"])
    got = utils.bilateralFilter(Fc, Fn, Fa, ss, sr, slices=slices)
    assert got.shape == (Fc.shape[0], 3) and np.isfinite(got).all()
    want = bc.brute(Fc, Fn, Fa, ss, sr, utils.bilateral_cells(Fc, slices), rows)
    err = float(np.abs((got if rows is None else got[rows]) - want).max())
    _report(what, err, dev32)
    assert err <= MARGIN * dev32
    return got


def test_edge_shapes(fx):
    # one face: zero extent on every axis, the reference's partition takes it nowhere
    one = utils.bilateralFilter(np.array([[0.5, 0.25, 1.0]], np.float32), np.array([[0, 0, 1]], np.float32),
                                np.array([0.5], np.float32), 0.1, 0.35)
    assert one.shape == (1, 3) and not one.any()
    # ... and through the op with one cell that holds it: its own normal
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda:0")  # noqa: E731
    out = ops.bilateral_filter(t([[0.5, 0.25, 1.0]], np.float32), t([[0, 0.6, 0.8]], np.float32), t([0.5], np.float32), 0.1,
                               0.35, t([0], np.int32), t([0, 1], np.int32), (1, 1, 1)).cpu().numpy()
    assert np.abs(out - np.array([[0, 0.6, 0.8]])).max() <= 2e-7
    # 20 faces, all in one cell
    V, F = icosphere(0)
    Fc, Fn, Fa = bc.mesh_inputs(V, F)
    _edge_case(fx, "20 faces, one cell", Fc, Fn, Fa, 0.8, 0.9, 1)
    # 70 000 random faces in ONE cell: 1 094 query chunks over one candidate range
    rs = np.random.RandomState(5)
    n = 70000
    Fc = rs.uniform(size=(n, 3)).astype(np.float32)
    Fn = utils.normalize(rs.normal(size=(n, 3))).astype(np.float32)
    Fa = rs.uniform(0.5, 1.5, size=n).astype(np.float32)
    rows = np.sort(rs.choice(n, size=512, replace=False))
    _edge_case(fx, "70000 random faces, one cell", Fc, Fn, Fa, 0.05, 0.35, 1, rows)
    # faces of zero area contribute nothing and are still filtered; rows with a zero normal (fake rows) stay finite
    V, F = bc.noisy_mesh("ico4")
    Fc, Fn, Fa = bc.mesh_inputs(V, F)
    ss = float(utils.getAverageEdgeLength(V, F)[0])
    Fa0 = Fa.copy()
    Fa0[::3] = 0
    got = _edge_case(fx, "zero areas", Fc, Fn, Fa0, ss, 0.35, 10)
    assert (np.abs(np.linalg.norm(got[::3], axis=1) - 1) < 1e-5).all()
    Fn0 = Fn.copy()
    Fn0[::5] = 0
    _edge_case(fx, "zero normals", Fc, Fn0, Fa, ss, 0.35, 10)
    # every area zero: zero sums stay zero, never NaN
    zero = utils.bilateralFilter(Fc, Fn, np.zeros_like(Fa), ss, 0.35)
    assert not zero.any()


def test_100k_faces_against_the_reference(fx):
    z32, z64 = fx
    Fc, Fn, Fa = bc.case_inputs(z32, "torus100k")
    assert Fc.shape[0] == 100000
    rows, dev32 = z32["torus100k_rows"], float(z32["torus100k_dev32"])
    assert np.array_equal(rows, z64["torus100k_rows"])
    got = utils.bilateralFilter(Fc, Fn, Fa, float(z32["torus100k_sigma_s"][0]), float(z32["torus100k_sigma_r"][0]))
    err = float(np.abs(got[rows].astype(np.float64) - z64["torus100k_out_rows"]).max())
    _report("torus100k (512 rows)", err, dev32)
    assert np.isfinite(got).all() and err <= MARGIN * dev32


@pytest.mark.parametrize("slices", ["auto", 10])
def test_denoise_mesh(slices):
    V, F = icosphere(4)
    F = F.astype(np.int32)
    Vn = add_noise(V, F, sigma_rel=0.2, seed=3).astype(np.float32)
    clean = utils.computeFacesNormals(V, F)
    noisy_err = utils.angularDiff(utils.computeFacesNormals(Vn, F), clean)[0]
    V_out, normals = bilateral.denoise_mesh(Vn, F, iterations=5, sigma_s=1.0, sigma_r=0.35, slices=slices)
    assert V_out.shape == V.shape and V_out.dtype == np.float32 and normals.shape == (F.shape[0], 3)
    n_err = utils.angularDiff(normals, clean)[0]
    v_err = utils.angularDiff(utils.computeFacesNormals(V_out, F), clean)[0]
    print("denoise_mesh slices %s: noisy %.2f deg, filtered normals %.2f deg, normals of the moved vertices %.2f deg"
          % (slices, noisy_err, n_err, v_err))
    assert n_err < noisy_err / 4
    assert v_err < noisy_err / 2


def _run_cli(module, *args):
    r = subprocess.run([sys.executable, "-m", "facet_graph_convolution_amd." + module, *[str(a) for a in args]],
                       cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_cli_end_to_end(tmp_path):
    gt, noisy, res = tmp_path / "gt", tmp_path / "noisy", tmp_path / "res"
    gt.mkdir()
    noisy.mkdir()
    for name, (V, F), seed in (("sphere", icosphere(3), 1), ("ball", icosphere(2), 2)):
        utils.write_mesh(V, F, str(gt / (name + ".obj")))
        utils.write_mesh(add_noise(V, F, sigma_rel=0.2, seed=seed), F, str(noisy / (name + "_n1.obj")))
    names = sorted(os.listdir(noisy))
    _run_cli("bilateral", noisy, res, "--iterations", "3")
    for f in names:
        Vd, _, _, Fd, _ = utils.load_mesh(str(res), f[:-4] + "_denoised.obj", 0, False)
        Vi, _, _, Fi, _ = utils.load_mesh(str(noisy), f, 0, False)
        assert Vd.shape == Vi.shape and np.array_equal(np.asarray(Fd), np.asarray(Fi)) and np.isfinite(Vd).all()
    assert sorted(os.listdir(res)) == sorted(f[:-4] + "_denoised.obj" for f in names)
    stamps = {f: os.stat(res / f).st_mtime_ns for f in os.listdir(res)}
    out = _run_cli("bilateral", noisy, res, "--iterations", "3")
    assert out.count("Skipping") == 2 and stamps == {f: os.stat(res / f).st_mtime_ns for f in os.listdir(res)}
    _run_cli("bilateral", noisy, res, "--iterations", "3", "--slices", "10", "--overwrite")
    assert all(os.stat(res / f).st_mtime_ns > t for f, t in stamps.items())
    # the results folder scores like a network's: one line per denoised file (the _n2 / _n3 files are not there)
    _run_cli("computeMetrics", gt, res)
    lines = open(res / "results_heat.csv").read().splitlines()
    assert sorted(ln.split(" ")[0] for ln in lines) == sorted(f[:-4] + "_denoised.obj" for f in names)
