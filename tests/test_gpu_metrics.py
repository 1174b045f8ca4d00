"""GPU checks of the evaluation metrics: fgc_nn_query is exact (float64 brute force on the same fp32 inputs, and
bit-identical to numpy's fp32 arithmetic in the reference's order), deterministic, honours its cell masks;
hausdorffOverSampled and the computeMetrics CLI reproduce the fixtures made by running the reference
(tests/golden/gen/make_golden_metrics.py); mesh_distances is exact.

Bounds: the scan computes the squared distance with the reference's fp32 operations in the reference's order and takes
a correctly rounded square root, so the measured distance to the fixtures is 0; the bounds allow one ulp (2e-7 relative)."""
import builtins
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from facet_graph_convolution_amd import ops, utils

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _gpu_nn(q, p, qc=None, pc=None):
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)  # noqa: E731
    d, i = ops.nn_query(t(q, np.float32), t(p, np.float32), t(qc, np.int32), t(pc, np.int32))
    torch.cuda.synchronize()
    return d.cpu().numpy(), i.cpu().numpy()


def _fp32_brute(q, p, ok=None, rows=512):
    """numpy, fp32, the reference's order: (dx*dx + dy*dy) + dz*dz; first index of the minimum."""
    dist, idx = np.empty(len(q), np.float32), np.empty(len(q), np.int64)
    for s in range(0, len(q), rows):
        d = q[s:s + rows, None, :] - p[None]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        if ok is not None:
            d2 = np.where(ok[s:s + rows], d2, np.float32(np.inf))
        j = np.argmin(d2, 1)
        m = d2[np.arange(len(j)), j]
        dist[s:s + rows] = np.sqrt(m)
        idx[s:s + rows] = np.where(np.isinf(m), -1, j)
    return dist, idx


def _f64_check(q, p, dist, idx, rows=512):
    """Against float64 on the same fp32 inputs: dist is the true minimum to fp32 rounding, idx attains it."""
    q64, p64 = q.astype(np.float64), p.astype(np.float64)
    for s in range(0, len(q), rows):
        d2 = ((q64[s:s + rows, None, :] - p64[None]) ** 2).sum(-1)
        m = d2.min(1)
        tol = 4e-7 * m + 1e-30 + 4e-7 * 1e-14 * (q64[s:s + rows] ** 2).sum(1)
        assert np.all(np.abs(dist[s:s + rows].astype(np.float64) ** 2 - m) <= 2 * tol + 1e-38)
        assert np.all(d2[np.arange(len(m)), idx[s:s + rows]] <= m + 2 * tol + 1e-38)


def _cloud(n, seed, kind="random", offset=0.0):
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    if kind == "coplanar":
        x[:, 2] = 0.25
    elif kind == "collinear":
        t = rs.uniform(-1, 1, size=n).astype(np.float32)
        x = np.stack([t, 2 * t, -t], 1).astype(np.float32)
    elif kind == "duplicates":
        x = x[rs.randint(0, max(1, n // 4), size=n)]
    elif kind == "equal":
        x = np.repeat(x[:1], n, axis=0)
    return (x + np.float32(offset)).astype(np.float32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099, 20000])
@pytest.mark.parametrize("kind", ["random", "duplicates", "coplanar", "collinear"])
def test_nn_query_exact(n, kind):
    p = _cloud(n, 1, kind)
    q = _cloud(max(1, n - 3) if n > 64 else n, 2, "random")
    dist, idx = _gpu_nn(q, p)
    rd, ri = _fp32_brute(q, p)
    assert np.array_equal(idx, ri), "index differs from the first fp32 minimum"
    assert np.array_equal(dist, rd)
    _f64_check(q, p, dist, idx)


@pytest.mark.parametrize("n", [1, 65, 4099])
def test_nn_query_ties_and_self(n):
    # all points equal: every query finds row 0
    p = _cloud(n, 3, "equal")
    d, i = _gpu_nn(_cloud(7, 4), p)
    assert (i == 0).all()
    # queries equal to the points, with duplicates: distance 0 at the FIRST equal row
    p = _cloud(n, 5, "duplicates")
    d, i = _gpu_nn(p, p)
    first = {}
    for j, row in enumerate(map(bytes, p)):
        first.setdefault(row, j)
    assert (d == 0).all()
    assert i.tolist() == [first[bytes(r)] for r in p]


def test_nn_query_offset_coordinates():
    for n in (65, 4099):
        p = _cloud(n, 6, offset=1e4)
        q = _cloud(n + 5, 7, offset=1e4)
        dist, idx = _gpu_nn(q, p)
        rd, ri = _fp32_brute(q, p)
        assert np.array_equal(idx, ri) and np.array_equal(dist, rd)


def test_nn_query_large_against_cdist_and_deterministic():
    n = 200_000
    p = _cloud(n, 8)
    q = _cloud(n, 9)
    d1, i1 = _gpu_nn(q, p)
    d2, i2 = _gpu_nn(q, p)
    assert np.array_equal(d1, d2) and np.array_equal(i1, i2)
    sample = np.random.RandomState(10).choice(n, 4096, replace=False)
    pt = torch.from_numpy(p).to(DEV)
    # (a few rows per call: torch.cdist's direct-difference kernel in the ROCm build of torch returned zeros past the
    #  first 8 rows of a 512 x 200k call)
    for s in range(0, len(sample), 4):
        rows = sample[s:s + 4]
        cd = torch.cdist(torch.from_numpy(q[rows]).to(DEV)[None], pt[None], compute_mode="donot_use_mm_for_euclid_dist")[0]
        m = cd.min(1).values.cpu().numpy()
        assert np.allclose(d1[rows], m, rtol=1e-6, atol=1e-7)
        at = cd[torch.arange(len(rows), device=DEV), torch.from_numpy(i1[rows].astype(np.int64)).to(DEV)].cpu().numpy()
        assert np.all(at <= m * (1 + 1e-6) + 1e-7)
    rd, ri = _fp32_brute(q[sample], p)
    assert np.array_equal(i1[sample], ri) and np.array_equal(d1[sample], rd)


def _unpack(c):
    c = np.asarray(c, np.int64)
    return np.stack([(c >> 20) & 1023, (c >> 10) & 1023, c & 1023], 1)


@pytest.mark.parametrize("nq,np_", [(1, 1), (300, 4099), (5000, 700)])
def test_nn_query_masks(nq, np_):
    rs = np.random.RandomState(nq)
    q, p = _cloud(nq, 11), _cloud(np_, 12)
    qijk = rs.randint(-1, 5, size=(nq, 3))
    pijk = rs.randint(-1, 6, size=(np_, 3))
    qc, pc = ops.pack_cells(qijk), ops.pack_cells(pijk)
    dist, idx = _gpu_nn(q, p, qc, pc)
    qu, pu = _unpack(qc), _unpack(pc)
    diff = pu[None] - qu[:, None]
    ok = ((diff >= 0) & (diff <= 1)).all(-1) & (qc >= 0)[:, None] & (pc >= 0)[None]
    rd, ri = _fp32_brute(q, p, ok)
    assert np.array_equal(idx, ri) and np.array_equal(dist, rd)
    none = ~ok.any(1)
    assert np.isinf(dist[none]).all() and (idx[none] == -1).all()
    if nq > 1:
        assert none.any() and (~none).any()


@pytest.fixture(scope="module")
def haus(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics_hausdorff.npz"))


@pytest.mark.parametrize("case", ["clouds", "ico4", "raise"])
@pytest.mark.parametrize("acc", [1, 0])
def test_hausdorff_over_sampled_matches_reference(haus, case, acc):
    args = [haus["%s_%s" % (case, k)] for k in ("V0", "V1", "sV0", "sV1")]
    tag = "%s_acc%d" % (case, acc)
    raised = str(haus[tag + "_raised"])
    if raised:
        with pytest.raises(getattr(builtins, raised)):
            utils.hausdorffOverSampled(*args, accuracyOnly=bool(acc))
        return
    got = np.array([float(v) for v in utils.hausdorffOverSampled(*args, accuracyOnly=bool(acc))])
    want = haus[tag]
    assert np.all(np.abs(got - want) <= 2e-7 * np.abs(want)), (got, want)


def test_hausdorff_clouds_differs_from_exact(haus):
    """The fixture's reference value is the approximate one: mesh_distances' exact mean is smaller."""
    A, B = haus["clouds_V0"], haus["clouds_V1"]
    d = utils.mesh_distances(A, B)
    assert d["acc_mean"] < haus["clouds_acc1"][2] / 1.001


def test_mesh_distances_exact():
    from facet_graph_convolution_amd.meshgen import icosphere, add_noise
    V, F = icosphere(4)
    A, B = add_noise(V, F, seed=2).astype(np.float32), V.astype(np.float32)
    d = utils.mesh_distances(A, B)
    lo = np.minimum(A.min(0), B.min(0)).astype(np.float64)
    hi = np.maximum(A.max(0), B.max(0)).astype(np.float64)
    a, b = (A - lo) / np.sqrt(((hi - lo) ** 2).sum()), (B - lo) / np.sqrt(((hi - lo) ** 2).sum())

    def one_side(x, y):
        return np.concatenate([np.sqrt(((x[s:s + 512, None] - y[None]) ** 2).sum(-1)).min(1) for s in range(0, len(x), 512)])
    acc, comp = one_side(a, b), one_side(b, a)
    want = {"acc_max": acc.max(), "acc_mean": acc.mean(), "comp_max": comp.max(), "comp_mean": comp.mean(),
            "hausdorff": max(acc.max(), comp.max())}
    for k, v in want.items():
        assert abs(float(d[k]) - v) <= 2e-5 * v, (k, d[k], v)


# ------------------------------------------------------------------------------------------------------------------
# the CLI end to end, in a fresh child process
# ------------------------------------------------------------------------------------------------------------------
def _run_cli(gt, res, *extra):
    r = subprocess.run([sys.executable, "-m", "facet_graph_convolution_amd.computeMetrics", str(gt), str(res), *extra],
                       cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _parse_csv(lines):
    out = {}
    for ln in lines:
        assert ln.endswith(" \n"), repr(ln)
        tok = ln[:-2].split(" ")
        assert len(tok) == 10
        out[tok[0]] = np.array([float(t) for t in tok[1:]])
    return out


def _check_rows(got, want):
    # haus, mean distance: distances; then angles (and the face count)
    tol = np.array([2e-7, 2e-7, 1e-4, 1e-4, 0, 1e-4, 1e-4, 1e-4, 1e-4])
    for name, w in want.items():
        g = got[name]
        assert np.array_equal(np.isnan(g), np.isnan(w)), name
        m = ~np.isnan(w)
        assert np.all(np.abs(g[m] - w[m]) <= tol[m] + 2e-7 * np.abs(w[m])), (name, g, w)


def test_compute_metrics_cli(golden_dir, tmp_path):
    z = np.load(os.path.join(golden_dir, "metrics_cli.npz"))
    gt, res = tmp_path / "gt", tmp_path / "res"
    gt.mkdir()
    res.mkdir()
    for key in z.files:
        if key.startswith("file_"):
            name = key[5:]
            (gt if "_denoised" not in name else res).joinpath(name).write_text(str(z[key]))
    want_lines = [str(s) for s in z["csv_lines"]]
    _run_cli(gt, res)
    got_lines = open(res / "results_heat.csv").read().splitlines(True)
    # the same names (sorted ground truths here, os.listdir order in the reference) and layout
    assert sorted(ln.split(" ")[0] for ln in got_lines) == sorted(ln.split(" ")[0] for ln in want_lines)
    want = _parse_csv(want_lines)
    _check_rows(_parse_csv(got_lines), want)
    exact = open(res / "results_exact.csv").read().splitlines(True)
    assert len(exact) == 6 and all(len(ln.split(" ")) == 7 for ln in exact)
    for name in want:
        base = name[:-len("_denoised.obj")]
        rows = [ln.split() for ln in open(res / (base + "_heatmap.obj"))]
        V = np.array([[float(t) for t in r[1:]] for r in rows if r[0] == "v"])
        F = np.array([[int(t) for t in r[1:]] for r in rows if r[0] == "f"])
        assert np.array_equal(F, z["heat_%s_F" % base])
        assert V.shape == z["heat_%s_V" % base].shape and np.abs(V - z["heat_%s_V" % base]).max() <= 2e-6
    try:
        import scipy.io
    except ImportError:
        scipy = None
    if scipy is not None:
        mat = scipy.io.loadmat(str(res / "angDiffFinal.mat"))
        keys = [k for k in z.files if k.startswith("mat_")]
        assert keys
        for k in keys:
            assert np.abs(mat[k[4:]] - z[k]).max() <= 1e-4
    # a second run skips every file and appends nothing
    before = open(res / "results_heat.csv").read()
    out = _run_cli(gt, res)
    assert out.count("Skipping") == 6 and open(res / "results_heat.csv").read() == before
    # --overwrite scores them again
    _run_cli(gt, res, "--overwrite")
    again = open(res / "results_heat.csv").read().splitlines(True)
    assert len(again) == 12
    _check_rows(_parse_csv(again[6:]), want)
    # a missing _n3 file is skipped with a message
    os.remove(res / "sphere_n3_denoised.obj")
    os.remove(res / "sphere_n3_heatmap.obj")
    out = _run_cli(gt, res)
    assert "sphere_n3_denoised.obj: file not found" in out
    assert open(res / "results_heat.csv").read().splitlines(True) == again
