"""CPU checks of the bilateral filter's host side: the binning reproduces the reference's partition (cell populations
and window sizes the reference printed, tests/golden/bilateral.npz), the ordering tables are well formed, the small
geometry helpers match the reference, and the boundaries (C ABI, ops, CLI) refuse bad arguments before any launch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from facet_graph_convolution_amd import _lib, utils

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bilateral_cases as bc  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden_dir):
    return bc.load(golden_dir)


@pytest.mark.parametrize("name", bc.CASES + ("torus100k",))
def test_host_binning_is_the_references_partition(fx, name):
    z32, _ = fx
    Fc, _, _ = bc.case_inputs(z32, name)
    cell = utils.bilateral_cells(Fc)                     # the default grid: 10 x 10 x 10
    pop, win = bc.occupancy(cell, (10, 10, 10))
    assert np.array_equal(pop, z32[name + "_pop"]) and np.array_equal(win, z32[name + "_win"])
    if name == "flat":
        assert (cell[:, 2] == -1).all() and len(pop) == 0          # zero extent: every face in no cell
        one = utils.bilateral_cells(Fc, 10, flat_axis_one_cell=True)
        assert (one[:, 2] == 0).all() and (one[:, :2] >= 0).all()
    else:
        assert pop.sum() == Fc.shape[0]                            # the 1.01 margin takes every face in


def test_order_is_a_permutation_and_the_table_covers_it(fx):
    z32, _ = fx
    Fc, _, _ = bc.case_inputs(z32, "torus2400")
    for slices in (10, (4, 7, 13), 1, utils.BILATERAL_MAX_SLICES):
        grid = utils.bilateral_grid(slices)
        cell = utils.bilateral_cells(Fc, slices)
        assert cell.min() >= 0 and (cell.max(0) < np.array(grid)).all() and (cell.max(0) == np.array(grid) - 1).all()
        order, ptr = utils.bilateral_order(cell, slices)
        assert order.dtype == np.int32 and ptr.dtype == np.int32 and ptr.shape == (grid[0] * grid[1] * grid[2] + 1,)
        assert np.array_equal(np.sort(order), np.arange(Fc.shape[0]))
        assert ptr[0] == 0 and ptr[-1] == Fc.shape[0] and (np.diff(ptr) >= 0).all()
        flat = (cell[:, 0] * grid[1] + cell[:, 1]) * grid[2] + cell[:, 2]
        for c in np.unique(flat)[:50]:
            members = order[ptr[c]:ptr[c + 1]]
            assert (flat[members] == c).all() and (np.diff(members) > 0).all()      # stable: face order inside a cell
    # a 3-tuple bins per axis with the same rule as the int
    c3 = utils.bilateral_cells(Fc, (4, 7, 13))
    for axis, s in enumerate((4, 7, 13)):
        assert np.array_equal(c3[:, axis], utils.bilateral_cells(Fc, s)[:, axis])
    # faces in no cell come last and are in no range
    cell = utils.bilateral_cells(Fc, 10)
    cell[5] = -1
    cell[77, 1] = -1
    order, ptr = utils.bilateral_order(cell, 10)
    assert ptr[-1] == Fc.shape[0] - 2 and sorted(order[-2:]) == [5, 77]
    for bad in (utils.BILATERAL_MAX_SLICES + 1, 0, (10, 10), (10, 0, 10), (10, 10, utils.BILATERAL_MAX_SLICES + 1), "auto"):
        with pytest.raises(ValueError):
            utils.bilateral_grid(bad)
    with pytest.raises(ValueError):
        utils.bilateral_cells(Fc, 65)
    assert utils.BILATERAL_MAX_SLICES >= 64


@pytest.mark.parametrize("name", ["ico3", "open"])
def test_area_edge_length_and_centres_match_the_reference(fx, name):
    z32, _ = fx
    V, F = z32["mesh_%s_V" % name], z32["mesh_%s_F" % name]
    rel = lambda got, want: np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max()  # noqa: E731
    area = utils.getTrianglesArea(V, F)
    assert area.dtype == np.float64 and area.shape == (F.shape[0],)
    assert rel(area, z32["mesh_%s_area" % name]) <= 1e-6
    assert rel(utils.getTrianglesArea(V, F, normalize=True), z32["mesh_%s_area_norm" % name]) <= 1e-6
    el, ne, eln = z32["mesh_%s_edge" % name]
    got_el, got_ne = utils.getAverageEdgeLength(V, F)
    assert got_ne == int(ne) == 3 * F.shape[0] and abs(got_el - el) <= 1e-6 * el
    assert abs(utils.getAverageEdgeLength(V, F, normalize=True)[0] - eln) <= 1e-6 * eln
    centres = utils.getTrianglesBarycenter(V, F, normalize=False)
    assert centres.dtype == np.float64 and rel(centres, z32["mesh_%s_centres" % name]) <= 1e-6


def test_abi_refuses_bad_arguments():
    L = _lib.lib()
    assert L.fgc_bilateral_filter(None, None, None, 4, None, None, 10, 10, 10, None, 1, None, 1, None, None, 0, None) == -22
    assert b"fgc_bilateral_filter" in L.fgc_last_error()
    need = L.fgc_bilateral_workspace_bytes(100, 10, 10, 10)
    assert need >= 100 * 32 and L.fgc_bilateral_workspace_bytes(100, 10, 10, 65) == 0
    a = C.c_void_p(4096)                     # never dereferenced: every call below is refused before any launch
    ss, sr = (C.c_float * 1)(0.1), (C.c_float * 1)(0.35)
    ok = dict(n=100, grid=(10, 10, 10), ss=ss, S=1, sr=sr, R=1, ws=a, nbytes=need)

    def call(**kw):
        p = dict(ok, **kw)
        return L.fgc_bilateral_filter(a, a, a, p["n"], a, a, *p["grid"], p["ss"], p["S"], p["sr"], p["R"], a, p["ws"],
                                      p["nbytes"], None)
    for kw in (dict(n=0), dict(S=0), dict(R=0), dict(grid=(0, 10, 10)), dict(grid=(10, 10, 65)),
               dict(ss=(C.c_float * 1)(0.0)), dict(ss=(C.c_float * 1)(-1.0)), dict(sr=(C.c_float * 1)(0.0)),
               dict(sr=(C.c_float * 1)(-2.0)), dict(nbytes=need - 1), dict(ws=C.c_void_p(4100))):
        assert call(**kw) == -22, kw
        assert b"fgc_bilateral_filter" in L.fgc_last_error()
    with pytest.raises(RuntimeError, match="fgc_bilateral_filter"):
        _lib.check(call(n=0), "fgc_bilateral_filter")


def test_op_refuses_cpu_tensors():
    import torch
    from facet_graph_convolution_amd import ops
    x = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bilateral_filter(x, x, torch.ones(4), 0.1, 0.35, torch.arange(4, dtype=torch.int32),
                             torch.tensor([0, 4], dtype=torch.int32), (1, 1, 1))


@pytest.mark.parametrize("args", [["--sigma-s", "0"], ["--slices", "0"], ["--slices", "65"], ["--slices", "3,3"],
                                  ["--sigma-r", "0"], ["--iterations", "-1"]])
def test_cli_argument_errors(tmp_path, args):
    r = subprocess.run([sys.executable, "-m", "facet_graph_convolution_amd.bilateral", str(tmp_path), str(tmp_path / "res"),
                        *args], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "usage:" in r.stderr and args[0] in r.stderr
    assert not (tmp_path / "res").exists()


def test_a_vertex_with_too_many_edges_is_reported_and_skipped(tmp_path):
    """The vertex update needs the edge tables (MAX_EDGES = 20 edges per vertex): denoise_mesh raises with the message
    inferNetOld uses, before any GPU work; the CLI's per-file step reports the mesh and goes on."""
    from facet_graph_convolution_amd import bilateral
    k = 24
    ang = 2 * np.pi * np.arange(k) / k
    V = np.concatenate([[[0, 0, 0.3]], np.stack([np.cos(ang), np.sin(ang), np.zeros(k)], 1)]).astype(np.float32)
    F = np.stack([np.zeros(k, dtype=np.int64), 1 + np.arange(k), 1 + (np.arange(k) + 1) % k], 1).astype(np.int32)
    with pytest.raises(RuntimeError, match="more than MAX_EDGES edges"):
        bilateral.denoise_mesh(V, F)
    utils.write_mesh(V, F, str(tmp_path / "fan.obj"))
    said = []
    assert bilateral.denoise_file(str(tmp_path), "fan.obj", str(tmp_path), log=said.append) is None
    assert len(said) == 1 and said[0].startswith("Skipping fan.obj") and "MAX_EDGES" in said[0]
    assert not (tmp_path / "fan_denoised.obj").exists()
