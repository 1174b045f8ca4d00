"""CPU checks of guided normal filtering (a build extension): the two host tables against brute force on every case mesh,
the ABI, meshgen.cube, and the oracle of tests/guided_cases.py against the quality conditions the GPU test holds the
kernels to (on the same inputs).  No GPU compute here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from facet_graph_convolution_amd import _lib, bilateral, utils
from facet_graph_convolution_amd.meshgen import cube

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bilateral_cases as bc  # noqa: E402
import guided_cases as gc  # noqa: E402


@pytest.mark.parametrize("name", gc.CASES)
def test_tables_against_brute_force(name):
    c = gc.case(name)
    F, ring, fe, n = c["F"].astype(np.int64), c["ring"], c["fe"], c["F"].shape[0]
    assert ring.dtype == np.int32 and fe.dtype == np.int32 and ring.shape == (n, c["ld"]) and fe.shape == (n, 3)
    assert c["ld"] % 4 == 0 and 4 <= c["ld"] <= utils.GUIDED_MAX_RING
    longest = 0
    for f in range(n):
        row = ring[f]
        k = int((row >= 0).sum())
        longest = max(longest, k)
        members = row[:k]
        assert (row[k:] == -1).all() and members[0] == f                   # self in slot 0, -1 padded behind the members
        assert len(set(members.tolist())) == k                            # no repeats
        share = np.nonzero(np.isin(F, F[f]).any(1))[0]                    # brute force: a common vertex
        assert set(members.tolist()) == set(share.tolist())
        for t in range(3):                                                # the face across edge (corner t, corner t + 1)
            a, b = F[f, t], F[f, (t + 1) % 3]
            across = [g for g in np.nonzero((F == a).any(1) & (F == b).any(1))[0] if g != f]
            assert len(across) <= 1
            assert fe[f, t] == (across[0] if across else -1)              # -1 exactly on border edges
            if across:
                assert f in fe[across[0]]                                 # symmetric
    assert c["ld"] == max(4, -(-longest // 4) * 4)
    # the order: the row of getFacesLargeAdj with the repeats dropped
    adj = utils.getFacesLargeAdj(c["F"], utils.GUIDED_MAX_RING) - 1
    for f in range(0, n, max(1, n // 50)):
        seen = []
        for g in adj[f]:
            if g >= 0 and g not in seen:
                seen.append(int(g))
        assert seen == ring[f][ring[f] >= 0].tolist()


def test_the_ring_ceiling_raises():
    V, F = gc.fan(70)
    with pytest.raises(RuntimeError) as e:
        utils.face_rings(F)
    assert str(e.value) == bilateral.NO_EDGE_TABLES
    assert utils.face_rings(gc.fan(60)[1])[1] == 60


def test_cube():
    for n in (1, 4, 12):
        V, F = cube(n)
        assert F.shape == (12 * n * n, 3) and V.shape == (6 * n * n + 2, 3) and V.dtype == np.float32
        e_map, _ = utils.getEdgeMap(F)
        assert e_map.shape[0] == 18 * n * n and (e_map[:, 3] >= 0).all()   # welded and closed: every edge has two faces
        Fn, Fc = utils.computeFacesNormals(V, F), utils.getTrianglesBarycenter(V, F, normalize=False)
        assert ((Fn * Fc).sum(1) > 0).all()                               # outward
        assert np.allclose(np.abs(Fn).max(1), 1) and np.allclose(utils.getTrianglesArea(V, F), 0.5 / (n * n))


def test_abi_115_binds_the_new_entry_points():
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 115 and L.fgc_version() == _lib.ABI_VERSION
    for name in ("fgc_guided_normals", "fgc_guided_workspace_bytes", "fgc_bilateral_filter_guided"):
        assert name in _lib.EXPORTS and hasattr(C.CDLL(_lib.LIB_PATH), name)
    assert L.fgc_guided_workspace_bytes(100, 16) >= 1600
    for n, ld in ((0, 16), (100, 0), (100, 18), (100, 68)):               # ld: a multiple of 4 in 4 .. 64
        assert L.fgc_guided_workspace_bytes(n, ld) == 0
    assert L.fgc_guided_normals(None, None, 4, None, 16, None, None, None, None, None, 0, None) == -22
    assert b"fgc_guided_normals" in L.fgc_last_error()
    assert L.fgc_bilateral_filter_guided(None, None, None, 4, None, None, 1, 1, 1, None, 1, None, 1, None, None, None, 0,
                                         None) == -22
    assert b"fgc_bilateral_filter_guided" in L.fgc_last_error()
    # one workspace size serves the plain and the guided filter: three float4 planes per candidate
    assert L.fgc_bilateral_workspace_bytes(100, 10, 10, 10) >= 100 * 48


def test_oracle_definitions_on_a_hand_made_patch():
    """Two triangles over one edge, normals at 90 degrees: P = both faces, E = the one edge, so Phi = phi = sqrt(2),
    R = 1 (up to the 1e-9), H = sqrt(2), M = the sum of the area-weighted normals; equal H: the first slot, the face itself."""
    N = np.array([[0, 0, 1], [0, 1, 0]], np.float64)
    A = np.array([0.5, 0.25])
    ring = np.array([[0, 1, -1, -1], [1, 0, -1, -1]], np.int32)
    fe = np.array([[1, -1, -1], [-1, 0, -1]], np.int32)
    G, pick, H, M = gc.guidance(N, A, ring, fe)
    assert np.allclose(H, np.sqrt(2)) and np.allclose(M, [[0, 0.25, 0.5], [0, 0.25, 0.5]]) and pick.tolist() == [0, 1]
    assert np.allclose(G, np.array([0, 0.25, 0.5]) / np.sqrt(0.3125))
    # without the edge: E empty, R = 0, H = 0
    assert not gc.guidance(N, A, ring, np.full((2, 3), -1, np.int32))[2].any()


def test_oracle_meets_the_quality_conditions():
    """cube(12), meshgen.add_noise at level 0.3, sigma_s = 1 edge length, sigma_r = 0.35, the window of denoise_mesh (dense
    here): one guided pass <= 0.5 x one bilateral pass, five <= 0.7 x five, mean angular error to the clean normals, both
    filters by their float64 oracles (DESIGN 8c.1 records the numbers)."""
    c, clean = gc.case("cube12"), gc.clean_cube12_normals()
    ng = nb = c["Fn"].astype(np.float64)
    err = {}
    for p in range(1, 6):
        ng = gc.full_pass(c, ng, 1.0, 0.35)[0]
        nb = bc.brute(c["Fc"], nb, c["Fa"], c["el"], 0.35, c["cell"])
        err[p] = (gc.angular_error(ng, clean), gc.angular_error(nb, clean))
        print("oracle pass %d: guided %.3f deg, bilateral %.3f deg, ratio %.3f" % (p, *err[p], err[p][0] / err[p][1]))
    assert err[1][0] <= 0.5 * err[1][1]
    assert err[5][0] <= 0.7 * err[5][1]
