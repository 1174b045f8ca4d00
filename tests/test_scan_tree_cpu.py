"""CPU checks of the ray cast through a bounding-box tree: the three entry points are exported, declared and bound under ABI
116, fgc_ray_tree_bytes, the argument checks of fgc_ray_tree_build and fgc_ray_cast_tree (before any launch), the scenes of
tests/scan_tree_cases.py are the ones the GPU tests were sized for, the default order of the faces (host code on CPU
tensors), and the refusals of the host layers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from facet_graph_convolution_amd import _lib, ops, utils

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_cases as sc  # noqa: E402
import scan_tree_cases as tc  # noqa: E402

NAMES = ("fgc_ray_tree_bytes", "fgc_ray_tree_build", "fgc_ray_cast_tree")
MAX_FACES = 1 << 30


def test_the_three_entry_points_are_exported_declared_and_bound():
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fgc.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None
        assert ("%s(" % name) in header
    # new entry points only: the number has not moved, and the header lists them under it
    assert L.fgc_version() == 116 and "#define FGC_ABI_VERSION 116" in header
    added = header[header.index("Added under 116"):header.index("#define FGC_ABI_VERSION")]
    assert "fgc_ray_tree_bytes / fgc_ray_tree_build / fgc_ray_cast_tree" in added


def test_tree_bytes():
    L = _lib.lib()
    for nf in (0, -1, -2 ** 31, MAX_FACES + 1, 2 ** 31 - 1):
        assert L.fgc_ray_tree_bytes(nf) == 0, nf
    sizes = [L.fgc_ray_tree_bytes(nf) for nf in range(1, 700)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes)
    # one chunk of records (4 x 48 bytes), its four face ids and one node of 48 dwords
    assert sizes[0] == sizes[3] == 4 * 48 + 4 * 4 + 192 and sizes[4] > sizes[3]
    # 5 120 faces: 1 280 leaves under 160 + 20 + 3 + 1 nodes - a tree of five levels
    assert L.fgc_ray_tree_bytes(5120) == 5120 * 52 + (160 + 20 + 3 + 1) * 192
    big = [L.fgc_ray_tree_bytes(nf) for nf in (10 ** 5, 10 ** 6, MAX_FACES - 1, MAX_FACES)]
    assert all(a <= b for a, b in zip(big, big[1:])) and big[-1] > MAX_FACES * 52


def test_argument_checks_answer_einval_before_any_launch():
    """Every call below must return FGC_EINVAL from the host checks: the pointers are made-up addresses nobody may touch."""
    L = _lib.lib()
    nv, nf, nq = 100, 196, 77
    need = L.fgc_ray_tree_bytes(nf)
    P = lambda k: C.c_void_p(0x10000 * (k + 1))  # noqa: E731

    good = dict(verts=P(0), nv=nv, faces=P(1), nf=nf, order=P(2), tree=P(3), tree_bytes=need, stream=None)

    def build(**kw):
        a = dict(good, **kw)
        return L.fgc_ray_tree_build(a["verts"], a["nv"], a["faces"], a["nf"], a["order"], a["tree"], a["tree_bytes"], a["stream"])
    for name in ("verts", "faces", "order", "tree"):
        assert build(**{name: None}) == -22, name
        assert b"fgc_ray_tree_build" in L.fgc_last_error()
    for name in ("nv", "nf"):
        assert build(**{name: 0}) == -22 and build(**{name: -5}) == -22, name
    assert build(nf=2 ** 31 - 1) == -22 and build(nf=MAX_FACES + 1) == -22
    assert build(tree_bytes=need - 1) == -22 and b"too small" in L.fgc_last_error()
    assert build(tree_bytes=0) == -22
    assert build(nf=nf + 4) == -22          # a tree sized for fewer faces
    assert build(tree=C.c_void_p(0x80008)) == -22 and b"alignment" in L.fgc_last_error()

    good = dict(tree=P(0), tree_bytes=need, nf=nf, origins=P(1), n_origins=1, dirs=P(2), nq=nq, t_min=0.0, t_out=P(3),
                face_out=P(4), bary_out=P(5), stream=None)

    def cast(**kw):
        a = dict(good, **kw)
        return L.fgc_ray_cast_tree(a["tree"], a["tree_bytes"], a["nf"], a["origins"], a["n_origins"], a["dirs"], a["nq"],
                                   a["t_min"], a["t_out"], a["face_out"], a["bary_out"], a["stream"])
    for name in ("tree", "origins", "dirs", "t_out", "face_out"):
        assert cast(**{name: None}) == -22, name
        assert b"fgc_ray_cast_tree" in L.fgc_last_error()
    for name in ("nf", "nq"):
        assert cast(**{name: 0}) == -22 and cast(**{name: -5}) == -22, name
    assert cast(nf=2 ** 31 - 1) == -22 and cast(nf=MAX_FACES + 1) == -22
    for n_origins in (0, 2, nq - 1, nq + 1, -1):
        assert cast(n_origins=n_origins) == -22, n_origins
    assert b"n_origins" in L.fgc_last_error()
    for t_min in (-1e-6, float("inf"), float("-inf"), float("nan")):
        assert cast(t_min=t_min) == -22, t_min
    assert b"t_min" in L.fgc_last_error()
    assert cast(tree_bytes=need - 1) == -22 and b"too small" in L.fgc_last_error()
    assert cast(tree_bytes=0) == -22 and cast(nf=nf + 4) == -22
    assert cast(tree=C.c_void_p(0x80008)) == -22 and b"alignment" in L.fgc_last_error()


def test_the_scenes_are_the_ones_the_tests_were_sized_for():
    """Skipped cases, counted here in float64 (about 20 s: every oracle of the GPU tests runs once).  Image rays: 3 / 2 / 1 of
    1 850 on the scenes of scan_cases, 2 on icosphere(4) and 3 on torus(64, 40); the tilted grid 17 / 16 / 2 of 1 849, the grid
    straight down on the rotated meshes 0; the prefixes of the icosphere 0 up to 257 faces and 3 at 1 279; ambiguous vertices
    of the two meshes of 5 120 faces 0 / 0 and 3 / 0."""
    for key, skipped in tc.SKIPPED.items():
        c = tc.case(*key)
        nq = 1850 if key[0] == "image" else 1849
        assert c["rays"].shape == (nq, 3) and c["rays"].dtype == np.float32 and c["origins"].shape in ((1, 3), (nq, 3))
        assert (~c["robust"]).sum() == skipped <= sc.CAP * nq, key
        assert 0.1 < (c["face"] >= 0).mean() < 0.95, key          # surface and background
    for name in tc.BIG:
        V, F, _ = tc.mesh(name)
        assert F.shape == (5120, 3) and V.shape[0] in (2560, 2562)
    for kind, zeros in (("tilt", 1), ("down", 2)):
        assert (tc.case(kind, "cube")["rays"] == 0).sum(1).tolist() == [zeros] * 1849
    # rotated once, in float64: the same mesh up to rounding, no axis-aligned face left
    V, R = tc.mesh("cube")[0], tc.mesh("rot:cube")[0]
    assert np.abs(np.linalg.norm(V, axis=1) - np.linalg.norm(R.astype(np.float64), axis=1)).max() < 1e-6
    assert (np.ptp(R[tc.mesh("cube")[1]], axis=1) > 1e-3).all()
    for k, skipped in tc.PREFIX_SKIPPED.items():
        assert (~tc.prefix_case(k)["robust"]).sum() == skipped, k
    for (name, view), ambiguous in tc.AMBIGUOUS.items():
        cls = tc.visibility_case(name, view)
        assert (cls < 0).sum() == ambiguous <= sc.CAP * cls.size, (name, view)
        assert 0.3 < (cls == 1).mean() < 0.6


def test_the_chunked_oracle_is_scan_cases_oracle():
    V, F, cam = sc.scene("cube")
    ic = sc.image_case("cube")
    got = tc.oracle(V, F, np.asarray(cam).reshape(1, 3), ic["rays"], chunk=97)
    for k in ("t", "face", "u", "v", "robust"):
        assert np.array_equal(got[k], ic[k]), k
    V, F, cam = sc.scene("torus")
    o, d = sc.perspective_rays(V, cam)
    assert np.array_equal(tc.classify(V, F, o, d, chunk=100), sc.visibility_case("torus", "camera"))


def test_the_default_order_is_a_permutation_with_the_invalid_faces_last():
    V, F, _ = tc.mesh("torus64")
    V, F = V.copy(), F.astype(np.int64)
    F[5] = [0, 1, V.shape[0]]                 # an id out of range
    F[77] = [-1, 2, 3]
    V[1000, 1] = np.nan                       # six faces hold vertex 1000
    V[2000, 0] = np.inf
    bad = np.zeros(F.shape[0], dtype=bool)
    bad[[5, 77]] = True
    bad |= (F == 1000).any(1) | (F == 2000).any(1)
    assert bad.sum() == 2 + 6 + 6
    order = ops.ray_tree_order(torch.from_numpy(V), torch.from_numpy(F))
    assert order.dtype == torch.int32 and order.shape == (F.shape[0],) and not order.is_cuda
    order = order.numpy()
    assert np.array_equal(np.sort(order), np.arange(F.shape[0]))
    assert np.array_equal(order[-bad.sum():], np.flatnonzero(bad))          # last, and (the sort is stable) in rising order
    # the order is coherent: four faces in a row - a leaf - lie close together (a torus of extent 3: random would give ~1.5)
    cen = np.asarray(tc.mesh("torus64")[0], dtype=np.float64)[F[order[:-bad.sum()]].clip(0, V.shape[0] - 1)].mean(1)
    k = cen.shape[0] // 4 * 4
    spread = np.ptp(cen[:k].reshape(-1, 4, 3), axis=1).max(1)
    assert np.median(spread) < 0.2
    # a mesh of one face, and one without a valid face
    one = ops.ray_tree_order(torch.zeros(3, 3), torch.tensor([[0, 1, 2]]))
    assert one.tolist() == [0]
    none = ops.ray_tree_order(torch.zeros(3, 3), torch.tensor([[0, 1, 3], [0, 1, 7]]))
    assert none.tolist() == [0, 1]


def test_the_host_layers_refuse_before_anything_reaches_the_gpu(tmp_path, capsys):
    from facet_graph_convolution_amd import scan
    V, F, cam = sc.scene("icosphere")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ray_tree(torch.from_numpy(V.copy()), torch.from_numpy(F.copy()))
    with pytest.raises(TypeError, match="RayTree"):
        ops.ray_cast_tree(torch.zeros(16), torch.zeros(1, 3), torch.ones(4, 3))
    handle = ops.RayTree(torch.zeros(16, dtype=torch.uint8), F.shape[0], V.shape[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ray_cast_tree(handle, torch.zeros(1, 3), torch.ones(4, 3))
    for accel in ("bvh", None, 3):
        with pytest.raises(ValueError, match="accel"):
            utils._ray_cast_host(V, F, np.zeros((1, 3)), np.ones((4, 3)), accel=accel)
    with pytest.raises(SystemExit) as e:
        scan.main([str(tmp_path), str(tmp_path), "--camera", "0,0,5", "--accel", "bvh"])
    assert e.value.code == 2 and "--accel" in capsys.readouterr().err
