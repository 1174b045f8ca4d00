"""CPU checks of the point-set training path (trainAccuracyNet): the new C-ABI entry points refuse bad arguments before any
launch, the inverse tables of the vertex-update adjoint follow the slot table, and `preprocess --with-vertices` pickles
the vertex data addMeshWithVertices gives."""
import ctypes as C
import os
import pickle

import numpy as np

from facet_graph_convolution_amd import _lib, ops
from facet_graph_convolution_amd.meshgen import icosphere, add_noise
from facet_graph_convolution_amd.utils import write_mesh


def _buf(n=1 << 16):
    b = (C.c_char * n)()
    return b, C.c_void_p((C.addressof(b) + 255) // 256 * 256)


def _rejects(rc, name):
    L = _lib.lib()
    assert rc == -22, rc
    msg = L.fgc_last_error()
    assert msg and name.encode() in msg, msg


def test_vertex_update_ms_traj_rejects_bad_arguments():
    L = _lib.lib()
    keep, p = _buf()
    it = (C.c_int32 * 3)(1, 1, 1)
    args = lambda **kw: [kw.get(k, d) for k, d in (   # noqa: E731
        ("x", p), ("nv", 10), ("faces", p), ("n0", 16), ("vf", p), ("kv", 4), ("a", p), ("b", p), ("c", p), ("it", it),
        ("traj", p), ("tf", 4 * 30), ("scr", p), ("sf", 3 * 21), ("st", None))]
    f = L.fgc_vertex_update_ms_traj
    _rejects(f(*args(x=None)), "fgc_vertex_update_ms_traj")
    _rejects(f(*args(traj=None)), "fgc_vertex_update_ms_traj")
    _rejects(f(*args(n0=15)), "fgc_vertex_update_ms_traj")
    _rejects(f(*args(nv=0)), "fgc_vertex_update_ms_traj")
    _rejects(f(*args(tf=4 * 30 - 1)), "traj too small")
    _rejects(f(*args(sf=3 * 21 - 1)), "scratch too small")
    _rejects(f(*args(it=(C.c_int32 * 3)(1, -1, 1))), "negative")


def test_vertex_update_ms_bwd_rejects_bad_arguments():
    L = _lib.lib()
    keep, p = _buf()
    it = (C.c_int32 * 3)(1, 1, 1)
    q = C.c_void_p(p.value + 1024)
    need = L.fgc_vertex_update_ms_bwd_workspace_floats(10, 16)
    assert need == 7 * 10 + 6 * (16 + 4 + 1)
    assert L.fgc_vertex_update_ms_bwd_workspace_floats(0, 16) == 0
    names = ("traj", "tf", "nv", "faces", "n0", "vf", "kv", "a", "b", "c", "it", "sp", "sv", "ip", "fi", "gout", "gx", "g0", "g1",
             "g2", "ws", "wsf", "st")
    base = dict(traj=p, tf=4 * 30, nv=10, faces=p, n0=16, vf=p, kv=4, a=p, b=p, c=p, it=it, sp=p, sv=p, ip=p, fi=p, gout=p, gx=q,
                g0=p, g1=p, g2=p, ws=p, wsf=need, st=None)
    f = lambda **kw: L.fgc_vertex_update_ms_bwd(*[kw.get(k, base[k]) for k in names])  # noqa: E731
    for k in ("traj", "sp", "sv", "ip", "fi", "gout", "gx", "g1", "ws"):
        _rejects(f(**{k: None}), "fgc_vertex_update_ms_bwd")
    _rejects(f(n0=24), "fgc_vertex_update_ms_bwd")
    _rejects(f(kv=0), "fgc_vertex_update_ms_bwd")
    _rejects(f(wsf=need - 1), "workspace too small")
    _rejects(f(tf=4 * 30 - 1), "traj too small")
    _rejects(f(gx=p), "distinct")
    _rejects(f(it=(C.c_int32 * 3)(-1, 0, 0)), "negative")


def test_point_loss_rejects_bad_arguments():
    L = _lib.lib()
    keep, p = _buf()
    need = L.fgc_point_loss_workspace_bytes(100, 200, 5, 7)
    assert need >= (5 + 7) * 20
    assert L.fgc_point_loss_workspace_bytes(100, 200, 0, 7) == 0
    names = ("p0", "np0", "p1", "np1", "i0", "ns0", "i1", "ns1", "thr", "loss", "g", "ws", "wsb", "st")
    base = dict(p0=p, np0=100, p1=p, np1=200, i0=p, ns0=5, i1=p, ns1=7, thr=5000.0, loss=p, g=None, ws=p, wsb=need, st=None)
    f = lambda **kw: L.fgc_point_loss(*[kw.get(k, base[k]) for k in names])  # noqa: E731
    for k in ("p0", "p1", "i0", "i1", "loss", "ws"):
        _rejects(f(**{k: None}), "fgc_point_loss")
    for k in ("np0", "np1", "ns0", "ns1"):
        _rejects(f(**{k: 0}), "fgc_point_loss")
    _rejects(f(wsb=need - 1), "workspace too small")
    _rejects(f(ws=C.c_void_p(p.value + 8)), "alignment")
    _rejects(f(ns0=16384 - 6), "at most 16384")


def test_inverse_tables_follow_the_slot_table():
    """Slot inverse from the (possibly truncated) v_faces slots, incidence from the faces' corners; fake rows name nothing."""
    faces = np.array([[0, 1, 2], [-1, -1, -1], [2, 1, 3], [0, 2, 3]])
    v_faces = np.array([[0, 3], [0, 2], [0, 2], [2, -1], [-1, -1]])     # vertex 2 lost face 3 to truncation
    sp, sv, ip, fi = ops.vertex_ms_tables(faces, v_faces, 5)
    assert sp.tolist() == [0, 3, 3, 6, 7]
    assert sv.tolist() == [0, 1, 2, 1, 2, 3, 0]
    assert ip.tolist() == [0, 2, 4, 7, 9, 9]
    assert fi.tolist() == [0, 3, 0, 2, 0, 2, 3, 2, 3]
    assert all(t.dtype == np.int32 for t in (sp, sv, ip, fi))


def test_preprocess_with_vertices(tmp_path):
    from facet_graph_convolution_amd import preprocess
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    V, F = icosphere(2)
    noisy, gt = tmp_path / "noisy", tmp_path / "gt"
    noisy.mkdir()
    gt.mkdir()
    Vn = add_noise(V, F, seed=3)
    write_mesh(Vn, F, str(noisy / "ball_n1.obj"))
    write_mesh(V, F, str(gt / "ball.obj"))
    out = tmp_path / "dump"
    preprocess.main([str(noisy), str(gt), str(out), "--with-vertices"])
    assert sorted(os.listdir(out)) == ["trainingSetWithVertices.pkl"]
    with open(out / "trainingSetWithVertices.pkl", "rb") as fh:
        ds = pickle.load(fh)
    ref = TrainingSet()
    Vr = np.loadtxt(str(noisy / "ball_n1.obj"), usecols=(1, 2, 3), max_rows=len(V)).astype(np.float32)
    Vg = np.loadtxt(str(gt / "ball.obj"), usecols=(1, 2, 3), max_rows=len(V)).astype(np.float32)
    ref.addMeshWithVertices(Vr, F, GTV=Vg, seed=ds.seed)
    for name in ("v_list", "gtv_list", "faces_list", "v_faces_list"):
        assert len(getattr(ds, name)) == len(getattr(ref, name)) == 1, name
    for name in ("v_list", "gtv_list", "v_faces_list"):
        got, want = getattr(ds, name), getattr(ref, name)
        assert got[0].shape == want[0].shape, (name, got[0].shape, want[0].shape)
    assert ds.v_list[0].shape == (1, len(V), 3) and ds.gtv_list[0].shape == (1, len(V), 3)
    assert ds.v_faces_list[0].shape == (1, len(V), 25)
    # (the coarsening is drawn at random: the padded node count may differ from run to run)
    assert ds.faces_list[0].shape == (1, ds.in_list[0].shape[1], 3) and ds.faces_list[0].shape[1] % 16 == 0
    assert (ds.faces_list[0] >= 0).all(-1).sum() == len(F)
    np.testing.assert_allclose(ds.v_list[0], ref.v_list[0], atol=1e-6)
    np.testing.assert_allclose(ds.gtv_list[0], ref.gtv_list[0], atol=1e-6)
