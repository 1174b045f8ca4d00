"""Thin functional wrappers over the C ABI (one call = one enqueue on torch's current stream).

No autograd here (see model.py); tensors are fp32, contiguous, on the GPU.  Everything raises
if libfgc.so is missing: there is no eager/CPU fallback by design.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, ConvBwdIO, ptr, stream_ptr, check, AG_LD, DL_LD, FGC_M

_WS = {}


def _workspace(nbytes, device, tag="ws"):
    """Grow-only scratch buffer per (device, tag); the library never allocates."""
    key = (str(device), tag)
    t = _WS.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _WS[key] = t
    return t


def _f32c(t):
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.contiguous().float()
    return t


def _req_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("facet_graph_convolution_amd ops need GPU tensors (no CPU fallback)")


def make_conv_desc(graph, x0, x1, shift, params, bias_mask, act, alpha):
    W0, b, u, c, v = params
    d = ConvDesc()
    d.n, d.nnz = graph.n, graph.nnz
    d.rowptr, d.col = graph.rowptr.data_ptr(), graph.col.data_ptr()
    d.x0 = x0.data_ptr()
    d.x1 = x1.data_ptr() if x1 is not None else None
    d.c0 = x0.shape[-1]
    d.c1 = x1.shape[-1] if x1 is not None else 0
    d.shift = shift
    d.cout = W0.shape[1]
    d.W0, d.b, d.u, d.c, d.v = W0.data_ptr(), b.data_ptr(), u.data_ptr(), c.data_ptr(), v.data_ptr()
    d.bias_mask = int(bool(bias_mask))
    d.act = int(act)
    d.alpha = float(alpha)
    d.max_deg = graph.max_deg
    return d


def attach_pairs(d, graph, hc):
    """Give a descriptor of a layer over a 4x-upsampled input its pair graph and the table of transformed coarse rows
    hc [(n >> 2), 9 * cout]: the library then runs the layer in the pair form if it qualifies (fgc_conv_uses_pairs)."""
    pg = graph.pairs()
    d.pair_rowptr, d.pair_col, d.pair_mul = pg.prow.data_ptr(), pg.pcol.data_ptr(), pg.pmul.data_ptr()
    d.n_pairs, d.max_pair_deg, d.max_pair_in_deg = pg.n_pairs, pg.max_deg, pg.max_in_deg
    d.hc = hc.data_ptr()
    return pg


def conv_fwd(graph, x0, x1, shift, params, bias_mask=True, act=0, alpha=0.1, want_pool=False, pairs=None):
    """Returns (y [n,cout], y_pool [n/4,cout] or None, ag [(n>>shift),24]).

    pairs: a dict - the layer (shift == 2) is described with its pair graph; on return pairs["hc"] holds the transformed
    coarse rows (pass the same dict to conv_bwd) and pairs["used"] whether the library took the pair form."""
    _req_cuda(x0, x1, *params)
    x0, x1 = _f32c(x0), _f32c(x1)
    params = [_f32c(p) for p in params]
    W0 = params[0]
    cin = x0.shape[-1] + (x1.shape[-1] if x1 is not None else 0)
    if W0.shape[0] != FGC_M or W0.shape[2] != cin:
        raise ValueError("W0 must be [9, cout, %d], got %s" % (cin, tuple(W0.shape)))
    rows = graph.n >> shift
    if x0.shape[0] != rows or (x1 is not None and x1.shape[0] != rows):
        raise ValueError("input rows %d != n>>shift = %d" % (x0.shape[0], rows))
    d = make_conv_desc(graph, x0, x1, shift, params, bias_mask, act, alpha)
    L = _lib.lib()
    dev = x0.device
    if pairs is not None:
        pairs["hc"] = torch.empty(rows, FGC_M * d.cout, dtype=torch.float32, device=dev)
        attach_pairs(d, graph, pairs["hc"])
        pairs["used"] = bool(L.fgc_conv_uses_pairs(C.byref(d)))
    ws_bytes = L.fgc_conv_workspace_bytes(C.byref(d))
    ws = _workspace(ws_bytes, dev)
    ag = torch.empty(rows, AG_LD, dtype=torch.float32, device=dev)
    y = torch.empty(graph.n, d.cout, dtype=torch.float32, device=dev)
    yp = torch.empty(graph.n // 4, d.cout, dtype=torch.float32, device=dev) if want_pool else None
    check(L.fgc_conv_fwd(C.byref(d), ptr(ag), ptr(y), ptr(yp), ptr(ws), ws.numel(), stream_ptr()), "fgc_conv_fwd")
    return y, yp, ag


def conv_bwd(graph, x0, x1, shift, params, ag, y, dy, bias_mask=True, act=0, alpha=0.1, need_dx=True,
             dx0=None, dx1=None, acc0=False, acc1=False, pairs=None):
    """Gradient of conv_fwd.  Returns (dx0, dx1, [dW0, db, du, dc, dv]).

    dx0/dx1 may be passed in (with acc flags) so that a tensor consumed by two layers
    accumulates both contributions in a fixed order; otherwise they are allocated.
    """
    _req_cuda(x0, x1, dy, *params)
    x0, x1, dy = _f32c(x0), _f32c(x1), _f32c(dy)
    y = _f32c(y)
    params = [_f32c(p) for p in params]
    d = make_conv_desc(graph, x0, x1, shift, params, bias_mask, act, alpha)
    L = _lib.lib()
    dev = x0.device
    n, cout = graph.n, d.cout
    trow, tcol, tedge = graph.transposed()
    f32 = dict(dtype=torch.float32, device=dev)
    ds = torch.empty(n, cout, **f32)
    dl = torch.empty(max(graph.nnz, 1), DL_LD, **f32)
    dag = torch.empty(n, AG_LD, **f32)
    r = torch.empty(n, FGC_M * cout + 24, **f32)
    grads = [torch.empty_like(p) for p in params]
    if need_dx:
        if dx0 is None:
            dx0 = torch.empty_like(x0)
            acc0 = False
        if x1 is not None and dx1 is None:
            dx1 = torch.empty_like(x1)
            acc1 = False
    else:
        dx0 = dx1 = None
    io = ConvBwdIO()
    io.trowptr, io.tcol, io.tedge = trow.data_ptr(), tcol.data_ptr(), tedge.data_ptr()
    io.max_in_deg = graph.max_in_deg
    io.ag, io.y, io.dy = ag.data_ptr(), (y.data_ptr() if y is not None else None), dy.data_ptr()
    io.ds, io.dl, io.dag, io.r = ds.data_ptr(), dl.data_ptr(), dag.data_ptr(), r.data_ptr()
    io.dx0 = dx0.data_ptr() if dx0 is not None else None
    io.dx1 = dx1.data_ptr() if dx1 is not None else None
    io.accumulate0, io.accumulate1 = int(bool(acc0)), int(bool(acc1))
    io.dW0, io.db, io.du, io.dc, io.dv = [g.data_ptr() for g in grads]
    if pairs is not None:
        pg = attach_pairs(d, graph, pairs["hc"])
        io.tpair_rowptr, io.tpair_col, io.tpair_edge = pg.trow.data_ptr(), pg.tcol.data_ptr(), pg.tedge.data_ptr()
        dt = torch.empty(max(pg.n_pairs, 1), cout, **f32)
        if dl.shape[0] < pg.n_pairs:
            dl = torch.empty(pg.n_pairs, DL_LD, **f32)
            io.dl = dl.data_ptr()
        io.dt = dt.data_ptr()
    ws_bytes = L.fgc_conv_bwd_workspace_bytes(C.byref(d))
    ws = _workspace(ws_bytes, dev, "bwd")
    check(L.fgc_conv_bwd(C.byref(d), C.byref(io), ptr(ws), ws.numel(), stream_ptr()), "fgc_conv_bwd")
    return dx0, dx1, grads


def mlp_fwd(x, W1, b1, W2, b2, alpha=0.1, want_abs_partial=False):
    _req_cuda(x, W1, b1, W2, b2)
    x, W1, b1, W2, b2 = map(_f32c, (x, W1, b1, W2, b2))
    n, cin = x.shape
    hidden, cout = W2.shape
    L = _lib.lib()
    ws = _workspace(L.fgc_mlp_workspace_bytes(cin, hidden, cout), x.device)
    y = torch.empty(n, cout, dtype=torch.float32, device=x.device)
    part = torch.empty(L.fgc_mlp_num_partials(n), dtype=torch.float32, device=x.device) if want_abs_partial else None
    check(L.fgc_mlp_fwd(ptr(x), n, cin, hidden, cout, ptr(W1), ptr(b1), ptr(W2), ptr(b2), alpha, ptr(y), ptr(part),
                        0, ptr(ws), ws.numel(), stream_ptr()), "fgc_mlp_fwd")
    return (y, part) if want_abs_partial else y


def mlp_bwd(x, dy, W1, b1, W2, alpha=0.1):
    _req_cuda(x, dy, W1, b1, W2)
    x, dy, W1, b1, W2 = map(_f32c, (x, dy, W1, b1, W2))
    n, cin = x.shape
    hidden, cout = W2.shape
    L = _lib.lib()
    ws = _workspace(L.fgc_mlp_bwd_workspace_bytes(n, cin, hidden, cout), x.device, "bwd")
    dx = torch.empty_like(x)
    dW1, db1, dW2 = torch.empty_like(W1), torch.empty_like(b1), torch.empty_like(W2)
    db2 = torch.empty(cout, dtype=torch.float32, device=x.device)
    check(L.fgc_mlp_bwd(ptr(x), ptr(dy), n, cin, hidden, cout, ptr(W1), ptr(b1), ptr(W2), alpha, ptr(dx), ptr(dW1),
                        ptr(db1), ptr(dW2), ptr(db2), 0, ptr(ws), ws.numel(), stream_ptr()), "fgc_mlp_bwd")
    return dx, dW1, db1, dW2, db2


def lrelu_fwd(x, alpha):
    x = _f32c(x)
    y = torch.empty_like(x)
    check(_lib.lib().fgc_lrelu_fwd(ptr(x), ptr(y), x.numel(), alpha, stream_ptr()), "fgc_lrelu_fwd")
    return y


def lrelu_bwd(y, dy, alpha):
    y, dy = _f32c(y), _f32c(dy)
    dx = torch.empty_like(y)
    check(_lib.lib().fgc_lrelu_bwd(ptr(y), ptr(dy), ptr(dx), y.numel(), alpha, stream_ptr()), "fgc_lrelu_bwd")
    return dx


def pool4_fwd(x):
    x = _f32c(x)
    n, c = x.shape
    if n % 4:
        raise ValueError("pooling needs a multiple of 4 rows, got %d" % n)
    y = torch.empty(n // 4, c, dtype=torch.float32, device=x.device)
    check(_lib.lib().fgc_pool4_fwd(ptr(x), ptr(y), n // 4, c, stream_ptr()), "fgc_pool4_fwd")
    return y


def pool4_bwd(x, y, dy, dx=None, accumulate=False):
    x, y, dy = _f32c(x), _f32c(y), _f32c(dy)
    if dx is None:
        dx = torch.empty_like(x)
        accumulate = False
    check(_lib.lib().fgc_pool4_bwd(ptr(x), ptr(y), ptr(dy), ptr(dx), y.shape[0], y.shape[1], int(accumulate),
                                   stream_ptr()), "fgc_pool4_bwd")
    return dx


def upsample4_fwd(x):
    x = _f32c(x)
    n, c = x.shape
    y = torch.empty(n * 4, c, dtype=torch.float32, device=x.device)
    check(_lib.lib().fgc_upsample4_fwd(ptr(x), ptr(y), n, c, stream_ptr()), "fgc_upsample4_fwd")
    return y


def upsample4_bwd(dy, dx=None, accumulate=False):
    dy = _f32c(dy)
    n4, c = dy.shape
    if dx is None:
        dx = torch.empty(n4 // 4, c, dtype=torch.float32, device=dy.device)
        accumulate = False
    check(_lib.lib().fgc_upsample4_bwd(ptr(dy), ptr(dx), n4 // 4, c, int(accumulate), stream_ptr()),
          "fgc_upsample4_bwd")
    return dx


def pool_fwd(x, group):
    """max over each `group` consecutive rows (custom_binary_tree_pooling with group = 2^steps, model.py:779-788)."""
    x = _f32c(x)
    n, c = x.shape
    if n % group:
        raise ValueError("pooling needs a multiple of %d rows, got %d" % (group, n))
    y = torch.empty(n // group, c, dtype=torch.float32, device=x.device)
    check(_lib.lib().fgc_pool_fwd(ptr(x), ptr(y), n // group, c, int(group), stream_ptr()), "fgc_pool_fwd")
    return y


def pool_bwd(x, y, dy, group):
    x, y, dy = _f32c(x), _f32c(y), _f32c(dy)
    dx = torch.empty_like(x)
    check(_lib.lib().fgc_pool_bwd(ptr(x), ptr(y), ptr(dy), ptr(dx), y.shape[0], y.shape[1], int(group), 0, stream_ptr()),
          "fgc_pool_bwd")
    return dx


def upsample_fwd(x, group):
    """every row repeated `group` times consecutively (custom_upsampling with group = 2^steps, model.py:817-825)."""
    x = _f32c(x)
    n, c = x.shape
    y = torch.empty(n * group, c, dtype=torch.float32, device=x.device)
    check(_lib.lib().fgc_upsample_fwd(ptr(x), ptr(y), n, c, int(group), stream_ptr()), "fgc_upsample_fwd")
    return y


def upsample_bwd(dy, group):
    dy = _f32c(dy)
    n, c = dy.shape
    dx = torch.empty(n // group, c, dtype=torch.float32, device=dy.device)
    check(_lib.lib().fgc_upsample_bwd(ptr(dy), ptr(dx), n // group, c, int(group), 0, stream_ptr()), "fgc_upsample_bwd")
    return dx


def lin_fwd(x, W, b):
    """custom_lin (model.py:763-769): x [n, cin] W [cin, cout] + b."""
    _req_cuda(x, W, b)
    x, W, b = _f32c(x), _f32c(W), _f32c(b)
    n, cin = x.shape
    cout = W.shape[1]
    if W.shape[0] != cin or b.shape[0] != cout:
        raise ValueError("custom_lin: x %s, W %s, b %s" % (tuple(x.shape), tuple(W.shape), tuple(b.shape)))
    y = torch.empty(n, cout, dtype=torch.float32, device=x.device)
    check(_lib.lib().fgc_lin_fwd(ptr(x), n, cin, cout, ptr(W), ptr(b), ptr(y), stream_ptr()), "fgc_lin_fwd")
    return y


def lin_bwd(x, dy, W, need_dx=True):
    """Returns (dx or None, dW, db)."""
    _req_cuda(x, dy, W)
    x, dy, W = _f32c(x), _f32c(dy), _f32c(W)
    n, cin = x.shape
    cout = W.shape[1]
    L = _lib.lib()
    ws = _workspace(L.fgc_lin_bwd_workspace_bytes(n, cin, cout), x.device, "lin")
    dx = torch.empty_like(x) if need_dx else None
    dW = torch.empty_like(W)
    db = torch.empty(cout, dtype=torch.float32, device=x.device)
    check(L.fgc_lin_bwd(ptr(x), ptr(dy), n, cin, cout, ptr(W), ptr(dx), ptr(dW), ptr(db), ptr(ws), ws.numel(), stream_ptr()),
          "fgc_lin_bwd")
    return dx, dW, db


def normalize_fwd(x, abs_partial=None):
    """normalizeTensor on [n,3]; returns (y, scratch) - scratch feeds normalize_bwd."""
    x = _f32c(x)
    n = x.shape[0]
    L = _lib.lib()
    scratch = torch.empty(2 + L.fgc_norm_num_partials(n), dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    npart = abs_partial.numel() if abs_partial is not None else 0
    check(L.fgc_normalize_fwd(ptr(x), n, ptr(abs_partial), npart, ptr(y), ptr(scratch), stream_ptr()),
          "fgc_normalize_fwd")
    return y, scratch


def normalize_bwd(x, dy, scratch):
    x, dy = _f32c(x), _f32c(dy)
    dx = torch.empty_like(x)
    check(_lib.lib().fgc_normalize_bwd(ptr(x), ptr(dy), x.shape[0], ptr(dx), ptr(scratch), stream_ptr()),
          "fgc_normalize_bwd")
    return dx


def angular_loss_fwd(fn, gt, sample_ind):
    fn, gt = _f32c(fn), _f32c(gt)
    out = torch.empty(2, dtype=torch.float32, device=fn.device)
    check(_lib.lib().fgc_angular_loss_fwd(ptr(fn), ptr(gt), ptr(sample_ind), sample_ind.numel(), ptr(out),
                                          stream_ptr()), "fgc_angular_loss_fwd")
    return out


def angular_loss_bwd(fn, gt, sample_ind, loss_out, dloss=1.0):
    fn, gt = _f32c(fn), _f32c(gt)
    dfn = torch.empty_like(fn)
    check(_lib.lib().fgc_angular_loss_bwd(ptr(fn), ptr(gt), ptr(sample_ind), sample_ind.numel(), fn.shape[0],
                                          ptr(loss_out), float(dloss), ptr(dfn), stream_ptr()),
          "fgc_angular_loss_bwd")
    return dfn


def rotate_rows(x, R):
    """Every 3-vector v of every row becomes R v (train.py:439-451).  R: 3x3 array-like or device tensor."""
    x = _f32c(x)
    n, c = x.shape
    if c % 3:
        raise ValueError("channels must be a multiple of 3")
    if not isinstance(R, torch.Tensor) or not R.is_cuda:
        R = torch.as_tensor(np.asarray(R, dtype=np.float32).reshape(9)).to(x.device)
    R = R.reshape(9).float().contiguous()
    y = torch.empty_like(x)
    check(_lib.lib().fgc_rotate_rows(ptr(x), ptr(y), n, c // 3, ptr(R), stream_ptr()), "fgc_rotate_rows")
    return y


def adam_step(p, g, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    check(_lib.lib().fgc_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), int(t), lr, b1, b2, eps,
                                   stream_ptr()), "fgc_adam_step")


def infer_epilogue(n_conv, perm, num_faces):
    n_conv = _f32c(n_conv)
    out = torch.empty(num_faces, 3, dtype=torch.float32, device=n_conv.device)
    check(_lib.lib().fgc_infer_epilogue(ptr(n_conv), ptr(perm), num_faces, ptr(out), stream_ptr()),
          "fgc_infer_epilogue")
    return out


def gather_rows(src, idx):
    src = _f32c(src)
    dst = torch.empty(idx.numel(), src.shape[1], dtype=torch.float32, device=src.device)
    check(_lib.lib().fgc_gather_rows(ptr(src), ptr(idx), idx.numel(), src.shape[1], ptr(dst), stream_ptr()),
          "fgc_gather_rows")
    return dst


def scatter_add_rows(src, idx, dst):
    src = _f32c(src)
    check(_lib.lib().fgc_scatter_add_rows(ptr(src), ptr(idx), idx.numel(), src.shape[1], ptr(dst), stream_ptr()),
          "fgc_scatter_add_rows")
    return dst


def vertex_update(x, normals, e_map, v_e_map, iters, lmbd=1.0 / 18):
    """update_position2 (train.py:1467-1557) on [V,3] positions; e_map int32 [E,4], v_e_map int32 [V,max_edges]."""
    _req_cuda(x, normals, e_map, v_e_map)
    x, normals = _f32c(x), _f32c(normals)
    e_map = e_map.to(torch.int32).contiguous()
    v_e_map = v_e_map.to(torch.int32).contiguous()
    out, tmp = torch.empty_like(x), torch.empty_like(x)
    check(_lib.lib().fgc_vertex_update(ptr(x), ptr(out), ptr(tmp), x.shape[0], ptr(normals), normals.shape[0],
                                       ptr(e_map), e_map.shape[0], ptr(v_e_map), v_e_map.shape[1], int(iters),
                                       float(lmbd), stream_ptr()), "fgc_vertex_update")
    return out


def vertex_update_dir(x, normals, e_map, v_e_map, dirs, iters, lmbd=1.0 / 18, return_t=False):
    """update_position_with_depth (train.py:1561-1665) on [V,3] positions: vertex_update with every contribution projected
    onto the vertex' direction, dirs [V,3] or [1,3] (used as given, nothing is normalised; include/fgc.h:
    fgc_vertex_update_dir).  Returns the positions [V,3]; return_t: (positions, t [V]), t the signed step along the
    direction, positions = fma(t, dirs, x)."""
    _req_cuda(x, normals, e_map, v_e_map, dirs)
    x, normals, dirs = _f32c(x), _f32c(normals), _f32c(dirs.reshape(-1, 3))
    e_map = e_map.to(torch.int32).reshape(-1, 4).contiguous()
    v_e_map = v_e_map.to(torch.int32).contiguous()
    nv = x.shape[0]
    if dirs.shape[0] not in (1, nv):
        raise ValueError("dirs has %d rows: one row, or one per vertex (%d)" % (dirs.shape[0], nv))
    if x.dim() != 2 or x.shape[1] != 3 or v_e_map.dim() != 2 or v_e_map.shape[0] != nv or normals.shape[-1] != 3:
        raise ValueError("x [V,3], normals [F,3], v_e_map [V,slots] with one row per vertex (%d)" % nv)
    L = _lib.lib()
    out = torch.empty_like(x)
    t = torch.empty(nv, dtype=torch.float32, device=x.device) if return_t else None
    ws = torch.empty(max(L.fgc_vertex_update_dir_workspace_floats(nv), 1), dtype=torch.float32, device=x.device)
    check(L.fgc_vertex_update_dir(ptr(x), ptr(out), ptr(t), ptr(ws), ws.numel(), nv, ptr(normals), normals.shape[0],
                                  ptr(e_map), e_map.shape[0], ptr(v_e_map), v_e_map.shape[1], ptr(dirs), dirs.shape[0],
                                  int(iters), float(lmbd), stream_ptr()), "fgc_vertex_update_dir")
    return (out, t) if return_t else out


def ray_cast(verts, faces, origins, dirs, t_min=0.0, want_bary=False):
    """First hit of every ray against a triangle list (include/fgc.h: fgc_ray_cast; a build extension) on GPU tensors:
    verts [V,3] fp32, faces int32 [F,3] (a row with an id outside [0, V) is skipped), origins [1,3] (a camera) or [Q,3],
    dirs [Q,3] used as given, never normalised: t is in units of |d|.  Returns (t [Q] fp32, face [Q] int32) - a miss is
    (+inf, -1) - and with want_bary also bary [Q,2] = (u, v) of the hit, the point being (1 - u - v) a + u b + v c."""
    _req_cuda(verts, faces, origins, dirs)
    verts, origins, dirs = _f32c(verts.reshape(-1, 3)), _f32c(origins.reshape(-1, 3)), _f32c(dirs.reshape(-1, 3))
    faces = faces.to(torch.int32).reshape(-1, 3).contiguous()
    nv, nf, nq = verts.shape[0], faces.shape[0], dirs.shape[0]
    if origins.shape[0] not in (1, nq):
        raise ValueError("origins has %d rows: one row, or one per ray (%d)" % (origins.shape[0], nq))
    if not (np.isfinite(t_min) and t_min >= 0):
        raise ValueError("t_min must be finite and >= 0 (got %r)" % (t_min,))
    L = _lib.lib()
    nbytes = L.fgc_ray_cast_workspace_bytes(nf, nq)
    if nbytes == 0 or nv == 0:
        raise ValueError("ray_cast needs at least one vertex, one face and one ray (got %d, %d, %d)" % (nv, nf, nq))
    t = torch.empty(nq, dtype=torch.float32, device=verts.device)
    face = torch.empty(nq, dtype=torch.int32, device=verts.device)
    bary = torch.empty(nq, 2, dtype=torch.float32, device=verts.device) if want_bary else None
    ws = _workspace(nbytes, verts.device, "ray_cast")
    check(L.fgc_ray_cast(ptr(verts), nv, ptr(faces), nf, ptr(origins), origins.shape[0], ptr(dirs), nq, float(t_min), ptr(t),
                         ptr(face), ptr(bary), ptr(ws), ws.numel(), stream_ptr()), "fgc_ray_cast")
    return (t, face, bary) if want_bary else (t, face)


def _morton30(p, ok=None):
    """30-bit Morton code of the rows of p [N,3] over the bounding box of the rows marked ok (default: the finite ones):
    int64 [N], 10 bits per axis, x the lowest of each triple; a row that is not ok gets 2^30, behind every code.  Plain
    torch on the tensor's device - plumbing that decides the ORDER of work only, never a result."""
    p = p.reshape(-1, 3).to(torch.float32)
    fin = torch.isfinite(p).all(1)
    ok = fin if ok is None else (ok & fin)
    code = torch.full((p.shape[0],), 1 << 30, dtype=torch.int64, device=p.device)
    if not bool(ok.any()):
        return code
    pk = p[ok].double()
    lo, hi = pk.min(0).values, pk.max(0).values
    ext = torch.where(hi > lo, hi - lo, torch.ones_like(lo))
    cell = ((pk - lo) / ext * 1024.0).floor().clamp_(0, 1023).to(torch.int64)
    c = torch.zeros(pk.shape[0], dtype=torch.int64, device=p.device)
    for bit in range(10):
        for axis in range(3):
            c |= ((cell[:, axis] >> bit) & 1) << (3 * bit + axis)
    code[ok] = c
    return code


def ray_tree_order(verts, faces):
    """The default order of ray_tree: int32 [F], a permutation of 0 .. F-1 - the faces sorted (stably) by the 30-bit Morton
    code of their centroids over the centroids' bounding box; a face with a vertex id outside [0, V) or a non-finite
    coordinate goes last.  Plain torch, on the tensors' device (CPU tensors are fine here)."""
    verts = verts.reshape(-1, 3).to(torch.float32)
    faces = faces.reshape(-1, 3).to(torch.int64)
    valid = ((faces >= 0) & (faces < verts.shape[0])).all(1)
    tri = verts[faces.clamp(0, max(verts.shape[0] - 1, 0))]                      # [F,3,3]
    valid = valid & torch.isfinite(tri).all(2).all(1)
    cen = tri.double().mean(1).to(torch.float32)
    return torch.sort(_morton30(cen, valid), stable=True).indices.to(torch.int32)


class RayTree:
    """What ray_tree returns: the device buffer of fgc_ray_tree_build and the sizes it was built for."""

    def __init__(self, tree, nf, nv):
        self.tree, self.nf, self.nv = tree, int(nf), int(nv)

    def __repr__(self):
        return "RayTree(nf=%d, nv=%d, %d bytes on %s)" % (self.nf, self.nv, self.tree.numel(), self.tree.device)


def ray_tree(verts, faces, order=None):
    """The bounding-box tree of a triangle list for ray_cast_tree (include/fgc.h: fgc_ray_tree_build; a build extension) on
    GPU tensors: verts [V,3] fp32, faces int [F,3].  order: int [F], a permutation of 0 .. F-1 that says which faces share
    a leaf (four in a row) and a node; ANY permutation gives the same results, only the speed depends on it.  None: the
    Morton order of ray_tree_order.  The tree is built once per mesh and serves any number of casts."""
    _req_cuda(verts, faces, order)
    verts = _f32c(verts.reshape(-1, 3))
    faces = faces.to(torch.int32).reshape(-1, 3).contiguous()
    nv, nf = verts.shape[0], faces.shape[0]
    L = _lib.lib()
    nbytes = L.fgc_ray_tree_bytes(nf)
    if nbytes == 0 or nv == 0:
        raise ValueError("ray_tree needs at least one vertex and one face (got %d, %d)" % (nv, nf))
    order = ray_tree_order(verts, faces) if order is None else order.to(torch.int32).reshape(-1).contiguous()
    if order.shape[0] != nf:
        raise ValueError("order has %d entries: one per face (%d)" % (order.shape[0], nf))
    tree = torch.empty(nbytes, dtype=torch.uint8, device=verts.device)
    check(L.fgc_ray_tree_build(ptr(verts), nv, ptr(faces), nf, ptr(order), ptr(tree), tree.numel(), stream_ptr()),
          "fgc_ray_tree_build")
    return RayTree(tree, nf, nv)


def _tree_query(key, inputs, want_bary, call):
    """What ray_cast_tree and closest_point_tree share.  key: the [Q,3] rows in whose (stable) Morton order the queries are
    made, None for the order given; inputs: the per-query tensors; Q is the row count of the LAST of them, and only the
    inputs with Q rows are permuted (one origin for all rays, a single row, stays as it is); call(inputs, outputs) makes the
    C call.  Returns [value [Q] fp32, face [Q] int32, bary [Q,2] fp32 or None], scattered back."""
    nq = inputs[-1].shape[0]
    perm = None
    if key is not None and nq > 1:
        perm = torch.sort(_morton30(key), stable=True).indices
        inputs = [x[perm].contiguous() if x.shape[0] == nq else x for x in inputs]
    dev = inputs[-1].device
    out = [torch.empty(nq, dtype=torch.float32, device=dev), torch.empty(nq, dtype=torch.int32, device=dev),
           torch.empty(nq, 2, dtype=torch.float32, device=dev) if want_bary else None]
    call(inputs, out)
    if perm is not None:
        out = [None if x is None else torch.empty_like(x).index_copy_(0, perm, x) for x in out]
    return out


def ray_cast_tree(tree, origins, dirs, t_min=0.0, want_bary=False, sort_rays=True):
    """ray_cast through a RayTree (include/fgc.h: fgc_ray_cast_tree): the same arguments and the same returns, the mesh
    being the one the tree was built of.  sort_rays: cast the rays in the (stable) Morton order of their unit directions
    (one origin) or of their origins, and scatter the results back - neighbours in a wave then walk the same nodes.  A ray's
    result does not depend on its neighbours, so this changes the time and not one bit of the result."""
    if not isinstance(tree, RayTree):
        raise TypeError("ray_cast_tree needs the RayTree that ray_tree returns (got %s)" % type(tree).__name__)
    _req_cuda(tree.tree, origins, dirs)
    origins, dirs = _f32c(origins.reshape(-1, 3)), _f32c(dirs.reshape(-1, 3))
    nq = dirs.shape[0]
    if origins.shape[0] not in (1, nq):
        raise ValueError("origins has %d rows: one row, or one per ray (%d)" % (origins.shape[0], nq))
    if not (np.isfinite(t_min) and t_min >= 0):
        raise ValueError("t_min must be finite and >= 0 (got %r)" % (t_min,))
    if nq == 0:
        raise ValueError("ray_cast_tree needs at least one ray")
    key = None
    if sort_rays and nq > 1:
        key = dirs / dirs.norm(dim=1, keepdim=True) if origins.shape[0] == 1 else origins
    t, face, bary = _tree_query(key, [origins, dirs], want_bary, lambda inp, out: check(_lib.lib().fgc_ray_cast_tree(
        ptr(tree.tree), tree.tree.numel(), tree.nf, ptr(inp[0]), inp[0].shape[0], ptr(inp[1]), nq, float(t_min), ptr(out[0]),
        ptr(out[1]), ptr(out[2]), stream_ptr()), "fgc_ray_cast_tree"))
    return (t, face, bary) if want_bary else (t, face)


CP_EXHAUSTIVE = 1  # FGC_CP_EXHAUSTIVE of include/fgc.h


def closest_point_tree(tree, points, want_bary=False, sort_points=True, exhaustive=False):
    """The closest point of the mesh of a RayTree to every row of points [Q,3] (include/fgc.h: fgc_closest_point_tree; a
    build extension) on GPU tensors.  Returns (dist [Q] fp32 = sqrt(dist2) in IEEE, face [Q] int32, the original face
    index) - a mesh without a face that takes part gives (+inf, -1) - and with want_bary also bary [Q,2] = (u, v), the
    point being (1 - u - v) a + u b + v c.  sort_points: query in the (stable) Morton order of the points and scatter the
    results back - neighbours in a wave then walk the same nodes.  exhaustive: no culling, every point against every
    record (points x faces pairs).  Neither changes one bit of the result."""
    if not isinstance(tree, RayTree):
        raise TypeError("closest_point_tree needs the RayTree that ray_tree returns (got %s)" % type(tree).__name__)
    _req_cuda(tree.tree, points)
    points = _f32c(points.reshape(-1, 3))
    nq = points.shape[0]
    if nq == 0:
        raise ValueError("closest_point_tree needs at least one point")
    d2, face, bary = _tree_query(points if sort_points else None, [points], want_bary, lambda inp, out: check(
        _lib.lib().fgc_closest_point_tree(ptr(tree.tree), tree.tree.numel(), tree.nf, ptr(inp[0]), nq,
                                          CP_EXHAUSTIVE if exhaustive else 0, ptr(out[0]), ptr(out[1]), ptr(out[2]), stream_ptr()),
        "fgc_closest_point_tree"))
    dist = torch.sqrt(d2)
    return (dist, face, bary) if want_bary else (dist, face)


def closest_point(verts, faces, points, want_bary=False):
    """closest_point_tree without a tree (include/fgc.h: fgc_closest_point; a build extension), over all points x faces
    pairs: verts [V,3] fp32, faces int [F,3] (a row with an id outside [0, V) takes no part), points [Q,3].  The same
    returns, bit for bit what closest_point_tree gives on a tree of the same mesh.  For a mesh that changes with every
    call and a few hundred points; anything larger wants the tree."""
    _req_cuda(verts, faces, points)
    verts, points = _f32c(verts.reshape(-1, 3)), _f32c(points.reshape(-1, 3))
    faces = faces.to(torch.int32).reshape(-1, 3).contiguous()
    nv, nf, nq = verts.shape[0], faces.shape[0], points.shape[0]
    L = _lib.lib()
    nbytes = L.fgc_closest_point_workspace_bytes(nf, nq)
    if nbytes == 0 or nv == 0:
        raise ValueError("closest_point needs at least one vertex, one face and one point (got %d, %d, %d)" % (nv, nf, nq))
    d2 = torch.empty(nq, dtype=torch.float32, device=verts.device)
    face = torch.empty(nq, dtype=torch.int32, device=verts.device)
    bary = torch.empty(nq, 2, dtype=torch.float32, device=verts.device) if want_bary else None
    ws = _workspace(nbytes, verts.device, "closest_point")
    check(L.fgc_closest_point(ptr(verts), nv, ptr(faces), nf, ptr(points), nq, ptr(d2), ptr(face), ptr(bary), ptr(ws),
                              ws.numel(), stream_ptr()), "fgc_closest_point")
    dist = torch.sqrt(d2)
    return (dist, face, bary) if want_bary else (dist, face)


def pool4_avg_iz(x):
    """custom_binary_tree_pooling(x, steps=2, 'avg_ignore_zeros') (model.py:792-814) on [n, c] rows."""
    _req_cuda(x)
    x = _f32c(x)
    n, c = x.shape
    y = torch.empty(n // 4, c, dtype=torch.float32, device=x.device)
    check(_lib.lib().fgc_pool4_avg_iz(ptr(x), n, c, ptr(y), stream_ptr()), "fgc_pool4_avg_iz")
    return y


def face_centers(x, faces):
    """Barycentres of faces [n0,3] (int, -1 = fake) of the vertices x [V,3] (train.py:1779-1787)."""
    _req_cuda(x, faces)
    x = _f32c(x)
    faces = faces.to(torch.int32).contiguous()
    out = torch.empty(faces.shape[0], 3, dtype=torch.float32, device=x.device)
    check(_lib.lib().fgc_face_centers(ptr(x), x.shape[0], ptr(faces), faces.shape[0], ptr(out), stream_ptr()),
          "fgc_face_centers")
    return out


def vertex_update_ms(x, normals, faces, v_faces, iters=(80, 20, 20)):
    """update_position_MS (train.py:1668-1798), coarsening_steps = 2.  x [V,3]; normals = [n0 [N0,3], n1 [N0/4,3],
    n2 [N0/16,3]]; faces int [N0,3] (-1 rows = fake nodes); v_faces int [V,K].  Returns (x_out [V,3], dx [3,V,3])."""
    return _ms_forward(x, normals, faces, v_faces, iters)


def pack_cells(ijk):
    """int [n,3] cell coordinates (0 <= c < 512; a row with any negative entry = in no cell) -> the packed int32 cells of
    fgc_nn_query, (i << 20) | (j << 10) | k, or -1."""
    ijk = np.asarray(ijk, dtype=np.int64).reshape(-1, 3)
    if (ijk >= 512).any():
        raise ValueError("cell coordinates must be < 512")
    packed = (ijk[:, 0] << 20) | (ijk[:, 1] << 10) | ijk[:, 2]
    return np.where((ijk < 0).any(1), -1, packed).astype(np.int32)


def nn_query(q, p, q_cell=None, p_cell=None):
    """Nearest point of p [np,3] for every query q [nq,3] (fp32 GPU tensors; include/fgc.h: fgc_nn_query): (dist [nq]
    float32, idx [nq] int32), ties to the lowest index.  With q_cell / p_cell (int32 [nq] / [np], packed by pack_cells)
    only the 2x2x2 candidate cells of a query's cell count; no candidate: (+inf, -1)."""
    _req_cuda(q, p, q_cell, p_cell)
    q, p = _f32c(q.reshape(-1, 3)), _f32c(p.reshape(-1, 3))
    if (q_cell is None) != (p_cell is None):
        raise ValueError("q_cell and p_cell go together")
    if q_cell is not None:
        q_cell = q_cell.to(torch.int32).contiguous()
        p_cell = p_cell.to(torch.int32).contiguous()
        if q_cell.numel() != q.shape[0] or p_cell.numel() != p.shape[0]:
            raise ValueError("one cell per point")
    nq, n_p = q.shape[0], p.shape[0]
    dist = torch.empty(nq, dtype=torch.float32, device=q.device)
    idx = torch.empty(nq, dtype=torch.int32, device=q.device)
    nbytes = _lib.lib().fgc_nn_workspace_bytes(nq, n_p)
    ws = _workspace(nbytes, q.device, "nn")
    check(_lib.lib().fgc_nn_query(ptr(q), nq, ptr(p), n_p, ptr(q_cell), ptr(p_cell), ptr(dist), ptr(idx), ptr(ws),
                                  ws.numel(), stream_ptr()), "fgc_nn_query")
    return dist, idx


def guidance_normals(normals, areas, ring, fe, want_pick=False, want_h=False):
    """Guidance normals of guided normal filtering (include/fgc.h: fgc_guided_normals; a build extension) on GPU tensors:
    normals [n,3] and areas [n] fp32, ring int32 [n, ld] (utils.face_rings), fe int32 [n,3] (utils.face_edge_neighbours).
    Returns G [n,3], or (G, pick int32 [n] and / or H [n]) when asked for them."""
    _req_cuda(normals, areas, ring, fe)
    normals, areas = _f32c(normals.reshape(-1, 3)), _f32c(areas.reshape(-1))
    n = normals.shape[0]
    ring, fe = ring.to(torch.int32).contiguous(), fe.to(torch.int32).contiguous()
    if areas.numel() != n or ring.dim() != 2 or ring.shape[0] != n or tuple(fe.shape) != (n, 3):
        raise ValueError("normals [n,3], areas [n], ring [n, ld] and fe [n,3] must have one row per face")
    ld = ring.shape[1]
    guide = torch.empty(n, 3, dtype=torch.float32, device=normals.device)
    pick = torch.empty(n, dtype=torch.int32, device=normals.device) if want_pick else None
    h = torch.empty(n, dtype=torch.float32, device=normals.device) if want_h else None
    nbytes = _lib.lib().fgc_guided_workspace_bytes(n, ld)
    if nbytes == 0:
        raise ValueError("ring [%d, %d]: at least one face, ld a multiple of 4 in 4 .. 64" % (n, ld))
    ws = _workspace(nbytes, normals.device, "guided")
    check(_lib.lib().fgc_guided_normals(ptr(normals), ptr(areas), n, ptr(ring), ld, ptr(fe), ptr(guide), ptr(pick), ptr(h),
                                        ptr(ws), ws.numel(), stream_ptr()), "fgc_guided_normals")
    extra = tuple(t for t in (pick, h) if t is not None)
    return (guide,) + extra if extra else guide


def bilateral_filter(centres, normals, areas, sigma_s, sigma_r, cell_order, cell_ptr, grid, guide=None):
    """Bilateral normal filter (include/fgc.h: fgc_bilateral_filter) on fp32 GPU tensors: centres [n,3], normals [n,3],
    areas [n]; sigma_s and sigma_r a number or a sequence each (sigma_r = -1: no range term); cell_order int32 [n] and
    cell_ptr int32 [sx sy sz + 1] the faces ordered by cell and the range table (utils.bilateral_order), grid =
    (sx, sy, sz).  Returns [n, 3 S R]: the filtered unit normal of every (sigma_s, sigma_r) pair, sigma_s-major, all
    pairs from one pass over the candidates.  A face in no cell gets a zero row.  guide [n,3] (optional): the range term
    reads these normals instead of `normals` (fgc_bilateral_filter_guided; None: the plain filter, no other launch)."""
    from .utils import BILATERAL_MAX_SLICES
    _req_cuda(centres, normals, areas, cell_order, cell_ptr)
    centres, normals = _f32c(centres.reshape(-1, 3)), _f32c(normals.reshape(-1, 3))
    areas = _f32c(areas.reshape(-1))
    n = centres.shape[0]
    if normals.shape[0] != n or areas.numel() != n:
        raise ValueError("centres, normals and areas must have one row per face")
    sx, sy, sz = (int(g) for g in grid)
    if min(sx, sy, sz) < 1 or max(sx, sy, sz) > BILATERAL_MAX_SLICES:
        raise ValueError("grid %s: 1 .. %d cells per axis" % ((sx, sy, sz), BILATERAL_MAX_SLICES))
    cell_order = cell_order.to(torch.int32).contiguous()
    cell_ptr = cell_ptr.to(torch.int32).contiguous()
    if cell_order.numel() != n or cell_ptr.numel() != sx * sy * sz + 1:
        raise ValueError("cell_order must have n entries and cell_ptr sx * sy * sz + 1")
    ss = np.atleast_1d(np.asarray(sigma_s, dtype=np.float32)).ravel()
    sr = np.atleast_1d(np.asarray(sigma_r, dtype=np.float32)).ravel()
    out = torch.empty(n, 3 * ss.size * sr.size, dtype=torch.float32, device=centres.device)
    nbytes = _lib.lib().fgc_bilateral_workspace_bytes(n, sx, sy, sz)
    ws = _workspace(nbytes, centres.device, "bilateral")
    if guide is not None:
        _req_cuda(guide)
        guide = _f32c(guide.reshape(-1, 3))
        if guide.shape[0] != n:
            raise ValueError("guide must have one row per face")
        check(_lib.lib().fgc_bilateral_filter_guided(ptr(centres), ptr(normals), ptr(areas), n, ptr(cell_order),
                                                     ptr(cell_ptr), sx, sy, sz, ss.ctypes.data, ss.size, sr.ctypes.data,
                                                     sr.size, ptr(guide), ptr(out), ptr(ws), ws.numel(), stream_ptr()),
              "fgc_bilateral_filter_guided")
        return out
    check(_lib.lib().fgc_bilateral_filter(ptr(centres), ptr(normals), ptr(areas), n, ptr(cell_order), ptr(cell_ptr), sx, sy,
                                          sz, ss.ctypes.data, ss.size, sr.ctypes.data, sr.size, ptr(out), ptr(ws),
                                          ws.numel(), stream_ptr()), "fgc_bilateral_filter")
    return out


def vertex_ms_tables(faces, v_faces, nv):
    """The two inverse tables of fgc_vertex_update_ms_bwd, built once per mesh on the host (int32 numpy):
    (slot_ptr [N0+1], slot_vert) - for every fine node f the vertices whose slots name f, in (vertex, slot) order - and
    (inc_ptr [nv+1], inc_face) - for every vertex the faces that name it as a corner, in (face, corner) order."""
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    v_faces = np.asarray(v_faces).reshape(nv, -1).astype(np.int64)
    n0 = faces.shape[0]
    flat = v_faces.reshape(-1)
    ok = (flat >= 0) & (flat < n0)
    f = flat[ok]
    v = np.repeat(np.arange(nv), v_faces.shape[1])[ok]
    order = np.argsort(f, kind="stable")
    slot_vert = v[order].astype(np.int32)
    slot_ptr = np.concatenate([[0], np.cumsum(np.bincount(f, minlength=n0))]).astype(np.int32)
    corners = faces.reshape(-1)
    ok = (corners >= 0) & (corners < nv)
    vv = corners[ok]
    ff = np.repeat(np.arange(n0), 3)[ok]
    order = np.argsort(vv, kind="stable")
    inc_face = ff[order].astype(np.int32)
    inc_ptr = np.concatenate([[0], np.cumsum(np.bincount(vv, minlength=nv))]).astype(np.int32)
    return slot_ptr, slot_vert, inc_ptr, inc_face


def _ms_args(x, normals, faces, v_faces):
    _req_cuda(x, faces, v_faces, *normals)
    x = _f32c(x.reshape(-1, 3))
    n0, n1, n2 = (_f32c(t.reshape(-1, 3)) for t in normals)
    faces = faces.to(torch.int32).contiguous()
    v_faces = v_faces.to(torch.int32).reshape(x.shape[0], -1).contiguous()
    N0 = faces.shape[0]
    if n0.shape[0] != N0 or n1.shape[0] * 4 != N0 or n2.shape[0] * 16 != N0:
        raise ValueError("normals must have N0, N0/4 and N0/16 rows (N0 = %d)" % N0)
    return x, (n0, n1, n2), faces, v_faces


def ray_rows(dirs, nv, device, name="dirs"):
    """Rows of rays ([V,3] or [1,3]; tensor or array-like) as the contiguous fp32 rows on `device` that the *_dir entry
    points read: one row, or one per vertex.  name: what the caller calls them, for the message."""
    if not isinstance(dirs, torch.Tensor):
        dirs = torch.from_numpy(np.ascontiguousarray(np.asarray(dirs, dtype=np.float32)))
    dirs = _f32c(dirs.to(device).reshape(-1, 3))
    if dirs.shape[0] not in (1, nv):
        raise ValueError("%s has %d rows: one row, or one per vertex (%d)" % (name, dirs.shape[0], nv))
    return dirs


def _given(dirs):
    if dirs is None:      # (None selects the free form in the two helpers below: not through a *_dir function)
        raise ValueError("dirs is None: the free update is vertex_update_ms")
    return dirs


def _ms_forward(x, normals, faces, v_faces, iters, dirs=None, traj=False, return_t=False):
    """The four forward entry points of the multi-scale update: free (dirs None) or along dirs, the plain form -> (x_out,
    dx) or, traj, the trajectory form -> traj [T+1, V, 3]; return_t (along dirs): t [V] appended."""
    x, (n0, n1, n2), faces, v_faces = _ms_args(x, normals, faces, v_faces)
    nv, N0 = x.shape[0], faces.shape[0]
    L = _lib.lib()
    f32 = dict(dtype=torch.float32, device=x.device)
    it = (C.c_int32 * 3)(*[int(i) for i in iters])
    mesh = (nv, ptr(faces), N0, ptr(v_faces), v_faces.shape[1], ptr(n0), ptr(n1), ptr(n2), it)
    nscr = 3 * (N0 + N0 // 4 + N0 // 16) + (0 if traj else 6 * nv)
    rays = t_arg = ()
    t = None
    if dirs is not None:
        dirs = ray_rows(dirs, nv, x.device)
        t = torch.empty(nv, **f32) if return_t else None
        rays, t_arg = (ptr(dirs), dirs.shape[0]), (ptr(t),)
        nscr = L.fgc_vertex_update_ms_dir_scratch_floats(nv, N0)
    scr = torch.empty(nscr, **f32)
    tail = (ptr(scr), scr.numel(), stream_ptr())
    if traj:
        res = (torch.empty(sum(int(i) for i in iters) + 1, nv, 3, **f32),)
        args = (ptr(x),) + mesh + rays + (ptr(res[0]), res[0].numel()) + t_arg + tail
    else:
        res = (torch.empty_like(x), torch.empty(3, nv, 3, **f32))
        args = (ptr(x), ptr(res[0])) + mesh + rays + t_arg + (ptr(res[1]),) + tail
    name = "fgc_vertex_update_ms" + ("_dir" if dirs is not None else "") + ("_traj" if traj else "")
    check(getattr(L, name)(*args), name)
    if return_t:
        res += (t,)
    return res[0] if len(res) == 1 else res


def _ms_backward(traj, normals, faces, v_faces, g_out, iters, tables, dirs=None):
    """The two adjoint entry points of the multi-scale update, free (dirs None) or along dirs: (dL/dx [V,3], [dL/dn0,
    dL/dn1, dL/dn2])."""
    form = "_dir" if dirs is not None else ""
    nv = traj.shape[1]
    if traj.dtype != torch.float32 or not traj.is_contiguous():
        raise ValueError("traj must be the contiguous float32 [T+1, V, 3] of vertex_update_ms%s_traj" % form)
    _, (n0, n1, n2), faces, v_faces = _ms_args(traj[0], normals, faces, v_faces)
    rays = ()
    if dirs is not None:
        dirs = ray_rows(dirs, nv, traj.device)
        rays = (ptr(dirs), dirs.shape[0])
    _req_cuda(g_out)
    g_out = _f32c(g_out.reshape(nv, 3))
    N0 = faces.shape[0]
    if tables is None:
        tables = [torch.as_tensor(t, device=traj.device)
                  for t in vertex_ms_tables(faces.cpu().numpy(), v_faces.cpu().numpy(), nv)]
    sp, sv, ip, fi = tables
    g_x = torch.empty(nv, 3, dtype=torch.float32, device=traj.device)
    g_n = [torch.empty_like(t) for t in (n0, n1, n2)]
    L = _lib.lib()
    name = "fgc_vertex_update_ms%s_bwd" % form
    ws = _workspace(getattr(L, name + "_workspace_floats")(nv, N0) * 4, traj.device, "vms%s_bwd" % form)
    it = (C.c_int32 * 3)(*[int(i) for i in iters])
    check(getattr(L, name)(ptr(traj), traj.numel(), nv, ptr(faces), N0, ptr(v_faces), v_faces.shape[1], ptr(n0), ptr(n1),
                           ptr(n2), it, *rays, ptr(sp), ptr(sv), ptr(ip), ptr(fi), ptr(g_out), ptr(g_x), ptr(g_n[0]),
                           ptr(g_n[1]), ptr(g_n[2]), ptr(ws), ws.numel() // 4, stream_ptr()), name)
    return g_x, g_n


def vertex_update_ms_traj(x, normals, faces, v_faces, iters=(80, 20, 20)):
    """vertex_update_ms keeping every iterate: traj [T+1, V, 3] (traj[0] = x, traj[-1] = vertex_update_ms's x_out, bit
    for bit; include/fgc.h: fgc_vertex_update_ms_traj)."""
    return _ms_forward(x, normals, faces, v_faces, iters, traj=True)


def vertex_update_ms_bwd(traj, normals, faces, v_faces, g_out, iters=(80, 20, 20), tables=None):
    """Adjoint of vertex_update_ms (include/fgc.h: fgc_vertex_update_ms_bwd): given the trajectory of
    vertex_update_ms_traj and g_out = dL/dx_out [V,3], returns (dL/dx [V,3], [dL/dn0, dL/dn1, dL/dn2]).  tables: the
    device tensors of vertex_ms_tables (built here when None)."""
    return _ms_backward(traj, normals, faces, v_faces, g_out, iters, tables)


def vertex_update_ms_dir(x, normals, faces, v_faces, dirs, iters=(80, 20, 20), return_t=False):
    """vertex_update_ms with every iteration's step projected onto the vertex' direction, dirs [V,3] or [1,3] (used as
    given; rows longer than 1 can diverge) - a build extension, include/fgc.h: fgc_vertex_update_ms_dir.  Returns
    (x_out [V,3], dx [3,V,3]); return_t: (x_out, dx, t [V]), t the signed step along the direction, x_out = fma(t, dirs,
    x)."""
    return _ms_forward(x, normals, faces, v_faces, iters, _given(dirs), return_t=return_t)


def vertex_update_ms_dir_traj(x, normals, faces, v_faces, dirs, iters=(80, 20, 20), return_t=False):
    """vertex_update_ms_dir keeping every iterate: traj [T+1, V, 3] (traj[0] = x, traj[-1] = vertex_update_ms_dir's x_out,
    bit for bit; include/fgc.h: fgc_vertex_update_ms_dir_traj); return_t: (traj, t [V])."""
    return _ms_forward(x, normals, faces, v_faces, iters, _given(dirs), traj=True, return_t=return_t)


def vertex_update_ms_dir_bwd(traj, normals, faces, v_faces, dirs, g_out, iters=(80, 20, 20), tables=None):
    """Adjoint of vertex_update_ms_dir (include/fgc.h: fgc_vertex_update_ms_dir_bwd): given the trajectory of
    vertex_update_ms_dir_traj and g_out = dL/dx_out [V,3], returns (dL/dx [V,3], [dL/dn0, dL/dn1, dL/dn2]); no gradient
    with respect to dirs.  tables: the device tensors of vertex_ms_tables (built here when None)."""
    return _ms_backward(traj, normals, faces, v_faces, g_out, iters, tables, _given(dirs))


def point_loss(p0, p1, sample_ind0, sample_ind1, threshold=5000.0, want_grad=True):
    """fullLoss (train.py:1373-1424; include/fgc.h: fgc_point_loss) of the points p0 [n0,3] against p1 [n1,3] on the
    sampled rows: (loss [1], dloss/dp0 [n0,3] or None)."""
    _req_cuda(p0, p1, sample_ind0, sample_ind1)
    p0, p1 = _f32c(p0.reshape(-1, 3)), _f32c(p1.reshape(-1, 3))
    i0 = sample_ind0.to(torch.int32).reshape(-1).contiguous()
    i1 = sample_ind1.to(torch.int32).reshape(-1).contiguous()
    loss = torch.empty(1, dtype=torch.float32, device=p0.device)
    g = torch.empty_like(p0) if want_grad else None
    nbytes = _lib.lib().fgc_point_loss_workspace_bytes(p0.shape[0], p1.shape[0], i0.numel(), i1.numel())
    ws = _workspace(nbytes, p0.device, "point_loss")
    check(_lib.lib().fgc_point_loss(ptr(p0), p0.shape[0], ptr(p1), p1.shape[0], ptr(i0), i0.numel(), ptr(i1), i1.numel(),
                                    float(threshold), ptr(loss), ptr(g), ptr(ws), ws.numel(), stream_ptr()),
          "fgc_point_loss")
    return loss, g


POINT_LOSS_MAX_TERMS = 16384  # FGC_POINT_LOSS_MAX_SAMPLES of include/fgc.h


def surface_loss(p0, faces0, p1, faces1, sample_ind0, sample_ind1, threshold=5000.0, want_grad=True):
    """The two-sided point-to-surface loss (include/fgc.h: fgc_surface_loss; a build extension) of the mesh (p0 [n0,3],
    faces0 int [F0,3], -1 rows allowed) against the mesh (p1 [n1,3], faces1 int [F1,3]) on the sampled rows of p0 and p1:
    (loss [1], dloss/dp0 [n0,3] or None).  fullLoss's scale; the two meshes need share nothing."""
    _req_cuda(p0, faces0, p1, faces1, sample_ind0, sample_ind1)
    p0, p1 = _f32c(p0.reshape(-1, 3)), _f32c(p1.reshape(-1, 3))
    f0 = faces0.to(torch.int32).reshape(-1, 3).contiguous()
    f1 = faces1.to(torch.int32).reshape(-1, 3).contiguous()
    i0 = sample_ind0.to(torch.int32).reshape(-1).contiguous()
    i1 = sample_ind1.to(torch.int32).reshape(-1).contiguous()
    L = _lib.lib()
    nbytes = L.fgc_surface_loss_workspace_bytes(f0.shape[0], f1.shape[0], i0.numel(), i1.numel())
    if nbytes == 0 or p0.shape[0] == 0 or p1.shape[0] == 0:
        raise ValueError("surface_loss needs vertices, faces and samples on both sides, and at most %d terms "
                         "(got %d + 3 x %d samples)" % (POINT_LOSS_MAX_TERMS, i0.numel(), i1.numel()))
    loss = torch.empty(1, dtype=torch.float32, device=p0.device)
    g = torch.empty_like(p0) if want_grad else None
    ws = _workspace(nbytes, p0.device, "surface_loss")
    check(L.fgc_surface_loss(ptr(p0), p0.shape[0], ptr(f0), f0.shape[0], ptr(p1), p1.shape[0], ptr(f1), f1.shape[0], ptr(i0),
                             i0.numel(), ptr(i1), i1.numel(), float(threshold), ptr(loss), ptr(g), ptr(ws), ws.numel(),
                             stream_ptr()), "fgc_surface_loss")
    return loss, g


def dense_normals_loss(fn, gt, R=None, g=None, dloss=1.0, want_grad=True):
    """faceNormalsLoss (train.py:1272-1294) over ALL rows of fn [n,3] against the ground truth gt [n,3] rotated by R
    (3x3 array-like or device tensor; None = identity) on the fly (include/fgc.h: fgc_dense_normals_loss_fwd / _bwd).
    Returns (loss [2] = {loss in degrees, real rows}, g): the gradient dloss * dL/dfn is ADDED to g [n,3] (a zero tensor
    when g is None); g is None when want_grad is False."""
    _req_cuda(fn, gt)
    fn, gt = _f32c(fn.reshape(-1, 3)), _f32c(gt.reshape(-1, 3))
    n = fn.shape[0]
    if gt.shape[0] != n:
        raise ValueError("fn has %d rows, gt %d" % (n, gt.shape[0]))
    if R is not None:
        if not isinstance(R, torch.Tensor) or not R.is_cuda:
            R = torch.as_tensor(np.asarray(R, dtype=np.float32).reshape(9)).to(fn.device)
        R = R.reshape(9).float().contiguous()
    L = _lib.lib()
    nsc = L.fgc_dense_normals_loss_scratch_floats(n)
    scr = torch.empty(max(nsc, 1), dtype=torch.float32, device=fn.device)
    loss = torch.empty(2, dtype=torch.float32, device=fn.device)
    check(L.fgc_dense_normals_loss_fwd(ptr(fn), ptr(gt), ptr(R), n, ptr(loss), None, None, ptr(scr), nsc, stream_ptr()),
          "fgc_dense_normals_loss_fwd")
    if not want_grad:
        return loss, None
    if g is None:
        g = torch.zeros_like(fn)
    elif g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != 3 * n or g.device != fn.device:
        raise ValueError("g must be a contiguous float32 [n,3] tensor on the device of fn (it is accumulated into)")
    check(L.fgc_dense_normals_loss_bwd(ptr(fn), ptr(gt), ptr(R), n, ptr(scr), nsc, float(dloss), ptr(g), stream_ptr()),
          "fgc_dense_normals_loss_bwd")
    return loss, g


def noise_words(step, sigma):
    """The three control words of the noise synthesis (include/fgc.h: fgc_synth_noise) as uint32 numpy: step low, step
    high, FGC_SYNTH_ON | float bits of sigma.  sigma None: three zeros, synthesis off."""
    if sigma is None:
        return np.zeros(3, dtype=np.uint32)
    sigma = np.float32(sigma)
    if not np.isfinite(sigma) or sigma < 0:
        raise ValueError("sigma must be finite and >= 0 (got %r)" % (sigma,))
    step = int(step)
    if not 0 <= step < 1 << 64:
        raise ValueError("step must fit 64 bits")
    bits = int(np.array([sigma], dtype=np.float32).view(np.uint32)[0]) & 0x7FFFFFFF      # (-0.0 -> 0.0)
    return np.array([step & 0xFFFFFFFF, step >> 32, bits | _lib.SYNTH_ON], dtype=np.uint32)


def _synth_prologue(verts, tables, row, step, sigma, ctl, out, scratch, scratch_floats):
    """What the three noise calls share: verts as contiguous float32 [V,3]; the per-vertex tables (None stays None) the same
    and refused unless each has V rows ("one <row> per vertex"); the control words of (step, sigma) on the device unless ctl
    is given; the output; a scratch of scratch_floats(V) floats unless one is given.
    Returns (verts, V, tables, ctl, out, scratch)."""
    verts = _f32c(verts.reshape(-1, 3))
    nv = verts.shape[0]
    tables = [None if t is None else _f32c(t.reshape(-1, 3)) for t in tables]
    if any(t is not None and t.shape[0] != nv for t in tables):
        raise ValueError("one %s per vertex" % row)
    if ctl is None:
        ctl = torch.from_numpy(noise_words(step, sigma).view(np.int32)).to(verts.device)
    if out is None:
        out = torch.empty_like(verts)
    if scratch is None:
        scratch = torch.empty(max(scratch_floats(nv), 1), dtype=torch.float32, device=verts.device)
    return verts, nv, tables, ctl, out, scratch


def synth_noise(verts, sigma, step, seed=0, stream=0, normals=None, out=None, scratch=None, ctl=None):
    """Build extension (include/fgc.h: fgc_synth_noise): the vertices verts [V,3] displaced by Philox4x32-10 Gaussian noise
    of standard deviation sigma - along a random direction, or along `normals` [V,3] (unit vertex normals) - for the
    64-bit counter `step`, the 64-bit `seed` and the 32-bit `stream` id.  Returns the displaced vertices [V,3] (`out`).
    ctl: the control words already on the device (int32 [3]) instead of (step, sigma); scratch: float32, at least
    fgc_synth_scratch_floats(V) - it receives the bounding-box partials face_features_rows(have_bbox=True) reads."""
    _req_cuda(verts, normals, out, scratch, ctl)
    verts, nv, (normals,), ctl, out, scratch = _synth_prologue(verts, (normals,), "normal", step, sigma, ctl, out, scratch,
                                                               _lib.lib().fgc_synth_scratch_floats)
    check(_lib.lib().fgc_synth_noise(ptr(verts), ptr(normals), nv, ptr(ctl), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                     int(stream) & 0xFFFFFFFF, ptr(out), ptr(scratch), scratch.numel(), stream_ptr()),
          "fgc_synth_noise")
    return out


def sensor_words(power, r_ref, q):
    """The four control words of the depth-sensor model (include/fgc.h: fgc_synth_noise_sensor) as uint32 numpy:
    FGC_SYNTH_ON | power, float bits of r_ref, float bits of q, 0.  power None: four zeros, the model off (plain noise along
    the rays).  Refused here, as the kernel switches them off: a power outside 0, 1, 2, an r_ref that is not a positive
    normal finite float, a q that is neither 0 nor a positive normal finite float."""
    if power is None:
        return np.zeros(4, dtype=np.uint32)
    if isinstance(power, (bool, np.bool_)) or int(power) != power or int(power) not in (0, 1, 2):
        raise ValueError("sensor: power must be 0, 1 or 2 (got %r)" % (power,))
    tiny = np.finfo(np.float32).tiny
    with np.errstate(over="ignore"):
        r_ref, q = np.float32(r_ref), np.float32(q)
    if not (np.isfinite(r_ref) and r_ref >= tiny):
        raise ValueError("sensor: the reference range must be finite and > 0 (got %r)" % (r_ref,))
    if not (np.isfinite(q) and (q == 0 or q >= tiny)):
        raise ValueError("sensor: the disparity step q must be finite and >= 0 (got %r)" % (q,))
    bits = np.array([r_ref, abs(q)], dtype=np.float32).view(np.uint32)
    return np.array([int(power) | _lib.SYNTH_ON, int(bits[0]), int(bits[1]), 0], dtype=np.uint32)


def sensor_camera(camera):
    c = np.asarray(camera, dtype=np.float64).reshape(-1)
    if c.shape != (3,) or not np.isfinite(c).all() or not np.isfinite(c.astype(np.float32)).all():
        raise ValueError("camera must be three finite numbers (got %r)" % (camera,))
    return np.ascontiguousarray(c.astype(np.float32))


def synth_noise_sensor(verts, rays, camera, sigma, step, power, r_ref, q, seed=0, stream=0, out=None, scratch=None, ctl=None,
                       sensor_ctl=None):
    """Build extension (include/fgc.h: fgc_synth_noise_sensor): synth_noise(verts, sigma, step, seed, stream, normals=rays)
    under the depth-sensor model - sigma is the standard deviation at range r_ref from `camera` and grows with
    (range / r_ref)^power, power 0, 1 or 2; q > 0 puts every range on the lattice 1 / (k q).  rays [V,3]: the unit viewing
    rays (required).  ctl / sensor_ctl: the control words already on the device (int32 [3] / [4]) instead of (step, sigma) /
    (power, r_ref, q); scratch as for synth_noise.  Returns the displaced vertices [V,3] (`out`)."""
    if rays is None:
        raise ValueError("the sensor model needs the table of viewing rays: rays is required")
    _req_cuda(verts, rays, out, scratch, ctl, sensor_ctl)
    verts, nv, (rays,), ctl, out, scratch = _synth_prologue(verts, (rays,), "ray", step, sigma, ctl, out, scratch,
                                                            _lib.lib().fgc_synth_scratch_floats)
    cam = sensor_camera(camera)
    if sensor_ctl is None:
        sensor_ctl = torch.from_numpy(sensor_words(power, r_ref, q).view(np.int32)).to(verts.device)
    check(_lib.lib().fgc_synth_noise_sensor(ptr(verts), ptr(rays), nv, ptr(ctl), ptr(sensor_ctl), cam.ctypes.data,
                                            int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF, ptr(out), ptr(scratch),
                                            scratch.numel(), stream_ptr()), "fgc_synth_noise_sensor")
    return out


def lf_words(amplitude, width):
    """The four control words of the low-frequency noise (include/fgc.h: fgc_synth_noise_lf) as uint32 numpy:
    FGC_SYNTH_ON | float bits of the amplitude, float bits of the width, 0, 0 - both ABSOLUTE, in mesh units.  amplitude
    None: four zeros, bumps off."""
    if amplitude is None:
        return np.zeros(4, dtype=np.uint32)
    amplitude, width = np.float32(amplitude), np.float32(width)
    if not np.isfinite(amplitude) or amplitude < 0:
        raise ValueError("amplitude must be finite and >= 0 (got %r)" % (amplitude,))
    if not np.isfinite(width) or width <= 0:
        raise ValueError("width must be finite and > 0 (got %r)" % (width,))
    bits = np.array([amplitude, width], dtype=np.float32).view(np.uint32)
    return np.array([(int(bits[0]) & 0x7FFFFFFF) | _lib.SYNTH_ON, int(bits[1]), 0, 0], dtype=np.uint32)


def lf_amplitude(lf_level, edge_len, width, bumps, area):
    """The bump amplitude A for a target RMS displacement of lf_level mean edge lengths: K bumps of absolute width w on a
    surface of `area` give, as planar shot noise, the variance A^2 (K / area) pi w^2, so
    A = lf_level * edge_len / sqrt(max(1, K pi w^2 / area)); with less than one bump per pi w^2 the PEAK is held at the
    level instead."""
    density = float(bumps) * np.pi * float(width) ** 2 / float(area)
    return float(lf_level) * float(edge_len) / np.sqrt(max(1.0, density))


def lf_plan(verts, faces, edge_len, width_rel=3.0, bumps=None):
    """What bind_clean(lf=(width_rel, bumps)) and makeNoisy derive from a clean mesh (host arrays; faces: the REAL faces):
    (K, absolute width, total area) - K = bumps, or ceil(faces / 6), the count of the reference's addLFGaussianNoise
    stub; width = width_rel mean edge lengths; the area in float64."""
    if not (np.isfinite(width_rel) and width_rel > 0):
        raise ValueError("lf: the width must be a positive number of mean edge lengths (got %r)" % (width_rel,))
    faces = np.asarray(faces).reshape(-1, 3)
    K = int(bumps) if bumps is not None else -(-faces.shape[0] // 6)
    if not 1 <= K <= _lib.SYNTH_LF_MAX_BUMPS:
        raise ValueError("lf: %d bumps (1 ... %d)" % (K, _lib.SYNTH_LF_MAX_BUMPS))
    p = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    area = 0.5 * np.linalg.norm(np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]]), axis=1).sum()
    if not area > 0:
        raise ValueError("lf: the clean mesh has no area")
    return K, float(width_rel) * float(edge_len), float(area)


def synth_noise_lf(verts, normals, sigma, step, amplitude, width, bumps, seed=0, stream=0, white_normals=None, out=None,
                   scratch=None, ctl=None, lf_ctl=None):
    """Build extension (include/fgc.h: fgc_synth_noise_lf): synth_noise(verts, sigma, step, seed, stream, white_normals)
    plus a smooth field of `bumps` Gaussian bumps of absolute `amplitude` and `width`, centred on random clean vertices,
    along the unit vertex `normals` [V,3] (required).  ctl / lf_ctl: the control words already on the device (int32 [3] /
    [4]) instead of (step, sigma) / (amplitude, width); scratch: float32, at least fgc_synth_lf_scratch_floats(V, bumps) -
    its head receives the bounding-box partials face_features_rows(have_bbox=True) reads."""
    if normals is None:
        raise ValueError("the bumps go along the vertex normals: normals is required")
    _req_cuda(verts, normals, white_normals, out, scratch, ctl, lf_ctl)
    bumps = int(bumps)      # (the library refuses a count outside 1 ... FGC_SYNTH_LF_MAX_BUMPS and a stream >= 2^31)
    verts, nv, (normals, white_normals), ctl, out, scratch = _synth_prologue(
        verts, (normals, white_normals), "normal", step, sigma, ctl, out, scratch,
        lambda nv: _lib.lib().fgc_synth_lf_scratch_floats(nv, bumps))
    if lf_ctl is None:
        lf_ctl = torch.from_numpy(lf_words(amplitude, width).view(np.int32)).to(verts.device)
    check(_lib.lib().fgc_synth_noise_lf(ptr(verts), ptr(normals), ptr(white_normals), nv, ptr(ctl), ptr(lf_ctl), bumps,
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF, ptr(out), ptr(scratch),
                                        scratch.numel(), stream_ptr()), "fgc_synth_noise_lf")
    return out


def point_sets_prepare(v, gt, R=None, gt_box=None, scratch=None, have_bbox=False, out=None):
    """Build extension (include/fgc.h: fgc_point_sets_prepare): the displaced vertices v [V,3] and the ground-truth
    vertices gt [Vgt,3] (raw units) divided by the bounding-box diagonal of their union and rotated by R (3x3 array-like or
    device tensor; None: no rotation) - bit-identical to utils.normalizePointSets(v, gt) followed by rotate_rows.
    Returns (v_out [V,3], gt_out [Vgt,3]) (`out`: the pair to write into).  gt_box: float32 [6] on the device, {min xyz,
    max xyz} of gt (computed here when None); have_bbox: `scratch` holds the bounding-box partials synth_noise has just
    left for v."""
    _req_cuda(v, gt, gt_box, scratch, *(out or ()))
    v, gt = _f32c(v.reshape(-1, 3)), _f32c(gt.reshape(-1, 3))
    nv, ngt = v.shape[0], gt.shape[0]
    if R is not None:
        if not isinstance(R, torch.Tensor) or not R.is_cuda:
            R = torch.as_tensor(np.asarray(R, dtype=np.float32).reshape(9)).to(v.device)
        R = R.reshape(9).float().contiguous()
    if gt_box is None:
        if ngt == 0:
            raise ValueError("no ground-truth vertices")
        gt_box = torch.cat([gt.min(0).values, gt.max(0).values])
    gt_box = _f32c(gt_box.reshape(6))
    v_out, gt_out = out if out is not None else (torch.empty_like(v), torch.empty_like(gt))
    need = _lib.lib().fgc_synth_scratch_floats(nv)
    if scratch is None:
        if have_bbox:
            raise ValueError("have_bbox needs the scratch synth_noise filled")
        scratch = torch.empty(max(need, 1), dtype=torch.float32, device=v.device)
    check(_lib.lib().fgc_point_sets_prepare(ptr(v), nv, ptr(gt), ngt, ptr(gt_box), ptr(R), 1 if have_bbox else 0, ptr(v_out),
                                            ptr(gt_out), ptr(scratch), scratch.numel(), stream_ptr()),
          "fgc_point_sets_prepare")
    return v_out, gt_out


def philox_words(first, n, step, seed=0, stream=0, device="cuda"):
    """The raw Philox4x32-10 words of synth_noise (include/fgc.h: fgc_philox_words): int32 [n,4] on the device (view as
    uint32), row i for the counter (first + i, step low, step high, stream) and the key seed."""
    out = torch.empty(int(n), 4, dtype=torch.int32, device=device)
    _req_cuda(out)
    check(_lib.lib().fgc_philox_words(int(first) & 0xFFFFFFFF, int(n), int(step) & 0xFFFFFFFFFFFFFFFF,
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF, ptr(out), stream_ptr()),
          "fgc_philox_words")
    return out


def face_features_rows(verts, faces_rows, out=None, scratch=None, have_bbox=False, ctl=None):
    """Build extension (include/fgc.h: fgc_face_features_rows): the network's six input channels [N,6] - unit normal |
    barycentre / bounding-box diagonal - of the faces faces_rows int32 [N,3] (-1 rows = fake nodes: zero rows) on the
    vertices verts [V,3], bit-identical to utils.face_features.  have_bbox: `scratch` holds the bounding-box partials
    synth_noise has just left for these vertices."""
    _req_cuda(verts, faces_rows, out, scratch, ctl)
    verts = _f32c(verts.reshape(-1, 3))
    faces_rows = faces_rows.reshape(-1, 3).to(torch.int32).contiguous()
    nv, n = verts.shape[0], faces_rows.shape[0]
    if out is None:
        out = torch.empty(n, 6, dtype=torch.float32, device=verts.device)
    need = _lib.lib().fgc_synth_scratch_floats(nv)
    if scratch is None:
        if have_bbox:
            raise ValueError("have_bbox needs the scratch synth_noise filled")
        scratch = torch.empty(max(need, 1), dtype=torch.float32, device=verts.device)
    check(_lib.lib().fgc_face_features_rows(ptr(verts), nv, ptr(faces_rows), n, ptr(ctl), 1 if have_bbox else 0, ptr(out),
                                            ptr(scratch), scratch.numel(), stream_ptr()), "fgc_face_features_rows")
    return out
