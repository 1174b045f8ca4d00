#!/usr/bin/env python3
"""Generate tests/golden/points_ico3.npz (+ _f64) by EXECUTING THE REFERENCE'S point-set training chain on tf_shim
(as make_golden.py does): get_model_reg_multi_scale (model.py:837-946), normalizeTensor on head 0 (utils.py:1700-1715,
train.py:767-773), update_position_MS with [80, 20, 20] iterations (train.py:1668-1798) and fullLoss
(train.py:1373-1424), then autograd for every weight's gradient - one step of trainAccuracyNet (train.py:636-916)
without the optimiser.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_points.py
    PYTHONDONTWRITEBYTECODE=1 TF_SHIM_DTYPE=float64 python tests/golden/gen/make_golden_points.py

Inputs: the 1 280-face icosphere of prep_ico3.npz / msvertex_ico3.npz (reference preprocessing: features, adjacency,
faces in node order, v_faces), its vertices and the clean vertices through the reference's normalizePointSets, 500 + 500
sampled rows and a rotation from fixed seeds, weights from make_golden.param_values(0) (= FacetDenoiser(seed=0)).  The
rotations of the inputs, the vertices and the ground truth (train.py:686-713) are restated with the same tf ops.

The shim's own file is left as it is; the two ops fullLoss needs that it lacks (tf.norm, tf.reduce_min) are registered
here.  Gradient tensors of more than SAMPLED entries are stored at a fixed random subset of their entries (RandomState(i)
.choice, sorted) plus their largest magnitude, which keeps the file within the size limit for a committed file.  Only data
is written.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (puts the shim and the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

tf = G.tf
SAMPLED = 4096
SAMP_NUM = 500      # train.py:653


def _norm(x, ord="euclidean", axis=None, keepdims=None, name=None):
    """tf.norm, Euclidean over one axis (the only form fullLoss uses)."""
    return torch.linalg.vector_norm(x, dim=axis, keepdim=bool(keepdims))


def _reduce_min(x, axis=None, keepdims=False, name=None):
    """tf.reduce_min over one axis.  (TensorFlow splits the gradient of an exact tie; no tie occurs in this fixture.)"""
    return x.min(dim=axis, keepdim=keepdims).values


for _name, _fn in (("norm", _norm), ("reduce_min", _reduce_min)):
    if not hasattr(tf, _name):
        setattr(tf, _name, _fn)


def sampled_indices(i, n):
    """The entries of gradient tensor i that the fixture keeps (all of them for a small tensor)."""
    if n <= SAMPLED:
        return np.arange(n)
    return np.sort(np.random.RandomState(i).choice(n, SAMPLED, replace=False))


def main():
    FDT = G.FDT
    prep = np.load(os.path.join(G.OUT, "prep_ico3.npz"))
    msv = np.load(os.path.join(G.OUT, "msvertex_ico3.npz"))
    x32 = prep["x"].astype(np.float32)
    adjs = [torch.tensor(prep["adj%d" % k].astype(np.int32)) for k in range(3)]
    Vn, GTn = G.ref_utils.normalizePointSets(prep["V"].astype(np.float32), prep["Vclean"].astype(np.float32))
    Vn, GTn = np.asarray(Vn, np.float32), np.asarray(GTn, np.float32)
    faces_p, v_faces = msv["faces_perm"], msv["v_faces"]
    n0, nv, ngt = x32.shape[1], Vn.shape[0], GTn.shape[0]
    rs = np.random.RandomState(21)
    i0 = rs.randint(nv, size=SAMP_NUM)
    i1 = rs.randint(ngt, size=SAMP_NUM)
    R = G.ref_utils.rand_rotation_matrix(randnums=rs.uniform(size=3))
    tile = lambda n: torch.tensor(np.tile(R.reshape(1, 1, 3, 3), (1, n, 1, 1)).astype(np.float32), dtype=FDT)  # noqa: E731
    rot, rot_v, rot_gt = tile(n0), tile(nv), tile(ngt)
    x_in = torch.tensor(x32, dtype=FDT)
    vp = torch.tensor(Vn[None], dtype=FDT)
    gtvp = torch.tensor(GTn[None], dtype=FDT)
    faces_t = torch.tensor(faces_p[None].astype(np.int32))
    vf_t = torch.tensor(v_faces[None].astype(np.int32))
    keep = {}

    def fn():
        # train.py:686-713 (bAddRot, NUM_INGOING_CHANNELS = 6), restated with the same tf ops; the rest is reference code
        vp_rot = tf.reshape(tf.matmul(rot_v, tf.reshape(vp, [1, -1, 3, 1])), [1, -1, 3])
        gtvp_rot = tf.reshape(tf.matmul(rot_gt, tf.reshape(gtvp, [1, -1, 3, 1])), [1, -1, 3])
        fn_rot = tf.transpose(tf.reshape(x_in, [1, -1, 2, 3]), [0, 1, 3, 2])
        fn_rot = tf.reshape(tf.transpose(tf.matmul(rot, fn_rot), [0, 1, 3, 2]), [1, -1, 6])
        y0, y1, y2 = G.ref_model.get_model_reg_multi_scale(fn_rot, adjs, 1.0, multiScale=True)
        n_conv0 = G.ref_utils.normalizeTensor(y0)
        refined, _ = G.ref_train.update_position_MS(vp_rot, [n_conv0, y1, y2], faces_t, vf_t, coarsening_steps=2,
                                                    iter_num_list=[80, 20, 20])
        keep["refined"] = refined
        return G.ref_train.fullLoss(refined, gtvp_rot, torch.tensor(i0), torch.tensor(i1))

    loss, variables = G.run_with_params(fn, 0)
    loss.backward()
    out = dict(x=x32, adj0=prep["adj0"].astype(np.int16), adj1=prep["adj1"].astype(np.int16),
               adj2=prep["adj2"].astype(np.int16), verts=Vn, gt_verts=GTn, faces=faces_p.astype(np.int32),
               v_faces=v_faces.astype(np.int16), sample_ind0=i0.astype(np.int32), sample_ind1=i1.astype(np.int32),
               R=R.astype(np.float32), loss=np.float64(loss.item()), n_vars=np.int64(len(variables)),
               refined=keep["refined"].detach().numpy()[0].astype(np.float32), sampled=np.int64(SAMPLED))
    for i, (name, v) in enumerate(variables):
        g = v.grad.detach().numpy().reshape(-1)
        out["g%02d" % i] = g[sampled_indices(i, g.size)].astype(np.float32)   # float64 run: true gradient rounded once
        out["gmax%02d" % i] = np.float64(np.abs(g).max())
        out["gsize%02d" % i] = np.int64(g.size)
        out["name%02d" % i] = np.array(name)
    G.save("points_ico3%s.npz" % ("_f64" if G.F64 else ""), **out)


if __name__ == "__main__":
    main()
