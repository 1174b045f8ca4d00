#!/usr/bin/env python3
"""Generate tests/golden/double_ico3.npz (+ _f64) by EXECUTING THE REFERENCE'S double-loss training chain on tf_shim
(as make_golden_points.py does): get_model_reg_multi_scale (model.py:837-946), normalizeTensor on ALL THREE heads
(train.py:1079-1081), update_position_MS on them with [80, 20, 20] iterations, fullLoss (train.py:1373-1424) plus
faceNormalsLoss of head 0 against the rotated ground-truth face normals (train.py:1100-1102, 1272-1294), then autograd
for every weight's gradient - one step of trainDoubleLossNet (train.py:919-1268) without the optimiser.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_double.py
    PYTHONDONTWRITEBYTECODE=1 TF_SHIM_DTYPE=float64 python tests/golden/gen/make_golden_double.py

Inputs: those of points_ico3.npz (make_golden_points.py: the same mesh, vertices, weights, sample rows and rotation;
they are not stored twice - a test reads them from points_ico3.npz).  New here: the ground-truth face normals, computed
from the clean vertices by the reference's computeFacesNormals, padded with zero rows for the fake nodes and put in node
order as dataClasses.py:380-411 does.  The rotation of the ground-truth normals (train.py:1019-1021) is restated with the
same tf ops.

Stored: the three losses (total, points, normals), n_conv0 (head 0, normalised) and the rotated ground-truth normals
(so a CPU test can check the normal loss on its own), the refined vertices, and every weight gradient subsampled as
make_golden_points.py does.  Only data is written.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden_points as P  # noqa: E402  (registers the tf ops fullLoss needs; imports make_golden)
import numpy as np  # noqa: E402
import torch  # noqa: E402

G = P.G
tf = G.tf


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
    rs = np.random.RandomState(21)          # (make_golden_points.py's draws, in its order)
    i0 = rs.randint(nv, size=P.SAMP_NUM)
    i1 = rs.randint(ngt, size=P.SAMP_NUM)
    R = G.ref_utils.rand_rotation_matrix(randnums=rs.uniform(size=3))
    # dataClasses.py:380-411: ground-truth face normals of the clean mesh, zero rows for the fake nodes, node order
    F = prep["F"].astype(np.int64)
    oldToNew = prep["permutations"].astype(np.int64)
    newToOld = np.empty_like(oldToNew)
    newToOld[oldToNew] = np.arange(oldToNew.shape[0])
    gtfn0 = G.ref_utils.computeFacesNormals(prep["Vclean"].astype(np.float32), F)
    gtfn = np.concatenate((gtfn0, np.zeros((n0 - F.shape[0], 3))), axis=0)[newToOld].astype(np.float32)
    padded = np.concatenate((F, -np.ones((n0 - F.shape[0], 3), dtype=np.int64)), axis=0)[newToOld]
    assert (padded == faces_p).all(), "node order of the faces differs from msvertex_ico3.npz"
    tile = lambda n: torch.tensor(np.tile(R.reshape(1, 1, 3, 3), (1, n, 1, 1)).astype(np.float32), dtype=FDT)  # noqa: E731
    rot, rot_v, rot_gt = tile(n0), tile(nv), tile(ngt)
    x_in = torch.tensor(x32, dtype=FDT)
    vp = torch.tensor(Vn[None], dtype=FDT)
    gtvp = torch.tensor(GTn[None], dtype=FDT)
    gtfn_t = torch.tensor(gtfn[None], dtype=FDT)
    faces_t = torch.tensor(faces_p[None].astype(np.int32))
    vf_t = torch.tensor(v_faces[None].astype(np.int32))
    keep = {}

    def fn():
        # train.py:1010-1032 (bAddRot, NUM_IN_CHANNELS = 6), restated with the same tf ops; the rest is reference code
        vp_rot = tf.reshape(tf.matmul(rot_v, tf.reshape(vp, [1, -1, 3, 1])), [1, -1, 3])
        gtvp_rot = tf.reshape(tf.matmul(rot_gt, tf.reshape(gtvp, [1, -1, 3, 1])), [1, -1, 3])
        gtfn_rot = tf.reshape(tf.matmul(rot, tf.reshape(gtfn_t, [1, -1, 3, 1])), [1, -1, 3])
        fn_rot = tf.transpose(tf.reshape(x_in, [1, -1, 2, 3]), [0, 1, 3, 2])
        fn_rot = tf.reshape(tf.transpose(tf.matmul(rot, fn_rot), [0, 1, 3, 2]), [1, -1, 6])
        y0, y1, y2 = G.ref_model.get_model_reg_multi_scale(fn_rot, adjs, 1.0, multiScale=True)
        n_conv0 = G.ref_utils.normalizeTensor(y0)
        n_conv1 = G.ref_utils.normalizeTensor(y1)
        n_conv2 = G.ref_utils.normalizeTensor(y2)
        refined, _ = G.ref_train.update_position_MS(vp_rot, [n_conv0, n_conv1, n_conv2], faces_t, vf_t,
                                                    coarsening_steps=2, iter_num_list=[80, 20, 20])
        points = G.ref_train.fullLoss(refined, gtvp_rot, torch.tensor(i0), torch.tensor(i1))
        normals = G.ref_train.faceNormalsLoss(n_conv0, gtfn_rot)
        keep.update(refined=refined, n_conv0=n_conv0, gtfn_rot=gtfn_rot, points=points, normals=normals)
        return points + normals

    loss, variables = G.run_with_params(fn, 0)
    loss.backward()
    f32 = lambda t: t.detach().numpy()[0].astype(np.float32)  # noqa: E731
    out = dict(gt_normals=gtfn, loss=np.float64(loss.item()), loss_points=np.float64(keep["points"].item()),
               loss_normals=np.float64(keep["normals"].item()), n_vars=np.int64(len(variables)),
               sample_ind0=i0.astype(np.int32), sample_ind1=i1.astype(np.int32), R=R.astype(np.float32),
               n_conv0=f32(keep["n_conv0"]), gtfn_rot=f32(keep["gtfn_rot"]), refined=f32(keep["refined"]),
               sampled=np.int64(P.SAMPLED))
    for i, (name, v) in enumerate(variables):
        g = v.grad.detach().numpy().reshape(-1)
        out["g%02d" % i] = g[P.sampled_indices(i, g.size)].astype(np.float32)   # float64 run: true gradient rounded once
        out["gmax%02d" % i] = np.float64(np.abs(g).max())
        out["gsize%02d" % i] = np.int64(g.size)
        out["name%02d" % i] = np.array(name)
    G.save("double_ico3%s.npz" % ("_f64" if G.F64 else ""), **out)


if __name__ == "__main__":
    main()
