"""Cost of the point-set training step (trainAccuracyNet) on the MI355X.

    python tools/points_probe.py [--faces 20000 100000] [--steps 20] [--out FILE] [--only all|network|vertex_fwd|vertex_bwd|loss]
        [--double-loss] [--surface-loss]

Per mesh size (a noisy torus): ms per point-set step eager and replayed from its hipGraph, the graph's node count
(launches per step), the multi-scale angular-loss step on the same mesh for comparison, and the parts of the step timed
alone with device events: network forward + backward, vertex update forward with trajectory, its adjoint, fullLoss.
--only runs one part in a loop (for a `rocprofv3 --kernel-trace --stats` run of its own).  --double-loss: the mesh is bound
with its ground-truth face normals, and the double-loss step (trainDoubleLossNet) is timed next to the point-set step,
eager and replayed, with the dense face-normal loss alone (forward + accumulating backward) as one more part; --only then
also takes `double` (the whole double-loss step) and `dense_loss`.  --surface-loss (nothing else is timed then): the mesh is
bound twice, without and with its own faces as ground-truth faces (bind_vertices(gt_faces=)), and per mesh size the two
losses alone (ops.point_loss, ops.surface_loss on the bound vertices) and the two captured point-set steps are timed in
alternating rounds in one process; the step without the faces issues the launches of a build without the surface loss."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import facet_graph_convolution_amd  # noqa: E402,F401  (before torch.cuda: hipGraph replay switch)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def surface_rows(args):
    """--surface-loss: fullLoss against the surface loss, alone and inside the captured step, in alternating rounds."""
    from facet_graph_convolution_amd import ops
    from facet_graph_convolution_amd.net import FacetDenoiser
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    from facet_graph_convolution_amd.meshgen import torus, add_noise
    from facet_graph_convolution_amd.utils import rand_rotation_matrix
    res = []
    for nf in args.faces:
        n = int(round((nf / 2) ** 0.5))
        V, F = torus(n, n)
        ds = TrainingSet()
        ds.addMeshWithVerticesAndGT(add_noise(V, F, seed=1), F, V, seed=0)
        v, faces, vf, gtv = ds.v_list[0][0], ds.faces_list[0][0], ds.v_faces_list[0][0], ds.gtv_list[0][0]
        rs = np.random.RandomState(0)
        Rm = rand_rotation_matrix(randnums=rs.uniform(size=3))
        i0, i1 = rs.randint(len(v), size=500), rs.randint(len(gtv), size=500)
        nets = {}
        for name, extra in (("points", {}), ("surface", {"gt_faces": faces.astype(np.int32)})):
            net = nets[name] = FacetDenoiser("cuda:0", multi_scale=True, seed=0)
            net.bind_vertices(0, ds.in_list[0], ds.adj_list[0], v, faces, vf, gtv, **extra)
            net.set_point_samples(i0, i1)
            net.set_rotation(Rm)
        Vb = nets["surface"]._mesh["verts"]
        steps = {k: (lambda net=net: net.pointset_forward_backward(rotate=True, capture=True)) for k, net in nets.items()}
        losses = {"points": lambda: ops.point_loss(Vb["x"], Vb["gt"], Vb["i0"], Vb["i1"]),
                  "surface": lambda: ops.surface_loss(Vb["x"], Vb["faces"], Vb["gt"], Vb["gt_faces"], Vb["i0"], Vb["i1"])}
        row = dict(faces=int(F.shape[0]), nodes=int(ds.in_list[0].shape[1]), vertices=int(len(v)), rounds=args.rounds,
                   step_loss={k: float(fn().item()) for k, fn in steps.items()})
        for what, fns in (("loss_ms", losses), ("step_replay_ms", steps)):
            row[what] = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k, fn in fns.items():
                    row[what][k].append(timed(fn, args.steps))
            row[what + "_median"] = {k: float(np.median(t)) for k, t in row[what].items()}
        row["step_replay_ms_surface_minus_points"] = (row["step_replay_ms_median"]["surface"] -
                                                      row["step_replay_ms_median"]["points"])
        print(json.dumps(row), flush=True)
        res.append(row)
        del nets, steps, losses, Vb
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="all")
    ap.add_argument("--double-loss", action="store_true")
    ap.add_argument("--surface-loss", action="store_true")
    ap.add_argument("--rounds", type=int, default=5, help="--surface-loss: alternating rounds of --steps calls each")
    args = ap.parse_args()
    if args.surface_loss:
        res = surface_rows(args)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        return
    from facet_graph_convolution_amd import ops
    from facet_graph_convolution_amd.net import FacetDenoiser
    from facet_graph_convolution_amd.schedule import _graph_node_count
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    from facet_graph_convolution_amd.meshgen import torus, add_noise
    from facet_graph_convolution_amd.utils import rand_rotation_matrix
    res = []
    for nf in args.faces:
        n = int(round((nf / 2) ** 0.5))
        V, F = torus(n, n)
        ds = TrainingSet()
        ds.addMeshWithVerticesAndGT(add_noise(V, F, seed=1), F, V, seed=0)
        x, adjs = ds.in_list[0], ds.adj_list[0]
        v, faces, vf, gtv = ds.v_list[0][0], ds.faces_list[0][0], ds.v_faces_list[0][0], ds.gtv_list[0][0]
        rs = np.random.RandomState(0)
        Rm = rand_rotation_matrix(randnums=rs.uniform(size=3))
        net = FacetDenoiser("cuda:0", multi_scale=True, seed=0)
        net.bind_vertices(0, x, adjs, v, faces, vf, gtv, gt_normals=ds.gt_list[0][0] if args.double_loss else None)
        net.set_point_samples(rs.randint(len(v), size=500), rs.randint(len(gtv), size=500))
        net.set_rotation(Rm)
        row = dict(faces=int(F.shape[0]), nodes=int(x.shape[1]), vertices=int(len(v)))
        B, Vb = net._mesh["B"], net._mesh["verts"]
        nrm = [B["nconv"], B["y1"], B["y2"]]
        dev = net.device
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
        xv, fc, vft = t(v.astype(np.float32)), t(faces.astype(np.int32)), t(vf.astype(np.int32))
        parts = {
            "vertex_fwd": lambda: ops.vertex_update_ms_traj(xv, nrm, fc, vft),
            "loss": lambda: ops.point_loss(xv, Vb["gt"], Vb["i0"], Vb["i1"]),
        }
        net.pointset_forward_backward(rotate=True)
        traj = ops.vertex_update_ms_traj(xv, nrm, fc, vft)
        g = torch.randn_like(xv)
        parts["vertex_bwd"] = lambda: ops.vertex_update_ms_bwd(traj, nrm, fc, vft, g, tables=Vb["tables"])
        def network():      # forward, the coarse heads' and the trunk's backward (the normals' gradients as they stand)
            net._drain(net._forward_gen(True))
            net._coarse_head_bwd("2")
            net._coarse_head_bwd("1")
            net._drain(net._params_backward_gen(False))
        parts["network"] = network
        if args.double_loss:
            gacc = torch.zeros_like(B["nconv"])
            parts["dense_loss"] = lambda: ops.dense_normals_loss(B["nconv"], Vb["gtn"], B["R"], g=gacc)
            parts["double"] = lambda: net.double_loss_forward_backward(rotate=True)
        if args.only != "all":
            for _ in range(args.steps):
                parts[args.only]()
            torch.cuda.synchronize()
            res.append(dict(row, only=args.only))
            continue
        row["pointset_eager_ms"] = timed(lambda: net.pointset_forward_backward(rotate=True), args.steps)
        row["pointset_replay_ms"] = timed(lambda: net.pointset_forward_backward(rotate=True, capture=True), args.steps)
        try:
            row["pointset_graph_nodes"] = _graph_node_count(net._mesh["captured"]["points"][0])
        except Exception as e:       # (the graph was instantiated without keep_graph)
            row["pointset_graph_nodes"] = repr(e)[:80]
        if args.double_loss:
            row["double_eager_ms"] = timed(lambda: net.double_loss_forward_backward(rotate=True), args.steps)
            row["double_replay_ms"] = timed(lambda: net.double_loss_forward_backward(rotate=True, capture=True), args.steps)
            try:
                row["double_graph_nodes"] = _graph_node_count(net._mesh["captured"]["double"][0])
            except Exception as e:
                row["double_graph_nodes"] = repr(e)[:80]
            row["double_minus_pointset_replay_ms"] = row["double_replay_ms"] - row["pointset_replay_ms"]
        for k, fn in parts.items():
            if k != "double":
                row[k + "_ms"] = timed(fn, args.steps)
        ang = FacetDenoiser("cuda:0", multi_scale=True, seed=0)
        ang.bind_mesh(x, adjs, gt=ds.gt_list[0])
        ang.set_samples(rs.randint(x.shape[1], size=4000))
        ang.set_rotation(Rm)
        row["angular_ms_eager_ms"] = timed(lambda: ang.forward_backward(rotate=True), args.steps)
        row["angular_ms_replay_ms"] = timed(lambda: ang.forward_backward(rotate=True, capture=True), args.steps)
        print(json.dumps(row), flush=True)
        res.append(row)
        del net, ang
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
