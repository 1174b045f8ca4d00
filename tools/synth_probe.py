"""Cost of the per-step noise synthesis (training from clean meshes) on the MI355X.

    python tools/synth_probe.py [--faces 20480 100000] [--steps 50] [--rounds 5] [--out FILE]

Per mesh size (a clean mesh: the 20 480-face icosphere, otherwise a torus): the DEVICE time of each of the two synthesis
kernels (noise + bounding boxes, then the input rows) from the library's hipEvent hooks (fgc_profile_*: events around
every launch) beside the bytes they move and bytes / 8 TB/s, and what a back-to-back stream of the two calls costs per
pair (event time over `steps` calls: the enqueue rate of the Python wrappers where that is the larger); and, for the
largest size, the captured training step with the synthesis (a clean mesh, new noise every step) against the captured
plain step (the same mesh bound with bind_mesh), alternating `rounds` times in this one process, with the launches
per step of both and the synthesis kernels' own device time from the library's hipEvent hooks.

    python tools/synth_probe.py --points [--faces 20480 100000] [--steps 50] [--rounds 5] [--out FILE]

The same for the vertex networks (FacetDenoiser.bind_clean_vertices): per mesh size the DEVICE time of
fgc_point_sets_prepare (both point sets normalised by their union box and rotated, one launch) beside its bytes / 8 TB/s;
and, for the largest size, the captured point-set step with the synthesis against the captured plain step (the same
graph levels and host-made inputs of one noisy draw, bound with bind_vertices), alternating `rounds` times in this one process, with the launches per step of both.

    python tools/synth_probe.py --lf [--faces 20480 100000] [--steps 20] [--rounds 5] [--out FILE]

The low-frequency noise (fgc_synth_noise_lf): per mesh size and for K = faces / 6 and K = vertices /
16 bumps the DEVICE time of its two launches (bump table, field + displacement) beside the issue-rate floor of the field
kernel - nv x K pairs x 8 VALU instructions over 256 CUs x 4 SIMDs, one wave64 instruction per SIMD every 4 cycles at 2.4
GHz - and beside the same with the exponential counted as four slots (11 per pair: an estimate, not a bound - the measured
slope between two bump counts is faster than it); and, for the largest size, the captured point-set step
and the captured trainNet step with the bumps against the same steps with white noise alone, alternating `rounds` times in
this one process.

    python tools/synth_probe.py --sensor [--faces 20480 100000] [--steps 50] [--rounds 5] [--out FILE]

The depth-sensor noise model (fgc_synth_noise_sensor): per mesh size the DEVICE time of the launch
(power 0 without quantisation, power 2, power 2 with quant 0.5) beside fgc_synth_noise on the same table of rays, the forms
alternating `rounds` times; and, for the largest size, the captured trainNet step and the captured point-set step
(ray_update) with the model against the same steps with plain ray noise, two networks alternating in this one process."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import facet_graph_convolution_amd  # noqa: E402,F401  (before torch.cuda: hipGraph replay switch)
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_BYTES_PER_S = 8e12


def timed(fn, steps, warmup=5):
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


def _clean_mesh(nf):
    from facet_graph_convolution_amd.meshgen import torus, icosphere
    if nf == 20480:
        return icosphere(5)
    n = int(round((nf / 2) ** 0.5))
    return torus(n, n)


def points(args):
    """--points: fgc_point_sets_prepare alone, and the captured point-set step with and without the synthesis."""
    import ctypes as C
    from facet_graph_convolution_amd import ops, _lib
    L = _lib.lib()
    from facet_graph_convolution_amd.net import FacetDenoiser
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    from facet_graph_convolution_amd.utils import rand_rotation_matrix
    res = []
    dev = "cuda:0"
    for nf in args.faces:
        V, F = _clean_mesh(nf)
        nv = V.shape[0]
        Vd = torch.as_tensor(V, device=dev)
        gt_box = torch.cat([Vd.min(0).values, Vd.max(0).values])
        R = torch.as_tensor(rand_rotation_matrix(randnums=np.random.RandomState(0).uniform(size=3)).astype(np.float32),
                            device=dev).reshape(9)
        scratch = torch.empty(6 * 1024, dtype=torch.float32, device=dev)
        out_v = ops.synth_noise(Vd, 0.01, 3, seed=1, scratch=scratch)
        outs = (torch.empty_like(Vd), torch.empty_like(Vd))
        prepare = lambda: ops.point_sets_prepare(out_v, Vd, R=R, gt_box=gt_box, scratch=scratch, have_bbox=True,  # noqa: E731
                                                 out=outs)
        # bytes: both sets are read once and written once (the boxes, at most 24 KB per workgroup, come from the L2)
        nbytes = 24 * (nv + nv)
        prepare()
        torch.cuda.synchronize()
        L.fgc_profile_enable(1)
        for _ in range(args.steps):
            prepare()
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1 << 16)
        L.fgc_profile_collect(buf, len(buf))
        L.fgc_profile_enable(0)
        dev_us = {}
        for line in buf.value.decode().splitlines():
            name, cnt, ms = line.rsplit(" ", 2)
            dev_us[name.split("/")[-1]] = float(ms) / int(cnt) * 1e3
        row = dict(faces=int(F.shape[0]), vertices=int(nv), prepare_bytes=nbytes,
                   prepare_floor_us=nbytes / HBM_BYTES_PER_S * 1e6, kernel_device_us=dev_us,
                   enqueued_back_to_back_us=timed(prepare, args.steps) * 1e3)
        if nf == max(args.faces):
            # the plain step runs on the SAME graph levels and on host-made inputs of the noisy vertices counter 1 draws:
            # the convolutions' work depends on the levels and fgc_point_loss's search on the points
            from facet_graph_convolution_amd.makeNoisy import make_noisy
            from facet_graph_convolution_amd.utils import face_features, normalizePointSets
            clean = TrainingSet()
            clean.addCleanMeshWithVertices(V, F, seed=0)
            Vn = make_noisy(V, F, 0.2, seed=0, step=1)
            n0 = clean.in_list[0].shape[1]
            per_face = np.concatenate([a.astype(np.float32) for a in face_features(Vn, F)], axis=1)
            new_to_old = np.empty(n0, dtype=np.int64)
            new_to_old[np.asarray(clean.permutations[0])] = np.arange(n0)
            rows = np.concatenate([per_face, np.zeros((n0 - len(per_face), 6), np.float32)])[new_to_old]
            vn, gn = normalizePointSets(Vn, V)
            rs = np.random.RandomState(0)
            i0, i1, Rm = rs.randint(nv, size=500), rs.randint(nv, size=500), rand_rotation_matrix(randnums=rs.uniform(size=3))
            nets = {"synth": FacetDenoiser(dev, multi_scale=True, seed=0), "plain": FacetDenoiser(dev, multi_scale=True, seed=0)}
            nets["synth"].bind_clean_vertices(0, clean.in_list[0], clean.adj_list[0], clean.clean_vertices[0],
                                              clean.clean_faces_rows[0], clean.v_faces_list[0], clean.clean_edge_len[0])
            nets["plain"].bind_vertices(0, rows, clean.adj_list[0], vn, clean.clean_faces_rows[0], clean.v_faces_list[0], gn)
            for net in nets.values():
                net.set_point_samples(i0, i1)
                net.set_rotation(Rm)
            nets["synth"].set_noise(1, 0.2)      # (the draw the plain step's inputs were made from: the same data)
            step = {k: (lambda net=net: net.pointset_forward_backward(rotate=True, capture=True)) for k, net in nets.items()}
            times = {"synth": [], "plain": []}
            for r in range(args.rounds):
                for k in ("synth", "plain"):
                    times[k].append(timed(step[k], args.steps))
            row["captured_synth_ms"] = times["synth"]
            row["captured_plain_ms"] = times["plain"]
            row["captured_difference_us"] = (float(np.median(times["synth"])) - float(np.median(times["plain"]))) * 1e3
            for k, net in nets.items():
                net.pointset_forward_backward(rotate=True)
                torch.cuda.synchronize()
                net.profile_start()
                for _ in range(10):
                    net.pointset_forward_backward(rotate=True)
                torch.cuda.synchronize()
                prof = net.profile_stop()
                row[k + "_launches_per_step"] = sum(c for c, _ in prof.values()) / 10.0
                if k == "synth":
                    row["synth_kernels_us"] = {name: ms / cnt * 1e3 for name, (cnt, ms) in prof.items()
                                               if "synth" in name or "prepare" in name}
            del nets
        print(json.dumps(row), flush=True)
        res.append(row)
        torch.cuda.empty_cache()
    return res


LF_VALU_PER_PAIR = 8        # 3 v_sub, v_mul + 2 v_fma, v_mul, v_exp_f32, v_fma: the --save-temps ISA of lf_field_kernel
LF_PAIRS_PER_S = 256 * 4 * 64 / (LF_VALU_PER_PAIR * 4) * 2.4e9      # the floor: one issue slot per instruction
LF_PAIRS_PER_S_QUARTER = LF_PAIRS_PER_S * 8 / 11                    # the estimate with v_exp_f32 at a quarter of the rate


def _device_us(L, fn, steps):
    """{kernel name: device microseconds per launch} of `steps` calls of fn, from the library's hipEvent hooks."""
    import ctypes as C
    fn()
    torch.cuda.synchronize()
    L.fgc_profile_enable(1)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    buf = C.create_string_buffer(1 << 16)
    L.fgc_profile_collect(buf, len(buf))
    L.fgc_profile_enable(0)
    out = {}
    for line in buf.value.decode().splitlines():
        name, cnt, ms = line.rsplit(" ", 2)
        out[name.split("/")[-1]] = float(ms) / int(cnt) * 1e3
    return out


def lf(args):
    """--lf: the two launches of fgc_synth_noise_lf, and the captured steps with and without the bumps."""
    from facet_graph_convolution_amd import ops, _lib
    from facet_graph_convolution_amd.net import FacetDenoiser
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    from facet_graph_convolution_amd.utils import rand_rotation_matrix, areaWeightedVertexNormals, getAverageEdgeLength
    L = _lib.lib()
    dev = "cuda:0"
    res = []
    for nf in args.faces:
        V, F = _clean_mesh(nf)
        nv, edge = V.shape[0], float(getAverageEdgeLength(V, F)[0])
        Vd = torch.as_tensor(V, device=dev)
        nd = torch.as_tensor(areaWeightedVertexNormals(V, F).astype(np.float32), device=dev)
        out_v = torch.empty_like(Vd)
        row = dict(faces=int(F.shape[0]), vertices=int(nv), launches={})
        for what, K in (("faces/6", -(-F.shape[0] // 6)), ("vertices/16", -(-nv // 16))):
            _, width, area = ops.lf_plan(V, F, edge, 3.0, K)
            amp = ops.lf_amplitude(0.3, edge, width, K, area)
            scratch = torch.zeros(L.fgc_synth_lf_scratch_floats(nv, K), dtype=torch.float32, device=dev)
            ctl = torch.from_numpy(ops.noise_words(3, 0.1 * edge).view(np.int32)).to(dev)
            lf_ctl = torch.from_numpy(ops.lf_words(amp, width).view(np.int32)).to(dev)
            call = lambda: ops.synth_noise_lf(Vd, nd, None, None, None, None, K, seed=1, out=out_v, scratch=scratch,  # noqa: E731
                                              ctl=ctl, lf_ctl=lf_ctl)
            us = _device_us(L, call, args.steps)
            pairs = float(nv) * K
            floor = pairs / LF_PAIRS_PER_S * 1e6
            field = [t for k, t in us.items() if "lf_field_kernel" in k][0]
            row["launches"][what] = dict(bumps=int(K), pairs=pairs, kernel_device_us=us, field_floor_us=floor,
                                         field_over_floor=field / floor,
                                         field_quarter_rate_exp_us=pairs / LF_PAIRS_PER_S_QUARTER * 1e6,
                                         enqueued_back_to_back_us=timed(call, args.steps) * 1e3)
        if nf == max(args.faces):
            rs = np.random.RandomState(0)
            Rm = rand_rotation_matrix(randnums=rs.uniform(size=3))
            # the captured trainNet step
            ds = TrainingSet()
            ds.addCleanMesh(V, F, seed=0)
            n0 = ds.in_list[0].shape[1]
            net = FacetDenoiser(dev, seed=0)
            net.bind_clean(0, ds.in_list[0], ds.adj_list[0], ds.gt_list[0], ds.clean_vertices[0], ds.clean_faces_rows[0],
                           ds.clean_edge_len[0], lf=(3.0, None))
            net.set_samples(rs.randint(n0, size=4000))
            net.set_rotation(Rm)
            step = lambda: net.forward_backward(rotate=True, capture=True)  # noqa: E731
            times = {"bumps": [], "white": []}
            for r in range(args.rounds):
                for k in ("bumps", "white"):
                    net.set_noise(r + 1, 0.1, 0.3 if k == "bumps" else None)
                    times[k].append(timed(step, args.steps))
            row["trainNet_captured_ms"] = times
            row["trainNet_difference_us"] = (float(np.median(times["bumps"])) - float(np.median(times["white"]))) * 1e3
            del net, ds
            torch.cuda.empty_cache()
            # the captured point-set step
            dv = TrainingSet()
            dv.addCleanMeshWithVertices(V, F, seed=0)
            net = FacetDenoiser(dev, multi_scale=True, seed=0)
            net.bind_clean_vertices(0, dv.in_list[0], dv.adj_list[0], dv.clean_vertices[0], dv.clean_faces_rows[0],
                                    dv.v_faces_list[0], dv.clean_edge_len[0], lf=(3.0, None))
            net.set_point_samples(rs.randint(nv, size=500), rs.randint(nv, size=500))
            net.set_rotation(Rm)
            step = lambda: net.pointset_forward_backward(rotate=True, capture=True)  # noqa: E731
            times = {"bumps": [], "white": []}
            for r in range(args.rounds):
                for k in ("bumps", "white"):
                    net.set_noise(r + 1, 0.1, 0.3 if k == "bumps" else None)
                    times[k].append(timed(step, args.steps))
            row["pointset_captured_ms"] = times
            row["pointset_difference_us"] = (float(np.median(times["bumps"])) - float(np.median(times["white"]))) * 1e3
            del net, dv
        print(json.dumps(row), flush=True)
        res.append(row)
        torch.cuda.empty_cache()
    return res


SENSOR_CAMERA = (2.5, 0.4, 1.2)


def sensor(args):
    """--sensor: fgc_synth_noise_sensor beside fgc_synth_noise on the same table of rays, and the captured steps with the
    model (power 2, quant 0.5) and with plain ray noise."""
    from facet_graph_convolution_amd import ops, _lib
    from facet_graph_convolution_amd.net import FacetDenoiser
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    from facet_graph_convolution_amd.utils import rand_rotation_matrix, getAverageEdgeLength, view_rays, sensor_model
    L = _lib.lib()
    dev = "cuda:0"
    res = []
    for nf in args.faces:
        V, F = _clean_mesh(nf)
        nv, edge = V.shape[0], float(getAverageEdgeLength(V, F)[0])
        rays = view_rays(V, camera=SENSOR_CAMERA)
        Vd, rd = torch.as_tensor(V, device=dev), torch.as_tensor(rays, device=dev)
        out_v = torch.empty_like(Vd)
        scratch = torch.empty(6 * 1024, dtype=torch.float32, device=dev)
        ctl = torch.from_numpy(ops.noise_words(3, 0.2 * edge).view(np.int32)).to(dev)
        row = dict(faces=int(F.shape[0]), vertices=int(nv), noise_bytes=36 * nv, noise_floor_us=36 * nv / HBM_BYTES_PER_S * 1e6,
                   kernel_device_us={})
        calls = {"plain": lambda: ops.synth_noise(Vd, None, None, seed=1, normals=rd, out=out_v, scratch=scratch, ctl=ctl)}
        for name, (power, quant) in (("power0", (0, 0.0)), ("power2", (2, 0.0)), ("power2_quant", (2, 0.5))):
            m = sensor_model(V, SENSOR_CAMERA, edge, power, quant)
            sctl = torch.from_numpy(ops.sensor_words(m.power, m.r_ref, m.q).view(np.int32)).to(dev)
            calls[name] = lambda m=m, sctl=sctl: ops.synth_noise_sensor(Vd, rd, m.camera, None, None, None, None, None, seed=1,
                                                                        out=out_v, scratch=scratch, ctl=ctl, sensor_ctl=sctl)
        for r in range(args.rounds):      # (alternating: every form in every round)
            for name, call in calls.items():
                us = _device_us(L, call, args.steps)
                row["kernel_device_us"].setdefault(name, []).append([t for k, t in us.items() if "synth_noise" in k][0])
        if nf == max(args.faces):
            rs = np.random.RandomState(0)
            Rm = rand_rotation_matrix(randnums=rs.uniform(size=3))
            model = sensor_model(V, SENSOR_CAMERA, edge, 2, 0.5)
            ds = TrainingSet()
            ds.addCleanMesh(V, F, seed=0)
            samp = rs.randint(ds.in_list[0].shape[1], size=4000)
            nets = {}
            for k, kw in (("sensor", dict(sensor=model)), ("rays", {})):
                nets[k] = FacetDenoiser(dev, seed=0)
                nets[k].bind_clean(0, ds.in_list[0], ds.adj_list[0], ds.gt_list[0], ds.clean_vertices[0], ds.clean_faces_rows[0],
                                   ds.clean_edge_len[0], direction=rays, **kw)
                nets[k].set_samples(samp)
                nets[k].set_rotation(Rm)
            times = {"sensor": [], "rays": []}
            for r in range(args.rounds):
                for k, net in nets.items():
                    net.set_noise(r + 1, 0.2)
                    times[k].append(timed(lambda: net.forward_backward(rotate=True, capture=True), args.steps))
            row["trainNet_captured_ms"] = times
            row["trainNet_difference_us"] = (float(np.median(times["sensor"])) - float(np.median(times["rays"]))) * 1e3
            del nets, ds
            torch.cuda.empty_cache()
            dv = TrainingSet()
            dv.addCleanMeshWithVertices(V, F, seed=0)
            i0, i1 = rs.randint(nv, size=500), rs.randint(nv, size=500)
            nets = {}
            for k, kw in (("sensor", dict(sensor=model)), ("rays", {})):
                nets[k] = FacetDenoiser(dev, multi_scale=True, seed=0)
                nets[k].bind_clean_vertices(0, dv.in_list[0], dv.adj_list[0], dv.clean_vertices[0], dv.clean_faces_rows[0],
                                            dv.v_faces_list[0], dv.clean_edge_len[0], direction=rays, ray_update=True, **kw)
                nets[k].set_point_samples(i0, i1)
                nets[k].set_rotation(Rm)
            times = {"sensor": [], "rays": []}
            for r in range(args.rounds):
                for k, net in nets.items():
                    net.set_noise(r + 1, 0.2)
                    times[k].append(timed(lambda: net.pointset_forward_backward(rotate=True, capture=True), args.steps))
            row["pointset_captured_ms"] = times
            row["pointset_difference_us"] = (float(np.median(times["sensor"])) - float(np.median(times["rays"]))) * 1e3
            del nets, dv
        print(json.dumps(row), flush=True)
        res.append(row)
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[20480, 100000])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--points", action="store_true", help="the point sets of the vertex networks (fgc_point_sets_prepare)")
    ap.add_argument("--lf", action="store_true", help="the low-frequency noise (fgc_synth_noise_lf)")
    ap.add_argument("--sensor", action="store_true", help="the depth-sensor noise model (fgc_synth_noise_sensor)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.points or args.lf or args.sensor:
        res = sensor(args) if args.sensor else lf(args) if args.lf else points(args)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        return
    import ctypes as C
    from facet_graph_convolution_amd import ops, _lib
    L = _lib.lib()
    from facet_graph_convolution_amd.net import FacetDenoiser
    from facet_graph_convolution_amd.dataClasses import TrainingSet
    from facet_graph_convolution_amd.meshgen import torus, icosphere
    from facet_graph_convolution_amd.utils import rand_rotation_matrix
    res = []
    for nf in args.faces:
        if nf == 20480:
            V, F = icosphere(5)
        else:
            n = int(round((nf / 2) ** 0.5))
            V, F = torus(n, n)
        ds = TrainingSet()
        ds.addCleanMesh(V, F, seed=0)
        x, adjs, gt = ds.in_list[0], ds.adj_list[0], ds.gt_list[0]
        n0, nv = x.shape[1], V.shape[0]
        dev = "cuda:0"
        Vd = torch.as_tensor(V, device=dev)
        rows = torch.as_tensor(ds.clean_faces_rows[0][0], device=dev)
        ctl = torch.from_numpy(ops.noise_words(3, 0.2 * ds.clean_edge_len[0]).view(np.int32)).to(dev)
        out_v, out_x = torch.empty_like(Vd), torch.empty(n0, 6, dtype=torch.float32, device=dev)
        scratch = torch.empty(6 * 1024, dtype=torch.float32, device=dev)
        noise = lambda: ops.synth_noise(Vd, None, None, seed=1, out=out_v, scratch=scratch, ctl=ctl)  # noqa: E731
        feats = lambda: ops.face_features_rows(out_v, rows, out=out_x, scratch=scratch, have_bbox=True, ctl=ctl)  # noqa: E731

        def both():
            noise()
            feats()
        # bytes: noise reads and writes the vertices; the rows kernel reads the face ids, gathers three vertices per row
        # (every vertex is read from HBM once, the other five uses hit the caches) and writes 24 bytes per row
        b_noise, b_feats = 24 * nv, 12 * n0 + 12 * nv + 24 * n0
        both()
        torch.cuda.synchronize()
        L.fgc_profile_enable(1)
        for _ in range(args.steps):
            both()
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1 << 16)
        L.fgc_profile_collect(buf, len(buf))
        L.fgc_profile_enable(0)
        dev_us = {}
        for line in buf.value.decode().splitlines():
            name, cnt, ms = line.rsplit(" ", 2)
            dev_us[name.split("/")[-1]] = float(ms) / int(cnt) * 1e3
        row = dict(faces=int(F.shape[0]), nodes=int(n0), vertices=int(nv), noise_bytes=b_noise, features_bytes=b_feats,
                   noise_floor_us=b_noise / HBM_BYTES_PER_S * 1e6, features_floor_us=b_feats / HBM_BYTES_PER_S * 1e6,
                   kernel_device_us=dev_us, pair_enqueued_back_to_back_us=timed(both, args.steps) * 1e3)
        if nf == max(args.faces):
            rs = np.random.RandomState(0)
            samp, Rm = rs.randint(n0, size=4000), rand_rotation_matrix(randnums=rs.uniform(size=3))
            nets = {}
            nets["synth"] = FacetDenoiser(dev, seed=0)
            nets["synth"].bind_clean(0, x, adjs, gt, ds.clean_vertices[0], ds.clean_faces_rows[0], ds.clean_edge_len[0])
            nets["plain"] = FacetDenoiser(dev, seed=0).bind_mesh(x, adjs, gt=gt)
            for net in nets.values():
                net.set_samples(samp)
                net.set_rotation(Rm)
            def synth_step():
                nets["synth"].forward_backward(rotate=True, capture=True)

            def plain_step():
                nets["plain"].forward_backward(rotate=True, capture=True)
            nets["synth"].set_noise(0, 0.2)
            times = {"synth": [], "plain": []}
            for r in range(args.rounds):
                nets["synth"].set_noise(r + 1, 0.2)
                times["synth"].append(timed(synth_step, args.steps))
                times["plain"].append(timed(plain_step, args.steps))
            row["captured_synth_ms"] = times["synth"]
            row["captured_plain_ms"] = times["plain"]
            row["captured_difference_us"] = (float(np.median(times["synth"])) - float(np.median(times["plain"]))) * 1e3
            # launches per step and the synthesis kernels' own device time, from the library's hipEvent hooks (eager steps)
            for k, net in nets.items():
                net.forward_backward(rotate=True)
                torch.cuda.synchronize()
                net.profile_start()
                for _ in range(10):
                    net.forward_backward(rotate=True)
                torch.cuda.synchronize()
                prof = net.profile_stop()
                row[k + "_launches_per_step"] = sum(c for c, _ in prof.values()) / 10.0
                if k == "synth":
                    row["synth_kernels_us"] = {name: ms / cnt * 1e3 for name, (cnt, ms) in prof.items() if "synth" in name}
            del nets
        print(json.dumps(row), flush=True)
        res.append(row)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
