"""bench.py host logic that needs no GPU: workload presets, the N > 1 self-launch (a fresh torchrun child, never an
exec), and that a failing child is reported as a failure instead of a hang or a silent success."""
import json
import os
import subprocess
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_config_presets_follow_the_survey():
    import bench
    a = bench.parse_args([])
    assert (a.gpus, a.nu, a.nv, a.multi_scale, a.scaling, a.what, a.dtype) == (1, 250, 200, False, "weak", "train", "f32")
    a = bench.parse_args(["--config", "c3"])
    assert (a.nu, a.nv, a.what, a.dtype) == (250, 100, "train", "bf16")          # 50 000 facets, bf16 storage
    assert bench.parse_args(["--config", "c3", "--dtype", "f32"]).dtype == "f32"
    a = bench.parse_args(["--config", "c4", "--gpus", "8"])
    assert (a.nu * a.nv * 2, a.scaling, a.what) == (1000000, "strong", "train")   # ONE 1M-facet mesh over the ranks
    a = bench.parse_args(["--config", "c5", "--gpus", "8"])
    assert (a.nu * a.nv * 2, a.multi_scale, a.scaling, a.what) == (500000, True, "strong", "denoise")
    a = bench.parse_args(["--nu", "40", "--nv", "30", "--multi-scale"])
    assert (a.nu, a.nv, a.what) == (40, 30, "denoise")


def test_launcher_command_is_the_drivers_torchrun_line():
    import bench
    cmd = bench.launcher_command(4, ["--gpus", "4", "--nu", "48", "--steps", "7", "--multi-scale"], 29999)
    assert cmd[0] == sys.executable and cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29999"
    assert cmd[-5] == os.path.join(REPO, "bench.py") and cmd[-4:] == ["--gpus", "4", "--steps", "7"]


def test_family_names_group_by_kernel_function():
    import bench
    f = bench.family_of
    assert f("conv_w8_kernel<fwd>") == f("conv_w8_kernel<data>") == "conv_w8"
    assert f("conv_bwd_logits_deep_kernel") == f("conv_bwd_logits_mfma_kernel") == "conv_bwd_logits"
    assert f("mlp_bwd_kernel") == "mlp" and f("gemm_tn_stream_kernel") == "gemm_tn"


def _env_without_a_gpu():
    """Two gloo ranks that see no GPU on any machine (an invalid device ordinal hides every device), so that their child
    group fails the same way with or without a GPU in the box, before any GPU work."""
    env = dict(os.environ, FGC_BENCH_BACKEND="gloo", HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    env.pop("WORLD_SIZE", None)
    return env


def test_self_launch_without_a_gpu_fails_loudly():
    """The child sees no GPU (_env_without_a_gpu): both of its ranks die in FacetDenoiser ("no CPU fallback").  The parent
    must come back with a non-zero exit code and no JSON line - not hang, not print a number."""
    env = _env_without_a_gpu()
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--nu", "12", "--nv", "10", "--no-cpu-baseline"], env=env, capture_output=True, text=True,
                       timeout=300, cwd=REPO)
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert "one more group" not in r.stderr          # eager launches are the default of N > 1: nothing to retry without


def test_self_launch_retries_once_with_eager_launches_when_a_graph_run_dies_without_a_line():
    """--graph 1 (hipGraph segments between the exchanges): a rank group that ends without a result line is followed by ONE
    fresh child group with --graph 0.  Here both groups die (no GPU visible): the parent says what it did and fails."""
    env = _env_without_a_gpu()
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--nu", "12", "--nv", "10", "--no-cpu-baseline", "--graph", "1"], env=env, capture_output=True,
                       text=True, timeout=600, cwd=REPO)
    assert r.returncode != 0 and not [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.stderr.count("one more group with --graph 0") == 1


def test_algorithmic_bytes_match_the_survey_formula():
    """SURVEY.md section 8d per-node forward bytes (1 584 B per padded level-0 node at d = 10.72/8.17/7.92)."""
    import bench

    class Net:
        def layer_dims(self):
            n0, n1, n2 = 123472, 30868, 7717
            z0, z1, z2 = 1323472, 252236, 61155
            return [("conv1", n0, z0, 6, 32), ("conv2", n1, z1, 32, 64), ("conv3", n2, z2, 64, 128),
                    ("dconv3", n2, z2, 128, 128), ("upconv2", n1, z1, 128, 64), ("dconv2", n1, z1, 128, 64),
                    ("upconv1", n0, z0, 64, 32), ("dconv1", n0, z0, 64, 32)]
    fwd, fb = bench.algorithmic_bytes_fwd_bwd(Net())
    assert abs(fwd / 123472 - 1584) < 12 and abs(fb / fwd - 3879 / 1584) < 1e-9
    fwd16, _ = bench.algorithmic_bytes_fwd_bwd(Net(), elem=2)
    assert 0.5 * fwd < fwd16 < 0.62 * fwd      # activations halve, the CSR and the 6 / 3-channel ends do not


def test_a_plain_run_is_the_default_and_full_adds_the_extras():
    import bench
    a = bench.parse_args(["--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, "")
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_writer_keeps_floats_and_samples_rows_within_the_limit(tmp_path):
    import numpy as np
    import bench
    rs = np.random.RandomState(1)
    arrays = {"a": rs.rand(100, 3), "b": rs.rand(10).astype(np.float16), "c": np.arange(5, dtype=np.int32)}
    assert bench.write_outputs(str(tmp_path / "x"), arrays) == ["a", "b", "c"]
    a, b, c = (np.load(tmp_path / "x" / (n + ".npy")) for n in "abc")
    assert a.dtype == np.float64 and np.array_equal(a, arrays["a"])
    assert b.dtype == c.dtype == np.float32 and np.array_equal(b, arrays["b"].astype(np.float32))
    assert np.array_equal(c, np.arange(5, dtype=np.float32))
    # over the limit: an array larger than its share keeps a seeded sample of its rows, in order, the same on every call
    big = {"big": rs.rand(4000, 3).astype(np.float32), "small": rs.rand(8).astype(np.float32)}
    for d in ("y", "z"):
        bench.write_outputs(str(tmp_path / d), big, limit=4096)
    y, z = np.load(tmp_path / "y" / "big.npy"), np.load(tmp_path / "z" / "big.npy")
    assert np.array_equal(y, z) and y.shape[1] == 3 and 0 < y.nbytes <= 2048
    assert np.array_equal(np.load(tmp_path / "y" / "small.npy"), big["small"])
    rows = [int(np.flatnonzero((big["big"] == r).all(1))[0]) for r in y]
    assert rows == sorted(set(rows))
