"""CPU: `python bench.py --gpus N` (N > 1) starts its own ranks -- torch.distributed.run as a CHILD process, before anything touches the
GPU -- and relays rank 0's line and the child's exit code.  (The reference's parallel loop needs no launcher, raytracer.cpp:104.)"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_self_launch_argv():
    argv = ["--gpus", "8", "--steps", "20", "--warmup", "3", "--workload", "imageplane"]
    cmd = bench.self_launch_argv(argv, 8, 29555, python="/usr/bin/python3")
    assert cmd[:3] == ["/usr/bin/python3", "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29555"
    k = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[k + 1:] == argv                           # the bench arguments are passed on unchanged, after the script
    assert 1024 < bench.free_port() < 65536


def test_rankless_multi_gpu_invocation_starts_its_ranks_and_relays_their_failure():
    # no GPU here: every rank must fail with the no-GPU message (from the CHILD ranks, not a launcher complaint), rc != 0
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode != 0
    assert "torch.distributed.run" in r.stderr and "--nproc-per-node=2" in r.stderr
    import torch
    if not torch.cuda.is_available():
        assert "needs a GPU" in r.stderr
    assert "must be launched with" not in r.stderr


def test_a_rank_with_the_wrong_world_size_is_refused():
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr


def test_dump_outputs_writes_float64_arrays_within_the_limit(tmp_path):
    """--dump-outputs: what the last timed step left in the result buffer, as <name>.npy in float64; image planes too large for the limit are cut to
    the same fixed, seeded pixel sample in every plane, so that two runs with the same arguments write the same set of values."""
    from types import SimpleNamespace
    import numpy as np
    N = 4096
    h = np.arange(7 * N * N + 1, dtype=np.float64)
    wl = SimpleNamespace(N=N)
    a, b = bench.ImagePlaneWorkload.outputs(wl, h), bench.ImagePlaneWorkload.outputs(wl, h)
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    pick = a["imageplane_nrays_sample"].astype(np.int64)
    assert len(pick) == bench.DUMP_SAMPLE_PIXELS and np.all(np.diff(pick) > 0)
    for q, k in enumerate(("flux", "r", "phi", "enshift", "time", "emis")):
        assert np.array_equal(a[f"imageplane_{k}_sample"], pick + (q + 1) * N * N)           # the same pixels in every plane
    assert a["imageplane_disc_rays"].tolist() == [7 * N * N]
    bench.dump_outputs(str(tmp_path / "out"), a, {"trace_counters": [3, 4]})
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == sorted([k + ".npy" for k in a] + ["trace_counters.npy"])
    assert sum(os.path.getsize(tmp_path / "out" / f) for f in files) <= bench.DUMP_LIMIT_BYTES
    got = np.load(tmp_path / "out" / "imageplane_r_sample.npy")
    assert got.dtype == np.float64 and np.array_equal(got, a["imageplane_r_sample"])
    assert np.load(tmp_path / "out" / "trace_counters.npy").tolist() == [3.0, 4.0]
    small = bench.ImagePlaneWorkload.outputs(SimpleNamespace(N=64), np.arange(7 * 64 * 64 + 1, dtype=np.float64))
    assert len(small["imageplane_nrays"]) == 64 * 64                                          # small images whole
    emis = bench.EmissivityWorkload.outputs(None, np.arange(5 * bench.NR + 1, dtype=np.float64))
    assert emis["emissivity_flux"].tolist() == list(range(bench.NR, 2 * bench.NR)) and emis["emissivity_disc_rays"].tolist() == [5 * bench.NR]
    rr = bench.ReturnRadiationWorkload.outputs(SimpleNamespace(nr=12), np.arange(48, dtype=np.float64))
    assert rr["return_radiation_table"].shape == (12, 4)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1)}, {})
