"""CPU: the two ray-path programs build with the other device-resident programs and, without a GPU, fail loudly: exit status 1, the reason named,
no output file."""
import os
import subprocess

import pytest

import paths_rules as pr

ROOT = pr.ROOT
APPS = os.path.join(ROOT, "raytrace_cpu_amd", "apps")


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", APPS], check=True)
    return os.path.join(APPS, "_build")


def test_programs_build(built):
    for app in ("kr_trace_rays", "kr_trace_rays_imageplane"):
        assert os.access(os.path.join(built, app), os.X_OK), app


@pytest.mark.parametrize("case", ["ps_euler", "ip_euler"])
def test_programs_fail_loudly_without_gpu(built, case, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    exe = os.path.join(built, pr.APP_OF[case])
    argv = [exe, pr.par_path(case)] if case.startswith("ip_") else [exe, f"--parfile={pr.par_path(case)}"]
    r = subprocess.run(argv, cwd=tmp_path, capture_output=True, text=True, timeout=120)      # (the fixtures name outfile = out.txt, relative)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "no HIP device available" in r.stderr
    assert not (tmp_path / "out.txt").exists() and os.listdir(tmp_path) == []


def test_missing_par_file_is_an_error(built, tmp_path):
    for app in ("kr_trace_rays", "kr_trace_rays_imageplane"):
        r = subprocess.run([os.path.join(built, app), "--parfile=/nonexistent.par"] if app == "kr_trace_rays" else [os.path.join(built, app), "/nonexistent.par"],
                           cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and r.stderr.strip()
