"""GPU: the two device-resident ray-path programs on the fixture parameter files write the file the reference's programs wrote
(tests/golden/paths/; the block rule of tests/paths_rules.py)."""
import os
import subprocess

import pytest

import parity
import paths_rules as pr

pytestmark = pytest.mark.gpu
APPS = os.path.join(pr.ROOT, "raytrace_cpu_amd", "apps", "_build")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-s", "-C", os.path.dirname(APPS)], check=True)


@pytest.mark.parametrize("case", sorted(pr.APP_OF))
def test_program_writes_the_reference_file(case, tmp_path):
    exe = os.path.join(APPS, pr.APP_OF[case])
    argv = [exe, pr.par_path(case), "--timing"] if case.startswith("ip_") else [exe, f"--parfile={pr.par_path(case)}", "--timing"]
    r = subprocess.run(argv, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout.strip().splitlines()[-2])
    got = open(tmp_path / "out.txt").read()
    want = pr.reference_text(case)
    res = pr.compare_texts(got, want)
    params, _, _ = pr.case_inputs(case)
    allowed = parity.allowed_bad_frac_strict(params, res["n_traced"])
    print(f"program {pr.APP_OF[case]} on {case}: blocks {res['n_blocks_got']} / {res['n_traced']}, byte-identical blocks {res['frac_blocks_identical']:.4f}, "
          f"bad rays {res['n_bad']}, whole file identical: {got == want}")
    parity.record_margin("test_program_writes_the_reference_file", case, res, allowed=allowed, frac_blocks_identical=res["frac_blocks_identical"],
                         file_identical=bool(got == want))
    assert res["n_blocks_got"] == res["n_traced"]
    assert res["frac_bad"] <= allowed, res


def test_outfile_option_of_trace_rays(tmp_path):
    out = tmp_path / "named.txt"
    r = subprocess.run([os.path.join(APPS, "kr_trace_rays"), f"--parfile={pr.par_path('ps_euler')}", f"--outfile={out}"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.exists() and not (tmp_path / "out.txt").exists()
    assert len(pr.blocks_of(out.read_text())) == 35
