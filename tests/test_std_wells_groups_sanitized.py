"""The checks and the packing of the resident wells' group production control (csrc/source_lists.cpp: std_wells_groups,
std_wells_groups_check_guide_rates, std_wells_group_targets, std_wells_groups_check_controls) under AddressSanitizer + UBSan + libstdc++'s
container assertions, as a stand-alone program (tests/san/std_wells_groups_san.cpp) - no GPU, no HIP runtime: the unit is linked alone, so
the link fails if it calls HIP.  Every refusal with its code and its text, the outputs untouched after it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opm-autodiff_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_std_wells_groups_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "std_wells_groups_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D_GLIBCXX_ASSERTIONS", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "san", "std_wells_groups_san.cpp"), os.path.join(CSRC, "source_lists.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    lines = out.splitlines()   # every case of the lists ran
    assert sum(l.startswith("ok  refused: ") for l in lines) == 35 and sum(l.startswith("ok  ") for l in lines) == 38
