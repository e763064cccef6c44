"""The host set-up of the open boundaries (csrc/boundary_setup.cpp) under AddressSanitizer + UBSan + libstdc++'s container assertions, as a
stand-alone program (tests/san/boundary_setup_san.cpp) - no GPU: the unit is linked with csrc/source_lists.cpp (the grouping by distinct
cell) and with no stand-in for a HIP runtime call, so the build fails if the set-up calls one.  The lists of a 9 x 9 x 2 box with all six
sides (234 faces, 162 distinct cells), of 3 x 1 x 1 (five faces per cell), of one cell and of one face against a quadratic restatement;
every refusal with its code, its text and the outputs untouched."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opm-autodiff_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_boundary_setup_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "boundary_setup_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D_GLIBCXX_ASSERTIONS", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "san", "boundary_setup_san.cpp"), os.path.join(CSRC, "boundary_setup.cpp"), os.path.join(CSRC, "source_lists.cpp"),
           "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    lines = out.splitlines()   # every case ran
    assert sum(l.startswith("ok  lists: ") for l in lines) == 1 and sum(l.startswith("ok  refused: ") for l in lines) == 1
    assert sum(l.startswith("ok  ") for l in lines) == 2
