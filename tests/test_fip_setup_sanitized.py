"""The host set-up of the fluid-in-place report (csrc/fip_setup.cpp) under AddressSanitizer + UBSan + libstdc++'s container assertions, as a
stand-alone program (tests/san/fip_setup_san.cpp) - no GPU, no HIP runtime, no include path of one: the unit is compiled and linked alone,
so the build fails if it includes or calls HIP.  The plans of regions of 1, 63, 64, 65, 255, 256, 257, 511, 513 and 65 537 cells - index
ranges, then the descriptors walked lane by lane against a restatement of the stated order -, the degenerate plans, every refusal with
its code, its text and the outputs untouched, and pressureAverage_ on both sides of its threshold."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opm-autodiff_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fip_setup_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "fip_setup_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D_GLIBCXX_ASSERTIONS", "-ffp-contract=off", os.path.join(ROOT, "tests", "san", "fip_setup_san.cpp"), os.path.join(CSRC, "fip_setup.cpp"),
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
    for case in ("plans: 1, 63, 64, 65, 255, 256, 257, 511, 513 and 65 537 cells in a region", "plans: no regions, no cells, every cell its own region",
                 "refused: count, null arrays, id above Nb, ranks, ghosts; accepted: id == Nb, 16 sets, none; the calls' checks",
                 "pressure averages: both weights, the 1e-10 threshold, no pore volume"):
        assert "ok  " + case in lines, case
    assert sum(l.startswith("ok  ") for l in lines) == 4
