"""The host set-up of the passive tracers (csrc/tracers_setup.cpp) under AddressSanitizer + UBSan + libstdc++'s container assertions, as a
stand-alone program (tests/san/tracers_san.cpp) - no GPU, no HIP runtime: the unit is linked with csrc/source_lists.cpp alone, so the link
fails if it calls HIP.  The level sets of a 4 x 3 x 2 pattern in the natural, a coloured and a line-coloured order against a restatement,
the rows' faces in natural column order, the phase batches, the grouping of connections by distinct cell, and every refusal with its
code, its text and the outputs untouched."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opm-autodiff_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_tracers_setup_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "tracers_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D_GLIBCXX_ASSERTIONS", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "san", "tracers_san.cpp"), os.path.join(CSRC, "tracers_setup.cpp"), os.path.join(CSRC, "source_lists.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    lines = out.splitlines()   # every case ran
    for case in ("levels: natural order", "levels: two colours", "levels: line colouring", "levels: a single row", "levels: no rows",
                 "refused: gas, phase, PVTG, ranks, ghosts, null arrays, count, non-finite, cap", "accepted: batches, the cap itself, none",
                 "refused: solver constants", "connections: a cell named twice keeps its connections in list order", "refused: connections"):
        assert "ok  " + case in lines, case
    assert sum(l.startswith("ok  ") for l in lines) == 10
