"""The host set-up of the device-resident multisegment wells (csrc/ms_wells_setup.cpp: the list check with every refusal of
opmhip_set_ms_wells' index arrays, and the list's layout - descriptors, forms, the tree wells' index lists, segment rows, cells in the
internal order, shared cells) under AddressSanitizer + UBSan + libstdc++'s container assertions, as a stand-alone program
(tests/san/ms_wells_list_san.cpp) - no GPU, no HIP runtime, no Python in the process: the unit is linked alone, so the link fails if it
calls HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opm-autodiff_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_ms_wells_list_setup_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ms_wells_list_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D_GLIBCXX_ASSERTIONS", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "san", "ms_wells_list_san.cpp"), os.path.join(CSRC, "ms_wells_setup.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    lines = out.splitlines()   # every case ran: 15 refusals of the list check, 2 lists with two defects, 2 refusals of the layout, 4 layouts
    assert sum(l.startswith("ok  refused: ") for l in lines) == 19 and sum(l.startswith("ok  ") for l in lines) == 23
