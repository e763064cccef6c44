"""The host set-up of the assembly (csrc/asm_setup.cpp) under AddressSanitizer + UBSan + libstdc++'s container assertions, as a stand-alone
program (tests/san/asm_setup_san.cpp) - no GPU.  The patterns are analysed by csrc/reorder.cpp, whose HIP runtime calls the program
serves from the host heap; asm_setup.cpp itself must make none, which its object file's undefined symbols show.  The tiles, the launch
schedule and the entry words of k_assemble on patterns of 1 cell, 7 and 9 tiles, two grids, one colour, ILU(1) and a decomposed
subdomain, at the shipped tile size and at a small one; the tile edges; every refusal of the static data, the water-compaction tables,
the end points and the source cells with its code, its text and the outputs untouched."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opm-autodiff_amd", "csrc")

PATTERNS = ("1 cell", "7 tiles", "9 tiles", "grid 3x3x3", "grid 5x4x3", "one colour", "ILU(1) on grid 3x3x3", "subdomain 3(+ghosts)x3x3, gids reversed")
SIZES = ("(T 64, cap 13)", "(T 8, cap 3)")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_asm_setup_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "asm_setup_san")
    flags = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
             "-D_GLIBCXX_ASSERTIONS", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
    # the unit alone: no undefined symbol of the HIP runtime
    obj = str(tmp_path / "asm_setup.o")
    b = subprocess.run(flags + ["-c", os.path.join(CSRC, "asm_setup.cpp"), "-o", obj], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    nm = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, timeout=60)
    assert nm.returncode == 0 and nm.stdout.strip(), nm.stderr
    assert not [l for l in nm.stdout.splitlines() if " hip" in l.lower() or " hsa" in l.lower()], nm.stdout
    b = subprocess.run(flags + [os.path.join(ROOT, "tests", "san", "asm_setup_san.cpp"), obj, os.path.join(CSRC, "reorder.cpp"),
                                os.path.join(CSRC, "fluid_tables.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("OPMHIP_TUNING", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    lines = out.splitlines()   # every case ran
    cases = ["plan: %s %s" % (p, s) for s in SIZES for p in PATTERNS]
    cases += ["tile edges: rows summing to T, T + 1, T - 1; single-entry runs of cap, cap + 1, 2 cap; a row of T + 1 blocks refused " + s for s in SIZES]
    cases += ["static data: accepted with ghost columns and with NULL thpres / pvtnum / satnum; every refusal, the earlier fault of two",
              "water compaction: 0, 1 and 2 tables, with and without trans_mult, the second table's offsets, nodes not ascending",
              "end points: a non-finite point names field and cell, a NULL field is the region's own, the refusal's text, the field-major internal-order layout",
              "eps_config: 432 option combinations",
              "source cells: n = 0, order of first mention, left-to-right sums bit for bit, dsource NULL, refusals in item order"]
    for case in cases:
        assert "ok  " + case in lines, case
    assert sum(l.startswith("ok  ") for l in lines) == len(cases) == 23
