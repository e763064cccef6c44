"""The library's host-side index logic (csrc/reorder.cpp: orderings, L/U split, tiles, launch schedules, stencil tables; csrc/fluid_tables.cpp:
table blobs) built with g++ under AddressSanitizer + UBSan + libstdc++'s container assertions and run over grids from 1 to 729 000 rows,
decomposed subdomains with ghost columns, irregular patterns with rows of up to 20 blocks, every ordering and chain lengths from 1 to 64
(tests/san/host_logic_san.cpp, which also checks the invariants every ordering must keep).  No GPU: the harness serves the three HIP
runtime calls of reorder.cpp from the host heap.  The GPU sanitizers are not available on the pool; this is the CPU build the brief asks
to run them on.  The CPR pressure-AMG set-up (csrc/cpr_setup.cpp) is built the same way, linked alone (tests/san/cpr_setup_san.cpp: level
invariants on every hierarchy, the oracle's hierarchy alongside; the joined level of decomposed runs on small worlds of ranks).  So is the host set-up of the resident standard wells and analytic
aquifers (csrc/source_lists.cpp, linked alone; tests/san/source_lists_san.cpp: the grouping by distinct cell against a quadratic restatement,
every refusal with its code and its text, the aquifers' tables, step scalars and sums).  So is the check of scaled saturation end
points that opmhip_set_endpoint_scaling and opmhip_set_hysteresis share (end_points_refusal in csrc/fluid_tables.cpp, linked alone;
tests/san/end_points_san.cpp: accepted and refused inputs over three saturation regions built by build_fluid_tables)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opm-autodiff_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_reorder_and_fluid_tables_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "host_logic_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D_GLIBCXX_ASSERTIONS", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "san", "host_logic_san.cpp"), os.path.join(CSRC, "reorder.cpp"), os.path.join(CSRC, "fluid_tables.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("OPMHIP_TUNING", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert out.count("\nok  ") > 150   # every case of the list ran


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpr_setup_under_asan_ubsan(tmp_path):
    # cpr_setup.cpp alone, no HIP stand-ins: the link fails if the set-up half of the CPR calls the HIP runtime
    exe = str(tmp_path / "cpr_setup_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D_GLIBCXX_ASSERTIONS", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "san", "cpr_setup_san.cpp"), os.path.join(CSRC, "cpr_setup.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("OPMHIP_TUNING", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert out.count("; oracle agrees: levels, n, nc, agg, coarsest matrix\n") == 104   # every set-up of the list, each against the oracle
    for stop in ("rows", "stall", "width"):   # every rule that ends a hierarchy was met
        assert "(last: %s)" % stop in out
    # the joined level of a decomposed run (cpr_joined_aggregates / _rows / _values, cpr_join_rows): eight worlds of two and four ranks, each
    # against the whole system's Galerkin product; six spoiled buffers, each refused with its rank named
    assert out.count(": pattern and values are the whole system's Galerkin product\n") == 8 and "8 of 8 joined levels checked" in out
    assert out.count("\nok  refused: ") == 6 and "6 of 6 spoiled buffers refused" in out
    for world in ("transfers 0..0", "transfers 3..3", "ghost couplings 0:"):   # level 0 joined, several transfers composed, no coupling at all
        assert world in out


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_source_lists_under_asan_ubsan(tmp_path):
    # source_lists.cpp alone, no HIP stand-ins: the link fails if the set-up of the resident wells and aquifers calls the HIP runtime
    exe = str(tmp_path / "source_lists_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D_GLIBCXX_ASSERTIONS", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "san", "source_lists_san.cpp"), os.path.join(CSRC, "source_lists.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    lines = out.splitlines()   # every case of the lists ran
    assert sum(l.startswith("ok  group_by_cell: ") for l in lines) == 30 and sum(l.startswith("ok  refused: ") for l in lines) == 50
    assert sum(l.startswith("ok  ") for l in lines) == 93


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_end_points_refusal_under_asan_ubsan(tmp_path):
    # the check of scaled end points (end_points_refusal, csrc/fluid_tables.cpp) that opmhip_set_endpoint_scaling and opmhip_set_hysteresis
    # share; fluid_tables.cpp alone, no HIP stand-ins
    exe = str(tmp_path / "end_points_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D_GLIBCXX_ASSERTIONS", "-ffp-contract=off", os.path.join(ROOT, "tests", "san", "end_points_san.cpp"), os.path.join(CSRC, "fluid_tables.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    lines = out.splitlines()   # every case of the list ran
    assert sum(l.startswith("ok  accepted: ") for l in lines) == 11 and sum(l.startswith("ok  refused: ") for l in lines) == 15
