"""tools/ab.py, the A/B runner of the measuring runs, on the CPU: the plan it writes, and its stop rule with stand-ins for bench.py
(tiny scripts that write a detail record, append one line to a marker file and leave with a given exit status)."""
import importlib.util
import json
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB_PATH = os.path.join(ROOT, "tools", "ab.py")
OTHER_TRACING = ("--sys-trace", "--runtime-trace", "--hip-trace", "--hsa-trace", "--memory-copy-trace", "--scratch-memory-trace",
                 "--marker-trace")


@pytest.fixture
def ab():
    spec = importlib.util.spec_from_file_location("ab_under_test", AB_PATH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def stand_in(tmp_path, fail_at=0, status=0, sleep=0.0):
    """A bench.py stand-in: the fail_at-th call (counted in the marker file) sleeps `sleep` s and leaves with `status`."""
    marker = tmp_path / "marker.txt"
    marker.write_text("")
    script = tmp_path / "stand_in.py"
    script.write_text(textwrap.dedent("""\
        import json, os, sys, time
        marker = %r
        with open(marker, "a") as fh:
            fh.write(" ".join(sys.argv[1:]) + " HP=" + os.environ.get("OPMHIP_HALF_PRODUCT", "-") + "\\n")
        with open(marker) as fh:
            calls = len(fh.readlines())
        if calls == %d:
            time.sleep(%r)
            print("stand-in failing on call %%d" %% calls, file=sys.stderr)
            sys.exit(%d)
        detail = sys.argv[sys.argv.index("--detail") + 1]
        with open(detail, "w") as fh:
            json.dump({"value": 90.0 + calls, "linear_iterations_per_newton": 17.05,
                       "kernels": {"spmv": {"avg_ms": 0.0779}, "ilu_apply": {"avg_ms": 0.0612}}}, fh)
        sys.exit(0)
        """ % (str(marker), fail_at, sleep, status)))
    return str(script), marker


def plan_of(out):
    with open(os.path.join(out, "plan.json")) as fh:
        return json.load(fh)["steps"]


def check_gpu_steps(steps):
    gpu = [s for s in steps if s["gpu"]]
    assert gpu
    for s in gpu:
        assert s["cmd"][:3] == ["timeout", "-k", "10"] and int(s["cmd"][3]) > 0, s["cmd"]
        if "rocprofv3" in s["cmd"]:
            assert s["cmd"][s["cmd"].index("--") + 1] == sys.executable, s["cmd"]
            if "--pmc" in s["cmd"]:
                assert s["cmd"].count("--pmc") == 1
                assert not set(OTHER_TRACING) & set(s["cmd"]), s["cmd"]
    return gpu


def test_run_plan_alternates_and_sets_the_tuning_switch(ab, tmp_path):
    out = str(tmp_path / "out")
    rc = ab.main(["run", out, "--rounds", "2", "--dry-run", "--rocprof-stats", "--variant", "base",
                  "--variant", "hp0 OPMHIP_HALF_PRODUCT=0", "--variant", "cl8 --chain-length 8", "--variant", "other FOO=1"])
    assert rc == 0
    steps = check_gpu_steps(plan_of(out))
    assert [s["label"] for s in steps] == ["base.1", "hp0.1", "cl8.1", "other.1", "base.2", "hp0.2", "cl8.2", "other.2"]
    for s in steps:
        assert s["cmd"][s["cmd"].index("--") + 2] == "bench.py"
        assert s["cmd"][-2:] == ["--detail", os.path.join(out, s["label"] + ".json")]
        tuning = s["env"].get("OPMHIP_TUNING")
        assert tuning == ("1" if s["label"].startswith("hp0") else None), s
    assert "--chain-length" in steps[2]["cmd"] and "--chain-length" not in steps[0]["cmd"]
    assert steps[3]["env"] == {"FOO": "1"}


def test_lib_variant_alone_leaves_the_tuning_switch_off(ab, tmp_path):
    out = str(tmp_path / "out")
    lib = tmp_path / "build_variants"
    lib.mkdir()
    ab.ROOT = str(tmp_path)
    (lib / "libopmhip_nt.so").write_bytes(b"")
    assert ab.main(["run", out, "--dry-run", "--rounds", "1", "--variant", "base", "--variant", "nt lib:nt"]) == 0
    steps = plan_of(out)
    assert steps[1]["env"] == {"OPMHIP_LIB": "build_variants/libopmhip_nt.so"}
    assert ab.main(["run", out, "--dry-run", "--rounds", "1", "--variant", "nthp lib:nt OPMHIP_HALF_PRODUCT=0"]) == 0
    assert plan_of(out)[0]["env"]["OPMHIP_TUNING"] == "1"


def test_pmc_and_snapshot_plans(ab, tmp_path):
    out = str(tmp_path / "pmc")
    assert ab.main(["pmc", out, "--dry-run", "FETCH_SIZE", "TCC_HIT_sum TCC_MISS_sum"]) == 0
    gpu = check_gpu_steps(plan_of(out))
    assert len(gpu) == 2
    for s, group in zip(gpu, (["FETCH_SIZE"], ["TCC_HIT_sum", "TCC_MISS_sum"])):
        c = s["cmd"]
        i = c.index("--pmc") + 1
        assert c[i:i + len(group)] == group and c[i + len(group)].startswith("--")
    snap = str(tmp_path / "snap")
    assert ab.main(["snapshot", "check", "--out", snap, "--dry-run"]) == 0
    gpu = check_gpu_steps(plan_of(snap))
    assert len(gpu) == 5 and sum("--stats" in s["cmd"] for s in gpu) == 1 and sum("--pmc" in s["cmd"] for s in gpu) == 3
    assert not os.path.exists(os.path.join(snap, "check_bench.json"))


def test_refusals_before_any_step(ab, tmp_path, capsys):
    ab.BENCH, marker = stand_in(tmp_path)
    out = str(tmp_path / "out")
    assert ab.main(["run", out, "--variant", "base", "--variant", "nt lib:no_such_variant"]) != 0
    assert "libopmhip_no_such_variant.so" in capsys.readouterr().err
    assert ab.main(["run", out, "--variant", "a", "--variant", "a OPMHIP_HALF_PRODUCT=0"]) != 0
    assert "not unique" in capsys.readouterr().err
    assert marker.read_text() == ""
    assert not os.path.exists(os.path.join(out, "plan.json"))


@pytest.mark.parametrize("status, klass", [(3, "other"), (134, "abort")])
def test_a_failed_step_ends_the_invocation(ab, tmp_path, capsys, status, klass):
    ab.BENCH, marker = stand_in(tmp_path, fail_at=2, status=status)
    rc = ab.main(["run", str(tmp_path / "out"), "--rounds", "2", "--variant", "base", "--variant", "hp0 OPMHIP_HALF_PRODUCT=0"])
    assert rc != 0
    lines = marker.read_text().splitlines()
    assert len(lines) == 2 and lines[1].endswith("HP=0")
    err = capsys.readouterr().err
    assert "'hp0.1' failed: %s (exit status %d)" % (klass, status) in err
    assert "stand-in failing on call 2" in err


def test_a_step_past_its_limit_is_a_time_limit(ab, tmp_path, capsys):
    ab.BENCH, marker = stand_in(tmp_path, fail_at=1, sleep=60.0)
    rc = ab.main(["run", str(tmp_path / "out"), "--bench-limit", "2", "--variant", "base", "--variant", "hp0 OPMHIP_HALF_PRODUCT=0"])
    assert rc != 0
    assert len(marker.read_text().splitlines()) == 1
    assert "'base.1' failed: time limit" in capsys.readouterr().err


def test_the_table_carries_the_detail_columns(ab, tmp_path, capsys):
    ab.BENCH, marker = stand_in(tmp_path)
    out = str(tmp_path / "out")
    rc = ab.main(["run", out, "--rounds", "2", "--cols", "value", "its", "kernels.spmv.avg_ms", "steady",
                  "--variant", "base", "--variant", "hp0 OPMHIP_HALF_PRODUCT=0"])
    assert rc == 0
    assert len(marker.read_text().splitlines()) == 4
    labels = ("base.1", "hp0.1", "base.2", "hp0.2")
    rows = {w[0]: w[1:] for w in map(str.split, capsys.readouterr().out.splitlines()) if w and w[0] in labels}
    assert rows == {"base.1": ["91", "17.05", "0.0779", "-"], "hp0.1": ["92", "17.05", "0.0779", "-"],
                    "base.2": ["93", "17.05", "0.0779", "-"], "hp0.2": ["94", "17.05", "0.0779", "-"]}


def test_importing_the_runner_leaves_torch_out():
    code = "import importlib.util, sys; s = importlib.util.spec_from_file_location('ab', %r); m = importlib.util.module_from_spec(s); " \
           "s.loader.exec_module(m); sys.exit('torch' in sys.modules)" % AB_PATH
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0
