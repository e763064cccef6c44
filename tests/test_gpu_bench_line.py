"""bench.py's one JSON line on a small grid: the keys the driver's contract names are there, with the roofline and (--full) the CPU
baseline objects, the numbers hang together, and the line stays short enough for the driver to parse from the tail of stdout (round 4's
22 KB line was cut in half); the full record is in the file the line names."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_contract(tmp_path):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    detail = str(tmp_path / "detail.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--n", "24", "--steps", "4", "--warmup", "2", "--steady-after", "8",
                        "--steady-steps", "3", "--detail", detail], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.strip().splitlines()
    lines = [ln for ln in out if ln.startswith("{")]
    assert len(lines) == 1 and out[-1] == lines[0]       # the LAST line of stdout is the one JSON object
    assert len(lines[0]) < 4096, len(lines[0])
    d = json.loads(lines[0])
    full = json.load(open(detail))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["scaling"] == "weak" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-3 * d["value"]     # both rounded to four decimals in the line
    ro = d["roofline"]
    assert ro["bound"] == "hbm" and ro["unit"] == "GB/s" and ro["peak"] == 8000.0 and abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-4
    assert ro["traffic"] is None     # PMC traffic is only quoted for the 100^3 configuration it was measured on
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb and cb["linear_solve_GBps"] > 0
    fcb = full["cpu_baseline"]
    assert fcb["host"]["physical_cores_in_mask"] >= 1 and abs(fcb["value"] - cb["value"]) < 1e-3
    assert cb["cores"] == 1 or str(cb["cores"]) in fcb["host"]["thread_sweep_newton_its_per_s"]
    assert d["full"] is True and d["steady_state"]["value"] > 0 and full["steady_state"]["steps"] == 3 and d["stream_read_GBps"] > 0
    # no ordering / smoother flag was passed: the line reports what the library chose (a 24^3 grid: the greedy colouring, red-black)
    assert d["config"]["ilu_ordering"] == "graph_coloring_greedy" and d["config"]["ilu_colors"] == 2 and d["config"]["ilu_chain_length"] == 0
    assert d["config"]["ilu_ordering_chosen_by"].startswith("library default") and d["cpr_amg_ilu_levels"] == 1
    # Flow's "cpr" (true-IMPES weights) and the quasi-IMPES variant, side by side under their reference names
    assert d["cpr"]["value"] > 0 and d["cpr_quasiimpes"]["value"] > 0 and d["cpr_reuse_setup_2"]["value"] > 0 and "rccl" not in d
    assert full["cpr"]["kernels"]["cpr_amg"]["launches"] > 0 and full["kernels"]["spmv"]["launches"] > 0


def test_dump_outputs_are_the_last_timed_newton_iteration(tmp_path, pkg):
    """--dump-outputs: two runs with the same arguments write the same arrays bit for bit, and they are what the simulation holds after
    exactly --warmup + --steps Newton iterations (the state, the last linear solve's update, that iteration's CNV norms)"""
    import importlib.util
    import numpy as np
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    n, steps, warmup = 16, 3, 2
    runs = []
    for k in range(2):
        d = tmp_path / ("dump%d" % k)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--n", str(n), "--steps", str(steps), "--warmup", str(warmup),
                            "--steady-after", "0", "--no-cpr-side-run", "--no-cpu-baseline", "--detail", str(tmp_path / ("detail%d.json" % k)),
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == steps and line["ms_per_step"] > 0
        names = sorted(os.listdir(d))
        assert names == ["cnv_residual_norms.npy", "newton_update.npy", "primary_variable_meaning.npy", "primary_variables.npy", "time_stepping.npy"]
        runs.append({f: np.load(d / f) for f in names})
    assert all(np.array_equal(runs[0][f], runs[1][f]) for f in runs[0])
    assert all(a.dtype in (np.float32, np.float64) for a in runs[0].values())

    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    case = pkg.decks.cartesian_case(n, n, n, state="mixed", heterogeneous=False)
    src = pkg.decks.five_spot_source(case, rate_sm3_per_day=pkg.decks.BENCH_RATE_SM3_PER_DAY * (n / 100.0) ** 2)
    model = pkg.capi.HipModel(case, device_id=0, tolerance=1e-2, maxit=200, ilu_relaxation=0.9, fused_reductions=0)
    model.set_state(case["pv"], case["meaning"])
    model.set_source(src)
    sim = bench.make_simulation(pkg, model)
    for _ in range(warmup + steps):
        sim.next_newton_iteration()
    pv, meaning = model.get_state()
    d = runs[0]
    assert np.array_equal(d["primary_variables.npy"], pv.reshape(-1, 3))
    assert np.array_equal(d["primary_variable_meaning.npy"], meaning.astype(np.float32))
    assert np.array_equal(d["newton_update.npy"], model.get_result().reshape(-1, 3))
    assert np.array_equal(d["cnv_residual_norms.npy"], np.array(sim.model.residual_norms_history[-1]))
    assert np.array_equal(d["time_stepping.npy"], np.array([sim.time, sim.dt, sim.iteration, sim.model.last_linear_iterations], np.float64))


def test_plain_run_times_the_steps_of_a_full_run_and_nothing_else(tmp_path):
    """without --full the run sets up, warms up, times the steps, dumps and prints: the line carries the contract's keys and what the timed
    steps' own profile gives (kernel scopes, the roofline's achieved bandwidth), none of the extras; and its timed steps are those of a --full
    run of the same arguments - the same linear iterations and time steps, the same arrays after the last of them, bit for bit"""
    import numpy as np
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    n, steps, warmup = 16, 3, 2
    runs = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--steady-after", "8", "--steady-steps", "2", "--no-cpr-side-run", "--no-cpu-baseline"])):
        detail, dump = tmp_path / (mode + ".json"), tmp_path / mode
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--n", str(n), "--steps", str(steps), "--warmup", str(warmup),
                            "--detail", str(detail), "--dump-outputs", str(dump)] + extra, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[mode] = (json.loads(r.stdout.strip().splitlines()[-1]), json.load(open(detail)), {f: np.load(dump / f) for f in sorted(os.listdir(dump))})
    d, rec, arrays = runs["plain"]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config", "roofline", "kernel_GBps"):
        assert k in d, k
    assert d["full"] is False and d["steps"] == steps and d["warmup"] == warmup and abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-3 * d["value"]
    assert d["roofline"]["achieved"] > 0 and d["kernel_GBps"]["spmv"] > 0 and "full_spmv" not in d["roofline"] and d["roofline"]["frac_of_stream_ceiling"] is None
    assert "cpu_baseline" not in d and d["steady_state"] is None and d["stream_read_GBps"] is None and "plugin" not in d and "cpr" not in d
    assert "cpu_baseline" not in rec and rec["stream_ceiling"] is None and rec["plugin"] is None
    assert all(rec[k] is None for k in ("steady_state", "cpr", "cpr_quasiimpes", "cpr_amg_jacobi_smoother", "cpr_reuse_setup_2", "cpr_reuse_setup_2_sync"))
    fd, frec, farrays = runs["full"]
    assert fd["full"] is True and fd["steady_state"]["value"] > 0 and fd["stream_read_GBps"] > 0
    assert rec["linear_iterations_per_newton"] == frec["linear_iterations_per_newton"] and rec["time_steps_days"] == frec["time_steps_days"]
    assert sorted(arrays) == sorted(farrays) and all(np.array_equal(arrays[f], farrays[f]) for f in arrays)
