#!/usr/bin/env python3
"""tools/ab.py: the measuring runs of this directory, one child process at a time, stopping at the first one that fails.

    python3 tools/ab.py run OUT --variant SPEC [--variant SPEC ...] [--rounds N] [--cols COL ...] [--bench-args "..."]
                                [--rocprof-stats] [--program "SCRIPT ARGS"]
    python3 tools/ab.py pmc OUT [--script "SCRIPT ARGS"] GROUP [GROUP ...]
    python3 tools/ab.py snapshot NAME [--out DIR]
    options of every subcommand: --build NAME="-DFLAG ..." (repeatable), --dry-run, --bench-limit / --stats-limit / --pmc-limit SECONDS

run       bench.py under each variant, alternating round by round (A B A B for two variants and --rounds 2), one table row per run.
          SPEC is one string: its first token is the label; then NAME=value sets an environment variable, lib:NAME loads
          build_variants/libopmhip_NAME.so (OPMHIP_LIB), anything else is passed to bench.py.  A variant that sets an OPMHIP_*
          switch other than OPMHIP_LIB gets OPMHIP_TUNING=1 (the library reads its measurement switches only under it).
          The rows come from bench.py --detail OUT/<label>.<round>.json.  --rocprof-stats: each run under rocprofv3
          --kernel-trace --stats, keeping OUT/<label>.<round>_kernel_stats.csv.  --program: another measuring script in place of
          bench.py (no base arguments, no --detail); its output is passed through.
pmc       one rocprofv3 --kernel-trace --pmc GROUP run per counter group (a group is one quoted string of counters) and nothing else
          traced, folded by pmc_summary.py (OUT/pmc_summary.txt) and pmc_to_json.py (OUT/pmc_traffic.json).
snapshot  the four files of a profiles/ snapshot under DIR (default snapshots/NAME, git-ignored): NAME_bench.json (+ _detail.json, with the CPU
          baseline and the CPR side runs), NAME_bench_under_rocprof.json (+ _detail.json) with NAME_kernel_stats.csv, NAME_pmc_traffic.json.

Before the first GPU step every check that can fail runs (labels unique, every lib: file present after the --build variants are
compiled with `make variant`), and OUT/plan.json records every command and environment that will run; --dry-run stops there.
Every GPU step runs under `timeout -k 10 LIMIT`.  The first step that leaves with a non-zero status ends the invocation: no later
step starts, the failed step, its class (time limit, abort, segmentation fault, other) and the tail of its stderr are printed,
and the exit status is 1.  There is no retry.  Standard library only: this process never opens the GPU itself.
"""
import argparse
import glob
import json
import os
import shlex
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = "bench.py"   # relative to ROOT, where every step runs
BASE_ARGS = ["--full", "--steps", "20", "--warmup", "5", "--steady-after", "0", "--no-cpu-baseline", "--no-cpr-side-run"]   # --full: the kernel probes run (column `stream`), --steady-after N opens the steady window
PMC_SCRIPT = "bench.py --full --steps 6 --warmup 1 --no-cpu-baseline --steady-after 0 --no-cpr-side-run"
SNAPSHOT_GROUPS = ["FETCH_SIZE", "WRITE_SIZE", "TCC_HIT_sum TCC_MISS_sum"]
DEFAULT_COLS = ["value", "its", "kernels.spmv.avg_ms", "kernels.ilu_apply.avg_ms", "kernels.ilu_factor.avg_ms", "kernels.vector.avg_ms"]
ALIASES = {"value": "value", "steady": "steady_state.value", "its": "linear_iterations_per_newton", "stream": "stream_ceiling.read_GBps"}


class Stop(Exception):
    """A check or a step failed: nothing further runs."""


def exit_class(rc):
    if rc in (124, 137):
        return "time limit"
    if rc in (134, -6):
        return "abort"
    if rc in (139, -11):
        return "segmentation fault"
    return "other"


# ---- the plan: a list of steps, each one child process ---------------------------------------------------------------------------
def step(label, cmd, out, err, env=None, limit=None, keep=None):
    """limit: a GPU step, run as `timeout -k 10 limit cmd`; keep: (directory, glob pattern, file) - copy the one match out of the
    directory once the step has succeeded, then remove the directory."""
    if limit is not None:
        cmd = ["timeout", "-k", "10", str(limit)] + cmd
    return {"label": label, "gpu": limit is not None, "cmd": cmd, "env": env or {}, "stdout": out, "stderr": err, "keep": keep}


def rocprof_stats(raw, cmd):
    return ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", raw, "-o", "bench", "--"] + cmd


def pmc_steps(out, script, groups, limit):
    steps = []
    for i, group in enumerate(groups, 1):
        prog = [sys.executable] + shlex.split(script)
        cmd = ["rocprofv3", "--kernel-trace", "--pmc"] + group.split() + ["--output-format", "csv", "-d", os.path.join(out, "p%d" % i),
                                                                          "-o", "p", "--"] + prog
        steps.append(step("pmc %d: %s" % (i, group), cmd, os.path.join(out, "p%d.log" % i), os.path.join(out, "p%d.err" % i), limit=limit))
    tools = os.path.join(ROOT, "tools")
    steps.append(step("pmc summary", [sys.executable, os.path.join(tools, "pmc_summary.py"), out],
                      os.path.join(out, "pmc_summary.txt"), os.path.join(out, "pmc_summary.err")))
    steps.append(step("pmc fold", [sys.executable, os.path.join(tools, "pmc_to_json.py"), out, os.path.join(out, "pmc_traffic.json")],
                      os.path.join(out, "pmc_fold.txt"), os.path.join(out, "pmc_fold.err")))
    return steps


def parse_variant(spec):
    tokens = shlex.split(spec)
    if not tokens:
        raise Stop("empty --variant")
    label, env, args = tokens[0], {}, []
    for t in tokens[1:]:
        if t.startswith("lib:"):
            env["OPMHIP_LIB"] = "build_variants/libopmhip_%s.so" % t[4:]
        elif "=" in t and not t.startswith("-") and t.split("=", 1)[0].isidentifier():
            k, v = t.split("=", 1)
            env[k] = v
        else:
            args.append(t)
    if any(k.startswith("OPMHIP_") and k != "OPMHIP_LIB" for k in env):
        env["OPMHIP_TUNING"] = "1"
    return label, env, args


def plan_run(a, out):
    variants = [parse_variant(s) for s in a.variant]
    labels = [v[0] for v in variants]
    if len(set(labels)) != len(labels):
        raise Stop("labels are not unique: %s" % " ".join(labels))
    steps = []
    for rnd in range(1, a.rounds + 1):
        for label, env, args in variants:
            name = "%s.%d" % (label, rnd)
            if a.program:
                cmd = [sys.executable] + shlex.split(a.program) + shlex.split(a.bench_args) + args
            else:
                cmd = [sys.executable, BENCH] + BASE_ARGS + shlex.split(a.bench_args) + args + ["--detail", os.path.join(out, name + ".json")]
            limit, keep = a.bench_limit, None
            if a.rocprof_stats:
                raw = os.path.join(out, name + "_rocprof")
                cmd, limit = rocprof_stats(raw, cmd), a.stats_limit
                keep = (raw, "*kernel_stats.csv", os.path.join(out, name + "_kernel_stats.csv"))
            steps.append(dict(step(name, cmd, os.path.join(out, name + ".out"), os.path.join(out, name + ".err"), env, limit, keep),
                              detail=None if a.program else os.path.join(out, name + ".json")))
    return steps


def plan_snapshot(a, out):
    n = a.name
    f = lambda suffix: os.path.join(out, n + suffix)   # noqa: E731
    full = [sys.executable, BENCH, "--full", "--steps", "20", "--warmup", "5"]
    raw = os.path.join(out, "rocprof")
    return [step("bench", full + ["--detail", f("_bench_detail.json")], f("_bench.json"), os.path.join(out, "bench.err"), limit=a.bench_limit),
            step("bench under rocprofv3 --stats",
                 rocprof_stats(raw, full + ["--no-cpu-baseline", "--detail", f("_bench_under_rocprof_detail.json")]),
                 f("_bench_under_rocprof.json"), os.path.join(out, "rocprof.err"), limit=a.stats_limit,
                 keep=(raw, "*kernel_stats.csv", f("_kernel_stats.csv")))] + \
        pmc_steps(os.path.join(out, "pmc"), PMC_SCRIPT, SNAPSHOT_GROUPS, a.pmc_limit)


# ---- running -----------------------------------------------------------------------------------------------------------------------
def tail(path, lines=20):
    try:
        with open(path, errors="replace") as fh:
            return "".join(fh.readlines()[-lines:])
    except OSError:
        return ""


def execute(s, index, total):
    os.makedirs(os.path.dirname(s["stdout"]), exist_ok=True)
    print("[%d/%d] %s" % (index, total, s["label"]), flush=True)
    with open(s["stdout"], "w") as so, open(s["stderr"], "w") as se:
        rc = subprocess.run(s["cmd"], cwd=ROOT, env=dict(os.environ, **s["env"]), stdout=so, stderr=se).returncode
    if rc != 0:
        raise Stop("step %d/%d '%s' failed: %s (exit status %d)\n--- %s (tail) ---\n%s"
                   % (index, total, s["label"], exit_class(rc), rc, s["stderr"], tail(s["stderr"])))
    if s["keep"]:
        src_dir, pattern, dst = s["keep"]
        found = sorted(glob.glob(os.path.join(src_dir, "**", pattern), recursive=True))
        if not found:
            raise Stop("step %d/%d '%s': no %s under %s" % (index, total, s["label"], pattern, src_dir))
        shutil.copyfile(found[0], dst)
        shutil.rmtree(src_dir)


def column(d, col):
    for key in ALIASES.get(col, col).split("."):
        if not isinstance(d, dict) or key not in d:
            return "-"
        d = d[key]
    return "%.4g" % d if isinstance(d, float) else str(d)


def build_variants(builds):
    for spec in builds:
        name, _, flags = spec.partition("=")
        cmd = ["make", "-B", "-j8", "-C", os.path.join(ROOT, "opm-autodiff_amd"), "variant", "NAME=" + name, "EXTRA=" + flags]
        print("build %s: %s" % (name, " ".join(shlex.quote(c) for c in cmd)), flush=True)
        if subprocess.run(cmd).returncode != 0:
            raise Stop("build of variant %s failed" % name)


def main(argv=None):
    common = argparse.ArgumentParser(add_help=False)
    common.add_argument("--build", action="append", default=[], metavar='NAME="-DFLAG ..."',
                        help="compile build_variants/libopmhip_NAME.so under these extra flags before any GPU step")
    common.add_argument("--dry-run", action="store_true", help="print the plan (and build the --build variants), run nothing on the GPU")
    common.add_argument("--bench-limit", type=int, default=300, help="seconds for one bench.py run (default 300)")
    common.add_argument("--stats-limit", type=int, default=400, help="seconds for one run under rocprofv3 --stats (default 400)")
    common.add_argument("--pmc-limit", type=int, default=150, help="seconds for one counter pass (default 150)")
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run", parents=[common])
    r.add_argument("out")
    r.add_argument("--variant", action="append", required=True, metavar="SPEC")
    r.add_argument("--rounds", type=int, default=2)
    r.add_argument("--cols", nargs="+", default=DEFAULT_COLS, help="value, steady, its, stream or a dotted key of the detail record")
    r.add_argument("--bench-args", default="", help="extra arguments of every run, e.g. \"--preconditioner cpr\"")
    r.add_argument("--rocprof-stats", action="store_true")
    r.add_argument("--program", default=None, help="another measuring script and its arguments, in place of bench.py")
    p = sub.add_parser("pmc", parents=[common])
    p.add_argument("out")
    p.add_argument("--script", default=PMC_SCRIPT, help="the script under the counters and its arguments (default: %(default)s)")
    p.add_argument("groups", nargs="+", metavar="GROUP")
    s = sub.add_parser("snapshot", parents=[common])
    s.add_argument("name")
    s.add_argument("--out", default=None, help="directory of the files (default snapshots/NAME)")
    a = ap.parse_args(argv)

    try:
        if a.cmd == "run":
            out = os.path.abspath(a.out)
            steps = plan_run(a, out)
        elif a.cmd == "pmc":
            out = os.path.abspath(a.out)
            steps = pmc_steps(out, a.script, a.groups, a.pmc_limit)
        else:
            out = os.path.abspath(a.out or os.path.join(ROOT, "snapshots", a.name))
            steps = plan_snapshot(a, out)
        build_variants(a.build)
        missing = sorted({s["env"]["OPMHIP_LIB"] for s in steps if "OPMHIP_LIB" in s["env"]
                          and not os.path.exists(os.path.join(ROOT, s["env"]["OPMHIP_LIB"]))})
        if missing:
            raise Stop("missing variant libraries (build them with --build NAME=\"-D...\"): %s" % " ".join(missing))
        os.makedirs(out, exist_ok=True)
        plan = {"root": ROOT, "builds": a.build, "steps": steps}
        with open(os.path.join(out, "plan.json"), "w") as fh:
            json.dump(plan, fh, indent=1)
        for i, s in enumerate(steps, 1):
            print("%2d. %s" % (i, " ".join(["%s=%s" % kv for kv in sorted(s["env"].items())] + [shlex.quote(c) for c in s["cmd"]])))
        if a.dry_run:
            return 0

        if a.cmd == "run" and not a.program:
            print("%-16s %s" % ("variant.round", "  ".join("%14s" % c for c in a.cols)), flush=True)
        for i, s in enumerate(steps, 1):
            execute(s, i, len(steps))
            if s.get("detail"):
                try:
                    with open(s["detail"]) as fh:
                        d = json.load(fh)
                except (OSError, ValueError):
                    d = {}
                print("%-16s %s" % (s["label"], "  ".join("%14s" % column(d, c) for c in a.cols)), flush=True)
            elif a.cmd == "run":
                print("== %s\n%s" % (s["label"], tail(s["stdout"], 200)), flush=True)
        if a.cmd == "snapshot":
            shutil.copyfile(os.path.join(out, "pmc", "pmc_traffic.json"), os.path.join(out, a.name + "_pmc_traffic.json"))
            for f in ("pmc_summary.txt", "pmc_fold.txt"):
                shutil.copyfile(os.path.join(out, "pmc", f), os.path.join(out, f))
            shutil.rmtree(os.path.join(out, "pmc"))
            with open(os.path.join(out, a.name + "_bench_detail.json")) as fh:
                d = json.load(fh)
            for c in ("value", "steady", "cpr.value", "cpu_baseline.value", "stream"):
                print("%-20s %s" % (c, column(d, c)))
            print("kernels (ms)        ", {k: v.get("avg_ms") for k, v in d.get("kernels", {}).items()})
            print(tail(os.path.join(out, "pmc_fold.txt"), 100), end="")
        elif a.cmd == "pmc":
            print(tail(os.path.join(out, "pmc_summary.txt"), 10000), end="")
        return 0
    except Stop as e:
        print("STOP: %s" % e, file=sys.stderr, flush=True)
        return 1


if __name__ == "__main__":
    sys.exit(main())
