"""tools/tracer_probe.py [--n N] [--phase water|oil] [--reorder NAME] [--counts 1,2,4,8] [--tolerance T]: the time of one
opmhip_tracers_end_time_step on the N^3 bench case (default 100: BASELINE.json configs[1], its five-spot as tracer connections, the injector's
phase carrying concentration 1 for the first tracer) with 1, 2, 4 and 8 tracers of one phase, split by HIP events on the context's stream into
system / ILU0 factorisation / BiCGStab (opmhip_get_tracer_timings), with the iteration counts and, for comparison, the wall time of one
Newton iteration of the same context.  The tracers start from different random fields, so that each right-hand side is its own.
Prints a table; profiles/tracers_at_scale.txt keeps one."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DAY = 86400.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--phase", choices=["water", "oil"], default="water")
    ap.add_argument("--reorder", default=None)
    ap.add_argument("--counts", default="1,2,4,8")
    ap.add_argument("--tolerance", type=float, default=1e-2)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    pkg = importlib.import_module("opm-autodiff_amd")
    n = a.n
    case = pkg.decks.cartesian_case(n, n, n, state="mixed", heterogeneous=False)
    src = pkg.decks.five_spot_source(case, rate_sm3_per_day=pkg.decks.BENCH_RATE_SM3_PER_DAY).reshape(-1, 3)     # equations: oil, water, gas
    cells = np.flatnonzero(np.abs(src).sum(axis=1) > 0).astype(np.int32)
    rates = np.ascontiguousarray(src[cells][:, [1, 0, 2]])                                                       # phases: water, oil, gas
    kw = dict(tolerance=1e-2, maxit=200, ilu_relaxation=0.9)
    if a.reorder:
        kw["reorder"] = a.reorder
    m = pkg.capi.HipModel(case, **kw)
    m.set_state(case["pv"], case["meaning"])
    m.set_source(src.reshape(-1))
    nm = pkg.newton.BlackoilModelHip(m)
    # one time step of the flow equations: the tracers are advanced at its converged state; the Newton iterations are timed on the way
    dt = 1.0 * DAY
    ph = pkg.tracers.PHASES[a.phase]
    rng = np.random.default_rng(5)
    info = m.ordering_info()
    print("tracer probe: %d^3 = %d cells, ordering %s (chain length %d, %d colours), %d connections, %s tracers, tolerance %g"
          % (n, case["Nb"], info["ilu_ordering"], info["chain_length"], info["colors"], len(cells), a.phase, a.tolerance))
    m.advance_time_level()
    nm.begin_time_step(dt)
    newton = []
    for it in range(20):
        m.synchronize()
        t0 = time.perf_counter()
        rep = nm.nonlinear_iteration(it, dt)
        m.synchronize()
        newton.append((time.perf_counter() - t0) * 1e3)
        if rep.converged:
            break
    solved = newton[:-1] if len(newton) > 1 else newton       # the converged iteration holds no solve
    print("flow step of 1 day: %d Newton iterations, %.2f ms each with its linear solve (median), %.2f ms the converged check alone"
          % (len(solved), float(np.median(solved)), newton[-1]))
    print("%8s %10s %10s %10s %10s %10s %8s %9s  %s" % ("tracers", "wall ms", "system ms", "factor ms", "solve ms", "sum ms", "levels", "launches", "iterations"))
    for nt in [int(x) for x in a.counts.split(",")]:
        best = None
        for rep_no in range(a.repeats):
            c = rng.uniform(0.0, 1.0, (nt, case["Nb"]))
            m.set_tracers([ph] * nt, c)
            m.set_tracer_solver(a.tolerance, 100)
            inj = np.zeros((nt, len(cells)))
            inj[0] = 1.0
            m.set_tracer_connections(cells, rates, inj)
            # begin at the old time level's records is what a run does; here the converged state stands in for both: storage differences
            # vanish, the fluxes and the connections make the right-hand sides
            m.tracers_begin_time_step()
            m.synchronize()
            t0 = time.perf_counter()
            res = m.tracers_end_time_step(dt)
            wall = (time.perf_counter() - t0) * 1e3
            t = m.tracer_timings()
            row = (wall, t, [r["iterations"] for r in res], all(r["converged"] for r in res))
            if best is None or wall < best[0]:
                best = row
        wall, t, its, conv = best
        print("%8d %10.3f %10.3f %10.3f %10.3f %10.3f %8d %9d  %r%s" % (nt, wall, t["system"], t["factor"], t["solve"], t["system"] + t["factor"] + t["solve"],
                                                                      t["levels"], t["launches"], its, "" if conv else "  NOT converged"))


if __name__ == "__main__":
    main()
