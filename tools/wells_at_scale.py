#!/usr/bin/env python3
"""What a host-side well model costs the device-resident Newton iteration at the bench's size: the 100^3 case with its five-spot as two
WELLS (wells.StandardWells: a water injector and an oil producer, one completion per layer - 100 each - on the bench's rates, the
producer with a BHP limit it never meets), under bench.py's time-step control, four ways inside one GPU session:
  sources    the bench itself: fixed-rate source terms, no well model
  per cell   the well model moving what its 200 perforated cells need (opmhip_get_iq_cells / opmhip_set_source_cells, ABI 11)
  whole grid the well model through the whole-grid calls (opmhip_get_iq: 544 B per cell back, opmhip_set_source: 96 B per cell over)
  device     the well equations resident on the device (opmhip_set_std_wells, wells.DeviceStandardWells): one read-back of 10 doubles per well
Prints Newton iterations/s and linear iterations per Newton iteration of each.    python tools/wells_at_scale.py [--n 100] [--steps 20]
--spe9: instead, the SPE9-shaped well case of the tests (decks.spe9_shaped_wells: 26 wells, 80 completions, 9 000 cells, producers'
BHP limit 235 bar) with its wells per cell (host) and on the device, alternating, each form in a context of its own.
--spe9 --heads: the resident wells alone, the head from the perforated cell's oil density against the head from the well-bore density
(opmhip_set_std_wells_head_model), alternating, three times each.
--matrix-add (with or without --spe9; --preconditioner ilu0 | cpr): the resident wells in their two forms, alternating, twice each: as the
operator A - C^T D^-1 B on the plain pattern and on the clique pattern (decks.with_well_cliques), and written into the Jacobian on the
clique pattern (opmhip_set_std_wells_matrix_add).  Per form: Newton iterations/s, linear iterations per Newton iteration, ms per BiCGStab
iteration (the solves' time over their iterations) and, for the matrix form, the add kernel's own time (HIP events).  A row holds at most
64 blocks, so the two long wells are completed in the top 60 layers here (in both forms).  Every line names the ordering the context
got and its number of colours; --reorder NAME asks for one (a clique of n cells needs n colours of a point colouring)."""
import argparse, importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--spe9", action="store_true")
ap.add_argument("--heads", action="store_true")
ap.add_argument("--matrix-add", action="store_true")
ap.add_argument("--preconditioner", default="ilu0", choices=["ilu0", "cpr"])
ap.add_argument("--reorder", default=None, help="the ordering of every context (default: the library's choice, which goes by the pattern)")
a = ap.parse_args()
if a.heads and not a.spe9:
    ap.error("--heads compares the head models on the SPE9-shaped case: give --spe9 with it")
pkg = importlib.import_module("opm-autodiff_amd")
n = a.n
if a.spe9:
    case = pkg.decks.cartesian_case(24, 25, 15, dx=91.44, dy=91.44, dz=6.0, heterogeneous=True, state="mixed")
else:
    case = pkg.decks.cartesian_case(n, n, n, state="mixed", heterogeneous=False)
rate = pkg.decks.BENCH_RATE_SM3_PER_DAY * n * n / 1e4
src = None if a.spe9 else pkg.decks.five_spot_source(case, rate_sm3_per_day=rate)


def two_wells():
    W = pkg.wells
    if a.spe9:
        return pkg.decks.spe9_shaped_wells(case, producer_bhp_limit=235e5)
    col = lambda i, j: [i + n * (j + n * k) for k in range(min(n, 60) if a.matrix_add else n)]
    tw = lambda cells: [W.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], 0.1524) for c in cells]
    ci, cp = col(0, 0), col(n - 1, n - 1)
    q = rate / 86400.0
    return W.StandardWells([W.Well("INJ", ci, tw(ci), case["depth"][ci[0]], False, ("rate", W.WATER, q), 1000e5, inj_phase="water"),
                            W.Well("PROD", cp, tw(cp), case["depth"][cp[0]], True, ("rate", W.OIL, q), 10e5)], case["depth"])


class WholeGrid:
    """the model without its per-cell calls: newton.BlackoilModelHip then asks for / hands over whole arrays"""

    def __init__(self, m):
        self._m = m

    def __getattr__(self, k):
        if k in ("iq_cells", "set_source_cells"):
            raise AttributeError(k)
        return getattr(self._m, k)


def add_kernel_ms(m, wells, reps=5):
    """the add kernel's own time: the assembly class's HIP-event time around the call alone, the smallest of `reps` (a new assemble each)"""
    m.profile_enable(True)
    best = float("inf")
    for _ in range(reps):
        wells.begin_iteration(1)
        m.assemble(bench.DAY, 1, fetch=False)
        m.synchronize()
        t0 = m.profile()["assemble"][1]
        m.std_wells_add_to_matrix()
        m.synchronize()
        best = min(best, m.profile()["assemble"][1] - t0)
    m.profile_enable(False)
    return best


def run(name, with_wells, whole_grid=False, device=False, head_model="cell_oil", matrix_add=False, on_case=None):
    m = pkg.capi.HipModel(on_case or case, tolerance=1e-2, maxit=200, ilu_relaxation=0.9, preconditioner=a.preconditioner, reorder=a.reorder)
    m.set_state(case["pv"], case["meaning"])
    wells = None
    if with_wells:
        wells = two_wells()
        if device:
            wells = pkg.wells.DeviceStandardWells(wells.wells, case["depth"], m, head_model=head_model, matrix_add=matrix_add)
    else:
        m.set_source(src)
    nm = pkg.newton.BlackoilModelHip(WholeGrid(m) if whole_grid else m, well_model=wells)
    sim = pkg.newton.AdaptiveTimeStepping(nm, pkg.newton.TimeSteppingParameters(initial_dt=bench.DAY, max_dt=10 * bench.DAY))
    for _ in range(a.warmup):
        sim.next_newton_iteration()
    m.synchronize()
    t0 = time.perf_counter()
    lin, t_lin = 0, 0.0
    for _ in range(a.steps):
        r = sim.next_newton_iteration()
        lin += r.total_linear_iterations
        t_lin += r.linear_solve_time
    m.synchronize()
    el = time.perf_counter() - t0
    extra = ""
    if device:
        wells.fetch()
    if wells is not None:
        extra = "   controls %s, q_inj %.1f m3/day, q_prod %.1f m3/day" % ("".join(w.control[0][0] for w in wells.wells), wells.x[0, 1] * 86400.0, -wells.x[1:, 0].sum() * 86400.0)
    if a.matrix_add:
        o = m.ordering_info()
        name = "%s [%s, %d colours]" % (name, o["ilu_ordering"], o["colors"])
        extra = "   %.4f ms per BiCGStab iteration%s%s" % (1e3 * t_lin / max(lin, 1), ", add kernel %.4f ms" % add_kernel_ms(m, wells) if matrix_add else "", extra)
    print("%-44s %8.2f Newton its/s   %5.2f lin/Newton   %6.2f ms per Newton iteration%s" % (name, a.steps / el, lin / a.steps, 1e3 * el / a.steps, extra), flush=True)


if a.matrix_add:
    clique = pkg.decks.with_well_cliques(case, two_wells())
    print("%s, preconditioner %s: %d entries on the plain pattern, %d with the wells' cliques; %d Newton iterations after %d of warm-up, each variant in a context of its own"
          % ("SPE9-shaped, 24 x 25 x 15 cells, 26 wells" if a.spe9 else "%d^3 cells, two wells of %d completions" % (n, min(n, 60)), a.preconditioner, len(case["col"]),
             len(clique["col"]), a.steps, a.warmup), flush=True)
    for rep in range(2):
        run("device wells: operator, plain pattern", True, device=True)
        run("device wells: operator, clique pattern", True, device=True, on_case=clique)
        run("device wells: in the matrix, clique pattern", True, device=True, matrix_add=True, on_case=clique)
    sys.exit(0)
if a.spe9:
    print("SPE9-shaped: 24 x 25 x 15 cells, 26 wells, %d Newton iterations after %d of warm-up, each variant in a context of its own" % (a.steps, a.warmup), flush=True)
    if a.heads:
        for rep in range(3):
            run("26 wells on the device: head cell_oil", True, device=True)
            run("26 wells on the device: head wellbore", True, device=True, head_model="wellbore")
    else:
        for rep in range(2):
            run("26 wells, 80 completions: per cell", True)
            run("26 wells, 80 completions: device", True, device=True)
    sys.exit(0)
print("%d^3 cells, %d Newton iterations after %d of warm-up, each variant in a context of its own" % (n, a.steps, a.warmup), flush=True)
for rep in range(2):
    run("sources (the bench, no well model)", False)
    run("two wells, 200 completions: per cell", True)
    run("two wells, 200 completions: whole grid", True, whole_grid=True)
    run("two wells, 200 completions: device", True, device=True)
