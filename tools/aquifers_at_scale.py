"""tools/aquifers_at_scale.py FORM [--steps N] [--warmup W]: Newton iterations per second of the Norne-shaped case (tests/helpers.py) with the
two aquifers of decks.two_aquifers - a Carter-Tracy aquifer on the I- side, a Fetkovich aquifer under the grid - through Flow's sub-stepping,
FORM = device (opmhip_set_aquifers: every assemble forms the influx itself), host (aquifers.HostAquifers: the connected cells' records come
down and their rates go up in front of every assemble, opmhip_get_iq_cells / opmhip_set_source_cells) or none (no aquifers: the same sources).
Run the forms in alternation with tools/ab.py run OUT --program "tools/aquifers_at_scale.py" --variant "device device" --variant "host host";
under rocprofv3 --kernel-trace --stats (ab.py --rocprof-stats) the k_aquifer_* rows are the per-assemble time of the new launches."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers  # noqa: E402

DAY = 86400.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("form", choices=["device", "host", "none"])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    pkg = importlib.import_module("opm-autodiff_amd")
    case, g, dims = helpers.norne_shaped_case(pkg)
    rng = np.random.default_rng(3)
    cells = rng.choice(case["Nb"], 24, replace=False)     # the sources of tools/norne_profile.py
    q = 200.0 / DAY
    sc = np.zeros((24, 3))
    sc[:12, 1], sc[12:, 0] = q, -q
    recs = pkg.decks.two_aquifers(case, g, dims)
    m = pkg.capi.HipModel(case, reorder="line_coloring", tolerance=1e-2, maxit=200, ilu_relaxation=0.9, chain_length=10)
    m.set_state(case["pv"], case["meaning"])
    m.set_source_cells(cells, sc.reshape(-1))
    aq = None
    if a.form == "device":
        aq = pkg.aquifers.DeviceAquifers(recs)
    elif a.form == "host":
        aq = pkg.aquifers.HostAquifers(recs, case["depth"], base_cells=(cells, sc))
    nm = pkg.newton.BlackoilModelHip(m, aquifer_model=aq)
    sim = pkg.newton.AdaptiveTimeStepping(nm, pkg.newton.TimeSteppingParameters(initial_dt=1 * DAY, max_dt=10 * DAY))
    for _ in range(a.warmup):
        sim.next_newton_iteration()
    m.synchronize()
    t0 = time.perf_counter()
    lin = 0
    for _ in range(a.steps):
        lin += sim.next_newton_iteration().total_linear_iterations
    m.synchronize()
    el = time.perf_counter() - t0
    extra = ""
    if aq is not None:
        d = aq.data(m)
        extra = ", W_flux %s m3 after %.1f days" % (np.array2string(d["W_flux"], precision=3), sim.time / DAY)
    print("aquifers %s: %d connections, %.2f Newton its/s, %.1f lin/newton, %d time steps (%d failed)%s"
          % (a.form, sum(len(r["cells"]) for r in recs), a.steps / el, lin / a.steps, sim.timesteps_done, sim.timesteps_failed, extra))


if __name__ == "__main__":
    main()
