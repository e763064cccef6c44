"""ILU0 against block ILU(1) (--ilu-fillin-level) in three orderings, on the 10^6-cell case (BASELINE.json configs[1]), configs[2]
(24 x 25 x 15, heterogeneous) and configs[4] (Norne-shaped): linear iterations per Newton iteration in the first time step (start-up)
and in the following ones (steady), device time per M^-1 application and per factorisation (HIP events, opmhip_profile_*), Newton
iterations per second, bytes of the factors.  One JSON line per configuration on stdout and the whole list in --out.

    python tools/ilun_study.py --out profiles/ilun_study.json [--cases c1,c2,c4] [--days 3]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("opm-autodiff_amd")
import helpers  # noqa: E402

DAY = 86400.0


def make_case(name):
    D = pkg.decks
    if name == "c1":
        case = D.cartesian_case(100, 100, 100, state="mixed", heterogeneous=False)
        return case, D.five_spot_source(case, rate_sm3_per_day=D.BENCH_RATE_SM3_PER_DAY)
    if name == "c2":
        case = D.cartesian_case(24, 25, 15, state="mixed", heterogeneous=True)
        return case, D.five_spot_source(case, rate_sm3_per_day=100.0)
    case, _, _ = helpers.norne_shaped_case(pkg)   # 24 source cells as in tools/norne_profile.py
    cells = np.random.default_rng(3).choice(case["Nb"], 24, replace=False)
    s = np.zeros((case["Nb"], 3))
    s[cells[:12], 1] = 200.0 / DAY
    s[cells[12:], 0] = -200.0 / DAY
    return case, np.ascontiguousarray(s.reshape(-1))


def run(name, case, src, reorder, n, days):
    m = pkg.capi.HipModel(case, reorder=reorder, ilu_fillin_level=n)
    m.set_state(case["pv"], case["meaning"])
    m.set_source(src)
    info, oinfo = m.ilu_info(), m.ordering_info()
    m.profile_enable(True)
    model = pkg.newton.BlackoilModelHip(m)
    steps = []
    for _ in range(days):
        model.begin_time_step(DAY)
        t0 = time.perf_counter()
        rep = model.step(DAY)
        t1 = time.perf_counter()
        model.end_time_step(DAY)
        steps.append((rep.total_newton_iterations, rep.total_linear_iterations, t1 - t0))
    prof = m.profile()
    Nb = case["Nb"]
    first, rest = steps[0], steps[1:]
    nit_rest = sum(s[0] for s in rest)
    out = dict(case=name, cells=Nb, n=n, reorder=reorder, in_force=oinfo["ilu_ordering"], levels=info["levels"],
               lu_blocks=info["nl"] + info["nu"] + Nb, lu_bytes=72 * (info["nl"] + info["nu"] + Nb),
               lin_per_newton_startup=first[1] / max(first[0], 1),
               lin_per_newton_steady=sum(s[1] for s in rest) / max(nit_rest, 1),
               newton_its=[s[0] for s in steps], newton_its_per_s=nit_rest / max(sum(s[2] for s in rest), 1e-12),
               ms_per_minv=prof["ilu_apply"][1] / max(prof["ilu_apply"][0], 1),
               ms_per_factor=prof["ilu_factor"][1] / max(prof["ilu_factor"][0], 1))
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default="c2,c4,c1")
    ap.add_argument("--days", type=int, default=3)
    a = ap.parse_args()
    rows = []
    for name in a.cases.split(","):
        case, src = make_case(name)
        for n in (0, 1):
            for reorder in ("auto", "level_scheduling", "distance2"):
                r = run(name, case, src, reorder, n, a.days)
                print(json.dumps(r), flush=True)
                rows.append(r)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
