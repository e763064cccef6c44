"""Per-iteration time of the resident standard wells' part on the 9 000-cell SPE9-shaped case, with and without group production control
(profiles/std_wells_groups.txt).  One context per line, after a begin_iteration(0) + assemble: loops of opmhip_std_wells_begin_iteration(1)
alone and of begin_iteration(1) + opmhip_assemble; a warm-up loop, then repeats.  "device": the assembly class of opmhip_profile_get (HIP
events around each launcher's scope); "wall": the host's clock around the loop with one synchronisation at its end.

    python tools/std_wells_groups_time.py [--out FILE]
    python tools/std_wells_groups_time.py --tree DIR [--out FILE]

--tree DIR: the package and the library of another checkout that has been built (e.g. `git archive PARENT | tar -x -C DIR` and
`make -C DIR/opm-autodiff_amd`), for the lines without groups only - a tree from before this feature has no `groups=`.  Run the two forms
one after the other on one box; the groups' cases are tests/groups_cases.py's."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAY = 86400.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=None, help="another built checkout: time its list without groups")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    other = a.tree is not None
    sys.path.insert(0, os.path.abspath(a.tree) if other else HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import groups_cases as GC
    pkg = importlib.import_module("opm-autodiff_amd")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def run(name, wells, groups):
        case = pkg.decks.cartesian_case(24, 25, 15, state="mixed", heterogeneous=True)
        m = pkg.capi.HipModel(case)
        m.set_state(case["pv"], case["meaning"])
        wd = pkg.wells.DeviceStandardWells(wells(case), case["depth"], m, **({} if other else dict(groups=groups)))
        wd.begin_iteration(0)
        m.assemble(DAY, 0, fetch=False)
        m.synchronize()
        m.profile_enable(True)
        for what in ("begin_iteration(1)", "begin_iteration(1) + assemble"):
            per_scope, per_wall, scopes = [], [], None
            for rep in range(a.repeats + 1):                 # the first loop is the warm-up
                n = a.warmup if rep == 0 else a.iterations
                m.synchronize()
                c0, ms0 = m.profile()["assemble"]
                t0 = time.perf_counter()
                for _ in range(n):
                    wd.begin_iteration(1)
                    if "assemble" in what:
                        m.assemble(DAY, 1, fetch=False)
                m.synchronize()
                t1 = time.perf_counter()
                c1, ms1 = m.profile()["assemble"]
                if rep:
                    per_scope.append((ms1 - ms0) / n * 1e3)
                    per_wall.append((t1 - t0) / n * 1e6)
                    scopes = (c1 - c0) / n
            say("%-26s %-30s scopes/iter %4.1f  device us/iter: median %8.2f min %8.2f max %8.2f   wall us/iter: median %8.2f min %8.2f max %8.2f"
                % (name, what, scopes, np.median(per_scope), min(per_scope), max(per_scope), np.median(per_wall), min(per_wall), max(per_wall)))

    say("SPE9-shaped case, 24 x 25 x 15 = 9000 cells, 1 injector + 25 producers (decks.spe9_shaped_wells); warm-up %d, %d repeats of %d iterations%s"
        % (a.warmup, a.repeats, a.iterations, "; tree " + a.tree if other else ""))
    plain = lambda case: pkg.decks.spe9_shaped_wells(case).wells
    grouped = lambda case: GC.spe9_groups(pkg)[1](pkg.decks.spe9_shaped_wells(case).wells)
    run("without groups", plain, None)
    if not other:
        run("3 groups (lrat only)", grouped, [pkg.wells.Group("G%d" % g, {"lrat": 12 * 900.0 * pkg.decks.STB_PER_DAY}) for g in range(3)])
        run("3 groups (lrat/resv/orat)", grouped, GC.spe9_groups(pkg)[0])
    run("without groups (again)", plain, None)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
