"""tools/boundary_at_scale.py [--cells N] [--repeat R] [--batch B] [--tree DIR] [--out FILE]: what the open boundaries
(opmhip_set_boundary_conditions) add to an assemble at the bench's size - N x N x N cells (default 100: 10^6) with all six sides FREE:
58 808 boundary cells, 60 000 faces.  In one process, alternating round by round: B assembles with the list set, B with the list
cleared (the launches of a context that never had one: k_assemble and nothing new) - wall time per assemble between two stream
drains, and k_assemble's own time from the library's HIP events (profile class "assemble").  The difference of the wall times is
k_boundary_apply + k_boundary_restore.
--tree DIR: the package and the library of another checkout that has been built (e.g. `git archive PARENT | tar -x -C DIR` and
`make -C DIR/opm-autodiff_amd`), for the no-list lines only - a tree from before this feature has no set_boundary_conditions.  Run the two
trees in alternation in one GPU session; each run appends its lines to --out (default profiles/boundary_at_scale.txt is written by
hand from those)."""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAY = 86400.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--tree", default=None, help="another built checkout: time its assemble without a list")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    other = a.tree is not None
    sys.path.insert(0, os.path.abspath(a.tree) if other else HERE)
    pkg = importlib.import_module("opm-autodiff_amd")
    n = a.cells
    case = pkg.decks.cartesian_case(n, n, n, state="mixed", heterogeneous=False)
    m = pkg.capi.HipModel(case, reorder="line_coloring")
    m.set_state(case["pv"], case["meaning"])
    recs, nf, nd = None, 0, 0
    if not other:
        B = pkg.boundary
        box = (0, n - 1, 0, n - 1, 0, n - 1)
        recs = [B.free(B.faces(case, box, f)) for f in ("I-", "I+", "J-", "J+", "K-", "K+")]
        cells = np.concatenate([r["cells"] for r in recs])
        nf, nd = len(cells), len(np.unique(cells))
    # an iterate away from the captured state, so that every face carries a flux
    pv = case["pv"].reshape(-1, 3).copy()
    pv[:, 1] -= 1.0e5
    dt = 5.0 * DAY
    m.profile_enable(True)

    def batch():
        p0 = m.profile()["assemble"]
        m.synchronize()
        t0 = time.perf_counter()
        for it in range(a.batch):
            m.assemble(dt, it, fetch=False)
        m.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / a.batch
        p1 = m.profile()["assemble"]
        return wall, (p1[1] - p0[1]) / max(p1[0] - p0[0], 1)

    rows = {"list": [], "none": []}
    for r in range(a.repeat + 1):                   # round 0 is the warm-up
        for form in (("none",) if other else ("list", "none")):
            if not other:
                m.set_state(case["pv"], case["meaning"])
                m.set_boundary_conditions(recs if form == "list" else None)
            m.set_state(pv.reshape(-1), case["meaning"])
            w = batch()
            if r > 0:
                rows[form].append(w)
    med = lambda v, k: statistics.median(x[k] for x in v)
    lines = ["%s: %d^3 = %d cells, line-coloured ordering; medians of %d rounds of %d assembles after one warm-up round; ms per assemble"
             % ("tree " + a.tree if other else "this tree", n, case["Nb"], a.repeat, a.batch)]
    if not other:
        lines.append("  list set (%d faces, %d distinct cells, all FREE): wall %8.4f   k_assemble (events) %8.4f" % (nf, nd, med(rows["list"], 0), med(rows["list"], 1)))
    lines.append("  no list:                                              wall %8.4f   k_assemble (events) %8.4f" % (med(rows["none"], 0), med(rows["none"], 1)))
    if not other:
        lines.append("  k_boundary_apply + k_boundary_restore (difference of the walls): %8.4f" % (med(rows["list"], 0) - med(rows["none"], 0)))
        # what the two kernels move, from the code: per distinct cell 12 doubles of source / dsource read, saved, written and restored (4 x 96 B)
        # plus its depth and indices; per FREE face 3 doubles of geometry, the fields it reads of the record (p, rho, mobility, 1/B, Rs: 13 x 32 B,
        # shared by the faces of a cell through the cache), the 14 doubles of the exterior record and 96 B of rates written
        per_cell, per_face = 4 * 96 + 8 + 16 + 13 * 32 + 14 * 8, 24 + 8 + 96
        lines.append("  bytes moved per assemble, from the code: %.2f MB (%d B per distinct cell, %d B per face)" % ((nd * per_cell + nf * per_face) / 1e6, per_cell, per_face))
    txt = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "a") as f:
            f.write(txt)
    print(txt)
    return 0


if __name__ == "__main__":
    sys.exit(main())
