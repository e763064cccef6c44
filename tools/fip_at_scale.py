"""tools/fip_at_scale.py [--cells N] [--repeat R] [--out FILE]: the fluid-in-place report at the bench's size (N x N x N cells, default 100:
10^6) on one GPU.  Writes profiles/fip_at_scale.txt:
  - one opmhip_fluid_in_place call with ONE region set (a single region of every cell: 3 907 + 16 + 1 chunks) - wall time of the call
    (launches, read-back of the sums, stream drain) and, by the HIP events the call records on the context's stream, k_fip_cells and the
    reduction's launches separately;
  - the report of THREE region sets (one region, 37 slabs, an interleaved set (i + j + k) % 3 + 1 whose list is nowhere contiguous in
    the internal order): three calls, the same split per set - the interleaved set against the single region is the gather through
    the sorted list against an (almost) contiguous read;
  - the path it replaces, in the same process: opmhip_get_iq (every record over the link) and fip.region_sums(..., "sequential") in NumPy,
    with the per-cell terms formed on the host; and that the two agree to rounding.
Medians over R repetitions after one warm-up; the counters (HBM traffic, occupancy) are not collected here."""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(v):
    return statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fip_at_scale.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("opm-autodiff_amd")
    n = a.cells
    case = pkg.decks.cartesian_case(n, n, n, state="mixed", heterogeneous=False)
    Nb = case["Nb"]
    c = np.arange(Nb)
    i, j, k = c % n, (c // n) % n, c // (n * n)
    sets = {"FIPNUM": np.ones(Nb, np.int32), "FIPSLAB": (k * 37 // n + 1).astype(np.int32), "FIPMIX": ((i + j + k) % 3 + 1).astype(np.int32)}
    m = pkg.capi.HipModel(case, reorder="line_coloring")
    m.set_state(case["pv"], case["meaning"])
    lines = ["Fluids in place per FIP region at scale: %d x %d x %d = %d cells, line-coloured ordering, one MI355X" % (n, n, n, Nb),
             "medians of %d repetitions after one warm-up; ms" % a.repeat, ""]

    def timed_call(name):
        wall, cells, red = [], [], []
        m.fluid_in_place(name)
        for _ in range(a.repeat):
            m.synchronize()
            t0 = time.perf_counter()
            ip = m.fluid_in_place(name)
            wall.append((time.perf_counter() - t0) * 1e3)
            t = m.fip_timings()
            cells.append(t["cells"])
            red.append(t["reduce"])
        return ip, med(wall), med(cells), med(red)

    # one set
    t0 = time.perf_counter()
    m.set_fip_regions({"FIPNUM": sets["FIPNUM"]})
    setup1 = (time.perf_counter() - t0) * 1e3
    info = m.fip_info("FIPNUM")
    ip1, wall, cells, red = timed_call("FIPNUM")
    lines += ["1 region set (one region: %d chunks at level 0, %d levels; set-up on the host and upload %.1f ms, once)" % (info["chunks"], info["levels"], setup1),
              "  opmhip_fluid_in_place, wall            %8.3f" % wall,
              "    k_fip_cells (events)                 %8.3f" % cells,
              "    k_fip_reduce x %d + k_fip_totals      %8.3f" % (info["levels"], red), ""]
    # three sets
    t0 = time.perf_counter()
    m.set_fip_regions(sets)
    setup3 = (time.perf_counter() - t0) * 1e3
    lines.append("3 region sets (set-up %.1f ms, once)" % setup3)
    total = 0.0
    got = {}
    for name in sets:
        info = m.fip_info(name)
        got[name], wall, cells, red = timed_call(name)
        total += wall
        lines.append("  %-8s %2d regions, %5d chunks, %d levels: wall %8.3f   k_fip_cells %8.3f   reduce + totals %8.3f"
                     % (name, info["max_id"], info["chunks"], info["levels"], wall, cells, red))
    lines += ["  the three calls together, wall         %8.3f" % total, ""]
    # the path it replaces
    t_iq, t_terms, t_sum = [], [], []
    for _ in range(max(1, a.repeat // 2)):
        m.synchronize()
        t0 = time.perf_counter()
        iq = m.iq()
        t1 = time.perf_counter()
        terms = pkg.fip.cell_terms(iq, case["volume"], case["poro"])
        t2 = time.perf_counter()
        seq = pkg.fip.inplace(terms, sets["FIPNUM"], "sequential")
        t3 = time.perf_counter()
        t_iq.append((t1 - t0) * 1e3)
        t_terms.append((t2 - t1) * 1e3)
        t_sum.append((t3 - t2) * 1e3)
    lines += ["the path it replaces, same process, 1 region set",
              "  opmhip_get_iq (%d B per cell, %.0f MB)   %8.3f" % (iq.shape[1] * 32, iq.nbytes / 1e6, med(t_iq)),
              "  fip.cell_terms (NumPy)                 %8.3f" % med(t_terms),
              "  fip.region_sums 'sequential' (NumPy)   %8.3f" % med(t_sum), ""]
    rel = np.abs(got["FIPNUM"]["field"][:12] - seq["field"][:12]) / np.maximum(np.abs(seq["field"][:12]), 1e-300)
    stated = pkg.fip.inplace(terms, sets["FIPNUM"], "stated")
    same = all(np.array_equal(got["FIPNUM"][key], stated[key], equal_nan=True) for key in ("regions", "field")) and \
        all(np.array_equal(got["FIPNUM"][key], ip1[key], equal_nan=True) for key in ("regions", "field"))
    lines += ["device against the sequential loop, field sums: largest relative difference %.2e (n u = %.2e)" % (rel.max(), Nb * 2.0 ** -53),
              "device against fip.region_sums 'stated', and the 1-set call against the 3-set call: %s" % ("the same bits" if same else "DIFFERENT BITS"),
              "FPR %.6f bar, FOIP %.6e sm3, FGIP %.6e sm3, FWIP %.6e sm3" % (got["FIPNUM"]["field"][12] / 1e5, got["FIPNUM"]["field"][10],
                                                                         got["FIPNUM"]["field"][11], got["FIPNUM"]["field"][9]), "",
              "NOT measured: hardware counters (HBM bytes, L2 hit rates, occupancy) of the new kernels; the cost of the gather through the sorted",
              "list beyond what the FIPMIX row shows against the FIPNUM row above (same launches, same bytes, another access pattern)."]
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)
    print(txt)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
