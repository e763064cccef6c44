#!/usr/bin/env python3
"""What multisegment wells cost a BiCGStab iteration at the bench's size: the 100^3 case's first Jacobian (ILU0, default configuration)
solved with generated multisegment wells (mswells.tree_well) in three forms inside one GPU session, alternating:
  none      no wells
  callback  the wells behind opmhip_wells.ms_apply: x and y to the host after every product, numpy applies the wells, y back
  device    the same wells through opmhip_set_ms_wells: D inverted on the device, one kernel per product; --form dense|tree|auto chooses
            the form of the device list (opmhip_set_ms_wells_form; the dense form takes wells of at most cap M / 4 segments)
Well lists: 0 wells (the three forms must agree), 1 and 8 wells of 30 segments, one well of the cap's size.  Prints per list and form the
ms per BiCGStab iteration (mean and the range over the repetitions) and the linear iterations.
    python tools/ms_wells_at_scale.py [--n 100] [--reps 5] [--forms none,callback,device] [--lists 0,1x30,8x30,cap] [--form dense]
Lists above the dense cap (1x200, 8x100, 1x1000) need --form tree or auto.
Kernel times of k_ms_wells_factor / k_ms_wells_apply (k_ms_wells_tree_factor / k_ms_wells_tree_apply): a run of its own under the profiler,
kernel trace only:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/ms_wells_at_scale.py --forms device --lists 8x30,cap --reps 2 [--form tree]"""
import argparse, importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--tol", type=float, default=1e-6)   # (tighter than Flow's 1e-2: the first Jacobian of the case is solved to that in under two iterations)
ap.add_argument("--forms", default="none,callback,device")
ap.add_argument("--lists", default="0,1x30,8x30,cap")
ap.add_argument("--form", default="dense", choices=["dense", "tree", "auto"])
a = ap.parse_args()
pkg = importlib.import_module("opm-autodiff_amd")
n = a.n
case = pkg.decks.cartesian_case(n, n, n, state="mixed", heterogeneous=False)
src = pkg.decks.five_spot_source(case, rate_sm3_per_day=pkg.decks.BENCH_RATE_SM3_PER_DAY * n * n / 1e4)
Nb = case["Nb"]
capM, _ = pkg.capi.ms_wells_caps()


def well_list(spec, scale):
    """'8x30' -> eight wells of 30 segments, 'cap' -> one of the largest size; one perforation per segment, columns of cells spread over the grid;
    B and C scaled so that the wells change the operator without dominating it"""
    if spec == "0":
        return []
    count, Mb = (1, capM // 4) if spec == "cap" else (int(spec.split("x")[0]), int(spec.split("x")[1]))
    out = []
    for w in range(count):
        i, j = (7 + 11 * w) % n, (5 + 17 * w) % n
        cells = [i + n * (j + n * (k % n)) + (k // n) for k in range(Mb)]
        well = pkg.mswells.tree_well(Mb, cells, seed=1000 + w)
        well["Bvals"] = 1e-2 * well["Bvals"]
        well["Cvals"] = scale * well["Cvals"]
        out.append(well)
    return out


class Callback:
    """the host form: per well the dense operators over its own cells"""

    def __init__(self, wells):
        self.ops = []
        for w in wells:
            cells = np.unique(w["Bcols"])
            local = dict(w, Bcols=np.searchsorted(cells, w["Bcols"]))
            B, C, D = pkg.mswells.dense_operators(local, len(cells))
            idx = (3 * cells[:, None] + np.arange(3)).reshape(-1)
            self.ops.append((idx, B, C, np.linalg.inv(D)))

    def __call__(self, hx, hy):
        for idx, B, C, Dinv in self.ops:
            hy[idx] -= C.T @ (Dinv @ (B @ hx[idx]))


m = pkg.capi.HipModel(case, tolerance=a.tol, maxit=200, ilu_relaxation=0.9)
m.set_state(case["pv"], case["meaning"])
m.set_source(src)
j, r = m.assemble(86400.0, 0)
diag = np.abs(j.reshape(-1, 3, 3)[np.asarray(case["rowptr"][:-1])]).max()   # (the first block of a row: the scale of the matrix is all that is wanted)
del j, r
print("%d^3 cells, ILU0 default configuration (%s), tolerance %g; %d repetitions after %d of warm-up, the forms alternating; cap M = %d; device form %s" %
      (n, m.ordering_info()["ilu_ordering"], a.tol, a.reps, a.warmup, capM, a.form), flush=True)
for spec in a.lists.split(","):
    wells = well_list(spec, 1e-4 * diag)
    cb = Callback(wells)
    t = {f: [] for f in a.forms.split(",")}
    it = {}
    fact0 = m.ms_wells_info()["factorisations"]
    for rep in range(a.warmup + a.reps):
        for form in t:
            if form != "none" and not wells and spec != "0":
                continue
            m.set_ms_wells(wells if form == "device" else None, form=a.form)
            W = dict(numWells=0, numMsWells=len(wells), N=3 * Nb, ms_apply=cb) if form == "callback" and wells else None
            m.assemble(86400.0, 0, fetch=False)
            res = m.solve_jacobian_system(wells=W)
            if rep >= a.warmup:
                t[form].append(1e3 * res.t_solve / max(res.it, 0.5))
            it[form] = (res.it, res.converged)
    m.set_ms_wells(None)
    for form, v in t.items():
        print("%-8s %-9s %8.3f ms per BiCGStab iteration (min %.3f max %.3f over %d)   %5.1f linear iterations, converged %d" %
              (spec, form, np.mean(v), np.min(v), np.max(v), len(v), it[form][0], it[form][1]), flush=True)
    if "device" in t and wells:
        info = m.ms_wells_info()
        m.set_ms_wells(wells, form=a.form)
        fi = m.ms_wells_form_info()
        m.set_ms_wells(None)
        print("%-8s device: %d wells dense, %d tree (largest %d segments, %d levels, %d KiB of blocks)" % (spec, fi["dense"], fi["tree"], fi["tree_max_segments"], fi["tree_max_depth"], fi["tree_kib"]), flush=True)
        print("%-8s device: %d inversions in %d solves (the alternation clears the list between them: one inversion per solve, as in a Flow run whose values change)" % (spec, info["factorisations"] - fact0, a.warmup + a.reps), flush=True)
