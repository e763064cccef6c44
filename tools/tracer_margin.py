"""The margin tests/tracer_states.py records as DX_MARGIN: tracers.HostTracers.end_time_step on the CPU, once with sequential and once with
numpy's pairwise scalar products, over the solve cases of the tracer tests (tracer_states.margin_cases: those of tests/test_gpu_tracers.py
and of tests/test_gpu_tracer_edges.py) in every ordering that can be formed without a device; prints the largest relative difference of
dx per case and ordering and the largest of all.  Needs the oracle library for the records only.  A case name as argument runs only the
cases whose name contains it."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import oracle_bind          # noqa: E402
import tracer_states as S   # noqa: E402

pkg = importlib.import_module("opm-autodiff_amd")
orc = oracle_bind.Oracle(os.path.join(ROOT, "oracle", "liboracle.so"))
worst = (0.0, None)
for label, dims, sc in S.margin_cases(pkg):
    if len(sys.argv) > 1 and sys.argv[1] not in label:
        continue
    case = sc["case"]
    o = oracle_bind.OracleModel(orc, case)
    for name, order in S.emulated_orders(*dims).items():
        dx = {}
        for dot in ("sequential", "pairwise"):
            h = pkg.tracers.HostTracers(case, sc["phase"], sc["c"], tolerance=1e-2, dot=dot)
            o.set_state(case["pv"], case["meaning"])
            h.begin_time_step(o.iq())
            o.set_state(sc["pv1"], case["meaning"])
            h.set_records(o.iq())
            h.set_connections(sc["cells"], sc["rates"], sc["injected"])
            res = h.end_time_step(S.DT, order)
            assert S.clear_decisions(res, 1e-2), (label, name, dot)
            assert all(r["converged"] for r in res), (label, name, dot)
            dx[dot] = (h.last_dx.copy(), [r["iterations"] for r in res])
        assert dx["sequential"][1] == dx["pairwise"][1]
        d = S.rel_diff(dx["sequential"][0], dx["pairwise"][0])
        print("%s %-9s iterations %r  rel. difference of dx %.3e" % (label, name, dx["sequential"][1], d))
        if d > worst[0]:
            worst = (d, "%s, %s" % (label, name))
print("DX_MARGIN = %.3e (%s)" % worst)
