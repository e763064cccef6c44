"""Split assembly (opmhip_get_split_assembly; csrc/assemble.hip: k_assemble<., SPLIT>, csrc/solver.hip: k_ilu_factor<0, SPLIT>, ensure_A):
on the plain ILU0 context of the half-product form the assembly writes the Jacobian into the two arrays the ILU0 solve reads (the matrix
beside its U part, the U part) and the factorisation copies nothing.  The form moves bytes, never a statement: everything it leaves behind
is compared, bit for bit, with what the same calls leave behind with OPMHIP_SPLIT_ASM=0 (under OPMHIP_TUNING=1), the form that writes
the matrix's own array and lets the factorisation copy.  The library reads its switches once per process, so each side is ONE child
process that runs every case and stores what it saw; the tests compare the two records."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = {"a": (4, 4, 20), "b": (5, 3, 11), "column": (1, 1, 7), "cube": (6, 6, 6)}

WORKER = r"""
import importlib, sys
import numpy as np
root, out_path = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
pkg = importlib.import_module("opm-autodiff_amd")
SHAPES = %r
DT = 5 * 86400.0
out = {}

def model(case, src=None, **kw):
    kw.setdefault("reorder", "line_coloring")
    kw.setdefault("half_product", 1)
    kw.setdefault("tolerance", 1e-6)
    m = pkg.capi.HipModel(case, **kw)
    m.set_state(case["pv"], case["meaning"])
    if src is not None:
        m.set_source(src)
    return m

def info(m):
    i = m.split_assembly()
    return np.array([i["on"], i["stale"], i["assemblies"], i["gathers"]], np.int64)

def factors(m, tag):
    f = m.ilu_factors()
    for k in ("L", "U", "invD"):
        out[tag + "." + k] = f[k].copy()
    out[tag + ".R"] = m.split_assembly(rest=True)["rest"].copy()

for name, shape in SHAPES.items():
    case = pkg.decks.cartesian_case(*shape, state="mixed", heterogeneous=True)
    src = pkg.decks.five_spot_source(case, rate_sm3_per_day=30.0)
    # assemble + factor: the factors, the two streams, the residual; then the matrix (the gather), and the factors once more from it
    m = model(case, src)
    out[name + ".info0"] = info(m)
    m.assemble(DT, 0, fetch=False)
    out[name + ".info1"] = info(m)
    out[name + ".resid"] = m.get_rhs()
    m.ilu0_factor(want_factors=False)
    factors(m, name + ".f")
    out[name + ".info2"] = info(m)
    out[name + ".matrix"] = m.split_assembly(matrix=True)["matrix"].copy()
    out[name + ".info3"] = info(m)
    d = np.random.default_rng(3).standard_normal(3 * case["Nb"])
    out[name + ".spmv"] = m.spmv(d)
    m.ilu0_factor(want_factors=False)     # now from the matrix's own array: the copying form on both sides
    factors(m, name + ".g")
    t, z = m.preconditioned_product(d)
    out[name + ".t"], out[name + ".z"] = t, z
    # a full solve
    m = model(case, src)
    m.assemble(DT, 0, fetch=False)
    res = m.solve_jacobian_system()
    out[name + ".x"] = m.get_result()
    out[name + ".it"] = np.array([res.it, res.converged, res.reduction])
    out[name + ".info4"] = info(m)
    # three Newton iterations through newton.py
    m = model(case, src, tolerance=1e-2)
    nm = pkg.newton.BlackoilModelHip(m)
    its = []
    for it in range(3):
        nm.nonlinear_iteration(it, DT)
        its.append(getattr(nm, "last_linear_iterations", -1))
    pv, mg = m.get_state()
    out[name + ".newton_pv"], out[name + ".newton_meaning"], out[name + ".newton_its"] = pv, mg, np.array(its)
    out[name + ".info5"] = info(m)

# a cell cut off from everything: an all-zero diagonal block, fixed up by the factorisation of the solve
case = pkg.decks.cartesian_case(6, 5, 4, state="mixed", heterogeneous=True)
cut = 37
rp, ci = np.asarray(case["rowptr"]), np.asarray(case["col"])
case["poro"] = np.asarray(case["poro"], float).copy()
case["poro"][cut] = 0.0
tr = np.asarray(case["trans"], float).copy()
tr[rp[cut]:rp[cut + 1]] = 0.0
tr[ci == cut] = 0.0
case["trans"] = tr
src = pkg.decks.five_spot_source(case, rate_sm3_per_day=50.0)
src.reshape(-1, 3)[cut] = 0.0
m = model(case, src)
m.assemble(86400.0, 0, fetch=False)
res = m.solve_jacobian_system()
out["zero.x"], out["zero.it"] = m.get_result(), np.array([res.it, res.converged])
factors(m, "zero.f")
out["zero.info"] = info(m)
out["zero.matrix"] = m.split_assembly(matrix=True)["matrix"].copy()
kd = [k for k in range(rp[cut], rp[cut + 1]) if ci[k] == cut][0]
out["zero.diag"] = out["zero.matrix"].reshape(-1, 9)[kd].copy()
e = np.zeros(3 * case["Nb"])
e[3 * cut:3 * cut + 3] = 1.0
out["zero.spmv"] = m.spmv(e)

# contexts that keep the matrix's own array: CPR, ILU(1), a well list in its matrix-add form
plain = pkg.decks.cartesian_case(6, 5, 4, state="mixed", heterogeneous=True)
psrc = pkg.decks.five_spot_source(plain, rate_sm3_per_day=30.0)
for tag, kw in (("cpr", dict(preconditioner="cpr_quasiimpes")), ("ilu1", dict(ilu_fillin_level=1))):
    m = model(plain, psrc, **kw)
    m.assemble(DT, 0, fetch=False)
    out["off." + tag] = info(m)

W = pkg.wells
def well_list(m):
    cells = [7, 37]   # neighbours in z: every block the well touches is in the grid's own pattern
    tw = [W.peaceman_factor(plain["perm"][c], plain["dx"], plain["dy"], plain["dz"], 0.15) for c in cells]
    wl = [W.Well("P", cells, tw, plain["depth"][cells[0]], True, ("rate", W.OIL, 4.0 / 86400.0), 150e5)]
    return W.DeviceStandardWells(wl, plain["depth"], m, matrix_add=True)

def well_iteration(m, w, it):
    w.begin_iteration(it)
    m.assemble(DT, it, fetch=False)
    m.std_wells_apply_residual()
    m.std_wells_add_to_matrix()
    res = m.solve_jacobian_system()
    return m.get_result().copy(), np.array([res.it, res.converged])

# the list arrives after two iterations without it ...
m = model(plain, psrc, tolerance=1e-2)
nm = pkg.newton.BlackoilModelHip(m)
for it in range(2):
    nm.nonlinear_iteration(it, DT)
out["late.info_before"] = info(m)
pv, mg = m.get_state()
w = well_list(m)
out["late.info_list"] = info(m)
out["late.x"], out["late.it"] = well_iteration(m, w, 2)
out["late.info_after"] = info(m)
# ... or was there from the start
m = model(plain, psrc, tolerance=1e-2)
w = well_list(m)
out["early.info_list"] = info(m)
m.assemble(DT, 0, fetch=False)   # the old time level's storage, formed at the initial state as in the other context
m.set_state(pv, mg)
out["early.x"], out["early.it"] = well_iteration(m, w, 2)
out["early.info_after"] = info(m)
# a host list written into the matrix after a split assembly
m = model(plain, psrc)
m.assemble(DT, 0, fetch=False)
rng = np.random.default_rng(15)
cells = np.array([7, 37], np.int32)
HW = dict(numWells=1, val_pointers=np.array([0, 2], np.int32), Ccols=cells.copy(), Bcols=cells.copy(), Cnnzs=rng.uniform(-0.05, 0.05, 24),
          Bnnzs=rng.uniform(-0.05, 0.05, 24), Dnnzs=(np.eye(4) + rng.uniform(-0.1, 0.1, (4, 4))).reshape(-1))
m.add_well_contributions(HW)
res = m.solve_jacobian_system()
out["host.x"], out["host.it"], out["host.info"] = m.get_result(), np.array([res.it, res.converged]), info(m)
np.savez(out_path, **out)
""" % (SHAPES,)


@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    """{1: record with the split form, 0: record with OPMHIP_SPLIT_ASM=0}"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("split")
    rec = {}
    for on in (1, 0):
        env = dict(os.environ)
        env.update(OPMHIP_TUNING="1", OPMHIP_SPLIT_ASM=str(on))
        f = str(tmp / ("side%d.npz" % on))
        r = subprocess.run([sys.executable, "-c", WORKER, root, f], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        assert "OPMHIP_SPLIT_ASM=%d is in force" % on in r.stderr
        rec[on] = dict(np.load(f))
    return rec


def same(sides, key):
    a, b = sides[1][key], sides[0][key]
    assert a.shape == b.shape and np.array_equal(a, b), key


@pytest.mark.parametrize("name", list(SHAPES))
def test_state_and_counters(sides, name):
    """[on, stale, assemblies, gathers]: the form is on where asked and off under the switch; an assembly leaves the matrix's own array
    stale until something reads it - ONE gather -, and neither a solve nor three Newton iterations read it"""
    s, u = sides[1], sides[0]
    assert list(s[name + ".info0"]) == [1, 0, 0, 0] and list(u[name + ".info0"]) == [0, 0, 0, 0]
    assert list(s[name + ".info1"]) == [1, 1, 1, 0] and list(s[name + ".info2"]) == [1, 1, 1, 0]   # the factorisation reads the streams
    assert list(s[name + ".info3"]) == [1, 0, 1, 1]
    assert list(s[name + ".info4"]) == [1, 1, 1, 0]
    assert list(s[name + ".info5"]) == [1, 1, 3, 0]
    for k in ("info1", "info2", "info3", "info4", "info5"):
        assert list(u[name + "." + k]) == [0, 0, 0, 0], k


@pytest.mark.parametrize("name", list(SHAPES))
def test_factors_streams_and_residual(sides, name):
    for k in ("resid", "f.L", "f.invD", "f.U", "f.R"):
        same(sides, name + "." + k)
    assert np.all(np.isfinite(sides[1][name + ".f.L"])) and np.all(np.isfinite(sides[1][name + ".f.invD"])) and np.any(sides[1][name + ".f.R"] != 0.0)
    # and the factorisation from the gathered matrix leaves what the one from the streams left
    for k in ("L", "invD", "U", "R"):
        assert np.array_equal(sides[1][name + ".g." + k], sides[1][name + ".f." + k]), k
        same(sides, name + ".g." + k)


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_matrix_is_gathered_on_demand(sides, name):
    same(sides, name + ".matrix")
    same(sides, name + ".spmv")
    same(sides, name + ".t")
    same(sides, name + ".z")
    assert np.any(sides[1][name + ".matrix"] != 0.0)


@pytest.mark.parametrize("name", list(SHAPES))
def test_a_full_solve(sides, name):
    same(sides, name + ".x")
    same(sides, name + ".it")
    assert sides[1][name + ".it"][1] == 1.0


@pytest.mark.parametrize("name", list(SHAPES))
def test_three_newton_iterations(sides, name):
    for k in ("newton_pv", "newton_meaning", "newton_its"):
        same(sides, name + "." + k)


def test_zero_diagonal_fix(sides):
    """the fix goes into the rest stream's diagonal block, where the product reads it, and reaches the matrix with the gather"""
    for k in ("x", "it", "f.L", "f.invD", "f.U", "f.R", "matrix", "diag", "spmv"):
        same(sides, "zero." + k)
    s = sides[1]
    assert list(s["zero.info"]) == [1, 1, 1, 0]
    assert np.array_equal(s["zero.diag"], np.array([1e-15, 0, 0, 0, 1e-15, 0, 0, 0, 1e-15]))
    assert np.array_equal(s["zero.spmv"].reshape(-1, 3)[37], np.full(3, 1e-15)) and s["zero.it"][1] == 1.0


def test_contexts_that_keep_the_matrix(sides):
    s = sides[1]
    assert list(s["off.cpr"]) == [0, 0, 0, 0] and list(s["off.ilu1"]) == [0, 0, 0, 0]
    assert list(s["early.info_list"]) == [0, 0, 0, 0] and list(s["early.info_after"]) == [0, 0, 0, 0]   # (two assemblies, none of them split)


def test_a_well_list_arrives_after_two_split_iterations(sides):
    s = sides[1]
    assert list(s["late.info_before"]) == [1, 1, 2, 0]
    assert s["late.info_list"][0] == 0                       # the list is to be added to the matrix: the next assembly writes the matrix itself
    assert list(s["late.info_after"]) == [0, 0, 2, 0]        # ... and did: nothing was gathered
    assert np.array_equal(s["late.x"], s["early.x"]) and np.array_equal(s["late.it"], s["early.it"]) and s["late.it"][1] == 1.0
    for k in ("late.x", "late.it", "early.x", "early.it", "host.x", "host.it"):
        same(sides, k)
    assert list(s["host.info"]) == [1, 0, 1, 1]              # a host list goes into the matrix's own array: gathered first, once
