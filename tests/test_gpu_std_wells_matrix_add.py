"""The matrix-add form of the resident standard wells (opmhip_set_std_wells_matrix_add, opmhip_std_wells_add_to_matrix): A -= C^T D^-1 B
written into the Jacobian on the pattern that holds the wells' cliques.

The case is decks.cartesian_case(6, 5, 4) - 120 cells, cell = i + 6 (j + 5 k) - on the clique pattern of five wells: a producer with three
completions in one column; a producer with four that shares a cell with it; a producer that perforates one cell twice; a one-completion
injector; a producer with allow_crossflow and an LRAT limit (another instantiation of the equations' kernel forms its blocks)."""
import numpy as np
import pytest

from std_wells_harness import launch_counts, minus

pytestmark = pytest.mark.gpu

DAY = 86400.0
DT = 5.0 * DAY
CELLS = [[7, 37, 67], [67, 68, 98, 99], [22, 52, 22], [119], [18, 48, 78, 108]]


def make_wells(pkg, case):
    W = pkg.wells

    def well(name, cells, producer, control, limit, **kw):
        tw = [W.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], 0.15) for c in cells]
        return W.Well(name, cells, tw, case["depth"][cells[0]], producer, control, limit, **kw)
    return [well("P3", CELLS[0], True, ("rate", W.OIL, 4.0 / DAY), 150e5),
            well("P4", CELLS[1], True, ("rate", W.OIL, 3.0 / DAY), 150e5),
            well("PTWICE", CELLS[2], True, ("rate", W.OIL, 2.0 / DAY), 150e5),
            well("I1", CELLS[3], False, ("rate", W.WATER, 6.0 / DAY), 400e5, inj_phase="water"),
            well("PX", CELLS[4], True, ("rate", W.OIL, 3.0 / DAY), 150e5, allow_crossflow=True, limits={"lrat": 50.0 / DAY})]


@pytest.fixture(scope="module")
def cases(pkg):
    plain = pkg.decks.cartesian_case(6, 5, 4, state="mixed", heterogeneous=True)
    clique = pkg.decks.with_well_cliques(plain, make_wells(pkg, plain))
    _, old_pos = pkg.grid.with_well_cliques(dict(Nb=plain["Nb"], rowptr=plain["rowptr"], col=plain["col"]), CELLS)
    return plain, clique, old_pos


def model(pkg, case, matrix_add, **kw):
    m = pkg.capi.HipModel(case, **kw)
    m.set_state(case["pv"], case["meaning"])
    w = pkg.wells.DeviceStandardWells(make_wells(pkg, case), case["depth"], m, matrix_add=matrix_add)
    return m, w


def host_list(w, blk):
    return dict(numWells=w.nw, val_pointers=w.vp, Ccols=w.cells, Bcols=w.cells.copy(), Cnnzs=np.ascontiguousarray(blk["C"].reshape(-1)),
                Bnnzs=np.ascontiguousarray(blk["B"].reshape(-1)), Dnnzs=np.ascontiguousarray(blk["Dinv"].reshape(-1)))


def iteration(m, w, it, add, relax=1.0):
    """newton.py's device branch, stage by stage -> (result of the solve, dx, x_w)"""
    w.begin_iteration(it)
    m.assemble(DT, it, fetch=False)
    m.std_wells_apply_residual()
    if add:
        m.std_wells_add_to_matrix()
    res = m.solve_jacobian_system()
    w.update(relax)
    dx, xw = m.get_result().copy(), m.std_wells_blocks()["xw"].copy()
    m.update(None, relax)
    return res, dx, xw


# ---- 1. the assembly on the clique pattern ----------------------------------------------------------------------------------------------------
def test_assembly_on_the_clique_pattern(pkg, cases):
    """a clique entry is a face with transmissibility zero: J and r of the plain pattern in every shared entry (== so that -0.0 passes),
    zero clique blocks.  The wells in operator form: no new kernel runs"""
    plain, clique, old_pos = cases
    (mp, wp), (mc, wc) = model(pkg, plain, False), model(pkg, clique, False)
    assert len(clique["col"]) == len(plain["col"]) + 2 + 6 + 6               # the pairs that are no face, both ways: (7, 67); (67, 98), (67, 99), (68, 99); (18, 78), (18, 108), (48, 108)
    for it in (0, 1):
        wp.begin_iteration(it)
        wc.begin_iteration(it)
        (jp, rp), (jc, rc) = mp.assemble(DT, it), mc.assemble(DT, it)
        jp, jc = jp.reshape(-1, 9), jc.reshape(-1, 9)
        fresh = np.ones(len(jc), bool)
        fresh[old_pos] = False
        assert np.all(np.isfinite(jc)) and np.all(jc[old_pos] == jp) and np.all(rc == rp), it
        assert fresh.sum() == 14 and np.all(jc[fresh] == 0.0), it
        bp, bc = mp.std_wells_blocks(), mc.std_wells_blocks()
        for k in ("Dinv", "B", "C"):
            assert np.array_equal(bp[k], bc[k]) and np.any(bc[k] != 0.0), k
        assert not mc.std_wells_matrix_add_info()["on"]
        for m in (mp, mc):   # move on, the same way on both
            pv = plain["pv"].reshape(-1, 3).copy()
            pv[:, 1] -= 1.0e5 * np.random.default_rng(5).uniform(0.0, 1.0, len(pv))
            m.set_state(pv.reshape(-1), plain["meaning"])


# ---- 2. the add, bit for bit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reorder", ["graph_coloring", "line_coloring"])
def test_the_add_bit_for_bit(pkg, orc, cases, reorder):
    _, clique, _ = cases
    Nb, rp, ci = clique["Nb"], clique["rowptr"], clique["col"]
    m, w = model(pkg, clique, True, reorder=reorder)
    info = m.std_wells_matrix_add_info()
    # distinct blocks: 9 + (16 - 1) + 4 + 1 + 16; pairs: 9 + 16 + 9 + 1 + 16
    assert info == dict(on=True, targets=45, pairs=51, in_matrix=False)
    w.begin_iteration(0)
    jac, _ = m.assemble(DT, 0)
    blk = m.std_wells_blocks()
    W = host_list(w, blk)
    assert np.all(np.isfinite(blk["Dinv"])) and all(np.any(blk[k][w.vp[4]:] != 0.0) for k in ("B", "C"))
    rc, vo = orc.wells_add_to_matrix(Nb, rp, ci, jac, W)
    assert rc == 0 and not np.array_equal(vo, jac)
    m.std_wells_add_to_matrix()
    to, fr, _ = m.ordering()
    rr, rc_, rv = orc.reorder_matrix(Nb, rp, ci, vo, to, fr)
    # the same blocks as a host list, into the same Jacobian on a second context
    s = pkg.capi.HipSolver(reorder=reorder, zero_diag_fix=False)
    s.set_pattern(Nb, rp, ci)
    s.upload_system(jac)
    s.add_well_contributions(W)
    for seed in range(3):
        x = np.random.default_rng(seed).standard_normal(Nb * 3)
        yo = orc.spmv(Nb, rr, rc_, rv, x.reshape(Nb, 3)[fr].reshape(-1)).reshape(Nb, 3)[to].reshape(-1)
        y = m.spmv(x)
        print("add, %s, x %d: max |y - oracle| = %.3e, max |y - host list| = %.3e" % (reorder, seed, np.abs(y - yo).max(), np.abs(y - s.spmv(x)).max()))
        assert np.array_equal(y, yo)
        assert np.array_equal(s.spmv(x), y)


# ---- 3. the same physics two ways -------------------------------------------------------------------------------------------------------------------
def dense_solve_longdouble(A, b):
    """Gaussian elimination with partial pivoting in np.longdouble (numpy's solvers stop at double)"""
    A, b = np.array(A, np.longdouble), np.array(b, np.longdouble)
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]], b[[k, p]] = A[[p, k]], b[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= f[:, None] * A[k, k:][None, :]
        b[k + 1:] -= f * b[k]
    x = np.zeros(n, np.longdouble)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


@pytest.mark.parametrize("preconditioner", ["ilu0", "cpr"])
def test_one_newton_iteration_two_ways(pkg, orc, cases, preconditioner):
    """one Newton iteration from one state with the wells as the operator A - C^T D^-1 B and with the wells in the matrix, linear tolerance
    1e-10 for both: the reservoir update and the well update agree to rtol 1e-6, atol 1e-8 - the bound of
    test_add_well_contributions_to_matrix for the same identity.  The figures (and both solves against a dense long-double solve of the
    system) are printed before the assertion."""
    _, clique, _ = cases
    Nb, rp, ci = clique["Nb"], clique["rowptr"], clique["col"]
    out = {}
    for form in ("operator", "matrix"):
        m, w = model(pkg, clique, form == "matrix", tolerance=1e-10, maxit=200, preconditioner=preconditioner)
        w.begin_iteration(0)
        jac, _ = m.assemble(DT, 0)
        m.std_wells_apply_residual()
        rhs = m.get_rhs()
        if form == "matrix":
            m.std_wells_add_to_matrix()
        res = m.solve_jacobian_system()
        w.update(1.0)
        out[form] = dict(res=res, dx=m.get_result().copy(), xw=m.std_wells_blocks()["xw"].copy(), jac=jac, rhs=rhs, W=host_list(w, m.std_wells_blocks()))
    op, mat = out["operator"], out["matrix"]
    assert op["res"].converged and mat["res"].converged
    assert np.array_equal(op["jac"], mat["jac"]) and np.array_equal(op["rhs"], mat["rhs"])       # one system
    rc, vo = orc.wells_add_to_matrix(Nb, rp, ci, op["jac"], op["W"])
    assert rc == 0
    A = np.zeros((3 * Nb, 3 * Nb))
    for i in range(Nb):
        for k in range(rp[i], rp[i + 1]):
            A[3 * i:3 * i + 3, 3 * ci[k]:3 * ci[k] + 3] = vo[9 * k:9 * k + 9].reshape(3, 3)
    exact = dense_solve_longdouble(A, op["rhs"])
    scale = np.abs(exact).astype(float)
    for name, key in (("reservoir update", "dx"), ("well update", "xw")):
        a, b = mat[key].reshape(-1), op[key].reshape(-1)
        excess = np.abs(a - b) - (1e-8 + 1e-6 * np.abs(b))
        print("%s, %s: linear iterations %d (operator) / %d (matrix); max |difference| %.3e, max relative %.3e, largest excess over atol + rtol |b| %.3e"
              % (preconditioner, name, op["res"].iterations, mat["res"].iterations, np.abs(a - b).max(), (np.abs(a - b) / np.maximum(np.abs(b), 1e-300)).max(), excess.max()))
    for form in ("operator", "matrix"):
        e = np.abs(out[form]["dx"] - exact).astype(float)
        print("%s, %s form against the dense long-double solve: max |error| %.3e, max |error| / (1e-8 + 1e-6 |x|) %.3e" % (preconditioner, form, e.max(), (e / (1e-8 + 1e-6 * scale)).max()))
    np.testing.assert_allclose(mat["dx"], op["dx"], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(mat["xw"], op["xw"], rtol=1e-6, atol=1e-8)
    assert np.any(op["xw"] != 0.0) and np.any(op["dx"] != 0.0)


def test_a_short_schedule_in_both_forms(pkg, cases):
    """three time steps through BlackoilModelHip: both forms converge and report the same controls in force (no bound on the iteration
    counts: the preconditioners differ by design)"""
    _, clique, _ = cases
    runs = {}
    for form in ("operator", "matrix"):
        m, w = model(pkg, clique, form == "matrix", tolerance=1e-6, maxit=200)
        mdl = pkg.newton.BlackoilModelHip(m, well_model=w)
        ts = pkg.newton.AdaptiveTimeStepping(mdl, pkg.newton.TimeSteppingParameters(initial_dt=DAY))
        controls, linear = [], 0
        for length in (DAY, 2.0 * DAY, 3.0 * DAY):
            reps = ts.advance_report_step(length)
            linear += sum(r.total_linear_iterations for r in reps)
            controls.append([q.control[0] for q in w.wells])
        runs[form] = dict(history=list(ts.history), time=ts.time, controls=controls, info=m.std_wells_matrix_add_info())
        print("schedule, %s form: steps %r, linear iterations %d, controls %r" % (form, [(round(h[0] / DAY, 3), h[1], h[2]) for h in ts.history], linear, controls[-1]))
    op, mat = runs["operator"], runs["matrix"]
    for r in (op, mat):
        assert len(r["history"]) >= 3 and all(ok for _, _, ok in r["history"]) and abs(r["time"] - 6.0 * DAY) < 1.0      # every step converged
    assert op["controls"] == mat["controls"]
    assert mat["info"]["on"] and not op["info"]["on"]


# ---- 4. bookkeeping ------------------------------------------------------------------------------------------------------------------------------------
def counts(m):
    m.synchronize()
    return launch_counts(m)


def test_launch_counts(pkg, cases):
    """a list without the switch launches what a list that never heard of it launches (here: one that had it on and off again); with the
    switch one more assembly-class scope per iteration, and the solve is the solve of a context without any wells on the same matrix and
    right-hand side - its launches class by class, its iterations, its bits"""
    _, clique, _ = cases
    per = {}
    for touched in (False, True):
        m, w = model(pkg, clique, False)
        if touched:
            m.set_std_wells_matrix_add(True)
            m.set_std_wells_matrix_add(False)
            assert m.std_wells_matrix_add_info() == dict(on=False, targets=0, pairs=0, in_matrix=False)
        m.profile_enable(True)
        res, dx, xw = iteration(m, w, 0, add=False)
        per[touched] = (counts(m), res.iterations, dx, xw)
    assert per[False][0] == per[True][0] and per[False][1] == per[True][1] and np.array_equal(per[False][2], per[True][2]) and np.array_equal(per[False][3], per[True][3])
    # (the assembly class of a time step's first iteration, as tests/test_gpu_std_wells_device.py counts it: the wells alone, the controls, the
    # equations with the source rows, the assembly kernel, the restore, and the update's axpy)
    assert per[False][0]["assemble"] == 6
    m, w = model(pkg, clique, True)
    m.profile_enable(True)
    w.begin_iteration(0)
    jac, _ = m.assemble(DT, 0)
    m.std_wells_apply_residual()
    c0 = counts(m)
    m.std_wells_add_to_matrix()
    c1 = counts(m)
    assert minus(c1, c0) == dict({k: 0 for k in c0}, assemble=1)                                   # exactly one scope, of the assembly class
    rhs = m.get_rhs()
    res = m.solve_jacobian_system()
    solve = minus(counts(m), c1)
    x = m.get_result().copy()
    w.update(1.0)
    m.update(None, 1.0)
    total = counts(m)
    assert total["assemble"] == per[False][0]["assemble"] + 1
    # a context without resident wells: the same Jacobian and right-hand side uploaded, the same blocks added as a host list (the same
    # bits: test_the_add_bit_for_bit), so that nothing of a well is left for its solve to launch
    s = pkg.capi.HipModel(clique)
    s.set_state(clique["pv"], clique["meaning"])
    s.upload_system(jac, rhs)
    s.add_well_contributions(host_list(w, m.std_wells_blocks()))
    s.profile_enable(True)
    c2 = counts(s)
    res2 = s.solve_jacobian_system()
    solve2 = minus(counts(s), c2)
    print("matrix form: solve launches %r, %d iterations; without wells on the same matrix %r, %d iterations; operator form's iteration %r" % (solve, res.iterations, solve2, res2.iterations, per[False][0]))
    assert solve == solve2 and res.iterations == res2.iterations and np.array_equal(x, s.get_result())


def test_the_record_of_what_is_in_the_matrix(pkg, cases):
    C = pkg.capi
    plain, clique, _ = cases
    m, w = model(pkg, clique, True)
    x = np.random.default_rng(3).standard_normal(3 * clique["Nb"])

    def refused(call, word):
        with pytest.raises(C.OpmHipError) as e:
            call()
        assert e.value.code == C.NOT_READY and word in str(e.value), str(e.value)

    in_matrix = lambda: m.std_wells_matrix_add_info()["in_matrix"]
    refused(m.std_wells_add_to_matrix, "before opmhip_assemble")                                   # an add before any assemble
    w.begin_iteration(0)
    refused(m.std_wells_add_to_matrix, "before opmhip_assemble")
    m.assemble(DT, 0, fetch=False)
    y0 = m.spmv(x)
    assert not in_matrix()
    m.std_wells_add_to_matrix()
    assert in_matrix()
    y1 = m.spmv(x)
    assert not np.array_equal(y0, y1)
    refused(m.std_wells_add_to_matrix, "already")                                                  # a second add would subtract twice
    assert np.array_equal(m.spmv(x), y1) and in_matrix()                                           # ... and the matrix keeps its bits
    m.std_wells_apply_residual()                                                                   # unchanged by the form
    assert m.solve_jacobian_system().converged
    w.update(1.0)
    m.update(None, 1.0)
    w.begin_iteration(1)
    m.assemble(DT, 1, fetch=False)
    assert not in_matrix()                                                                         # 0 -> 1 -> 0 across assemble / add / assemble
    # the switch off again: NOT_READY, and the values 0 / 1 only
    m.set_std_wells_matrix_add(False)
    refused(m.std_wells_add_to_matrix, "not switched on")
    with pytest.raises(C.OpmHipError) as e:
        m.set_std_wells_matrix_add(2)
    assert e.value.code == C.INVALID_ARGUMENT and "on = 2" in str(e.value)
    m.set_std_wells_matrix_add(True)
    assert m.std_wells_matrix_add_info()["targets"] == 45
    # replacing the list clears the switch, clearing it too; without a list NOT_READY
    w2 = pkg.wells.DeviceStandardWells(make_wells(pkg, clique), clique["depth"], m)
    assert m.std_wells_matrix_add_info() == dict(on=False, targets=0, pairs=0, in_matrix=False) and not w2.matrix_add
    m.set_std_wells(None)
    refused(lambda: m.set_std_wells_matrix_add(True), "no resident list")
    refused(m.std_wells_add_to_matrix, "no resident list")


def test_the_plain_pattern_is_refused(pkg, cases):
    """the switch on a pattern without the cliques: INVALID_ARGUMENT (a ValueError in the Python classes) whose text names the well and the two
    cells; the switch stays off and the next iteration in operator form gives the bits of a context that never asked"""
    C = pkg.capi
    plain, _, _ = cases
    (ma, wa), (mb, wb) = model(pkg, plain, False), model(pkg, plain, False)
    assert C.lib().opmhip_set_std_wells_matrix_add(ma._h, 1) == C.INVALID_ARGUMENT
    msg = C.lib().opmhip_last_error(ma._h).decode()
    assert "block (7, 67) of well 0" in msg and "not in the pattern" in msg, msg
    with pytest.raises(ValueError, match="of well 0"):
        ma.set_std_wells_matrix_add(True)
    assert ma.std_wells_matrix_add_info() == dict(on=False, targets=0, pairs=0, in_matrix=False)
    with pytest.raises(C.OpmHipError):
        ma.std_wells_add_to_matrix()
    (ra, dxa, xwa), (rb, dxb, xwb) = iteration(ma, wa, 0, add=False), iteration(mb, wb, 0, add=False)
    assert ra.converged and ra.iterations == rb.iterations and np.array_equal(dxa, dxb) and np.array_equal(xwa, xwb)
    assert np.array_equal(ma.get_state()[0], mb.get_state()[0])
    with pytest.raises(ValueError, match="not in the pattern"):                                    # the wells class hands the refusal on
        pkg.wells.DeviceStandardWells(make_wells(pkg, plain), plain["depth"], ma, matrix_add=True)


def test_time_levels_with_the_switch_on(pkg, cases):
    """advance_time_level / update_failed round trips: the step given up is repeated bit for bit"""
    _, clique, _ = cases
    m, w = model(pkg, clique, True)
    assert iteration(m, w, 0, add=True)[0].converged
    m.advance_time_level()
    first = [iteration(m, w, it, add=True) for it in (0, 1)]
    state = m.get_state()[0].copy()
    assert m.std_wells_matrix_add_info()["in_matrix"]
    m.update_failed()
    info = m.std_wells_matrix_add_info()
    assert info["on"] and info["targets"] == 45
    again = [iteration(m, w, it, add=True) for it in (0, 1)]
    for (ra, dxa, xwa), (rb, dxb, xwb) in zip(first, again):
        assert ra.converged and ra.iterations == rb.iterations and np.array_equal(dxa, dxb) and np.array_equal(xwa, xwb)
    assert np.array_equal(m.get_state()[0], state) and np.any(first[1][1] != 0.0)
