"""Cases the tracer tests share (tests/test_tracers.py on the CPU, tests/test_gpu_tracers.py on the device): grids with a THPRES-blocked
face, a begin-of-step and an end-of-step state with flow in both directions, connection lists that name a cell twice, the solve cases
whose stopping decisions are clear, and the measured margin between two summation orders of the solver's scalar products."""
import numpy as np

DAY = 86400.0
DT = 30.0 * DAY
WATER, OIL, GAS = 0, 1, 2

# The largest relative difference of dx (rel_diff below) between two runs of tracers.HostTracers.end_time_step on the CPU that differ only
# in how the scalar products of BiCGStab are summed - sequentially (dot="sequential") against numpy's pairwise sums (dot="pairwise") -
# over solve_case(9, 9, 2) and solve_case(12, 12, 12) at tolerance 1e-2 in the natural order, a red-black order and an order by the
# levels i + j + k.  It came from solve_case(12, 12, 12) in the red-black order (tools/tracer_margin.py prints all of them).  The device's
# two-stage reductions are a third summation order: tests/test_gpu_tracers.py holds it to 10 x this.
DX_MARGIN = 9.912e-15


def rel_diff(a, b):
    """largest over the tracers of max |a_t - b_t| / max |a_t| (tracers whose a_t is zero must agree exactly)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    out = 0.0
    for x, y in zip(a, b):
        s = np.abs(x).max()
        if s == 0.0:
            assert np.array_equal(x, y)
            continue
        out = max(out, float(np.abs(x - y).max() / s))
    return out


def entry(case, i, j):
    rp, col = case["rowptr"], case["col"]
    ks = np.arange(rp[i], rp[i + 1])
    return int(ks[col[ks] == j][0])


def block_face(case, a, b, value=1e9):
    """a THPRES value on the face between cells a and b that no pressure difference of these cases passes"""
    if case.get("thpres") is None:
        case["thpres"] = np.zeros(len(case["col"]))
    case["thpres"][entry(case, a, b)] = value
    case["thpres"][entry(case, b, a)] = value


def moved_state(case, seed=0, dp=2.0e5, dsw=0.01):
    """the state at the end of a time step: pressures moved by random amounts of the order of dp - flow across every face, in both
    directions - and water saturations by dsw"""
    rng = np.random.default_rng(seed)
    pv = case["pv"].reshape(-1, 3).copy()
    pv[:, 1] += dp * rng.standard_normal(len(pv))
    pv[:, 0] += dsw * rng.uniform(-1.0, 1.0, len(pv))
    return np.ascontiguousarray(pv.reshape(-1))


def system_case(pkg, dims, ext=False):
    """heterogeneous `mixed` case with gravity; ext: the extended (19-field) record of helpers.hysteresis_case; one THPRES-blocked face where
    the grid has one.  -> (case, end-of-step primary variables)"""
    import helpers
    nx, ny, nz = dims
    case = helpers.hysteresis_case(pkg, nx, ny, nz, heterogeneous=True) if ext else pkg.decks.cartesian_case(nx, ny, nz, state="mixed", heterogeneous=True)
    if nx > 2:
        a = (nx // 2) + nx * (ny // 2)
        block_face(case, a, a + 1)
    return case, moved_state(case)


def system_tracers(case):
    """a water batch of three and an oil batch of one, interleaved in the caller's list: phases and initial concentrations"""
    rng = np.random.default_rng(7)
    Nb = case["Nb"]
    phase = [WATER, OIL, WATER, WATER]
    c = rng.uniform(0.0, 1.0, (4, Nb))
    c[2] = 0.5
    c[3, ::2] = 0.0
    return phase, c


def system_connections(case, ntracers):
    """four connections, the first cell named twice (once injecting, once producing): (cells, rates [n, 3] water / oil / gas, injected)"""
    Nb = case["Nb"]
    cells = np.array([0, Nb - 1, 0, Nb // 2], np.int32)
    rates = np.array([[1.5e-3, 2.0e-4, 0.0], [-1.0e-3, -2.5e-3, -0.1], [-3.0e-4, 1.0e-4, 0.0], [0.0, -5.0e-4, 0.0]])
    rng = np.random.default_rng(11)
    return cells, rates, rng.uniform(0.0, 1.0, (ntracers, len(cells)))


def solve_case(pkg, dims):
    """three oil tracers with very different right-hand sides - one present only at the injector (concentration 0 in place, 1 in what is
    injected), one uniform, one zero everywhere and not injected - on a closed box with an oil injector in the middle of the top layer and a
    producer in the last cell.  (The water phase of these cases hardly moves: its systems are diagonal to rounding and every solve ends
    after half an iteration.)  -> dict(case, pv1, phase, c, cells, rates, injected)"""
    nx, ny, nz = dims
    case = pkg.decks.cartesian_case(nx, ny, nz, state="mixed", heterogeneous=True)
    Nb = case["Nb"]
    c = np.zeros((3, Nb))
    c[1] = 1.0
    cells = np.array([(nx // 2) + nx * (ny // 2), Nb - 1], np.int32)
    rates = np.array([[0.0, 2.0e-3, 0.0], [0.0, -2.0e-3, 0.0]])
    injected = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 0.0]])
    return dict(case=case, pv1=moved_state(case), phase=[OIL, OIL, OIL], c=c, cells=cells, rates=rates, injected=injected)


def emulated_orders(nx, ny, nz):
    """(toOrder, fromOrder) of orderings that can be formed without a device: natural, red-black (a two-colouring of the 7-point grid),
    the levels i + j + k"""
    Nb = nx * ny * nz
    idx = np.arange(Nb)
    i, j, k = idx % nx, (idx // nx) % ny, idx // (nx * ny)
    out = {"natural": None}
    for name, key in (("red-black", (i + j + k) % 2), ("levels", i + j + k)):
        fr = np.lexsort((idx, key))
        to = np.empty(Nb, np.int64)
        to[fr] = idx
        out[name] = (to, fr)
    return out


def clear_decisions(results, tol, window=1e-6):
    """every stopping decision of a host run is clear: | ||r|| / ||b|| - tol | > window tol at every half iteration"""
    for r in results:
        for norm, norm0 in r["history"]:
            if not abs(norm / norm0 - tol) > window * tol:
                return False
    return True


def dense(case, M):
    Nb = case["Nb"]
    A = np.zeros((Nb, Nb))
    rp, col = case["rowptr"], case["col"]
    for i in range(Nb):
        A[i, col[rp[i]:rp[i + 1]]] = M[rp[i]:rp[i + 1]]
    return A
