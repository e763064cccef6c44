"""Cases the tracer tests share (tests/test_tracers.py on the CPU, tests/test_gpu_tracers.py and tests/test_gpu_tracer_edges.py on the
device): grids with a THPRES-blocked face, a begin-of-step and an end-of-step state with flow in both directions, connection lists that
name a cell twice, the solve cases whose stopping decisions are clear, the edge cases (wide batches, grids of several reduction
workgroups, cells without mobile water, a pivot that is not finite, connections beyond one wave), and the measured margin between two
summation orders of the solver's scalar products."""
import numpy as np

DAY = 86400.0
DT = 30.0 * DAY
WATER, OIL, GAS = 0, 1, 2

# The largest relative difference of dx (rel_diff below) between two runs of tracers.HostTracers.end_time_step on the CPU that differ only
# in how the scalar products of BiCGStab are summed - sequentially (dot="sequential") against numpy's pairwise sums (dot="pairwise") -
# over every solve case of margin_cases() below at tolerance 1e-2 in the natural order, a red-black order and an order by the levels
# i + j + k.  It came from wide_solve_case(32, OIL) - 32 random oil tracers on 9 x 9 x 2 - in the red-black order (tools/tracer_margin.py
# prints all of them; over solve_case(9, 9, 2) and solve_case(12, 12, 12) alone it was 9.912e-15, from solve_case(12, 12, 12) in the
# red-black order).  The device's two-stage reductions are a third summation order: tests/test_gpu_tracers.py and
# tests/test_gpu_tracer_edges.py hold it to 10 x this.
DX_MARGIN = 2.262e-14


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


# ---- the cases of tests/test_gpu_tracer_edges.py; tests/test_tracers.py proves their properties on the CPU ---------------------------------
WIDTHS = (8, 9, 17, 32)     # a full chunk of TR_CH = 8, one past it, two chunks and one, the cap OPMHIP_TRACERS_MAX_PER_PHASE


def wide_tracers(case, nt, wide=WATER):
    """a batch of nt tracers in the phase `wide` and a batch of one in the other, the single tracer second in the caller's list - the wide
    batch's members are 0, 2, 3, ... nt -, random concentrations, no two tracers alike: phases and initial concentrations"""
    rng = np.random.default_rng(100 + nt)
    phase = [wide] * (nt + 1)
    phase[1] = OIL if wide == WATER else WATER
    return phase, rng.uniform(0.0, 1.0, (nt + 1, case["Nb"]))


def wide_solve_case(pkg, nt, wide):
    """system_case(9 x 9 x 2) with wide_tracers and the connections of system_connections widened to the nt + 1 tracers"""
    case, pv1 = system_case(pkg, (9, 9, 2))
    phase, c = wide_tracers(case, nt, wide)
    cells, rates, injected = system_connections(case, len(phase))
    return dict(case=case, pv1=pv1, phase=phase, c=c, cells=cells, rates=rates, injected=injected)


# the prototypes of solve_case (0 injector-only, 1 uniform, 2 zero) per slot.  17: every chunk [0, 8), [8, 16), [16, 17) holds each prototype
# that fits, the zero tracer sits in slot 16 and in slot 2; 9: no period of three, so that a slot taken modulo 3 or 8 meets another prototype
PROTO_17 = (0, 1, 2, 0, 1, 2, 0, 1, 0, 1, 2, 0, 1, 2, 0, 1, 2)
PROTO_9 = (0, 1, 2, 2, 0, 1, 1, 2, 0)
PERM_17 = (11, 16, 3, 8, 0, 13, 5, 2, 15, 10, 4, 12, 1, 14, 7, 9, 6)     # slot s of the permuted run holds tracer PERM_17[s] of the first
REDUCTION_GRIDS = ((17, 17, 1), (23, 23, 1))                             # 289 and 529 cells: two and three reduction workgroups


def proto_solve_case(pkg, dims, proto):
    """solve_case with len(proto) oil tracers, the one in slot s a copy of prototype proto[s]"""
    sc = solve_case(pkg, dims)
    p = np.asarray(proto)
    return dict(sc, phase=[OIL] * len(p), c=sc["c"][p].copy(), injected=sc["injected"][p].copy(), proto=p)


def ext_solve_case(pkg):
    """system_case(9 x 9 x 2) on the extended record with the tracers and connections of the system comparison, as a solve case"""
    case, pv1 = system_case(pkg, (9, 9, 2), ext=True)
    phase, c = system_tracers(case)
    cells, rates, injected = system_connections(case, len(phase))
    return dict(case=case, pv1=pv1, phase=phase, c=c, cells=cells, rates=rates, injected=injected)


DRY_SW = 0.0      # the SWOF table of the deck gives k_rw = 0 at and below its connate saturation: S_w = 0 itself is immobile


def dry_cells(nx=6, ny=5, nz=3):
    """a 2 x 2 x 3 column in the middle of the 6 x 5 x 3 grid and one isolated cell in the top layer's corner"""
    col = [i + nx * (j + ny * k) for k in range(nz) for j in (1, 2) for i in (2, 3)]
    return np.array(col + [(nx - 1) + nx * (ny - 1)], np.int64)


def dry_case(pkg):
    """cartesian_case(6, 5, 3, mixed, heterogeneous) with S_w = DRY_SW in dry_cells() at the start and at the end of the step: the water
    mobility of the record is exactly 0 there and S_w b_w porosity falls under the clamp of 1e-10 (the deck's tables leave no mobility at
    S_w = 0, so no connate value had to be chosen in its place: tests/test_tracers.py shows it on the oracle's records).  A water batch of
    two (random, uniform) around an oil tracer; water is produced from a cell inside the dry column - the rate is handed in, nothing asks
    whether a well could draw it - and injected outside"""
    case = pkg.decks.cartesian_case(6, 5, 3, state="mixed", heterogeneous=True)
    dry = dry_cells()
    pv0 = case["pv"].reshape(-1, 3).copy()
    pv0[dry, 0] = DRY_SW
    case["pv"] = np.ascontiguousarray(pv0.reshape(-1))
    pv1 = moved_state(case).reshape(-1, 3)
    pv1[dry, 0] = DRY_SW
    rng = np.random.default_rng(5)
    Nb = case["Nb"]
    c = rng.uniform(0.0, 1.0, (3, Nb))
    c[2] = 0.5
    cells = np.array([dry[5], 0, Nb - 2], np.int32)
    rates = np.array([[-4.0e-4, -1.0e-3, 0.0], [1.5e-3, 2.0e-3, 0.0], [-2.0e-4, 0.0, 0.0]])
    injected = rng.uniform(0.0, 1.0, (3, len(cells)))
    return dict(case=case, pv1=np.ascontiguousarray(pv1.reshape(-1)), phase=[WATER, OIL, WATER], c=c, cells=cells, rates=rates, injected=injected, dry=dry)


def pivot_case(pkg):
    """4 x 3 x 2; two oil tracers around a water tracer.  Two producing oil connections of -1e308 in one cell: each rate is finite, their sum on
    that row's diagonal is not.  The first oil tracer's concentration is 0 in that cell.  `sane`: the list that replaces it"""
    case = pkg.decks.cartesian_case(4, 3, 2, state="mixed", heterogeneous=True)
    Nb = case["Nb"]
    cell = 13
    rng = np.random.default_rng(9)
    c = rng.uniform(0.1, 1.0, (3, Nb))
    c[0, cell] = 0.0
    cells = np.array([cell, 0, cell], np.int32)
    rates = np.array([[0.0, -1e308, 0.0], [1.0e-3, 0.0, 0.0], [0.0, -1e308, 0.0]])
    injected = rng.uniform(0.0, 1.0, (3, 3))
    sane = (np.array([0, Nb - 1], np.int32), np.array([[1.0e-3, 1.0e-3, 0.0], [-1.0e-3, -1.0e-3, 0.0]]), rng.uniform(0.0, 1.0, (3, 2)))
    return dict(case=case, pv1=moved_state(case), phase=[OIL, WATER, OIL], c=c, cell=cell, cells=cells, rates=rates, injected=injected, sane=sane)


def wave_connections(case, ntracers):
    """one connection in each of 70 distinct cells in shuffled cell order, rates of mixed sign in both phases, and one more cell named five
    times - inject, produce, zero, produce, inject - spread through the list: 71 distinct cells, more than a wave of 64"""
    rng = np.random.default_rng(13)
    Nb = case["Nb"]
    pick = rng.permutation(Nb)[:71]
    many, cells = int(pick[70]), pick[:70]
    rates = np.zeros((70, 3))
    rates[:, :2] = rng.uniform(0.2, 2.0, (70, 2)) * 1e-3 * rng.choice([-1.0, 1.0], (70, 2))
    five = np.array([[1.0e-3, 7.0e-4, 0.0], [-6.0e-4, -1.1e-3, 0.0], [0.0, 0.0, 0.0], [-3.0e-4, -2.0e-4, 0.0], [5.0e-4, 9.0e-4, 0.0]])
    at = (3, 20, 37, 54, 71)      # places of the five in the list of 75
    cl, rt = list(cells), list(rates)
    for a, r in zip(at, five):
        cl.insert(a, many)
        rt.insert(a, r)
    return np.array(cl, np.int32), np.array(rt), rng.uniform(0.0, 1.0, (ntracers, 75)), many


def margin_cases(pkg):
    """every solve case whose dx the device tests hold to 10 x DX_MARGIN: (name, grid, case) - tools/tracer_margin.py walks them"""
    out = [("solve_case%r" % (d,), d, solve_case(pkg, d)) for d in ((9, 9, 2), (12, 12, 12))]
    for nt in WIDTHS:
        for wide in (WATER, OIL):
            out.append(("wide_solve_case(%d, %s)" % (nt, "WATER" if wide == WATER else "OIL"), (9, 9, 2), wide_solve_case(pkg, nt, wide)))
    out.append(("proto_solve_case((9, 9, 2), PROTO_17)",(9, 9, 2), proto_solve_case(pkg, (9, 9, 2), PROTO_17)))
    for d in REDUCTION_GRIDS:
        out.append(("solve_case%r" % (d,), d, solve_case(pkg, d)))
        out.append(("proto_solve_case(%r, PROTO_9)" % (d,), d, proto_solve_case(pkg, d, PROTO_9)))
    out.append(("dry_case", (6, 5, 3), dry_case(pkg)))
    out.append(("ext_solve_case", (9, 9, 2), ext_solve_case(pkg)))
    return out


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
