"""Passive tracers (TRACER, TBLK / TVDPF, WTRACER): EclTracerModel of the reference, once on the host in plain numpy - the comparator -
and once over the device's calls (opmhip_set_tracers ... opmhip_tracers_end_time_step).

Restated from ebos/ecltracermodel.hh:113-134, 156-439 and ebos/eclgenerictracermodel.cc:86-281:
  computeVolume_ (:158-179)            vol = max(S b porosity, 1e-10) of the tracer's phase
  updateStorageCache (:340-359)        c_initial = c, storage1 = vol c_initial at the start of a time step
  assembleTracerEquations_ (:216-337)  per cell I: r_t = ((vol c_t - storage1_t) V) / dt, M_II = (vol V) / dt; per face f = A v b_up with the
                                       phase's volume flux as the assembly evaluates it with I as the interior cell, r_t += f c_t[up]; where I
                                       is upstream M_II += f and M_JI = -f; per connection with rate q (positive into the reservoir): q > 0:
                                       r_t -= q c_inj, q < 0: r_t -= q c_t and M_II -= q
  advanceTracerFields (:362-383)       M dx_t = r_t from x = 0 for every tracer, c_t -= dx_t
  linearSolve_ (eclgenerictracermodel.cc:248-281)  ILU0 (relaxation 1) + BiCGStab, reduction 1e-2, at most 100 iterations
UNVERIFIED (not in the reference tree): the order of a cell's faces (opm-grid's stencil; here ascending natural column, the order the
assembly sums in), Dune's BiCGSTABSolver and SeqILU (here the block solver's recurrence, bda/cusparseSolverBackend.cu:60-184, and a
row-wise ILU0 that keeps the inverse pivots), opm-common's TVDPF table class (from_tvdpf).
Every sum is stated sequentially, in the order the device's lanes run (wells.sequential_sums is the same idea): the system agrees with
opmhip_get_tracer_system bit for bit."""
import numpy as np

GRAVITY = 9.80665
PHASES = {"water": 0, "oil": 1, "gas": 2}
# records: field numbers of the intensive-quantity cache (capi.HipModel.iq(), the oracle's iq()): value at [:, field, 0]
F_S, F_P, F_B, F_MOB, F_RHO = 0, 3, 6, 9, 12


def _layout(iq):
    nf = iq.shape[1]
    ext = nf == 19
    return ext, (18 if ext else 16)


def phase_volume(iq, phase):
    """computeVolume_ (ecltracermodel.hh:158-179): max(S b porosity, 1e-10) per cell"""
    _, fporo = _layout(iq)
    v = iq[:, F_S + phase, 0] * iq[:, F_B + phase, 0] * iq[:, fporo, 0]
    return np.where(v > 1e-10, v, 1e-10)


def face_values(case, iq, phase):
    """per entry k = (I, J) of the case's pattern: f = A v b_up of the phase with I as the interior cell and whether I is upstream - the value
    arithmetic of the assembly's face flux (ebos/eclfluxmodule.hh:212-357; csrc/assemble.hip face_flux, csrc/tracers.hip tracer_face),
    operation by operation.  Diagonal entries and the faces the flux skips carry (0, False)."""
    rowptr, col = np.asarray(case["rowptr"]), np.asarray(case["col"])
    Nb = int(case["Nb"])
    I = np.repeat(np.arange(Nb), np.diff(rowptr))
    J = col.astype(np.int64)
    ext, _ = _layout(iq)
    trans, area = np.asarray(case["trans"], float), np.asarray(case["area"], float)
    thp = np.asarray(case["thpres"], float) if case.get("thpres") is not None else np.zeros(len(col))
    z, V = np.asarray(case["depth"], float), np.asarray(case["volume"], float)
    g = lambda f, c: iq[c, f + phase, 0]
    mobIn, rhoIn, pIn, bIn = g(F_MOB, I), g(F_RHO, I), g(F_P, I), g(F_B, I)
    mobEx, rhoEx, pEx, bEx = g(F_MOB, J), g(F_RHO, J), g(F_P, J), g(F_B, J)
    tmIn = iq[I, 17, 0] if ext else np.ones(len(I))
    tmEx = iq[J, 17, 0] if ext else np.ones(len(I))
    with np.errstate(all="ignore"):
        skip = ((mobIn <= 0.0) & (mobEx <= 0.0)) | (I == J)
        distZ = z[I] - z[J]
        rhoAvg = (rhoIn + rhoEx) / 2.0
        pressureExterior = pEx + rhoAvg * (distZ * GRAVITY)
        dp = pressureExterior - pIn
        up = np.where(dp > 0.0, False, np.where(dp < 0.0, True, np.where(V[I] > V[J], True, np.where(V[I] < V[J], False, I < J))))
        skip = skip | ~(np.abs(dp) > thp)
        dp = np.where(dp < 0.0, dp + thp, dp - thp)
        surf_in = bIn * (dp * mobIn * tmIn * (-trans / area))
        surf_ex = bEx * (dp * (mobEx * tmEx * (-trans / area)))
        f = (0.0 + np.where(up, surf_in, surf_ex)) * area
    f = np.where(skip, 0.0, f)
    up = np.where(skip, False, up)
    return f, up


def _transpose_entries(Nb, rowptr, col):
    pos = {}
    for i in range(Nb):
        for k in range(rowptr[i], rowptr[i + 1]):
            pos[(i, int(col[k]))] = k
    return np.array([pos[(int(col[k]), i)] for i in range(Nb) for k in range(rowptr[i], rowptr[i + 1])], np.int64)


# ---- scalar ILU0 + BiCGStab (the comparator's solver) ---------------------------------------------------------------------------------
def permute_csr(Nb, rowptr, col, val, order=None):
    """the matrix in the ordering (toOrder, fromOrder) of opmhip_get_ordering: row p = natural row fromOrder[p], columns toOrder[col]
    ascending.  None: natural order.  -> rowptr, col, val, diag as Python lists"""
    if order is None:
        to = fr = np.arange(Nb)
    else:
        to, fr = np.asarray(order[0]), np.asarray(order[1])
    rp, ci, va, dg = [0], [], [], []
    for p in range(Nb):
        i = int(fr[p])
        ks = list(range(rowptr[i], rowptr[i + 1]))
        ks.sort(key=lambda k: to[col[k]])
        for k in ks:
            if int(to[col[k]]) == p:
                dg.append(len(ci))
            ci.append(int(to[col[k]]))
            va.append(float(val[k]))
        rp.append(len(ci))
    return rp, ci, va, dg


def ilu0(rp, ci, va, dg):
    """row-wise ILU0 on the matrix's own pattern: multipliers a_ij (1 / u_jj) in the lower part, inverse pivots kept (csrc/tracers.hip
    k_tracer_ilu_level).  -> (LU values, inverse pivots, a pivot was zero or not finite)"""
    lu = list(va)
    n = len(rp) - 1
    invd = [0.0] * n
    bad = False
    for i in range(n):
        kd, ke = dg[i], rp[i + 1]
        for k in range(rp[i], kd):
            j = ci[k]
            l = lu[k] * invd[j]
            lu[k] = l
            kk = k + 1
            for m in range(dg[j] + 1, rp[j + 1]):
                cj = ci[m]
                while kk < ke and ci[kk] < cj:
                    kk += 1
                if kk < ke and ci[kk] == cj:
                    lu[kk] = lu[kk] - l * lu[m]
        d = lu[kd]
        if not np.isfinite(d) or d == 0.0:
            bad, d = True, 1.0
            lu[kd] = d
        invd[i] = 1.0 / d
    return lu, invd, bad


def ilu0_apply(rp, ci, dg, lu, invd, d):
    n = len(rp) - 1
    y = [0.0] * n
    for i in range(n):
        a = d[i]
        for k in range(rp[i], dg[i]):
            a = a - lu[k] * y[ci[k]]
        y[i] = a
    z = [0.0] * n
    for i in range(n - 1, -1, -1):
        a = y[i]
        for k in range(dg[i] + 1, rp[i + 1]):
            a = a - lu[k] * z[ci[k]]
        z[i] = a * invd[i]
    return z


def _spmv(rp, ci, va, x):
    out = [0.0] * (len(rp) - 1)
    for i in range(len(out)):
        a = 0.0
        for k in range(rp[i], rp[i + 1]):
            a = a + va[k] * x[ci[k]]
        out[i] = a
    return out


def _dot_sequential(a, b):
    p = np.asarray(a) * np.asarray(b)
    return float(np.cumsum(p)[-1]) if len(p) else 0.0     # cumsum adds left to right


def _dot_pairwise(a, b):
    return float(np.sum(np.asarray(a) * np.asarray(b)))     # numpy's pairwise summation


def bicgstab(rp, ci, va, dg, b, tol=1e-2, maxit=100, dot="sequential", factors=None):
    """right-preconditioned BiCGStab with the stopping test at each half iteration, x0 = 0 (bda/cusparseSolverBackend.cu:60-184).
    b in the matrix's ordering.  -> (x, dict(converged, iterations, reduction, history: (norm, norm_0) per half iteration))"""
    ddot = _dot_sequential if dot == "sequential" else _dot_pairwise
    lu, invd, bad = factors if factors is not None else ilu0(rp, ci, va, dg)
    n = len(b)
    x = np.zeros(n)
    r = np.array(b, float)
    rw, p = r.copy(), r.copy()
    norm0 = float(np.sqrt(ddot(r, r)))
    hist = []
    if norm0 == 0.0:    # a zero right-hand side: x = 0 is the solution
        return x, dict(converged=not bad, iterations=0.0, reduction=0.0, history=hist)
    rho, alpha, omega, norm = 1.0, 0.0, 0.0, norm0
    v = np.zeros(n)
    halves, conv = 0, False
    with np.errstate(all="ignore"):
        for it in range(1, maxit + 1):
            rhop = rho
            rho = ddot(rw, r)
            if it > 1:
                beta = (rho / rhop) * (alpha / omega)
                p = beta * (p + (-omega) * v) + r
            pw = np.array(ilu0_apply(rp, ci, dg, lu, invd, p.tolist()))
            v = np.array(_spmv(rp, ci, va, pw.tolist()))
            alpha = rho / ddot(rw, v)
            r = r + (-alpha) * v
            x = x + alpha * pw
            norm = float(np.sqrt(ddot(r, r)))
            halves += 1
            hist.append((norm, norm0))
            if norm < tol * norm0:
                conv = True
                break
            s = np.array(ilu0_apply(rp, ci, dg, lu, invd, r.tolist()))
            t = np.array(_spmv(rp, ci, va, s.tolist()))
            omega = ddot(t, r) / ddot(t, t)
            x = x + omega * s
            r = r + (-omega) * t
            norm = float(np.sqrt(ddot(r, r)))
            halves += 1
            hist.append((norm, norm0))
            if norm < tol * norm0:
                conv = True
                break
    return x, dict(converged=conv and not bad, iterations=0.5 * halves if conv else float(maxit), reduction=norm / norm0, history=hist)


class HostTracers:
    """The tracer model on the host.  case: the static arrays (Nb, rowptr, col, trans, area, thpres, volume, depth); phase: per tracer
    0 water, 1 oil (2 gas is refused as the device refuses it); concentration: (num_tracers, Nb).  The records - capi.HipModel.iq() or the
    oracle's iq() - are handed to begin_time_step and set_records; a connection list to set_connections."""
    on_device = False

    def __init__(self, case, phase, concentration, tolerance=1e-2, maxit=100, dot="sequential"):
        self.case = case
        self.Nb = int(case["Nb"])
        self.phase = [int(p) for p in phase]
        if any(p == 2 for p in self.phase):
            raise ValueError("gas tracers: the fluid always carries dissolved gas, and the reference refuses gas tracers under DISGAS (ecltracermodel.hh:465-467)")
        if any(p not in (0, 1) for p in self.phase):
            raise ValueError("phase: 0 water, 1 oil")
        if any(p == 1 for p in self.phase) and any("pvtg" in r for r in getattr(case.get("fluid"), "pvt", [])):
            raise ValueError("oil tracers on a fluid with PVTG (ecltracermodel.hh:455-457)")
        self.c = np.array(concentration, float).reshape(len(self.phase), self.Nb)
        if not np.isfinite(self.c).all():
            raise ValueError("a concentration is not finite")
        self.tolerance, self.maxit, self.dot = float(tolerance), int(maxit), dot
        self.c_initial = self.c.copy()
        self.storage1 = None
        self.iq = None
        self.conn = (np.zeros(0, np.int64), np.zeros((0, 3)), np.zeros((len(self.phase), 0)))
        self.rowptr, self.col = np.asarray(case["rowptr"]), np.asarray(case["col"])
        self._tr = _transpose_entries(self.Nb, self.rowptr, self.col)
        self.last_results = None
        self.last_dx = None

    def members(self, phase):
        return [t for t, p in enumerate(self.phase) if p == phase]

    def set_records(self, iq):
        self.iq = np.asarray(iq)[:self.Nb]

    def set_connections(self, cells, rates, injected):
        """cells [n]; rates [n, 3]: component surface rates of water, oil, gas, positive into the reservoir; injected [num_tracers, n]"""
        cells = np.asarray(cells, np.int64).reshape(-1)
        self.conn = (cells, np.asarray(rates, float).reshape(len(cells), 3), np.asarray(injected, float).reshape(len(self.phase), len(cells)))

    def begin_time_step(self, iq=None):
        """updateStorageCache (:340-359)"""
        if iq is not None:
            self.set_records(iq)
        self.c_initial = self.c.copy()
        self.storage1 = np.zeros_like(self.c)
        for ph in (0, 1):
            m = self.members(ph)
            if m:
                self.storage1[m] = phase_volume(self.iq, ph)[None, :] * self.c_initial[m]

    def system(self, phase, dt):
        """assembleTracerEquations_ (:216-337) for one phase -> (M [nnzb] in the case's pattern order, residual [tracers of the phase, Nb])"""
        m = self.members(phase)
        Nb, rowptr, col = self.Nb, self.rowptr, self.col
        vol = phase_volume(self.iq, phase)
        V = np.asarray(self.case["volume"], float)
        c = self.c[m]
        res = (vol[None, :] * c - self.storage1[m]) * V[None, :] / dt
        M = np.zeros(len(col))
        diag = vol * V / dt
        f, up = face_values(self.case, self.iq, phase)
        dk = np.zeros(Nb, np.int64)
        for i in range(Nb):
            for k in range(rowptr[i], rowptr[i + 1]):       # faces in ascending natural column index
                j = int(col[k])
                if j == i:
                    dk[i] = k
                    continue
                u = i if up[k] else j
                res[:, i] = res[:, i] + f[k] * c[:, u]
                if up[k]:
                    diag[i] = diag[i] + f[k]
                    M[self._tr[k]] = -f[k]                   # (*tracerMatrix_)[J][I] = -flux.derivative(0) (:286)
        cells, rates, inj = self.conn
        for n in range(len(cells)):                          # wells, in list order (:293-336)
            i, q = int(cells[n]), rates[n, phase]
            if q > 0.0:
                res[:, i] = res[:, i] - q * inj[m, n]
            elif q < 0.0:
                res[:, i] = res[:, i] - q * c[:, i]
                diag[i] = diag[i] - q
        M[dk] = diag
        return M, res

    def end_time_step(self, dt, order=None):
        """advanceTracerFields (:362-383): per phase assemble, solve every tracer from x = 0 in the ordering `order` = (toOrder, fromOrder)
        of opmhip_get_ordering (None: natural), c -= dx.  -> per tracer dict(converged, iterations, reduction, history)"""
        out = [None] * len(self.phase)
        self.last_dx = np.zeros_like(self.c)
        fr = np.arange(self.Nb) if order is None else np.asarray(order[1])
        to = np.arange(self.Nb) if order is None else np.asarray(order[0])
        for ph in (0, 1):
            m = self.members(ph)
            if not m:
                continue
            M, res = self.system(ph, dt)
            rp, ci, va, dg = permute_csr(self.Nb, self.rowptr, self.col, M, order)
            factors = ilu0(rp, ci, va, dg)
            for j, t in enumerate(m):
                x, info = bicgstab(rp, ci, va, dg, res[j][fr], self.tolerance, self.maxit, self.dot, factors)
                self.last_dx[t] = x[to]
                out[t] = info
        self.c = self.c - self.last_dx
        self.last_results = out
        return out

    # the hooks of newton.BlackoilModelHip
    def on_begin_time_step(self, model):
        self.begin_time_step(model.iq())

    def on_end_time_step(self, model, dt, connections=None):
        self.set_records(model.iq())
        if connections is not None:
            self.set_connections(*self.connection_arrays(connections))
        return self.end_time_step(dt, order=model.ordering()[:2])

    def connection_arrays(self, connections):
        """(cells, rates) of connection_rates() with this model's injected concentrations (set_injected)"""
        cells, rates = connections
        inj = getattr(self, "injected", None)
        if inj is None:
            inj = np.zeros((len(self.phase), len(cells)))
        return cells, rates, inj

    def set_injected(self, injected):
        """WTRACER: injected[t, i], the concentration of tracer t in what connection i of the well model's list injects"""
        self.injected = np.asarray(injected, float)


class DeviceTracers:
    """The tracer model on the device: model is a capi.HipModel whose static data is set"""
    on_device = True

    def __init__(self, model, phase, concentration, tolerance=None, maxit=None):
        self.m = model
        self.phase = [int(p) for p in phase]
        model.set_tracers(self.phase, concentration)
        if tolerance is not None or maxit is not None:
            model.set_tracer_solver(1e-2 if tolerance is None else tolerance, 100 if maxit is None else maxit)
        self.injected = None
        self.last_results = None

    def members(self, phase):
        return [t for t, p in enumerate(self.phase) if p == phase]

    def set_connections(self, cells, rates, injected):
        self.m.set_tracer_connections(cells, rates, injected)

    def set_injected(self, injected):
        self.injected = np.asarray(injected, float)

    def begin_time_step(self):
        self.m.tracers_begin_time_step()

    def system(self, phase, dt):
        return self.m.tracer_system(phase, dt, len(self.members(phase)))

    def end_time_step(self, dt):
        self.last_results = self.m.tracers_end_time_step(dt)
        return self.last_results

    @property
    def c(self):
        return self.m.get_tracers()

    def on_begin_time_step(self, model):
        self.begin_time_step()

    def on_end_time_step(self, model, dt, connections=None):
        if connections is not None:
            cells, rates = connections
            inj = self.injected if self.injected is not None else np.zeros((len(self.phase), len(cells)))
            self.set_connections(cells, rates, inj)
        return self.end_time_step(dt)


def connection_rates(well_model):
    """(cells [n], rates [n, 3]) of a well model's perforations: per connection the component surface rates of water, oil and gas, positive
    into the reservoir - what volumetricSurfaceRateForConnection returns (wells/WellInterface_impl.hpp:434-445).  Host StandardWells: its
    last assembled perforation rates; DeviceStandardWells: the rate values of opmhip_get_std_wells_blocks, one read-back per time step."""
    if getattr(well_model, "on_device", False):
        comp = well_model.m.std_wells_blocks()["rates"][:, :, 0]
    else:
        comp = getattr(well_model, "last_perf_rates", None)
        if comp is None:
            raise ValueError("connection_rates: the well model has not assembled yet")
    comp = np.asarray(comp, float)
    return np.asarray(well_model.cells, np.int64), np.ascontiguousarray(comp[:, [1, 0, 2]])   # components: oil, water, gas -> phases: water, oil, gas


BUCKET_PR_DAY = 10.0 / (1000.0 * 3600.0 * 24.0)   # "keeps (some) trouble away" (ecltracermodel.hh:432)


def well_tracer_rates(perf_pointers, producer, cells, rates, injected, concentration, official_rate):
    """wellTracerRate_ per well (ecltracermodel.hh:298-327, 385-438) for the tracers of one phase.  perf_pointers: the wells' connection
    ranges; producer: per well; rates [n]: the phase's connection rates; injected [tracers, n]; concentration [tracers, Nb]: get_tracers()
    after the step; official_rate [wells]: the well's official rate of the phase (wellState().wellRates).  Injection rates come from the
    injected concentrations (every well, :322-327), a producer's from its cells' concentrations at the producing connections, scaled by
    official / producing where the well crossflows (0 below a bucket per day).  -> [wells, tracers]"""
    conc, inj, rates = np.asarray(concentration, float), np.asarray(injected, float), np.asarray(rates, float)
    nw, nt = len(perf_pointers) - 1, conc.shape[0]
    out = np.zeros((nw, nt))
    for w in range(nw):
        ks = range(int(perf_pointers[w]), int(perf_pointers[w + 1]))
        for k in ks:
            if rates[k] > 0:
                out[w] = out[w] + rates[k] * inj[:, k]
        if not producer[w]:
            continue
        neg = pos = 0.0
        for k in ks:
            if rates[k] < 0:
                neg += rates[k]
                out[w] = out[w] + rates[k] * conc[:, int(cells[k])]
            else:
                pos += rates[k]
        total = float(official_rate[w])
        if total > neg:   # cross flow
            out[w] = out[w] * (total / neg if total < -BUCKET_PR_DAY else 0.0)
    return out


def from_tvdpf(depths, values, cell_depth):
    """TVDPF: the initial concentration against depth, linear between the table's nodes and constant beyond its ends (UNVERIFIED: the
    table class is opm-common's, not in the reference tree)"""
    d, v = np.asarray(depths, float), np.asarray(values, float)
    if len(d) != len(v) or len(d) < 1 or np.any(np.diff(d) <= 0.0):
        raise ValueError("from_tvdpf: depths must rise strictly and match values")
    return np.interp(np.asarray(cell_depth, float), d, v)
