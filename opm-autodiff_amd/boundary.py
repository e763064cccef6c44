"""Open boundaries (the BC keyword: FREE and RATE faces): the face set-up, the record builders, and the boundary term itself in NumPy.

Restated from the reference tree, statement by statement:
  EclProblem::boundary              ebos/eclproblem.hh:1602-1671 (the lists: readBoundaryConditions_ :2686-2830)
  calculateBoundaryGradients_       ebos/eclfluxmodule.hh:362-468
  transmissibilityBoundary          ebos/ecltransmissibility.cc:241-282 (the interior cell's half transmissibility alone)
What lives in opm-models and is NOT in that tree: BlackOilBoundaryRateVector::setFreeFlow / setMassRate and evalPhaseFluxes_, the step
from phase volume fluxes to the three conservation equations.  Restated from the published form, UNVERIFIED: per phase the raw phase
pressures (no gravity term) of the captured and the interior state choose whose 1/B, Rs and Rv the flux carries, equal pressures add
nothing; a mass rate is divided by the component's reference density (Flow conserves surface volumes).

Sign: a boundary rate is positive OUT of the domain (the rate vector is added to the residual; boundary() passes the deck's RATE on
unchanged), so it is subtracted from the source terms, which are rates into the cell.

The device form is capi.HipModel.set_boundary_conditions (opmhip_set_boundary_conditions); HostBoundary is its CPU form and the
comparator of the tests: the same statement order as the kernels (csrc/boundary.hip), so that the two agree to the bit.
"""
import numpy as np

from . import transmissibility as _T

GRAVITY = 9.80665   # the assembly's constant (csrc/internal.hpp)
FACES = {"I-": 0, "I+": 1, "J-": 2, "J+": 3, "K-": 4, "K+": 5, "X-": 0, "X+": 1, "Y-": 2, "Y+": 3, "Z-": 4, "Z+": 5}   # indexInInside
F_P, F_B, F_MOB, F_RHO, F_RS, F_RV, F_TMULT = 3, 6, 9, 12, 15, 16, 17   # fields of the intensive-quantity record (F_RV, F_TMULT: extended record)
WATER, OIL, GAS = 0, 1, 2
EQ_OIL, EQ_WATER, EQ_GAS = 0, 1, 2
COMP = (EQ_WATER, EQ_OIL, EQ_GAS)   # the equation of each phase's own component


def faces(grid, box, face, perm=None, corners=None):
    """The boundary faces of a box: the cells of box = (i1, i2, j1, j2, k1, k2) (zero-based, inclusive) whose face `face` ("I-" .. "K+" or
    "X-" .. "Z+") is a grid boundary - no active cell across it -, each with its area, the depth of the face centre and the boundary half
    transmissibility (transmissibility.half_transmissibility with the cell's own permeability along the face's axis; no NTG, no MULT*:
    the reference applies them to interior faces only).
    grid: a decks.cartesian_case dict (nx, ny, nz, dx, dy, dz, depth, perm: every cell active), or (g, dims) with
    g = transmissibility.cornerpoint_faces(...), dims = (nx, ny, nz), corners = transmissibility.cornerpoint_corners(...) and perm (n, 3)
    per active cell; there a face counts as a grid boundary when no connection of the cell leaves through it.
    -> dict(cells (compressed natural ids, ascending), direction, area, trans, depth)"""
    f = FACES[face]
    axis, plus = f // 2, f % 2
    if isinstance(grid, dict):
        nx, ny, nz = grid["nx"], grid["ny"], grid["nz"]
        cart = np.arange(nx * ny * nz)
    else:
        g, (nx, ny, nz) = grid
        cart = np.asarray(g["cart"])
    i1, i2, j1, j2, k1, k2 = box
    ci, cj, ck = cart % nx, (cart // nx) % ny, cart // (nx * ny)
    inbox = (ci >= i1) & (ci <= i2) & (cj >= j1) & (cj <= j2) & (ck >= k1) & (ck <= k2)
    cells = np.nonzero(inbox)[0]
    if isinstance(grid, dict):
        lim = [0, nx - 1, 0, ny - 1, 0, nz - 1][f]
        cells = cells[[ci, ci, cj, cj, ck, ck][f][cells] == lim]
        n = len(cells)
        size = [grid["dx"], grid["dy"], grid["dz"]]
        a = 1.0
        for o in range(3):
            if o != axis:
                a = a * size[o]
        area = np.full(n, float(a))
        sign = 1.0 if plus else -1.0
        nrm, dist = np.zeros((n, 3)), np.zeros((n, 3))
        nrm[:, axis] = sign * area
        dist[:, axis] = sign * 0.5 * size[axis]
        depth = np.asarray(grid["depth"], float)[cells] + dist[:, 2]
        k = np.asarray(grid["perm"] if perm is None else perm, float)
        kdd = k[cells] if k.ndim == 1 else k[cells, axis]
    else:
        if corners is None or perm is None:
            raise ValueError("boundary.faces on a corner-point grid needs corners = cornerpoint_corners(...) and perm (n, 3)")
        fc = g["faces"]
        used = np.zeros(len(cart), bool)
        used[np.asarray(fc["cell1"])[np.asarray(fc["face1"]) == f]] = True
        used[np.asarray(fc["cell2"])[np.asarray(fc["face2"]) == f]] = True
        cells = cells[~used[cells]]
        c = np.asarray(corners, float)[cart[cells]]          # [cell, kk, jj, ii, xyz]
        quad = {0: (c[:, 0, 0, 0], c[:, 1, 0, 0], c[:, 1, 1, 0], c[:, 0, 1, 0]), 1: (c[:, 0, 0, 1], c[:, 0, 1, 1], c[:, 1, 1, 1], c[:, 1, 0, 1]),
                2: (c[:, 0, 0, 0], c[:, 0, 0, 1], c[:, 1, 0, 1], c[:, 1, 0, 0]), 3: (c[:, 0, 1, 0], c[:, 1, 1, 0], c[:, 1, 1, 1], c[:, 0, 1, 1]),
                4: (c[:, 0, 0, 0], c[:, 0, 1, 0], c[:, 0, 1, 1], c[:, 0, 0, 1]), 5: (c[:, 1, 0, 0], c[:, 1, 0, 1], c[:, 1, 1, 1], c[:, 1, 1, 0])}[f]
        nrm = _T._quad_area_vector(*quad)
        area = np.sqrt((nrm ** 2).sum(axis=1))
        centre = (quad[0] + quad[1] + quad[2] + quad[3]) / 4.0
        dist = centre - np.asarray(g["centroid"], float)[cells]
        depth = centre[:, 2]
        kdd = np.asarray(perm, float)[cells, axis]
    trans = _T.half_transmissibility(kdd, nrm, dist) if len(cells) else np.zeros(0)
    return dict(cells=cells.astype(np.int32), direction=np.full(len(cells), f, np.int32), area=area, trans=trans, depth=depth)


def _group(kind, fc):
    return dict(type=kind, cells=np.asarray(fc["cells"], np.int32), direction=np.asarray(fc["direction"], np.int32), area=np.asarray(fc["area"], float),
                trans=np.asarray(fc["trans"], float), depth=np.asarray(fc["depth"], float))


def free(fc):
    """record of FREE faces (BC ... FREE): the exterior state is the cells' own state at the moment the list is set.  fc: faces(...)"""
    return _group("free", fc)


def rate(fc, mass_rate):
    """record of RATE faces (BC ... RATE): mass_rate [kg / (m^2 s)] per equation (oil, water, gas), one triple for all faces or one per
    face, positive out of the domain - an influx is negative.  fc: faces(...)"""
    r = _group("rate", fc)
    r["rate"] = np.ascontiguousarray(np.broadcast_to(np.asarray(mass_rate, float).reshape(-1, 3), (len(r["cells"]), 3)))
    return r


class DeviceBoundary:
    """The list on the device (opmhip_set_boundary_conditions) behind the hooks newton.BlackoilModelHip calls: every assemble picks the
    faces' rates up without the host."""
    on_device = True

    def __init__(self, records):
        self.records = list(records)

    def initial_solution_applied(self, model):
        model.set_boundary_conditions(self.records)

    def rates(self, model):
        return model.boundary_rates()


# value + three derivatives in columns 0 .. 3: the expression trees of csrc/fluid_device.hpp's Ad
def _mul(a, b):
    out = np.empty_like(a)
    out[:, 0] = a[:, 0] * b[:, 0]
    out[:, 1:] = a[:, 1:] * b[:, :1] + b[:, 1:] * a[:, :1]
    return out


def _scale(a, s):
    return a * np.asarray(s, float).reshape(-1, 1)


class HostBoundary:
    """The same term in NumPy, driven through a model object's iq_cells / set_source_cells (capi.HipModel) or iq / set_source (whole
    arrays: the oracle's model wrapper).  depth: per cell, natural order; fluid: the case's fluid.Fluid (reference densities); pvtnum:
    per cell or None; wet_gas: the fluid has PVTG (default: read from the fluid).  base_source / base_dsource: the caller's own source
    terms (Nb x 3 / Nb x 9, whole arrays) from which the faces' rates are subtracted; or base_cells = (cells, source [n x 3]): the same
    per cell, so that only the cells named cross to the device (opmhip_set_source_cells)."""
    on_device = False

    def __init__(self, records, depth, fluid, pvtnum=None, wet_gas=None, base_source=None, base_dsource=None, base_cells=None):
        recs = list(records)
        cat = lambda k, dt: np.concatenate([np.asarray(r[k], dt).reshape(-1) for r in recs]) if recs else np.zeros(0, dt)
        self.cells = cat("cells", np.int64)
        self.direction = cat("direction", np.int64)
        self.area, self.trans, self.zface = cat("area", float), cat("trans", float), cat("depth", float)
        self.free = np.concatenate([np.full(len(r["cells"]), r["type"] == "free") for r in recs]) if recs else np.zeros(0, bool)
        if any(r["type"] not in ("free", "rate") for r in recs):
            raise ValueError("boundary: a record is \"free\" or \"rate\"")
        self.mass_rate = np.concatenate([np.asarray(r["rate"], float).reshape(-1, 3) if r["type"] == "rate" else np.zeros((len(r["cells"]), 3))
                                         for r in recs]) if recs else np.zeros((0, 3))
        if len(set(zip(self.cells.tolist(), self.direction.tolist()))) != len(self.cells):
            raise ValueError("boundary: a (cell, direction) pair is listed twice")
        self.depth = np.asarray(depth, float)
        pvt = fluid.pvt
        region = np.zeros(len(self.cells), np.int64) if pvtnum is None else np.asarray(pvtnum, np.int64)[self.cells]
        self.rho_ref = np.array([pvt[r]["density"] for r in region], float).reshape(-1, 3)      # oil, water, gas: the equations' order
        self.wet = bool(any("pvtg" in p for p in pvt)) if wet_gas is None else bool(wet_gas)
        self.base = None if base_source is None else np.array(base_source, float).reshape(-1, 3)
        self.dbase = None if base_dsource is None else np.array(base_dsource, float).reshape(-1, 9)
        self.base_cells = None if base_cells is None else (np.asarray(base_cells[0], np.int64), np.asarray(base_cells[1], float).reshape(-1, 3))
        self.ext = None
        self.Q = np.zeros((len(self.cells), 12))

    def _records(self, model, cells):
        if hasattr(model, "iq_cells"):      # a cell with several faces is gathered once
            if not len(cells):
                return np.zeros((0, 17, 4))
            distinct, of = np.unique(cells, return_inverse=True)
            return model.iq_cells(distinct)[of]
        return model.iq()[cells]

    # -- initialFluidStates_[globalDofIdx] of every face's cell: values only ---------------------------------------------------------------
    def capture(self, rec):
        """rec: the records of the faces' cells, rows in face order"""
        ext_rec = rec.shape[1] > 17
        self.ext = dict(p=rec[:, F_P:F_P + 3, 0].copy(), rho=rec[:, F_RHO:F_RHO + 3, 0].copy(), mob=rec[:, F_MOB:F_MOB + 3, 0].copy(),
                        b=rec[:, F_B:F_B + 3, 0].copy(), rs=rec[:, F_RS, 0].copy(), rv=rec[:, F_RV, 0].copy() if ext_rec else np.zeros(len(rec)))

    def initial_solution_applied(self, model):
        self.capture(self._records(model, self.cells))

    # -- boundary() on every face --------------------------------------------------------------------------------------------------------
    def rates(self, rec):
        """every face's contribution to its cell's residual from the cells' records (rows in face order) -> (faces, 12): the three
        equations, then their 3 x 3 derivative; also kept in self.Q.  upwind_exterior (faces, 3) records which phases took the exterior
        mobility, composition (faces, 3) whose 1/B, Rs, Rv a phase carried: +1 the captured, -1 the interior's, 0 none"""
        n = len(self.cells)
        ext_rec = rec.shape[1] > 17
        X = self.ext
        r = np.zeros((3, n, 4))
        area, distZ = self.area, self.depth[self.cells] - self.zface
        self.upwind_exterior, self.composition = np.zeros((n, 3), bool), np.zeros((n, 3), int)
        for ph in range(3):
            rhoIn, pIn = rec[:, F_RHO + ph, :], rec[:, F_P + ph, :]
            rhoAvg = rhoIn.copy()
            rhoAvg[:, 0] = rhoIn[:, 0] + X["rho"][:, ph]
            rhoAvg = rhoAvg / 2.0
            pEx = _scale(rhoAvg, distZ * GRAVITY)
            pEx[:, 0] = X["p"][:, ph] + pEx[:, 0]
            pEx[:, 1:] = 0.0 + pEx[:, 1:]
            dp = pEx - pIn
            up_ex = dp[:, 0] > 0.0
            tm = self.trans * rec[:, F_TMULT, 0] if ext_rec else self.trans
            q_ex = _scale(_scale(dp, X["mob"][:, ph]), -self.trans / area)
            q_in = _scale(_mul(dp, rec[:, F_MOB + ph, :]), -tm / area)
            q = np.where(up_ex[:, None], q_ex, q_in)
            pB = X["p"][:, ph]
            out, inn = pB < pIn[:, 0], pB > pIn[:, 0]
            surf_in, surf_ex = _mul(rec[:, F_B + ph, :], q), _scale(q, X["b"][:, ph])
            surf = np.where(out[:, None], surf_in, surf_ex)
            none = ~(out | inn)          # equal raw pressures: the phase adds nothing
            e = COMP[ph]
            r[e] = np.where(none[:, None], r[e], r[e] + surf)
            if ph == OIL:
                dis = np.where(out[:, None], _mul(rec[:, F_RS, :], surf), _scale(surf, X["rs"]))
                r[EQ_GAS] = np.where(none[:, None], r[EQ_GAS], r[EQ_GAS] + dis)
            if ph == GAS and ext_rec and self.wet:
                vap = np.where(out[:, None], _mul(rec[:, F_RV, :], surf), _scale(surf, X["rv"]))
                r[EQ_OIL] = np.where(none[:, None], r[EQ_OIL], r[EQ_OIL] + vap)
            self.upwind_exterior[:, ph] = up_ex
            self.composition[:, ph] = np.where(inn, 1, np.where(out, -1, 0))
        Q = np.zeros((n, 12))
        for e in range(3):
            fr = _scale(r[e], area)
            Q[:, e] = np.where(self.free, fr[:, 0], (self.mass_rate[:, e] / self.rho_ref[:, e]) * area)
            Q[:, 3 + 3 * e:6 + 3 * e] = np.where(self.free[:, None], fr[:, 1:], 0.0)
        self.Q = Q
        return Q

    def rates_now(self, model):
        return self.rates(self._records(model, self.cells))

    # -- the rates out of the source terms -----------------------------------------------------------------------------------------------
    def add_to_source(self, model, cells=None, source=None, dsource=None):
        """forms the faces' rates at the model's present state and hands the model its source terms: the caller's (cells / source / dsource
        as set_source_cells takes them, e.g. a well model's; else base_source of the constructor) minus the rates, face by face in list
        order"""
        Q = self.rates_now(model)
        if cells is None and self.base_cells is not None:
            cells, source = self.base_cells
        whole = cells is None and (self.base is not None or not hasattr(model, "set_source_cells"))
        if whole:
            Nb = len(self.depth)
            s = np.zeros((Nb, 3)) if self.base is None else self.base.copy()
            d = np.zeros((Nb, 9)) if self.dbase is None else self.dbase.copy()
            np.subtract.at(s, self.cells, Q[:, :3])       # a cell with several faces: one after the other, in list order
            np.subtract.at(d, self.cells, Q[:, 3:])
            model.set_source(s.reshape(-1), d.reshape(-1))
            return
        cl, s, d = self.cells, -Q[:, :3], -Q[:, 3:]
        if cells is not None:      # the caller's rates first: a cell named twice receives the sum in the order of mention
            m = len(cells)
            d0 = np.zeros((m, 9)) if dsource is None else np.asarray(dsource, float).reshape(m, 9)
            cl, s, d = np.concatenate([np.asarray(cells, np.int64), cl]), np.vstack([np.asarray(source, float).reshape(m, 3), s]), np.vstack([d0, d])
        model.set_source_cells(cl, s.reshape(-1), d.reshape(-1))
