"""Analytic aquifers (Carter-Tracy, Fetkovich): the connection set-up, the record builders, and the model itself in NumPy.

Restated from the reference tree, statement by statement:
  AquiferInterface      opm/simulators/aquifers/AquiferInterface.hpp     (initializeConnections :224-317, beginTimeStep :109-128,
                        addToSource :130-153, calculateReservoirEquilibrium :330-373)
  AquiferCarterTracy    opm/simulators/aquifers/AquiferCarterTracy.hpp   (calculateEqnConstants / calculateInflowRate :135-169, endTimeStep :62-70)
  AquiferFetkovich      opm/simulators/aquifers/AquiferFetkovich.hpp     (dpai / calculateInflowRate :112-148, endTimeStep :64-70, aquiferPressure :122-133)
  BlackoilAquiferModel  opm/simulators/aquifers/BlackoilAquiferModel_impl.hpp (Carter-Tracy before Fetkovich, :112-127)
What lives in opm-common and is NOT in that tree: the deck-level formulas for the time constant and the influx constant (AQUCT_data /
AQUFETP_data), the AQUTAB default influence table, Aquancon's influx coefficients and linearInterpolation.  The builders therefore take Tc and
beta directly; anything restated from memory is tagged UNVERIFIED.

The device form of the same model is capi.HipModel.set_aquifers (opmhip_set_aquifers); HostAquifers is its CPU form and the comparator of
the tests: the same statement order as the kernels, so that the two agree to the bit.
"""
import math

import numpy as np

GRAVITY = 9.80665   # the assembly's constant (csrc/assemble.hip)
FACES = {"I-": 0, "I+": 1, "J-": 2, "J+": 3, "K-": 4, "K+": 5}   # the face tags of transmissibility.py (XM .. ZP) under the names AQUANCON uses
F_PW, F_RHOW = 3, 12   # fields of the intensive-quantity record: water pressure, water density (include/opmhip.h, opmhip_get_iq)


def connections(grid, box, face, influx_coeff=None):
    """AquiferInterface::initializeConnections on the package's grids.  grid: a decks.cartesian_case dict (nx, ny, nz, dx, dy, dz: every cell
    active) or (g, dims) with g = transmissibility.cartesian_faces / cornerpoint_faces(...) and dims = (nx, ny, nz).  box = (i1, i2, j1, j2, k1, k2),
    zero-based and inclusive as indices (AQUANCON's box); face: "I-" .. "K+".  A cell of the box is connected when it is active; its
    faceArea_connected_ is its influx coefficient where the named face of the cell is a grid boundary - no active cell across it - and 0
    otherwise (:264-305).  influx_coeff: one value or one per connected cell (box order); None: the face's area on a cartesian_case, 1 on other
    grids (Aquancon computes it in opm-common; UNVERIFIED: area times the influx multiplier).  alpha = area / sum, all 0 where the sum is below
    sqrt(eps) (:310-316).  -> dict(cells (compressed natural ids, ascending), alpha, area)"""
    f = FACES[face]
    if isinstance(grid, dict):
        nx, ny, nz = grid["nx"], grid["ny"], grid["nz"]
        cart = np.arange(nx * ny * nz)
        faces = None
        face_area = [grid["dy"] * grid["dz"], grid["dx"] * grid["dz"], grid["dx"] * grid["dy"]][f // 2]
    else:
        g, (nx, ny, nz) = grid
        cart, faces, face_area = np.asarray(g["cart"]), g["faces"], 1.0
    i1, i2, j1, j2, k1, k2 = box
    ci, cj, ck = cart % nx, (cart // nx) % ny, cart // (nx * ny)
    inbox = (ci >= i1) & (ci <= i2) & (cj >= j1) & (cj <= j2) & (ck >= k1) & (ck <= k2)
    cells = np.nonzero(inbox)[0]
    if faces is None:
        lim = [0, nx - 1, 0, ny - 1, 0, nz - 1][f]
        boundary = [ci, ci, cj, cj, ck, ck][f][cells] == lim
    else:   # a face is a grid boundary when no connection of the cell leaves through it
        used = np.zeros(len(cart), bool)
        used[np.asarray(faces["cell1"])[np.asarray(faces["face1"]) == f]] = True
        used[np.asarray(faces["cell2"])[np.asarray(faces["face2"]) == f]] = True
        boundary = ~used[cells]
    coeff = np.broadcast_to(np.asarray(face_area if influx_coeff is None else influx_coeff, float), (len(cells),))
    area = np.where(boundary, coeff, 0.0)
    denom = 0.0
    for a in area:              # the element loop's running sum (:305)
        denom += a
    alpha = np.zeros(len(cells)) if denom < np.sqrt(np.finfo(float).eps) else area / denom
    return dict(cells=cells.astype(np.int32), alpha=alpha, area=area)


def carter_tracy(aquifer_id, conn, time_constant, influx_constant, water_density, datum_depth, td, pd, initial_pressure=None):
    """record of one Carter-Tracy aquifer (what the in-tree code reads from AQUCT_data): Tc [s] and beta [m^3/Pa] directly, the influence table
    (ascending td, at least two nodes); initial_pressure None = equilibrate with the reservoir.  conn: connections(...)"""
    return dict(type="carter_tracy", id=int(aquifer_id), cells=np.asarray(conn["cells"], np.int32), alpha=np.asarray(conn["alpha"], float),
                time_constant=float(time_constant), influx_constant=float(influx_constant), water_density=float(water_density),
                datum_depth=float(datum_depth), td=np.asarray(td, float), pd=np.asarray(pd, float), initial_pressure=initial_pressure, restart=None)


def fetkovich(aquifer_id, conn, time_constant, prod_index, total_compr, initial_watvolume, water_density, datum_depth, initial_pressure=None,
              restart=None):
    """record of one Fetkovich aquifer (what the in-tree code reads from AQUFETP_data): Tc [s], productivity index [m^3/s/Pa], total
    compressibility [1/Pa], initial water volume [m^3]; restart: None or dict(W_flux, pressure)"""
    return dict(type="fetkovich", id=int(aquifer_id), cells=np.asarray(conn["cells"], np.int32), alpha=np.asarray(conn["alpha"], float),
                time_constant=float(time_constant), prod_index=float(prod_index), total_compr=float(total_compr),
                initial_watvolume=float(initial_watvolume), water_density=float(water_density), datum_depth=float(datum_depth),
                initial_pressure=initial_pressure, restart=restart)


def fetkovich_time_constant(total_compr, initial_watvolume, prod_index):
    """AQUFETP_data::timeConstant as opm-common has it (not in the reference tree; UNVERIFIED): C_t V_0 / J"""
    return total_compr * initial_watvolume / prod_index


def _interval(x, xv):
    """opm-common's tableIndex (UNVERIFIED): the interval j with x[j] <= xv; the first / last one outside the table"""
    return int(min(max(np.searchsorted(x, xv, side="right") - 1, 0), len(x) - 2))


def table_value(x, y, xv):
    """linearInterpolation with linear extrapolation (opm-common, UNVERIFIED)"""
    j = _interval(x, xv)
    return (y[j + 1] - y[j]) / (x[j + 1] - x[j]) * (xv - x[j]) + y[j]


def table_slope(x, y, xv):
    """linearInterpolationDerivative (opm-common, UNVERIFIED)"""
    j = _interval(x, xv)
    return (y[j + 1] - y[j]) / (x[j + 1] - x[j])


class DeviceAquifers:
    """The aquifers on the device (opmhip_set_aquifers) behind the hooks newton.BlackoilModelHip calls: every assemble picks the influx up
    without the host; opmhip_end_time_step advances the state."""
    on_device = True

    def __init__(self, records):
        self.records = list(records)

    def initial_solution_applied(self, model):
        model.set_aquifers(self.records)

    def begin_time_step(self, model, time, dt):
        model.aquifers_begin_time_step(time, dt)

    def data(self, model):
        return model.get_aquifers()


class HostAquifers:
    """The same model in NumPy, driven through a model object's iq_cells / set_source_cells (capi.HipModel) or iq / set_source (whole
    arrays: the oracle's model wrapper).  depth: per cell, natural order.  base_source / base_dsource: the caller's own source terms
    (Nb x 3 / Nb x 9, whole arrays), to which the influx is added; or base_cells = (cells, source [n x 3]): the same per cell, so that
    only the cells named cross to the device (opmhip_set_source_cells)."""
    on_device = False

    def __init__(self, records, depth, base_source=None, base_dsource=None, base_cells=None):
        self.a = [dict(r) for r in records]
        kinds = [r["type"] for r in self.a]
        if any(k not in ("carter_tracy", "fetkovich") for k in kinds) or kinds != sorted(kinds):
            raise ValueError("aquifers: Carter-Tracy first, then Fetkovich")
        self.depth = np.asarray(depth, float)
        self.base = None if base_source is None else np.array(base_source, float).reshape(-1, 3)
        self.dbase = None if base_dsource is None else np.array(base_dsource, float).reshape(-1, 9)
        self.base_cells = None if base_cells is None else (np.asarray(base_cells[0], np.int64), np.asarray(base_cells[1], float).reshape(-1, 3))
        for r in self.a:
            r["cells"] = np.asarray(r["cells"], np.int64)
            r["alpha"] = np.asarray(r["alpha"], float)
            if len(np.unique(r["cells"])) != len(r["cells"]):
                raise ValueError("aquifer %d: a cell is repeated" % r["id"])
            n = len(r["cells"])
            r["gdz"] = GRAVITY * (self.depth[r["cells"]] - r["datum_depth"])
            r["p_prev"], r["Q"] = np.zeros(n), np.zeros((n, 4))
            if r["type"] == "carter_tracy":
                r["_x"], r["_y"] = np.asarray(r["td"], float), np.asarray(r["pd"], float)
                if len(r["_x"]) < 2 or len(r["_x"]) != len(r["_y"]) or np.any(np.diff(r["_x"]) <= 0.0):
                    raise ValueError("aquifer %d: the influence table needs two or more ascending nodes" % r["id"])
        self.cells = np.concatenate([r["cells"] for r in self.a]) if self.a else np.zeros(0, np.int64)
        self.dt = None

    def _records(self, model, cells):
        if hasattr(model, "iq_cells"):
            return model.iq_cells(cells) if len(cells) else np.zeros((0, 17, 4))
        return model.iq()[cells]

    # -- initialSolutionApplied -> initQuantities (AquiferInterface.hpp:167-183) ---------------------------------------------------------
    def initial_solution_applied(self, model):
        for r in self.a:
            rs = r.get("restart")
            if rs is not None and r["type"] == "carter_tracy":
                raise ValueError("Restart-based initialization not currently supported for Carter-Tracey analytic aquifers")
            r["W_flux"] = float(rs["W_flux"]) if rs is not None else 0.0
            if r.get("initial_pressure") is None:      # calculateReservoirEquilibrium: the element loop visits the cells in ascending order
                order = np.argsort(r["cells"], kind="stable")
                rec = self._records(model, r["cells"][order])
                sum_alpha = 0.0
                for a in r["alpha"]:
                    sum_alpha += a
                sum_pw = 0.0
                for k, i in enumerate(order):
                    sum_pw += r["alpha"][i] * (rec[k, F_PW, 0] - rec[k, F_RHOW, 0] * r["gdz"][i])
                r["pa0"] = sum_pw / sum_alpha
            else:
                r["pa0"] = float(r["initial_pressure"])
            r["flux_value"] = 0.0                                                        # Carter-Tracy: fluxValue_
            r["pressure"] = float(rs["pressure"]) if rs is not None else r["pa0"]        # Fetkovich: aquifer_pressure_

    # -- beginTimeStep (:109-128) and the per-step scalars ---------------------------------------------------------------------------------
    def begin_time_step(self, model, time, dt):
        rec = self._records(model, self.cells)
        o = 0
        for r in self.a:
            n = len(r["cells"])
            r["p_prev"] = rec[o:o + n, F_PW, 0].copy()
            o += n
            if r["type"] == "fetkovich":      # AquiferFetkovich.hpp:143-144
                td_Tc = dt / r["time_constant"]
                r["coef"] = (1 - math.exp(-td_Tc)) / td_Tc   # libm's exp, as std::exp on the host side of the device form
        self.dt = dt
        self._time = time

    def rates(self, rec):
        """Qai_ of every connection from the connected cells' records (rows in connection order) -> (connections, 4), also kept per aquifer"""
        out = np.zeros((len(self.cells), 4))
        o = 0
        for r in self.a:
            n = len(r["cells"])
            pw = rec[o:o + n, F_PW, :]
            if r["type"] == "carter_tracy":      # AquiferCarterTracy.hpp:135-169
                Tc, beta = r["time_constant"], r["influx_constant"]
                x, y = r["_x"], r["_y"]
                td_plus_dt = (self.dt + self._time) / Tc
                td = self._time / Tc
                PItd, PItdprime = table_value(x, y, td_plus_dt), table_slope(x, y, td_plus_dt)
                dpai = r["pa0"] + r["water_density"] * r["gdz"] - r["p_prev"]
                denom = Tc * (PItd - td * PItdprime)
                a = (beta * dpai - r["flux_value"] * PItdprime) / denom
                b = beta / denom
                q = np.empty((n, 4))
                q[:, 0] = r["alpha"] * (a - b * (pw[:, 0] - r["p_prev"]))
                q[:, 1:] = r["alpha"][:, None] * (-(b * pw[:, 1:]))
            else:                                 # AquiferFetkovich.hpp:112-148
                c = r["coef"] * r["alpha"] * r["prod_index"]
                q = np.empty((n, 4))
                q[:, 0] = c * ((r["pressure"] + r["water_density"] * r["gdz"]) - pw[:, 0])
                q[:, 1:] = c[:, None] * (-pw[:, 1:])
            r["Q"] = q
            out[o:o + n] = q
            o += n
        return out

    # -- addToSource (:130-153) for every connected cell, Carter-Tracy first ---------------------------------------------------------------
    def add_to_source(self, model, cells=None, source=None, dsource=None):
        """forms Qai_ at the model's present state and hands the model its source terms: the caller's (cells / source / dsource as
        set_source_cells takes them, e.g. a well model's; else base_source of the constructor) plus the influx in the water equation"""
        q = self.rates(self._records(model, self.cells))
        if cells is None and self.base_cells is not None:
            cells, source = self.base_cells
        whole = cells is None and (self.base is not None or not hasattr(model, "set_source_cells"))
        if whole:
            Nb = len(self.depth)
            s = np.zeros((Nb, 3)) if self.base is None else self.base.copy()
            d = np.zeros((Nb, 9)) if self.dbase is None else self.dbase.copy()
            for r in self.a:       # a cell is named at most once per aquifer: the sum runs in aquifer order
                s[r["cells"], 1] += r["Q"][:, 0]
                d[r["cells"], 3:6] += r["Q"][:, 1:]
            model.set_source(s.reshape(-1), d.reshape(-1))
            return
        n = len(self.cells)
        s, d = np.zeros((n, 3)), np.zeros((n, 9))
        s[:, 1], d[:, 3:6] = q[:, 0], q[:, 1:]
        cl = self.cells
        if cells is not None:      # the caller's rates first: a cell named twice receives the sum in the order of mention
            m = len(cells)
            d0 = np.zeros((m, 9)) if dsource is None else np.asarray(dsource, float).reshape(m, 9)
            cl, s, d = np.concatenate([np.asarray(cells, np.int64), cl]), np.vstack([np.asarray(source, float).reshape(m, 3), s]), np.vstack([d0, d])
        model.set_source_cells(cl, s.reshape(-1), d.reshape(-1))

    # -- endTimeStep of both classes ---------------------------------------------------------------------------------------------------------
    def end_time_step(self, dt):
        for r in self.a:
            for qv in r["Q"][:, 0]:
                r["W_flux"] += qv * dt
            if r["type"] == "carter_tracy":
                r["flux_value"] = r["W_flux"]
            else:
                r["pressure"] = r["pa0"] - (r["W_flux"] / (r["total_compr"] * r["initial_watvolume"]))

    def data(self, model=None):
        """what capi.HipModel.get_aquifers reports"""
        flux_rate = []
        for r in self.a:
            f = 0.0
            for qv in r["Q"][:, 0]:
                f += qv
            flux_rate.append(f)
        return dict(W_flux=np.array([r["W_flux"] for r in self.a]), flux_rate=np.array(flux_rate),
                    pressure=np.array([r["pa0"] if r["type"] == "carter_tracy" else r["pressure"] for r in self.a]),
                    init_pressure=np.array([r["pa0"] for r in self.a]))
