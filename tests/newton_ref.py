"""Plain numpy statements of the three things that steer the non-linear loop - the chopped Newton update with the
primary-variable switch, the convergence check and the relative change of a time step - written from the reference's
text and from the update rules quoted in SURVEY.md App. B.7, not from the kernels and without ctypes.  They are the
third party between the device and the CPU oracle (whose update() / adapt() is a sibling of the kernel): a mistake the
two share does not get past these.

  update              BlackOilNewtonMethod::update_ + BlackOilPrimaryVariables::adaptPrimaryVariables for the two dry-gas
                      meanings (Sw_po_Sg = 0, Sw_po_Rs = 1), one cell at a time in Python floats (IEEE double, no
                      contraction), with a label of the branches each cell took and its distance from the thresholds
  convergence         localConvergenceData + computeCnvErrorPv + getReservoirConvergence (flow/BlackoilModelEbos.hpp:628-904)
  relative_change     BlackoilModelEbos::relativeChange (flow/BlackoilModelEbos.hpp:431-510)
  census_case / census_dx    the seeded case and the update vectors tests/test_newton_ref.py and the GPU edge tests share
"""
import math

import numpy as np

SW_PO_SG, SW_PO_RS = 0, 1
DP_MAX_REL, DS_MAX, OSC_THRESHOLD = 0.3, 0.2, 1e-5
EQ_OIL, EQ_WATER, EQ_GAS = 0, 1, 2
EQ_OF_PHASE = (EQ_WATER, EQ_OIL, EQ_GAS)          # canonicalToActiveComponentIndex(solventComponentIndex(phase)), phases water, oil, gas

# the adaptPrimaryVariables branch of a cell
BRANCHES = ("water_only_from_sg", "water_only_from_rs", "gas_disappears", "gas_appears", "stays", "stays_band")
# which saturation delta was the largest (the one the 0.2 chop is measured on)
SAT_PHASES = ("water", "oil", "gas")


def _rel(a, b):
    """relative distance of a deciding quantity a from its threshold b (absolute where the threshold is 0)"""
    return abs(a - b) / abs(b) if b != 0.0 else abs(a - b)


def update(pv, meaning, was_switched, dx, relax, rs_sat, rs_max=None):
    """x_new = x - relax * dx with the saturation and pressure chops, then the primary-variable switch.

    pv (Nb, 3) = (Sw, po, Sg | Rs), meaning (Nb,), was_switched (Nb,) flags of the previous update, dx (Nb, 3),
    rs_sat: p -> saturated Rs (decks.rs_sat bound to the case's fluid), rs_max: per-cell cap or None.
    -> (pv_new, meaning_new, flags_new, switch count, labels, margin)
    labels: dict of per-cell arrays - sat_chop (bool), sat_phase (index into SAT_PHASES), p_chop (+1, -1, 0), rs_clamp (bool),
    branch (index into BRANCHES).  margin: per cell, the smallest relative distance between a quantity a comparison of this
    cell read and its threshold (0.2, 0.3 p, x[2], 1.0, -eps, min(RsMax, RsSat (1 + eps))); 0.0 = the two are one double."""
    pv = np.array(pv, np.float64).reshape(-1, 3)
    dx = np.asarray(dx, np.float64).reshape(-1, 3)
    Nb = pv.shape[0]
    out = pv.copy()
    mng = np.array(meaning, np.uint8).copy()
    flags = np.zeros(Nb, np.uint8)
    lab = dict(sat_chop=np.zeros(Nb, bool), sat_phase=np.zeros(Nb, np.int8), p_chop=np.zeros(Nb, np.int8),
               rs_clamp=np.zeros(Nb, bool), branch=np.zeros(Nb, np.int8))
    margin = np.full(Nb, np.inf)
    nswitched = 0
    for c in range(Nb):
        x = [float(v) for v in pv[c]]
        u = [float(v) for v in dx[c]]
        if relax != 1.0:                       # the relaxed update is formed first, then chopped
            u = [v * relax for v in u]
        m = int(mng[c])
        d_sw = u[0]
        d_so, d_sg = -d_sw, 0.0
        if m == SW_PO_SG:
            d_sg = u[2]
            d_so = d_so - d_sg
        mags = (abs(d_sw), abs(d_so), abs(d_sg))
        max_sat = max(mags)
        lab["sat_phase"][c] = int(np.argmax(mags))
        alpha = 1.0
        if max_sat > DS_MAX:
            alpha = DS_MAX / max_sat
            lab["sat_chop"][c] = True
        mg = [_rel(max_sat, DS_MAX)]
        n0 = x[0] - u[0] * alpha
        d = u[1]
        mg.append(_rel(abs(d), DP_MAX_REL * x[1]))
        if abs(d) > DP_MAX_REL * x[1]:
            d = (-1.0 if d < 0.0 else 1.0) * DP_MAX_REL * x[1]
            lab["p_chop"][c] = -1 if d < 0.0 else 1
        n1 = x[1] - d
        d = u[2]
        if m == SW_PO_SG:
            d = d * alpha
        else:
            mg.append(_rel(d, x[2]))
            if d > x[2]:                       # Rs must not become negative
                d = x[2]
                lab["rs_clamp"][c] = True
        n2 = x[2] - d
        eps = OSC_THRESHOLD if was_switched[c] else 0.0
        cap = float(rs_max[c]) if rs_max is not None else np.finfo(np.float64).max / 2.0
        switched = False
        mg.append(_rel(n0, 1.0))
        if n0 >= 1.0:                          # cells with (almost) only water
            lab["branch"][c] = BRANCHES.index("water_only_from_sg" if m == SW_PO_SG else "water_only_from_rs")
            n0, n2 = 1.0, 0.0
            switched = m != SW_PO_SG
            m = SW_PO_SG
        elif m == SW_PO_SG:
            so = 1.0 - n0 - n2
            mg.append(_rel(n2, -eps))
            if n2 < -eps:
                mg.append(abs(so))
            if n2 < -eps and so > 0.0:         # the gas phase disappears
                lab["branch"][c] = BRANCHES.index("gas_disappears")
                m = SW_PO_RS
                n2 = min(cap, float(rs_sat(n1)))
                switched = True
            else:
                lab["branch"][c] = BRANCHES.index("stays_band" if (eps > 0.0 and n2 < 0.0 and so > 0.0) else "stays")
        else:
            sat = float(rs_sat(n1))
            thr = min(cap, sat * (1.0 + eps))
            mg.append(_rel(n2, thr))
            if n2 > thr:                       # the gas phase appears
                lab["branch"][c] = BRANCHES.index("gas_appears")
                m = SW_PO_SG
                n2 = 0.0
                switched = True
            else:
                lab["branch"][c] = BRANCHES.index("stays_band" if (eps > 0.0 and n2 > min(cap, sat)) else "stays")
        out[c] = (n0, n1, n2)
        mng[c] = m
        flags[c] = 1 if switched else 0
        nswitched += int(switched)
        margin[c] = min(mg)
    return out, mng, flags, nswitched, lab, margin


def _fsum(v):
    """math.fsum that states what IEEE addition gives for non-finite terms (fsum itself refuses +inf and -inf together)"""
    v = np.asarray(v, np.float64).ravel()
    if np.all(np.isfinite(v)):
        return math.fsum(v)
    if np.isnan(v).any() or (np.isposinf(v).any() and np.isneginf(v).any()):
        return float("nan")
    return float("inf") if np.isposinf(v).any() else float("-inf")


def _max_dropping_nan(v):
    """std::max(m, v) from lowest(): a NaN operand never replaces m, so NaN entries are passed over"""
    v = np.asarray(v, np.float64).ravel()
    return float(np.max(v[~np.isnan(v)], initial=-np.finfo(np.float64).max))


def convergence(resid, poro, volume, inv_b, dt, tol_cnv, b_avg=None):
    """resid (Nb, 3) in equation order (oil, water, gas), inv_b (Nb, 3) = 1 / B of the phases (water, oil, gas).
    -> (the 17 numbers of opmhip_convergence: R_sum[3] maxCoeff[3] B_avg[3] pvSum cnvErrorPv CNV[3] MB[3], by equation;
        violated mask; per cell | |CNV| / tol - 1 | of the component nearest the tolerance)
    b_avg: decide the violated set with these averages in place of the statement's own (they differ by rounding)."""
    resid = np.asarray(resid, np.float64).reshape(-1, 3)
    inv_b = np.asarray(inv_b, np.float64).reshape(-1, 3)
    Nb = resid.shape[0]
    pvv = np.asarray(poro, np.float64) * np.asarray(volume, np.float64)
    c = np.zeros(17)
    for ph in range(3):
        e = EQ_OF_PHASE[ph]
        c[6 + e] = _fsum(1.0 / inv_b[:, ph]) / float(Nb)
        c[e] = _fsum(resid[:, e])
        c[3 + e] = _max_dropping_nan(np.abs(resid[:, e]) / pvv)
    c[9] = _fsum(pvv)
    B = c[6:9] if b_avg is None else np.asarray(b_avg, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        cnv = resid * dt * B[None, :] / pvv[:, None]
        violated = (np.abs(cnv) > tol_cnv).any(axis=1)           # a NaN compares false, as in the reference
        dist = np.nanmin(np.abs(np.abs(cnv) / tol_cnv - 1.0), axis=1)
        c[10] = _fsum(pvv[violated])
        for e in range(3):
            c[11 + e] = c[6 + e] * dt * c[3 + e]
            c[14 + e] = abs(c[6 + e] * c[e]) * dt / c[9]
    return c, violated, dist


def failure(c17, max_residual_allowed=1e7):
    """what getConvergence's worst severity makes BlackoilModelEbos::nonlinearIteration throw (:313-321): the message or None"""
    res = np.asarray(c17[11:17], np.float64)
    if np.isnan(res).any():
        return "NaN residual found!"
    if (res > max_residual_allowed).any():
        return "Too large residual found!"
    return None


def relative_change(pv, meaning, pv_old, meaning_old):
    """-> (resultDelta, resultDenom, ratio, per-cell delta terms, per-cell denominator terms); per cell the terms are added
    in the reference's order (pressure, then water, oil, gas), the cells by math.fsum"""
    a = np.asarray(pv, np.float64).reshape(-1, 3)
    b = np.asarray(pv_old, np.float64).reshape(-1, 3)

    def sats(x, m):
        sw = x[:, 0]
        sg = np.where(np.asarray(m) == SW_PO_SG, x[:, 2], 0.0)
        return sw, (1.0 - sw) - sg, sg

    sn, so = sats(a, meaning), sats(b, meaning_old)
    tmp = a[:, 1] - b[:, 1]
    d = tmp * tmp
    q = a[:, 1] * a[:, 1]
    for ph in range(3):
        t = sn[ph] - so[ph]
        d = d + t * t
        q = q + sn[ph] * sn[ph]
    delta, denom = math.fsum(d), math.fsum(q)
    return delta, denom, (delta / denom if denom > 0.0 else 0.0), d, q


# ---- the case and the update vectors the CPU and the GPU tests share ----------------------------------------------------------
def census_case(pkg, nx=9, ny=8, nz=7, fluid=None, seed=11, **kw):
    """a "mixed" Cartesian case with the state spread out: Sw in 0.05 - 0.98, Sg up to 1 - Sw, Rs 0.3 - 1.0 of saturated"""
    case = pkg.decks.cartesian_case(nx, ny, nz, state="mixed", fluid=fluid, **kw)
    rng = np.random.default_rng(seed)
    Nb = case["Nb"]
    pv = case["pv"].reshape(-1, 3).copy()
    gas = case["meaning"] == SW_PO_SG
    pv[:, 0] = rng.uniform(0.05, 0.98, Nb)
    pv[:, 2] = np.where(gas, rng.uniform(0.0, 1.0, Nb) * (1.0 - pv[:, 0]), rng.uniform(0.3, 1.0, Nb) * pkg.decks.rs_sat(case["fluid"], pv[:, 1]))
    case["pv"] = np.ascontiguousarray(pv.reshape(-1))
    return case


def census_dx(rng, pv, meaning, flags, rs_sat):
    """an update vector for the state (pv, meaning) whose entries come from a few magnitudes on either side of each chop and,
    per cell, from one of a few intents: anything, water-only, gas disappears, gas appears, Rs clamp, and - for the cells that
    switched in the update before (flags) - a step into the 1e-5 oscillation band"""
    pv = np.asarray(pv).reshape(-1, 3)
    Nb = pv.shape[0]
    sw, p, x2 = pv[:, 0], pv[:, 1], pv[:, 2]
    gas = np.asarray(meaning) == SW_PO_SG
    jit = lambda: rng.uniform(0.8, 1.2, Nb)
    sgn = lambda: np.where(rng.random(Nb) < 0.5, -1.0, 1.0)
    dx = np.zeros((Nb, 3))
    s = np.where(sw < 0.3, -1.0, sgn())                                  # (keeps Sw away from 0)
    dx[:, 0] = s * rng.choice([0.01, 0.05, 0.15, 0.19, 0.21, 0.3, 0.6], Nb) * jit()
    dx[:, 1] = sgn() * p * rng.choice([0.01, 0.1, 0.25, 0.35, 0.6], Nb) * jit()
    sat = rs_sat(p)
    intent = rng.integers(0, 4, Nb)
    # Sg cells: a step of either sign, or past Sg = 0
    dsg = np.where(intent == 0, x2 + rng.choice([1e-3, 0.05], Nb) * jit(), sgn() * rng.choice([0.01, 0.1, 0.19, 0.25], Nb) * jit())
    dsg = np.where((x2 < 0.05) & (intent == 1), -0.1 * jit(), dsg)       # (gas that has just appeared grows)
    # Rs cells: past the saturated value, past Rs = 0 (the clamp), or a step of either sign
    drs = np.where(intent == 0, x2 - sat * (1.0 + rng.uniform(0.01, 0.3, Nb)), np.where(intent == 1, x2 * rng.uniform(1.1, 3.0, Nb), sgn() * x2 * rng.uniform(0.0, 0.5, Nb)))
    dx[:, 2] = np.where(gas, dsg, drs)
    # water-only: Sw past 1 without the saturation chop in the way
    wet = (sw > 0.82) & (rng.random(Nb) < 0.6)
    dx[wet, 0] = -(1.0 - sw[wet]) * rng.uniform(1.05, 1.1, wet.sum())
    dx[wet & gas, 2] = 0.01
    # the band: cells that switched a moment ago stop half-way into it, the pressure left alone
    band = (np.asarray(flags) != 0) & (sw < 0.9) & (rng.random(Nb) < 0.6)
    dx[band, 0] = 0.01
    dx[band, 1] = 0.0
    dx[band, 2] = np.where(gas[band], x2[band] + 0.5 * OSC_THRESHOLD, x2[band] - sat[band] * (1.0 + 0.5 * OSC_THRESHOLD))
    return dx


def census_counts(labels_per_step):
    """cells per label over a run of updates: {name: count}"""
    n = {}
    for lab in labels_per_step:
        for i, name in enumerate(BRANCHES):
            n[name] = n.get(name, 0) + int((lab["branch"] == i).sum())
        for i, name in enumerate(SAT_PHASES):
            n["largest_" + name] = n.get("largest_" + name, 0) + int((lab["sat_phase"] == i).sum())
        for name, v in (("sat_chop_on", lab["sat_chop"]), ("sat_chop_off", ~lab["sat_chop"]), ("p_chop_plus", lab["p_chop"] == 1),
                        ("p_chop_minus", lab["p_chop"] == -1), ("p_chop_off", lab["p_chop"] == 0), ("rs_clamp", lab["rs_clamp"])):
            n[name] = n.get(name, 0) + int(v.sum())
    return n
