"""Host-side standard wells for the device-resident Newton iteration: the well equations a deck's SCHEDULE section asks for, assembled on
the host (as in the reference: only the reservoir part of the linearisation and the Schur-complement operator are accelerated) and handed
to the device as the blocks bda::WellContributions carries - B, C (4 x 3 per perforation), D^-1 (4 x 4 per well).

What of the reference this restates, minimally (vertical wells, rate, BHP or THP control and several rate limits per well, crossflow in producers and vaporised oil in
the connection rates on request, no well storage term):
  wells/StandardWell_impl.hpp: computePerfRate (:195-420; producing perforations: phase rate = -Tw mob drawdown, surface rate through
      1/B, dissolved gas with the oil; injecting perforations: total mobility, the injected phase's 1/B), assembleWellEqWithoutIteration
      (:516-640: mass-balance equation per component = surface rate - sum of connection rates, one control equation), apply (:1254-1296),
      recoverSolutionWell (:1298-1311), updateWellState (full Newton update of the well unknowns);
  wells/BlackoilWellModel_impl.hpp: assemble / computeTotalRatesForDof (:496-512: the connection rates as source terms of the perforated
      cells), updateWellControls (:rate control <-> BHP limit), getWellConvergence.
Well unknowns per well (dim_wells = 4, bda/WellContributions.cpp:215-225): the surface rates of oil, water and gas INTO the reservoir
(production negative) and the bottom-hole pressure - a linear re-parametrisation of the reference's (WQTotal, WFrac, GFrac, BHP).

Coupled system per Newton iteration (x = reservoir update, x_w = well update; the reference's sign convention: new = old - update):
    [ A   C^T ] [ x   ]   [ r   ]        A : reservoir Jacobian with -d(connection rates)/d(cell variables) on the perforated cells' diagonal
    [ B   D   ] [ x_w ] = [ r_w ]            blocks (opmhip_set_source's dsource), C^T = d r_cell / d x_w, B = d r_w / d x_cell, D = d r_w / d x_w
The device solves (A - C^T D^-1 B) x = r - C^T D^-1 r_w (opmhip_wells_apply_residual, opmhip_solve_system with the wells in operator form)
and returns x_w = D^-1 (r_w - B x) (opmhip_wells_recover_solution).

The model object (capi.HipModel, or the oracle behind the same method names) supplies iq(): the cached intensive quantities of the cells.

The head between a well's reference depth and a completion (head_model):
  "cell_oil" (the default): (rho_o of the perforated cell * g) * dz - the minimal form;
  "wellbore": the reference's, from the density of the mixture in the well bore above every completion -
      StandardWell::computeWellConnectionPressures (wells/StandardWell_impl.hpp:1195-1210): computePropertiesForWellConnectionPressures
      (:899-1012), computeWellConnectionDensitesPressures (:1124-1189), StandardWellEval::computeConnectionDensities
      (wells/StandardWellEval.cpp:814-960), StandardWellGeneric::computeConnectionPressureDelta (wells/StandardWellGeneric.cpp:158-193);
      the state it reads - a pressure and three component rates per perforation - is WellState's (wells/WellState.cpp:298,
      StandardWell_impl.hpp:468).  Left out: solvent, salt, temperature, distributed wells' global perforation order, InjectorType::MULTI.
  Components are in the equations' order (oil, water, gas), phases in the record's (water, oil, gas): phase ph belongs to component
  COMPONENT_OF_PHASE[ph].

Crossflow (Well(allow_crossflow=True), off by default; WELSPECS item 10, which Flow defaults to YES): a producer's perforation whose
drawdown dd = p_o - (bhp + head) is not > 0 puts the well bore's mixture back into the formation - the injecting branch of
StandardWellEval::computePerfRate (wells/StandardWellEval.cpp:1023-1090) with allow_cf.  q = (q_o, q_w, q_g) are the well's rate unknowns:
    p_c = -q_c where q_c < 0, else 0;  P = (p_o + p_w) + p_g;  cmix_c = p_c / P         (wellSurfaceVolumeFraction, :233-243; the clamp is
    d cmix_c / d q_j = -((delta_cj - cmix_c) / P) where q_j < 0, else 0                   processFractions' on WFrac / GFrac)
    cqt_i = -tw * (((mob_w + mob_o) + mob_g) * dd)
    volumeRatio = (cmix_w / b_w + cmix_o / b_o) + (cmix_g - rs * cmix_o) / b_g           (b = 1/B of the perforated cell)
    cqt_is = cqt_i / volumeRatio;  rate_c = cmix_c * cqt_is
  Every quantity carries the value and seven derivatives (A8: value, d/dSw, d/dp, d/dX of the cell, d/dbhp, d/dq_o, d/dq_w, d/dq_g);
  a product is `mul` (a0 b0; a0 b_i + b0 a_i), a quotient `div` (v = a0 / b0; (a_i - v b_i) / b0), sums and differences entry by entry,
  in the order written above.  A well whose P is not > 0 (it has not flowed yet) and a perforation whose volumeRatio is not > 0 stay
  closed for that evaluation: nothing is divided by zero or a negative.  Then D = I - sum_p d rate / d q beside its bhp column and C gains
  its first three rows, C[j][c] = 0 - d rate_c / d q_j.  Perforations with dd > 0 and wells without the switch take the expressions above
  unchanged.  The default is the dry-gas form (rv = 0, d = 1, tmp_oil = cmix_o: as the producing branch, which by default adds rs q_o to
  the gas and nothing to the oil); StandardWells(vaporised_oil=True) takes the wet-gas form below.  Left out: openCrossFlowAvoidSingularity
  (the guard for a well without a flowing completion stays).
  Injectors: refused (ValueError).  In the reference an injector re-injects what crosses into it, because its composition (WFrac, GFrac)
  is an unknown while getQs pins the other components to zero; this parametrisation fixes the injected composition, and a half-measure
  would let oil leave through an injector's wellhead.

Vaporised oil in the connection rates (StandardWells(vaporised_oil=True) / DeviceStandardWells(vaporised_oil=True), per list, off by
default; needs the 19-field record of a fluid with PVTG): the oil the produced gas carries counts as oil - computePerfRate's rs / rv terms
(wells/StandardWellEval.cpp:999-1021, 1055-1073, 1092-1112).  surf[ph] = b_ph * (-tw * (mob_ph * dd)); rs, rv: the record's F_RS, F_RV with
their three cell derivatives.
    producing perforation (dd > 0, N = 5):  rate_o = surf_o + rv * surf_g;  rate_g = surf_g + rs * surf_o;  rate_w = surf_w
        (both products from the surf values before either sum); for a producer perf_dis_gas = (rs * surf_o).value,
        perf_vap_oil = (rv * surf_g).value
    reversed perforation of a producer with the crossflow switch (N = 8):
        d = 1 - rv * rs;  tmp_oil = (cmix_o - rv * cmix_g) / d;  tmp_gas = (cmix_g - rs * cmix_o) / d
        volumeRatio = (cmix_w / b_w + tmp_oil / b_o) + tmp_gas / b_g;  cqt_is and rate_c as above
        a perforation whose d is not > 0 stays closed for that evaluation, like one whose volumeRatio is not > 0 (the reference throws
        a NumericalIssue where d == 0)
        on values only (:1105-1111):  perf_vap_oil = rv * (q_g - rs * q_o) / d;  perf_dis_gas = rs * (q_o - rv * q_g) / d   (q = rate_c)
    injectors: unchanged - the injected composition is fixed, nothing of rv enters.
  solution_rates(): per well the sums of perf_dis_gas and perf_vap_oil over a producer's perforations as the last assemble formed them,
  in perforation order (StandardWell_impl.hpp:313-336, WellState.cpp:562-563), in this module's sign: rates into the reservoir, production
  negative.  Zeros for injectors and - both - with the switch off: the default model keeps the code it had, which forms neither.
  With the switch off a wet-gas record gives the dry-gas rates: no oil for the condensate, no sink for it in the perforated cells' oil rows.
  UNVERIFIED in the usual sense: the reference tree holds no number for a well's rates.

A tubing-head-pressure limit (Well(thp_limit=, vfp_table=, alq=), StandardWells(vfp=[tables])): a third control beside the rate target and
the BHP limit, through the VFPPROD (producers) / VFPINJ (injectors) tables of vfp.py.
  dp = (rho * g) * dh, dh = the table's datum depth - the well's reference depth (wells/WellHelpers.hpp:149-155), rho what the head model
      uses for the first perforation (the well-bore density there under "wellbore" - the reference's perf_densities_[0], getRho() -, the
      perforated cell's oil density otherwise); set with the heads, constant through the time step's Newton iterations;
  under ("thp", limit) the control equation is bhp - (V - dp) with V = vfp.bhp(table, q_w, q_o, q_g, limit, alq) and its derivatives by the
      three rates (control_eq = bhp - bhp_from_thp, wells/WellInterfaceEval.cpp:351-354, 433-436; calculateBhpFromThp :463-504);
  update_well_controls checks the limits in the reference's order (wells/WellInterfaceFluidSystem.cpp:170-268, injectors :100-166): the
      first that is violated and is not the control in force wins - BHP, the rate target, then THP: current = vfp.thp(table, q_w, q_o, q_g,
      bhp + dp, alq) (wells/StandardWellGeneric.cpp:116-156, wells/StandardWellEval.cpp:546-583); a producer switches when its limit >
      current, an injector when its limit < current, and its bhp becomes V - dp at the rates at hand (updateWellStateWithTarget's THP case,
      wells/WellInterface_impl.hpp:659-667, 882-890).
  Left out: gas lift (alq is a constant), bhpwithflo and the robust BHP-THP intersection (computeBhpAtThpLimitProd), well potentials.

Several rate limits per well (Well(limits={"orat": , "wrat": , "grat": , "lrat": , "resv": }); WCONPROD's ORAT, WRAT, GRAT, LRAT, RESV and
WCONINJE's RESV): positive surface volume rates, "resv" a reservoir volume rate; a limit that is absent does not exist.  They stand beside
the well's own ("rate", component, target), which keeps its place among them (an oil target is the well's ORAT limit, and so on; for an
injector it is WCONINJE's RATE); Well(use_list_target=False) takes it out of the limits - a deck record without a limit on a single
component.  The control tuples ("orat", v) ... ("resv", v) name the limit in force.
  control rows, in this module's sign (the unknowns are rates into the reservoir, a producer's are negative):
      ORAT / WRAT / GRAT   x[c] + limit                                      D[3][c] = 1
      LRAT                 (x_o + x_w) + limit                               D[3][o] = D[3][w] = 1
      RESV, producer       ((c_w x_w + c_o x_o) + c_g x_g) + limit           D[3][j] = c_j, c = calc_coeff (prediction mode,
                                                                             wells/WellInterfaceEval.cpp:320-331)
      RESV, injector       c_inj x[inj] - limit                              D[3][inj] = c_inj, c = calc_inj_coeff (:215-228)
  the rate converter (wells/RateConverter.hpp): reservoir_averages is defineState (:433-554) for the one region Flow's well model uses -
      hydrocarbon-pore-volume-weighted averages of p_o, Rs, Rv over all cells, the pore-volume-weighted ones where there is no hydrocarbon
      pore volume; calc_coeff, calc_inj_coeff, calc_reservoir_voidage_rates are calcCoeff, calcInjCoeff, calcReservoirVoidageRates
      (:592-777) operation by operation in the reference's statement order, 1/B through props.probe / probe_gas at the PVT region of the
      well's first perforated cell (wells/BlackoilWellModel_impl.hpp:748-759).  The averages are the model's (records()), frozen with the
      coefficients in calculate_explicit_quantities: constant through a time step's Newton iterations, as the heads are.
  update_well_controls, in the reference's order (wells/WellInterfaceFluidSystem.cpp:100-268): producers BHP, ORAT, WRAT, GRAT, LRAT, RESV,
      THP; injectors BHP, RATE, RESV, THP; the first limit that is violated and is not the control in force wins.  For RESV the current
      rate is the sum of calc_reservoir_voidage_rates at the well's present rates (:66-81, 217-231), not the coefficient form.
  KNOWN DIFFERENCES FROM FLOW: on a switch to a rate-type mode the well's state is left as it is (updateWellStateWithTarget's rescaling is
      left out, as under control 0).  The reference's injector RESV and THP branches assign a local copy of the control and return true
      without changing the well state (:140-166); here the well switches.  props.probe takes the saturated curve where Rs >= RsSat(p)
      (probe_gas where Rv >= RvSat); the reference's converter evaluates the undersaturated function at the averages as they are.
  Left out: CRAT, history-mode RESV (prediction_mode == false; a caller forms WCONHIST's target from the averages and hands it
      in as "resv"), FIP regions other than the whole field, salt and temperature in the converter.

Group production control (StandardWells(groups=[Group(...)], nupcol=), Well(group=, guide_rate=, available_for_group_control=); GCONPROD
with the exceed action RATE, WGRUPCON): a flat list of production groups, each a direct child of FIELD, every well in at most one.  A group
has targets "orat", "wrat", "grat", "lrat" (surface m^3/s), "resv" (reservoir m^3/s) and a mode, "none" or one of them; a well has one guide
rate per target mode (the converted values of opm-common's GuideRate::get stay with the caller).  A well that can hold its share is under
the control ("grup",), code GRUP_CODE = 8.  UNVERIFIED against Flow's numbers: the reference tree holds no output of a deck with groups.
  update_well_controls(iteration) runs BlackoilWellModel::updateWellControls (wells/BlackoilWellModel_impl.hpp:1239-1287): group data, the
      groups' check, group data, every well's group check, group data, the individual check of the wells that did not just switch, group data.
  group data (BlackoilWellModelGeneric.cpp:1494-1539, WellGroupHelpers.cpp:300-427): while iteration < nupcol the rates of the groups' producers
      are copied to the NUPCOL rates; per group and component reduction = 0 - the NUPCOL rates of its producers not under GRUP, guide_sum = the
      mode's guide rates of its producers under GRUP, rates = 0 - the present rates of its producers, voidage = their _resv_current (groups
      with a RESV target); every sum in list order starting from 0.  The record stays as it is until the next group data.
  the group's check (BlackoilWellModelGeneric.cpp:537-650, 888-943), only while iteration <= nupcol (the asymmetry with the copy's < is the
      reference's): ORAT, WRAT, GRAT, LRAT, RESV in that order, the first target that is < current and is not the mode in force wins;
      current from the present rates (LRAT: oil sum + water sum; RESV: the voidage sum); on a switch the rates of the group's wells under
      GRUP are multiplied by target / current when current > 1e-12 (updateWellRatesFromGroupTargetScale, WellGroupHelpers.cpp:429-).
  a well's group check (WellInterfaceFluidSystem.cpp:363-432, WellGroupHelpers.cpp:1055-1180) - a producer not under GRUP, available, in a group
      whose mode is not "none": mode(v) is v[c] for ORAT / WRAT / GRAT, v_o + v_w for LRAT, (c_w v_w + c_o v_o) + c_g v_g with the well's
      calc_coeff for RESV (TargetCalculator::calcModeRateFromRates, TargetCalculator.cpp:53-90); current = -mode(x);
      fraction = g_w / (guide_sum + g_w), 0 where that sum is <= 1e-12; target_rate = max(1e-12, ((target - mode(reduction)) + current) fraction);
      where current > target_rate the control becomes GRUP and the three rates are multiplied by target_rate / current (current > 1e-12).
  the control row under GRUP (WellInterfaceEval.cpp:178-266): target_rate = max(0, (target - mode(reduction)) (g_w / guide_sum)), the fraction 0
      where guide_sum <= 1e-12; the row is mode(x) + target_rate with the mode's derivatives - the rows of "orat" .. "resv" with target_rate in
      the limit's place; a group of mode "none" gives the BHP row bhp - bhp_limit (:189-221).
  A well leaves GRUP only through its individual limits: the existing rule.  Without groups every statement is the one it was.
  KNOWN DIFFERENCE FROM FLOW: updateWellStateWithTarget's second rescaling on a switch to GRUP (wells/WellInterface_impl.hpp:902-921) is left out,
      as it is for every other mode here.
  Left out: nested groups and a control on FIELD (updateGroupHigherControls), group guide rates, group and well efficiency factors (all 1),
      GCONINJE, GCONSALE / GCONSUMP, exceed actions other than RATE, CRAT / PRBL, injectors in a group's arithmetic (an injector may name a
      group and is ignored by it), well potentials.
"""
import numpy as np

from . import vfp as vfp_mod

OIL, WATER, GAS = 0, 1, 2          # equation / component order of the blocks (csrc/internal.hpp: EQ_OIL, EQ_WATER, EQ_GAS)
PH_W, PH_O, PH_G = 0, 1, 2         # phase order of the intensive-quantity record (opmhip_get_iq)
F_S, F_P, F_B, F_MOB, F_RHO, F_RS = 0, 3, 6, 9, 12, 15
F_RV = 16                          # in the 19-field record only (a fluid with PVTG, ROCKTAB or pc_scaling)
GRAVITY = 9.80665
COMPONENT_OF_PHASE = (WATER, OIL, GAS)      # indexed by PH_W, PH_O, PH_G
PHASE_BY_NAME = {"water": PH_W, "oil": PH_O, "gas": PH_G}
HEAD_MODELS = ("cell_oil", "wellbore")
INVBW, INVBO, RSSAT = 0, 2, 3              # columns of props.probe (capi.HipFluid.COLUMNS)
G_INVB, G_RVSAT = 0, 2                     # columns of props.probe_gas


def peaceman_factor(perm, dx, dy, dz, diameter, skin=0.0):
    """connection transmissibility factor of a vertical well in an isotropic cell (opm-common's Connection / Peaceman:
    2 pi K h / (ln(r0 / rw) + S), r0 = 0.28 sqrt(dx^2 + dy^2) / 2)"""
    r0 = 0.28 * np.sqrt(dx * dx + dy * dy) / 2.0
    return 2.0 * np.pi * perm * dz / (np.log(r0 / (0.5 * diameter)) + skin)


class SingularWellEquations(ValueError):
    """invert4_stated met a column without a non-zero pivot; .column says which"""

    def __init__(self, column):
        ValueError.__init__(self, "D is singular: no non-zero pivot in column %d of its elimination" % column)
        self.column = column


def invert4_stated(D):
    """D^-1 of one 4 x 4 matrix in an order a kernel can follow (csrc/device_blocks.hpp invert4_stated is this routine): Gauss-Jordan on [D | I],
    column by column; the pivot is the largest |entry| of the column at or below the diagonal, the lowest row on ties; the pivot row is
    divided by the pivot, every other row is updated as a - f * b - one rounding per operation.  A column without a non-zero pivot
    raises SingularWellEquations instead of dividing by it."""
    a = [[float(D[i][j]) for j in range(4)] + [1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for col in range(4):
        piv = col
        for r in range(col + 1, 4):
            if abs(a[r][col]) > abs(a[piv][col]):
                piv = r
        if not abs(a[piv][col]) > 0.0:
            raise SingularWellEquations(col)
        a[col], a[piv] = a[piv], a[col]
        p = a[col][col]
        a[col] = [v / p for v in a[col]]
        for r in range(4):
            if r != col:
                f = a[r][col]
                a[r] = [a[r][j] - f * a[col][j] for j in range(8)]
    return np.array([row[4:] for row in a])


def sequential_sums(a, pointers):
    """per range [pointers[k], pointers[k + 1]) of the rows of a (n x m): their sum, added row by row in ascending order starting from the
    first row - the loop a single lane runs.  (np.add.reduceat reduces pairwise and gives other bits.)"""
    a = np.asarray(a, float)
    out = np.zeros((len(pointers) - 1,) + a.shape[1:])
    for k in range(len(pointers) - 1):
        if pointers[k + 1] > pointers[k]:
            s = a[pointers[k]].copy()
            for j in range(pointers[k] + 1, pointers[k + 1]):
                s = s + a[j]
            out[k] = s
    return out


def row_times_vector(M, r):
    """M r for one 4 x 4 matrix, every row's products added in ascending column order starting from the first"""
    out = []
    for i in range(4):
        s = float(M[i][0]) * float(r[0])
        for j in range(1, 4):
            s += float(M[i][j]) * float(r[j])
        out.append(s)
    return np.array(out)


class Well:
    """name; cells: perforated cells (natural order, from the top of the well down); tw: connection transmissibility factors; ref_depth;
    producer or injector of `phase`; control: ("rate", component, target > 0 surface m^3/s) or ("bhp", pascal); bhp_limit: lower (producer) / upper (injector) limit;
    allow_crossflow (WELSPECS item 10; producers only): perforations whose drawdown is reversed inject the well bore's mixture;
    thp_limit (pascal) with vfp_table (the deck number of a VFPPROD / VFPINJ table handed to StandardWells) and alq: the tubing-head-pressure
    limit - lower (producer) / upper (injector); control may then also be ("thp", thp_limit);
    limits: dict of further rate limits, any of "orat", "wrat", "grat", "lrat" (surface m^3/s) and "resv" (reservoir m^3/s), all > 0 - an
    injector's only "resv" - and control may be (kind, that limit); use_list_target=False: the rate target of `rate_control` is not a limit
    of this well (the control must then be another one); rate_control: the well's own rate target where control is not the "rate" tuple;
    group: the index of the well's group in StandardWells(groups=) (None: directly under FIELD, no group control); guide_rate: one value for
    all five target modes or five (ORAT, WRAT, GRAT, LRAT, RESV), >= 0 and finite; available_for_group_control: WGRUPCON item 2; control may be
    ("grup",) for an available producer in a group (rate_control then names the well's own target)"""

    def __init__(self, name, cells, tw, ref_depth, producer, control, bhp_limit, inj_phase=None, preferred_phase="oil", allow_crossflow=False,
                 thp_limit=None, vfp_table=None, alq=0.0, limits=None, use_list_target=True, rate_control=None, group=None, guide_rate=0.0,
                 available_for_group_control=True):
        self.name, self.cells, self.tw = name, np.asarray(cells, np.int32), np.asarray(tw, float)
        self.ref_depth, self.producer, self.inj_phase = float(ref_depth), bool(producer), inj_phase
        self.preferred_phase = preferred_phase     # a producer's (WELSPECS item 6): the well bore's content where nothing flows (head_model="wellbore")
        self.control, self.bhp_limit = control, float(bhp_limit)
        self.rate_control = control if rate_control is None else rate_control   # the deck's rate target, kept for switching back from another limit
        self.use_list_target = bool(use_list_target)
        self.limits = _check_limits(name, self.producer, self.rate_control, limits, self.use_list_target, control)
        self.allow_crossflow = bool(allow_crossflow)
        _crossflow_flags([self])
        if (thp_limit is None) != (vfp_table is None):
            raise ValueError("well %s: thp_limit and vfp_table come together" % name)
        self.thp_limit = None if thp_limit is None else float(thp_limit)
        self.vfp_table, self.alq = None if vfp_table is None else int(vfp_table), float(alq)
        if control[0] == "thp" and (self.thp_limit is None or float(control[1]) != self.thp_limit):
            raise ValueError("well %s: THP control needs thp_limit, and the limit as its target" % name)
        self.group = None if group is None else int(group)
        self.guide_rate = _check_guide_rate(name, guide_rate)
        self.available_for_group_control = bool(available_for_group_control)
        if control[0] == "grup" and (not self.producer or self.group is None or not self.available_for_group_control):
            raise ValueError("well %s: GRUP control is for an available producer in a group" % name)


class Group:
    """a production group directly under FIELD (GCONPROD, exceed action RATE): name; targets: dict of any of "orat", "wrat", "grat", "lrat"
    (surface m^3/s) and "resv" (reservoir m^3/s), all > 0, None / +infinity: none; mode: the production control mode the group starts
    under, "none" or one of its targets"""

    def __init__(self, name, targets=None, mode="none"):
        self.name = name
        self.targets = {}
        for kind, v in (targets or {}).items():
            if kind not in LIMIT_KINDS:
                raise ValueError("group %s: unknown target %r (one of %s)" % (name, kind, ", ".join(LIMIT_KINDS)))
            if v is None or v == np.inf:
                continue
            v = float(v)
            if not v > 0.0:
                raise ValueError("group %s: the %s target %r is not > 0" % (name, kind, v))
            self.targets[kind] = v
        if mode not in GROUP_MODES or (mode != "none" and mode not in self.targets):
            raise ValueError("group %s: mode %r is not 'none' or one of the group's targets" % (name, mode))
        self.mode = mode


def _check_guide_rate(name, guide_rate):
    g = np.asarray(guide_rate, float).reshape(-1)
    if g.size == 1:
        g = np.repeat(g, 5)
    if g.size != 5 or not np.all(np.isfinite(g)) or np.any(g < 0.0):
        raise ValueError("well %s: guide_rate is one value or five (ORAT, WRAT, GRAT, LRAT, RESV), >= 0 and finite: %r" % (name, guide_rate))
    return g.copy()


class CellRecords:
    """the intensive-quantity records of some cells (model.iq_cells(cells)), addressed by cell id like the full array model.iq() returns"""

    def __init__(self, cells, records):
        self.row = {int(c): i for i, c in enumerate(cells)}
        self.rec = records

    def rows(self, cells):
        return self.rec[[self.row[int(c)] for c in cells]]


def _rows(iq, cells):
    return iq.rows(cells) if isinstance(iq, CellRecords) else np.asarray(iq)[np.asarray(cells, int)]


def _crossflow_flags(wells):
    """per well: allow_crossflow; an injector with the switch is refused (see the module's text)"""
    for w in wells:
        if getattr(w, "allow_crossflow", False) and not w.producer:
            raise ValueError("well %s: allow_crossflow on an injector is not modelled (the injected composition is fixed)" % w.name)
    return np.array([bool(getattr(w, "allow_crossflow", False)) for w in wells], bool)


CONTROL_CODE = {"rate": 0, "bhp": 1, "thp": 2, "orat": 3, "wrat": 4, "grat": 5, "lrat": 6, "resv": 7}     # opmhip_get_std_wells / opmhip_set_std_wells_state (0 - 2)
LIMIT_KINDS = ("orat", "wrat", "grat", "lrat", "resv")       # in the order update_well_controls looks at them
LIMIT_OF_COMPONENT = {OIL: "orat", WATER: "wrat", GAS: "grat"}
COMPONENT_OF_LIMIT = {"orat": OIL, "wrat": WATER, "grat": GAS}
GRUP_CODE = 8                                                # the control ("grup",): exists only with groups in force, so it is not in CONTROL_CODE
GROUP_MODES = ("none",) + LIMIT_KINDS                        # a group's production control mode, codes 0 .. 5 (opmhip_std_wells_groups.mode)
NUPCOL_DEFAULT = 3                                           # the deck keyword's default


def control_code(control):
    """the code of a control tuple: CONTROL_CODE's, GRUP_CODE for ("grup",)"""
    return GRUP_CODE if control[0] == "grup" else CONTROL_CODE[control[0]]


def reservoir_averages(iq, volume):
    """RateConverter::SurfaceToReservoirVoidage::defineState (wells/RateConverter.hpp:433-554) over all cells, by a sequential loop in cell
    order: iq (cells, 17 | 19 fields, 4) as model.iq() returns it, volume per cell -> array (pressure, rs, rv, pv, 1.0 | 0.0): the
    hydrocarbon-pore-volume-weighted averages where the field has hydrocarbon pore volume (last entry 1.0), else the pore-volume-weighted
    ones (0.0).  What capi.HipModel.reservoir_averages() forms on the device (there in a reduction's order: equal to rounding)."""
    iq = np.asarray(iq, float)
    nf = iq.shape[1]
    f_rv, f_poro = (16, 18) if nf == 19 else (None, 16)
    hpv_s = [0.0, 0.0, 0.0, 0.0]           # pv, pressure, rs, rv
    pv_s = [0.0, 0.0, 0.0, 0.0]
    for c in range(iq.shape[0]):
        pv_cell = float(volume[c]) * float(iq[c, f_poro, 0])
        hydrocarbon = 1.0
        hydrocarbon -= float(iq[c, F_S + PH_W, 0])
        po, rs = float(iq[c, F_P + PH_O, 0]), float(iq[c, F_RS, 0])
        rv = 0.0 if f_rv is None else float(iq[c, f_rv, 0])
        hpv = pv_cell * hydrocarbon
        if hpv > 0.0:
            hpv_s[0] += hpv
            hpv_s[1] += po * hpv
            hpv_s[2] += rs * hpv
            hpv_s[3] += rv * hpv
        if pv_cell > 0.0:
            pv_s[0] += pv_cell
            pv_s[1] += po * pv_cell
            pv_s[2] += rs * pv_cell
            pv_s[3] += rv * pv_cell
    if hpv_s[0] > 0.0:
        return np.array([hpv_s[1] / hpv_s[0], hpv_s[2] / hpv_s[0], hpv_s[3] / hpv_s[0], hpv_s[0], 1.0])
    if not pv_s[0] > 0.0:
        raise ValueError("reservoir_averages: the field's pore volume is %r, not > 0" % pv_s[0])
    return np.array([pv_s[1] / pv_s[0], pv_s[2] / pv_s[0], pv_s[3] / pv_s[0], pv_s[0], 0.0])


def _inv_b(props, averages_p, rs, rv, region):
    """(1/B_w(p), 1/B_o(p, rs), 1/B_g(p, rv)) out of the evaluator, as the well-bore heads take them"""
    p = np.array([float(averages_p)])
    bw = float(props.probe(p, pvt_region=int(region))[0, INVBW])
    bo = float(props.probe(p, float(rs), pvt_region=int(region))[0, INVBO])
    bg = float(props.probe_gas(p, float(rv), pvt_region=int(region))[0, G_INVB])
    return bw, bo, bg


def calc_coeff(props, averages, pvt_region=0):
    """RateConverter::calcCoeff (wells/RateConverter.hpp:592-646): coeff (oil, water, gas) with sum_c coeff[c] q_c = the reservoir voidage
    rate of the surface rates q at the averages (pressure, rs, rv, ...)"""
    p, Rs, Rv = float(averages[0]), float(averages[1]), float(averages[2])
    bw, bo, bg = _inv_b(props, p, Rs, Rv, pvt_region)
    coeff = [0.0, 0.0, 0.0]
    coeff[WATER] = 1.0 / bw
    detR = 1.0 - (Rs * Rv)
    den = bo * detR
    coeff[OIL] += 1.0 / den
    coeff[GAS] -= Rv / den
    den = bg * detR
    coeff[GAS] += 1.0 / den
    coeff[OIL] -= Rs / den
    return np.array(coeff)


def calc_inj_coeff(props, averages, pvt_region=0):
    """RateConverter::calcInjCoeff (:648-683): every phase alone, nothing dissolved or vaporised in what is injected"""
    bw, bo, bg = _inv_b(props, float(averages[0]), 0.0, 0.0, pvt_region)
    coeff = [0.0, 0.0, 0.0]
    coeff[WATER] = 1.0 / bw
    coeff[OIL] += 1.0 / bo
    coeff[GAS] += 1.0 / bg
    return np.array(coeff)


def calc_reservoir_voidage_rates(props, averages, surface_rates, pvt_region=0):
    """RateConverter::calcReservoirVoidageRates (:702-777): the reservoir volume rates (oil, water, gas) of the surface rates (oil, water,
    gas), with Rs = min(average, q_g / (q_o + 1e-15)) and Rv = min(average, q_o / (q_g + 1e-15))"""
    p = float(averages[0])
    qo, qw, qg = np.float64(surface_rates[OIL]), np.float64(surface_rates[WATER]), np.float64(surface_rates[GAS])
    with np.errstate(all="ignore"):                # (a rate of exactly -1e-15 divides by zero, as in the reference: IEEE's answer, no exception)
        a = np.float64(averages[1])
        b = qg / (qo + 1.0e-15)
        Rs = b if b < a else a                     # std::min(a, b)
        a = np.float64(averages[2])
        b = qo / (qg + 1.0e-15)
        Rv = b if b < a else a
    bw, bo, bg = _inv_b(props, p, Rs, Rv, pvt_region)
    out = [0.0, 0.0, 0.0]
    out[WATER] = qw / bw
    detR = 1.0 - (Rs * Rv)
    den = bo * detR
    v = qo
    v -= Rv * qg
    out[OIL] = v / den
    den = bg * detR
    v = qg
    v -= Rs * qo
    out[GAS] = v / den
    return np.array(out)


def _check_limits(name, producer, rate_control, limits, use_list_target, control):
    """the limits of one well as a dict kind -> float; ValueError with the reason for what opmhip_set_std_wells_limits refuses"""
    out = {}
    for kind, v in (limits or {}).items():
        if kind not in LIMIT_KINDS:
            raise ValueError("well %s: unknown limit %r (one of %s)" % (name, kind, ", ".join(LIMIT_KINDS)))
        if v is None or v == np.inf:
            continue                              # no such limit
        v = float(v)
        if not v > 0.0 or v != v:
            raise ValueError("well %s: the %s limit %r is not > 0" % (name, kind, v))
        if not producer and kind != "resv":
            raise ValueError("well %s: the %s limit is a producer's; an injector has its rate target and RESV" % (name, kind))
        if use_list_target and producer and rate_control[0] == "rate" and LIMIT_OF_COMPONENT[rate_control[1]] == kind:
            raise ValueError("well %s: a %s limit beside the well's own target on the same component" % (name, kind))
        out[kind] = v
    if not use_list_target and control[0] == "rate":
        raise ValueError("well %s: use_list_target=False for a well under its own rate target" % name)
    if control[0] in LIMIT_KINDS and (control[0] not in out or float(control[1]) != out[control[0]]):
        raise ValueError("well %s: %s control needs that limit, and the limit as its target" % (name, control[0].upper()))
    return out


def _thp_tables(wells, tables):
    """per well: the vfp.VFPTable of its THP limit (VFPPROD for a producer, VFPINJ for an injector, by deck number) or None"""
    out = []
    for w in wells:
        if getattr(w, "thp_limit", None) is None:
            out.append(None)
            continue
        kind = vfp_mod.PROD if w.producer else vfp_mod.INJ
        t = [t for t in (tables or []) if t.kind == kind and t.table_num == w.vfp_table]
        if len(t) != 1:
            raise ValueError("well %s: %d %s tables with the number %d" % (w.name, len(t), "VFPPROD" if w.producer else "VFPINJ", w.vfp_table))
        if len(t[0].thp_axis) < 2:
            raise ValueError("well %s: the THP axis of table %d has fewer than two entries" % (w.name, w.vfp_table))
        out.append(t[0])
    return out


def _group_lists(obj, groups, nupcol):
    """onto obj (StandardWells / DeviceStandardWells, with .wells): groups, nupcol, group_of_well (-1: under FIELD), guide (wells, 5),
    available, group_wells (per group its PRODUCERS, ascending: an injector may name a group and is ignored by it), group_target (groups, 5;
    +infinity: none), group_mode (codes of GROUP_MODES), group_resv (per well: a producer in a group with a RESV target), nupcol_rates and
    the group record of the last group data; ValueError for what opmhip_set_std_wells_groups refuses"""
    obj.groups = list(groups or [])
    ng, nw = len(obj.groups), len(obj.wells)
    obj.nupcol = int(nupcol)
    if obj.nupcol < 0:
        raise ValueError("nupcol = %d is not >= 0" % obj.nupcol)
    obj.group_of_well = np.full(nw, -1, np.int32)
    obj.guide = np.zeros((nw, 5))
    obj.available = np.ones(nw, np.int32)
    for k, w in enumerate(obj.wells):
        g = getattr(w, "group", None)
        if g is not None:
            if not 0 <= g < ng:
                raise ValueError("well %s: group %d is outside [0, %d)" % (w.name, g, ng))
            obj.group_of_well[k] = g
        obj.guide[k] = _check_guide_rate(w.name, getattr(w, "guide_rate", 0.0))
        obj.available[k] = int(bool(getattr(w, "available_for_group_control", True)))
        if w.control[0] == "grup" and (not w.producer or g is None or not obj.available[k]):
            raise ValueError("well %s: GRUP control is for an available producer in a group" % w.name)
    obj.group_wells = [[k for k in range(nw) if obj.group_of_well[k] == g and obj.wells[k].producer] for g in range(ng)]
    obj.group_target = np.array([[G.targets.get(kind, np.inf) for kind in LIMIT_KINDS] for G in obj.groups], float).reshape(ng, 5)
    obj.group_mode = [GROUP_MODES.index(G.mode) for G in obj.groups]
    obj.group_resv = np.zeros(nw, bool)
    for g in range(ng):
        if obj.group_target[g, 4] < np.inf:
            obj.group_resv[obj.group_wells[g]] = True
    obj.nupcol_rates = np.zeros((nw, 3))
    obj.group_record = dict(rates=np.zeros((ng, 3)), voidage=np.zeros(ng), reduction=np.zeros((ng, 3)), guide_sum=np.zeros(ng))


class StandardWells:
    """All wells at once: every step below is one pass of array arithmetic over the perforations (nperf x 5: value, d/dSw, d/dp, d/dX of the
    perforated cell, d/dbhp), per-well sums in the order of the perforations.

    arithmetic="numpy" (the default): the sums by np.add.reduceat (which reduces pairwise), D^-1 by np.linalg.  arithmetic="stated": the
    same equations in an order a kernel can follow, operation by operation - the sums by sequential_sums, D^-1 by invert4_stated, D^-1 r
    by row_times_vector; everything else (the product rule, the drawdown, the branches, the guard, the control rows) is elementwise IEEE
    arithmetic in both.  The stated form is what the device-resident wells (opmhip_set_std_wells, DeviceStandardWells) compute, bit for
    bit; a singular D raises SingularWellEquations there."""

    def __init__(self, wells, cell_depth, arithmetic="numpy", head_model="cell_oil", props=None, pvtnum=None, vfp=None, volume=None, vaporised_oil=False,
                 groups=None, nupcol=NUPCOL_DEFAULT):
        """groups: the list of Group objects the wells' `group` indices name (the module's text; None or empty: no group control, every
        statement as it was); nupcol: the deck's NUPCOL, >= 0.
        vaporised_oil: the wet-gas rate model (the module's text); the records handed in must then have 19 fields (ValueError otherwise).
        volume: the cells' volumes, for the reservoir averages of a RESV limit where the model has no reservoir_averages() of its own
        (a RESV limit also needs props).  head_model="wellbore" needs props: the fluid's property functions behind probe(p, rs, pvt_region=) and probe_gas(p, rv,
        pvt_region=) - capi.HipFluid(fluid), the device's, or the CPU oracle's in tests, as equil.py takes them - with the deck-level
        tables as props.fluid (the surface densities); pvtnum: PVT region per cell (None: region 0); vfp: the vfp.VFPTable list the wells' THP
        limits name (a list without limits computes what it computes with vfp=None)"""
        if arithmetic not in ("numpy", "stated"):
            raise ValueError("arithmetic: 'numpy' or 'stated'")
        if head_model not in HEAD_MODELS:
            raise ValueError("head_model: 'cell_oil' or 'wellbore'")
        if head_model == "wellbore" and props is None:
            raise ValueError("head_model='wellbore' needs props (probe / probe_gas)")
        self.arithmetic = arithmetic
        self.vaporised_oil = bool(vaporised_oil)
        self.head_model, self.props = head_model, props
        self.wells = list(wells)
        self.nw = len(self.wells)
        self.allow_crossflow = _crossflow_flags(self.wells)
        self.thp_tables = _thp_tables(self.wells, vfp)
        self.thp_dp = np.zeros(self.nw)            # per well with a limit: (rho g) dh of this time step
        self.thp_current = np.zeros(self.nw)       # ... the tubing-head pressure the last update_well_controls formed from the well's state
        self.bhp_from_thp = np.zeros(self.nw)      # ... V - dp of the last assemble()
        self._from_thp = np.zeros(self.nw)
        self.has_resv = any("resv" in getattr(w, "limits", {}) for w in self.wells)
        _group_lists(self, groups, nupcol)
        self.has_resv = self.has_resv or bool(self.group_resv.any())     # a group's RESV target needs the averages and the coefficients too
        self.volume = None if volume is None else np.asarray(volume, float)
        self.pvt_of_well = np.array([0 if pvtnum is None else int(np.asarray(pvtnum)[w.cells[0]]) for w in self.wells], int)
        self._model_averages = None                # what records() / set_reservoir_averages last took
        self.resv_averages = np.zeros(5)           # frozen by calculate_explicit_quantities: pressure, rs, rv, pv, hydrocarbon weights used
        self.resv_coeff = np.zeros((self.nw, 3))   # per well with a RESV limit: calc_coeff (producer) / calc_inj_coeff (injector), (oil, water, gas)
        self.resv_current = np.zeros(self.nw)      # ... the voidage rate the last update_well_controls formed from the well's rates
        self.vp = np.concatenate([[0], np.cumsum([len(w.cells) for w in self.wells])]).astype(np.int32)
        self.cells = np.concatenate([w.cells for w in self.wells]).astype(np.int32)
        self.tw = np.concatenate([w.tw for w in self.wells])
        self._rate_dq = None                       # d rate_c / d q_j of the last _perf_rates, (nperf, 3, 3); None: no perforation crossflows
        self.rate_dq = np.zeros((len(self.cells), 3, 3))   # ... of the last _assemble_wells, zeros without crossflow
        self._perf_solution = np.zeros((len(self.cells), 2))   # perf_dis_gas, perf_vap_oil of the last _perf_rates (vaporised_oil; zeros without)
        self._solution_rates = np.zeros((self.nw, 2))          # their per-well sums of the last _assemble_wells
        self.well_of_perf = np.repeat(np.arange(self.nw), np.diff(self.vp))
        # the cells the model is asked about / told about: every perforated cell once
        self.ucells, self.perf_row = np.unique(self.cells, return_inverse=True)
        self.ucells = self.ucells.astype(np.int32)
        self.depth = np.asarray(cell_depth, float)
        self.ref_depth_of_perf = np.array([w.ref_depth for w in self.wells])[self.well_of_perf]
        self.x = np.zeros((self.nw, 4))            # q_oil, q_water, q_gas (into the reservoir), bhp
        self.head = None                           # per perforation: pressure in the well bore there - bhp (calculate_explicit_quantities)
        self.initialised = False
        if head_model == "wellbore":
            for w in self.wells:
                if (w.producer and w.preferred_phase not in PHASE_BY_NAME) or (not w.producer and w.inj_phase not in PHASE_BY_NAME):
                    raise ValueError("head_model='wellbore': well %s has no known preferred / injected phase" % w.name)
            self.perf_depth = self.depth[self.cells]
            self.pvt_of_perf = np.zeros(len(self.cells), int) if pvtnum is None else np.asarray(pvtnum, int)[self.cells]
            self.surface_density = np.array([props.fluid.pvt[r]["density"] for r in self.pvt_of_perf], float)     # (nperf, 3): oil, water, gas
            self.perf_pressure = None                      # per perforation; None: the perforated cells' oil pressures when first needed
            self.perf_rates = np.zeros((len(self.cells), 3))   # the component rates of the last assemble()
            self.wellbore = None                           # dict(density, p_avg, mixture, x, b, rsmax, rvmax) of the last calculate_explicit_quantities

    def records(self, model):
        """the perforated cells' intensive quantities from the model - the perforated cells only (updatePerforationIntensiveQuantities,
        wells/BlackoilWellModel_impl.hpp:1606-1630); a model without iq_cells hands over its whole array"""
        if self.has_resv:                          # (a list without a RESV limit asks the model for what it asked before)
            if hasattr(model, "reservoir_averages"):
                self._model_averages = np.array(model.reservoir_averages(), float)
            else:
                if self.volume is None:
                    raise ValueError("a RESV limit needs the cells' volumes (StandardWells(volume=)) with a model that has no reservoir_averages()")
                self._model_averages = reservoir_averages(model.iq(), self.volume)
        if hasattr(model, "iq_cells"):
            return CellRecords(self.ucells, model.iq_cells(self.ucells))
        return model.iq()

    def set_reservoir_averages(self, averages):
        """the averages the next calculate_explicit_quantities freezes, handed in (pressure, rs, rv[, pv, weights]) instead of taken from a
        model in records() - e.g. the device's own, read back"""
        a = np.zeros(5)
        a[:len(averages)] = np.asarray(averages, float)
        self._model_averages = a

    def calculate_explicit_quantities(self, iq):
        """The pressure differences between the reference depth and the completions, once per time step from the state it starts with and
        constant through its Newton iterations (BlackoilWellModel::assemble, iteration 0: calculateExplicitQuantities ->
        StandardWell::computeWellConnectionPressures, wells/BlackoilWellModel_impl.hpp:824-827, wells/StandardWell_impl.hpp:1198-1245).
        Minimal form: the column between the reference depth and a completion weighs what the oil of the completion's cell weighs (the
        reference averages the well-bore mixture's phase densities segment by segment, StandardWellGeneric::computeConnectionPressureDelta)."""
        if self.head_model == "wellbore":
            self._wellbore_heads(iq)
            rho = self.wellbore["density"]
        else:
            q = _rows(iq, self.cells)
            rho = q[:, F_RHO + PH_O, 0]
            self.head = rho * GRAVITY * (self.depth[self.cells] - self.ref_depth_of_perf)
        for k, t in enumerate(self.thp_tables):      # the hydrostatic correction between the table's datum and the reference depth
            if t is not None:
                self.thp_dp[k] = (rho[self.vp[k]] * GRAVITY) * (t.datum_depth - self.wells[k].ref_depth)
        if self.has_resv:                            # RateConverter::defineState at the start of the time step (BlackoilWellModel::beginTimeStep)
            if self._model_averages is None or self.props is None:
                raise ValueError("a RESV limit needs props (probe / probe_gas) and the reservoir averages: records(model) or set_reservoir_averages")
            self.resv_averages = self._model_averages.copy()
            for k, w in enumerate(self.wells):
                if "resv" in w.limits or self.group_resv[k]:
                    self.resv_coeff[k] = (calc_coeff if w.producer else calc_inj_coeff)(self.props, self.resv_averages, self.pvt_of_well[k])
        if self.groups:                              # the group record the wells-alone solve reads: frozen through it, as the reference's group state is
            self._group_data(0)

    def _resv_current(self, k):
        """the voidage rate of well k at its present rates: the sum of calc_reservoir_voidage_rates, positive for what a producer takes out /
        an injector puts in (wells/WellInterfaceFluidSystem.cpp:145-152, 217-226)"""
        v = calc_reservoir_voidage_rates(self.props, self.resv_averages, self.x[k, :3], self.pvt_of_well[k])
        cur = 0.0
        if self.wells[k].producer:
            cur -= float(v[WATER])
            cur -= float(v[OIL])
            cur -= float(v[GAS])
        else:
            cur += float(v[WATER])
            cur += float(v[OIL])
            cur += float(v[GAS])
        return cur

    def _bhp_at_thp_limit(self, k):
        """vfp.bhp at well k's rates and limit: (9,) - value, the five partials, d/d(aqua, liquid, vapour)"""
        w, x = self.wells[k], self.x[k]
        return vfp_mod.bhp(self.thp_tables[k], float(x[WATER]), float(x[OIL]), float(x[GAS]), w.thp_limit, w.alq)

    def _initial_bhp(self, iq):
        q = _rows(iq, [w.cells[0] for w in self.wells])
        return q[:, F_P + PH_O, 0] + np.where([w.producer for w in self.wells], -1e5, 1e5)

    def _wellbore_pvt(self, p_avg):
        """computePropertiesForWellConnectionPressures (:931-1004) for all perforations: b (nperf, 3 components), rsmax, rvmax - elementwise,
        every value out of the evaluator; the well rates are the well unknowns now present"""
        n = len(self.cells)
        oilrate, gasrate = np.abs(self.x[:, OIL])[self.well_of_perf], np.abs(self.x[:, GAS])[self.well_of_perf]
        b, rsmax, rvmax = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
        for r in np.unique(self.pvt_of_perf):
            sel = np.flatnonzero(self.pvt_of_perf == r)
            p, qo, qg = p_avg[sel], oilrate[sel], gasrate[sel]
            first = self.props.probe(p, pvt_region=int(r))
            b[sel, WATER], rsmax[sel] = first[:, INVBW], first[:, RSSAT]
            rvmax[sel] = self.props.probe_gas(p, pvt_region=int(r))[:, G_RVSAT]
            with np.errstate(divide="ignore", invalid="ignore"):
                rv = np.minimum(np.where(qg > 0.0, qo / qg, 0.0), rvmax[sel])
                rs = np.minimum(np.where(qo > 0.0, qg / qo, 0.0), rsmax[sel])
            rv = np.where(qo > 0.0, rv, rvmax[sel])           # no oil rate: the saturated curve (the probes take it where rv >= RvSat)
            rs = np.where(qg > 0.0, rs, rsmax[sel])
            b[sel, GAS] = self.props.probe_gas(p, rv, pvt_region=int(r))[:, G_INVB]
            b[sel, OIL] = self.props.probe(p, rs, pvt_region=int(r))[:, INVBO]
        return b, rsmax, rvmax

    def _wellbore_heads(self, iq):
        """computeWellConnectionPressures.  arithmetic="stated": loop by loop in the reference's statement order, every sum sequential;
        "numpy": the same formulas vectorised, the sums by cumsum"""
        q = _rows(iq, self.cells)
        n = len(self.cells)
        if self.perf_pressure is None:           # WellState::init: the perforated cell's pressure (wells/WellState.cpp:298)
            self.perf_pressure = q[:, F_P + PH_O, 0].copy()
            self.perf_rates = np.zeros((n, 3))
        if not self.initialised:                 # ... and its bottom-hole pressure: the one solve_well_equations is about to start from
            self.x[:, 3] = self._initial_bhp(iq)
        first = self.vp[:-1]
        p_above = np.concatenate([[0.0], self.perf_pressure[:-1]])
        p_above[first] = self.x[:, 3]            # communicateAboveValues, serial: the bhp for the first perforation
        p_avg = (self.perf_pressure + p_above) / 2
        b, rsmax, rvmax = self._wellbore_pvt(p_avg)
        producer = np.array([w.producer for w in self.wells])
        rates = self.perf_rates.copy()
        # for producers where all perforations have zero rate: the mixture by the mobility ratio, the perforations weighted by tw (:1154-1184)
        # KNOWN DIFFERENCE FROM FLOW: every phase goes to its own component's place.  The reference writes the fractions in phase order
        # (water, oil, gas) into the component slots (oil, water, gas), so that a producer at rest in oil-bearing cells starts with a column
        # of water; a producer's first-step heads therefore differ from Flow's
        for k in range(self.nw):
            lo, hi = self.vp[k], self.vp[k + 1]
            if producer[k] and np.all(rates[lo:hi] == 0.0):
                if self.arithmetic == "stated":
                    total_tw = 0.0
                    for p in range(lo, hi):
                        total_tw += float(self.tw[p])
                    for p in range(lo, hi):
                        frac = float(self.tw[p]) / total_tw
                        total_mobility = 0.0
                        for ph in (PH_W, PH_O, PH_G):
                            total_mobility += float(q[p, F_B + ph, 0]) * float(q[p, F_MOB + ph, 0])
                        for ph in (PH_W, PH_O, PH_G):
                            rates[p, COMPONENT_OF_PHASE[ph]] = frac * float(q[p, F_MOB + ph, 0]) / total_mobility
                else:
                    frac = self.tw[lo:hi] / self.tw[lo:hi].sum()
                    tm = (q[lo:hi, F_B:F_B + 3, 0] * q[lo:hi, F_MOB:F_MOB + 3, 0]).sum(axis=1)
                    for ph in (PH_W, PH_O, PH_G):
                        rates[lo:hi, COMPONENT_OF_PHASE[ph]] = frac * q[lo:hi, F_MOB + ph, 0] / tm
        no_flow_mix = np.zeros((self.nw, 3))     # injector: the injected phase; producer: the preferred phase, for its first perforation
        for k, w in enumerate(self.wells):
            no_flow_mix[k, COMPONENT_OF_PHASE[PHASE_BY_NAME[w.preferred_phase if w.producer else w.inj_phase]]] = 1.0
        dens_fn = self._connection_densities_stated if self.arithmetic == "stated" else self._connection_densities_numpy
        density, mix, xcorr = dens_fn(rates, b, rsmax, rvmax, producer, no_flow_mix)
        # computeConnectionPressureDelta: dz to the perforation above (the reference depth for the first), then the running sum per well
        z_above = np.concatenate([[0.0], self.perf_depth[:-1]])
        z_above[first] = [w.ref_depth for w in self.wells]
        dp = (self.perf_depth - z_above) * density * GRAVITY
        head = np.zeros(n)
        for k in range(self.nw):
            lo, hi = self.vp[k], self.vp[k + 1]
            if self.arithmetic == "stated":
                acc = float(dp[lo])
                head[lo] = acc
                for p in range(lo + 1, hi):
                    acc = acc + float(dp[p])
                    head[p] = acc
            else:
                head[lo:hi] = np.cumsum(dp[lo:hi])
        self.head = head
        self.wellbore = dict(density=density, p_avg=p_avg, mixture=mix, x=xcorr, b=b, rsmax=rsmax, rvmax=rvmax)

    def _connection_densities_stated(self, rates, b, rsmax, rvmax, producer, no_flow_mix):
        """StandardWellEval::computeConnectionDensities (wells/StandardWellEval.cpp:814-960), statement by statement"""
        n = len(self.cells)
        density, mixture, xs = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
        rho = self.surface_density
        for k in range(self.nw):
            lo, hi = int(self.vp[k]), int(self.vp[k + 1])
            # 1. the flow exiting up the well bore from each perforation, from the bottom to the top
            q_out = [[0.0, 0.0, 0.0] for _ in range(hi - lo)]
            for p in range(hi - 1, lo - 1, -1):
                for c in range(3):
                    v = 0.0 if p == hi - 1 else q_out[p + 1 - lo][c]
                    v -= float(rates[p, c])
                    q_out[p - lo][c] = v
            # 2. the component mix, the volume ratio, the density of the segment above each perforation
            x = [0.0, 0.0, 0.0]
            for p in range(lo, hi):
                qo = q_out[p - lo]
                tot = ((0.0 + qo[0]) + qo[1]) + qo[2]              # std::accumulate
                if tot != 0.0:
                    mix = [abs(qo[c] / tot) for c in range(3)]
                elif not producer[k] or p == lo:
                    mix = [float(v) for v in no_flow_mix[k]]
                else:
                    mix = list(x)                                   # x, not mix, of the perforation above: as the reference has it
                x = list(mix)
                rs = rv = 0.0
                if mix[OIL] > 1e-12:
                    rs = min(mix[GAS] / mix[OIL], float(rsmax[p]))
                if mix[GAS] > 1e-12:
                    rv = min(mix[OIL] / mix[GAS], float(rvmax[p]))
                if rs != 0.0:
                    x[GAS] = (mix[GAS] - mix[OIL] * rs) / (1.0 - rs * rv)
                if rv != 0.0:
                    x[OIL] = (mix[OIL] - mix[GAS] * rv) / (1.0 - rs * rv)
                volrat = 0.0
                for c in range(3):
                    volrat += x[c] / float(b[p, c])
                sd = 0.0
                for c in range(3):                                  # std::inner_product
                    sd += float(rho[p, c]) * mix[c]
                density[p] = sd / volrat
                mixture[p], xs[p] = mix, x
        return density, mixture, xs

    def _connection_densities_numpy(self, rates, b, rsmax, rvmax, producer, no_flow_mix):
        """the same formulas over all perforations at once; only a perforation without flow looks at the one above"""
        n = len(self.cells)
        q_out = np.zeros((n, 3))
        for k in range(self.nw):
            lo, hi = self.vp[k], self.vp[k + 1]
            q_out[lo:hi] = -np.cumsum(rates[lo:hi][::-1], axis=0)[::-1]
        tot = q_out.sum(axis=1)
        flows = tot != 0.0
        mix = np.zeros((n, 3))
        mix[flows] = np.abs(q_out[flows] / tot[flows, None])
        x = np.zeros((n, 3))
        density = np.zeros(n)
        rho = self.surface_density

        def finish(sel):
            m = mix[sel]
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                rs = np.where(m[:, OIL] > 1e-12, np.minimum(m[:, GAS] / m[:, OIL], rsmax[sel]), 0.0)
                rv = np.where(m[:, GAS] > 1e-12, np.minimum(m[:, OIL] / m[:, GAS], rvmax[sel]), 0.0)
            xs = m.copy()
            xs[:, GAS] = np.where(rs != 0.0, (m[:, GAS] - m[:, OIL] * rs) / (1.0 - rs * rv), m[:, GAS])
            xs[:, OIL] = np.where(rv != 0.0, (m[:, OIL] - m[:, GAS] * rv) / (1.0 - rs * rv), m[:, OIL])
            x[sel] = xs
            density[sel] = (rho[sel] * m).sum(axis=1) / (xs / b[sel]).sum(axis=1)
        finish(np.flatnonzero(flows))
        for p in np.flatnonzero(~flows):                            # ascending: the perforation above is done
            k = self.well_of_perf[p]
            mix[p] = no_flow_mix[k] if (not producer[k] or p == self.vp[k]) else x[p - 1]
            finish(np.array([p]))
        return density, mix, x

    # ---- connection rates of every perforation with their derivatives: (nperf, 3 components, 1 + 3 cell variables + bhp) ----------------
    def _perf_rates(self, iq, bhp):
        """bhp: per well.  With crossflow the rates also depend on the wells' rate unknowns self.x[:, :3]: those derivatives, (nperf, 3
        components, 3 unknowns), are left in self._rate_dq (None where no perforation crossflows)"""
        self._rate_dq = None
        if self.head is None:
            self.calculate_explicit_quantities(iq)
        q = _rows(iq, self.cells)
        n = len(self.cells)
        ad = lambda f: np.concatenate([q[:, f, :], np.zeros((n, 1))], axis=1)     # value, d/dSw, d/dp, d/dX of the cell, d/dbhp

        def mul(a, b):
            out = np.empty_like(a)
            out[:, 0] = a[:, 0] * b[:, 0]
            out[:, 1:] = a[:, :1] * b[:, 1:] + b[:, :1] * a[:, 1:]
            return out
        dd = ad(F_P + PH_O)
        dd[:, 0] -= np.asarray(bhp)[self.well_of_perf] + self.head      # the head between the reference depth and the completion: explicit, see above
        dd[:, 4] = -1.0                                                 # d(drawdown)/d(bhp)
        b = [ad(F_B + ph) for ph in range(3)]
        mob = [ad(F_MOB + ph) for ph in range(3)]
        rs = ad(F_RS)
        rv = None
        self._perf_solution = np.zeros((n, 2))
        if self.vaporised_oil:
            if q.shape[1] != 19:
                raise ValueError("vaporised_oil=True needs the 19-field record of a fluid with PVTG: these records have %d fields" % q.shape[1])
            rv = ad(F_RV)
        tw = self.tw[:, None]
        out = np.zeros((n, 3, 5))
        producer = np.array([w.producer for w in self.wells])[self.well_of_perf]
        # producing perforations: phase rate = -Tw mob drawdown (reservoir volumes, out of the cell), surface volumes through 1/B, dissolved gas
        # with the oil
        flows = producer & (dd[:, 0] > 0.0)
        if flows.any():
            surf = [mul(b[ph], -tw * mul(mob[ph], dd)) for ph in range(3)]
            if rv is None:
                out[flows, OIL] = surf[PH_O][flows]
                out[flows, WATER] = surf[PH_W][flows]
                out[flows, GAS] = (surf[PH_G] + mul(rs, surf[PH_O]))[flows]
            else:                                  # the oil the gas carries counts as oil
                dis_gas, vap_oil = mul(rs, surf[PH_O]), mul(rv, surf[PH_G])
                out[flows, OIL] = (surf[PH_O] + vap_oil)[flows]
                out[flows, WATER] = surf[PH_W][flows]
                out[flows, GAS] = (surf[PH_G] + dis_gas)[flows]
                self._perf_solution[flows, 0] = dis_gas[flows, 0]
                self._perf_solution[flows, 1] = vap_oil[flows, 0]
        # injecting perforations: total mobility, the injected phase's 1/B
        inj = ~producer & (dd[:, 0] < 0.0)
        if inj.any():
            tot = mob[0] + mob[1] + mob[2]
            vol = -tw * mul(tot, dd)
            for name, ph, comp in (("gas", PH_G, GAS), ("water", PH_W, WATER), ("oil", PH_O, OIL)):
                sel = inj & np.array([w.inj_phase == name for w in self.wells])[self.well_of_perf]
                if sel.any():
                    out[sel, comp] = mul(b[ph], vol)[sel]
        # a perforation that would flow against the well's kind is closed, unless it is a producer's and the well allows crossflow
        cross = producer & self.allow_crossflow[self.well_of_perf] & ~(dd[:, 0] > 0.0)
        if cross.any():
            self._crossflow_rates(np.flatnonzero(cross), dd, b, mob, rs, out, rv)
        return out

    def _crossflow_rates(self, sel, dd, b, mob, rs, out, rv=None):
        """the perforations `sel` of producers with the switch: the module's formulas on A8 arrays, into out and self._rate_dq; rv: the
        wet-gas form (vaporised_oil), which also leaves the split of the rates in self._perf_solution"""
        mix = np.zeros((self.nw, 3, 8))            # cmix_c of every well: value and d/dq
        flowing = np.zeros(self.nw, bool)
        for k in np.flatnonzero(self.allow_crossflow):
            s = [bool(self.x[k, c] < 0.0) for c in range(3)]
            p = [-float(self.x[k, c]) if s[c] else 0.0 for c in range(3)]
            P = (p[OIL] + p[WATER]) + p[GAS]
            if not P > 0.0:
                continue                           # a well that has not flowed yet: its reversed perforations stay closed
            flowing[k] = True
            for c in range(3):
                mix[k, c, 0] = p[c] / P
                for j in range(3):
                    if s[j]:
                        mix[k, c, 5 + j] = -(((1.0 if c == j else 0.0) - mix[k, c, 0]) / P)
        sel = sel[flowing[self.well_of_perf[sel]]]
        if not len(sel):
            return
        wide = lambda a: np.concatenate([a[sel], np.zeros((len(sel), 3))], axis=1)

        def mul(x, y):
            o = np.empty_like(x)
            o[:, 0] = x[:, 0] * y[:, 0]
            o[:, 1:] = x[:, :1] * y[:, 1:] + y[:, :1] * x[:, 1:]
            return o

        def div(x, y):
            o = np.empty_like(x)
            o[:, 0] = x[:, 0] / y[:, 0]
            o[:, 1:] = (x[:, 1:] - o[:, :1] * y[:, 1:]) / y[:, :1]
            return o
        cmix = [mix[self.well_of_perf[sel], c] for c in range(3)]
        d8, b8, mob8, rs8 = wide(dd), [wide(v) for v in b], [wide(v) for v in mob], wide(rs)
        cqt_i = -self.tw[sel, None] * mul((mob8[PH_W] + mob8[PH_O]) + mob8[PH_G], d8)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):      # rows that end closed below
            if rv is None:
                ratio = (div(cmix[WATER], b8[PH_W]) + div(cmix[OIL], b8[PH_O])) + div(cmix[GAS] - mul(rs8, cmix[OIL]), b8[PH_G])
                ok = ratio[:, 0] > 0.0             # a volume ratio that is not positive: closed for this evaluation
            else:
                rv8 = wide(rv)
                one = np.zeros_like(rs8)
                one[:, 0] = 1.0
                d = one - mul(rv8, rs8)
                tmp_oil = div(cmix[OIL] - mul(rv8, cmix[GAS]), d)
                tmp_gas = div(cmix[GAS] - mul(rs8, cmix[OIL]), d)
                ratio = (div(cmix[WATER], b8[PH_W]) + div(tmp_oil, b8[PH_O])) + div(tmp_gas, b8[PH_G])
                ok = (d[:, 0] > 0.0) & (ratio[:, 0] > 0.0)     # ... and a d that is not positive (the reference throws where d == 0)
            cqt_is = div(cqt_i, ratio)
            rates = [mul(cmix[c], cqt_is) for c in range(3)]
            if rv is not None:                     # the split, on values only
                rs0, rv0, d0 = rs8[:, 0], rv8[:, 0], d[:, 0]
                vap_oil = rv0 * (rates[GAS][:, 0] - rs0 * rates[OIL][:, 0]) / d0
                dis_gas = rs0 * (rates[OIL][:, 0] - rv0 * rates[GAS][:, 0]) / d0
        if not ok.any():
            return
        self._rate_dq = np.zeros((len(self.cells), 3, 3))
        for c in range(3):
            out[sel[ok], c] = rates[c][ok, :5]
            self._rate_dq[sel[ok], c] = rates[c][ok, 5:]
        if rv is not None:
            self._perf_solution[sel[ok], 0] = dis_gas[ok]
            self._perf_solution[sel[ok], 1] = vap_oil[ok]

    def _control_rows(self):
        """(residual, d/d(q_o, q_w, q_g, bhp)) of every well's control equation"""
        r, g = np.zeros(self.nw), np.zeros((self.nw, 4))
        for k, (w, x) in enumerate(zip(self.wells, self.x)):
            if self.thp_tables[k] is not None:
                V = self._bhp_at_thp_limit(k)
                self._from_thp[k] = V[0] - self.thp_dp[k]
            if w.control[0] == "thp":
                r[k] = x[3] - self._from_thp[k]
                g[k, OIL], g[k, WATER], g[k, GAS], g[k, 3] = 0.0 - V[7], 0.0 - V[6], 0.0 - V[8], 1.0
            elif w.control[0] == "bhp":
                r[k], g[k, 3] = x[3] - w.control[1], 1.0
            elif w.control[0] == "grup":
                gi = self.group_of_well[k]
                mode = self.group_mode[gi]
                if mode == 0:                      # the group has no target in force: the BHP row
                    r[k], g[k, 3] = x[3] - w.bhp_limit, 1.0
                else:
                    rec = self.group_record
                    gsum = float(rec["guide_sum"][gi])
                    frac = float(self.guide[k, mode - 1]) / gsum if gsum > 1e-12 else 0.0
                    t = (float(self.group_target[gi, mode - 1]) - self._mode_rate(k, mode, rec["reduction"][gi])) * frac
                    target_rate = t if t > 0.0 else 0.0
                    r[k] = self._mode_rate(k, mode, x) + target_rate
                    if mode <= 3:
                        g[k, mode - 1] = 1.0
                    elif mode == 4:
                        g[k, OIL], g[k, WATER] = 1.0, 1.0
                    else:
                        g[k, :3] = self.resv_coeff[k]
            elif w.control[0] in COMPONENT_OF_LIMIT:
                comp = COMPONENT_OF_LIMIT[w.control[0]]
                r[k], g[k, comp] = x[comp] + w.control[1], 1.0
            elif w.control[0] == "lrat":
                r[k], g[k, OIL], g[k, WATER] = (x[OIL] + x[WATER]) + w.control[1], 1.0, 1.0
            elif w.control[0] == "resv":
                c = self.resv_coeff[k]
                if w.producer:
                    r[k] = ((c[WATER] * x[WATER] + c[OIL] * x[OIL]) + c[GAS] * x[GAS]) + w.control[1]
                    g[k, :3] = c
                else:
                    comp = COMPONENT_OF_PHASE[PHASE_BY_NAME[w.inj_phase]]
                    r[k], g[k, comp] = c[comp] * x[comp] - w.control[1], c[comp]
            else:
                comp, target = w.control[1], w.control[2]
                r[k], g[k, comp] = x[comp] - (-1.0 if w.producer else 1.0) * target, 1.0
        return r, g

    def update_well_controls(self, iteration=0):
        """BlackoilWellModel::updateWellControls: the limits in the reference's order, the first that is violated and is not the control in
        force wins.  A well leaves its rate target (or its THP limit) for BHP control when its BHP leaves the limit; it returns to the rate
        target once the rate exceeds it; with a THP limit it goes under THP control when the tubing-head pressure its state implies is
        beyond the limit; the further rate limits (Well(limits=)) stand between BHP and THP in the order ORAT, WRAT, GRAT, LRAT, RESV, the
        well's own target at its component's place (the module's text).  On a switch to a rate-type mode the state stays as it is.
        With groups (iteration: the reference's iterationIdx): the groups' check and every well's group check come first; a well that has
        just gone under GRUP is not looked at individually; group data in between and at the end (the module's text)."""
        just_switched = ()
        if self.groups:
            self._group_data(iteration)
            self._group_check(iteration)
            self._group_data(iteration)
            just_switched = [k for k in range(self.nw) if self._well_group_check(k)]
            self._group_data(iteration)
        for k, (w, x) in enumerate(zip(self.wells, self.x)):
            if k in just_switched:
                continue
            sign = -1.0 if w.producer else 1.0
            t = self.thp_tables[k]
            if t is not None:
                self.thp_current[k] = vfp_mod.thp(t, float(x[WATER]), float(x[OIL]), float(x[GAS]), float(x[3] + self.thp_dp[k]), w.alq)
            limits = getattr(w, "limits", {})
            if "resv" in limits:
                self.resv_current[k] = self._resv_current(k)
            own = w.rate_control if w.rate_control[0] == "rate" and getattr(w, "use_list_target", True) else None
            if w.control[0] != "bhp" and ((w.producer and x[3] < w.bhp_limit) or (not w.producer and x[3] > w.bhp_limit)):
                w.control = ("bhp", w.bhp_limit)
                x[3] = w.bhp_limit
                continue
            switched = False
            for kind in LIMIT_KINDS if w.producer else ("rate", "resv"):
                comp = COMPONENT_OF_LIMIT.get(kind, own[1] if own else None)
                if own is not None and comp == own[1] and kind != "lrat" and kind != "resv":     # the well's own target, at its component's place
                    hit = w.control[0] != "rate" and sign * x[comp] > own[2]
                    target = own
                elif kind not in limits or w.control[0] == kind:
                    continue
                else:
                    target = (kind, limits[kind])
                    if kind == "lrat":
                        current = -x[OIL]
                        current -= x[WATER]
                    elif kind == "resv":
                        current = self.resv_current[k]
                    else:
                        current = -x[comp]
                    hit = limits[kind] < current
                if hit:
                    w.control = target
                    switched = True
                    break
            if switched:
                continue
            if t is not None and w.control[0] != "thp" and (w.thp_limit > self.thp_current[k] if w.producer else w.thp_limit < self.thp_current[k]):
                w.control = ("thp", w.thp_limit)
                x[3] = self._bhp_at_thp_limit(k)[0] - self.thp_dp[k]
        if self.groups:
            self._group_data(iteration)

    # ---- group production control (the module's text) ------------------------------------------------------------------------------------
    def _mode_rate(self, k, mode, v):
        """calcModeRateFromRates for well k: the group mode's combination (code 1 .. 5) of the three values v (oil, water, gas)"""
        if mode <= 3:
            return float(v[mode - 1])
        if mode == 4:
            return float(v[OIL]) + float(v[WATER])
        c = self.resv_coeff[k]
        return (float(c[WATER]) * float(v[WATER]) + float(c[OIL]) * float(v[OIL])) + float(c[GAS]) * float(v[GAS])

    def _group_sums(self, g):
        """(rates (3), voidage) of group g's producers at their present rates, every sum in list order starting from 0"""
        s, void = [0.0, 0.0, 0.0], 0.0
        for k in self.group_wells[g]:
            for c in range(3):
                s[c] -= float(self.x[k, c])
            if self.group_target[g, 4] < np.inf:
                void += self._resv_current(k)
        return s, void

    def _group_data(self, iteration):
        rec = self.group_record
        for g, members in enumerate(self.group_wells):
            mode = self.group_mode[g]
            red, gsum = [0.0, 0.0, 0.0], 0.0
            for k in members:
                if iteration < self.nupcol:
                    self.nupcol_rates[k] = self.x[k, :3]
                if self.wells[k].control[0] == "grup":
                    if mode != 0:
                        gsum += float(self.guide[k, mode - 1])
                else:
                    for c in range(3):
                        red[c] -= float(self.nupcol_rates[k, c])
            s, void = self._group_sums(g)
            rec["rates"][g], rec["voidage"][g], rec["reduction"][g], rec["guide_sum"][g] = s, void, red, gsum

    def _group_check(self, iteration):
        if iteration > self.nupcol:
            return
        for g, members in enumerate(self.group_wells):
            s, void = self._group_sums(g)
            for mode in range(1, 6):
                target = float(self.group_target[g, mode - 1])
                if not target < np.inf or self.group_mode[g] == mode:
                    continue
                current = s[mode - 1] if mode <= 3 else (s[OIL] + s[WATER] if mode == 4 else void)
                if target < current:
                    self.group_mode[g] = mode
                    if current > 1e-12:
                        scale = target / current
                        for k in members:
                            if self.wells[k].control[0] == "grup":
                                for c in range(3):
                                    self.x[k, c] = self.x[k, c] * scale
                    break

    def _well_group_check(self, k):
        """-> whether well k has just gone under GRUP"""
        w, g = self.wells[k], int(self.group_of_well[k])
        if not w.producer or w.control[0] == "grup" or not self.available[k] or g < 0 or self.group_mode[g] == 0:
            return False
        mode, rec = self.group_mode[g], self.group_record
        current = -self._mode_rate(k, mode, self.x[k])
        gw = float(self.guide[k, mode - 1])
        gsum = float(rec["guide_sum"][g]) + gw
        frac = gw / gsum if gsum > 1e-12 else 0.0
        t = float(self.group_target[g, mode - 1]) - self._mode_rate(k, mode, rec["reduction"][g])
        t = t + current
        t = t * frac
        target_rate = t if t > 1e-12 else 1e-12
        if not current > target_rate:
            return False
        w.control = ("grup",)
        scale = target_rate / current if current > 1e-12 else 1.0
        for c in range(3):
            self.x[k, c] = self.x[k, c] * scale
        return True

    def group_rates(self):
        """per group, as the last group data left them: dict(mode (codes of GROUP_MODES), rates (groups, 3: oil, water, gas produced),
        voidage (groups with a RESV target; 0 otherwise), reduction (groups, 3), guide_sum)"""
        out = {k: v.copy() for k, v in self.group_record.items()}
        out["mode"] = np.array(self.group_mode, np.int32)
        return out

    def set_rate_target(self, k, target):
        """a WCONPROD / WCONINJE record at a report step (ScheduleEvents::PRODUCTION_UPDATE / INJECTION_UPDATE, wells/WellState.hpp:57): the
        well is under the deck's control mode again with the new target and its rate unknown starts there (updateWellStateWithTarget from
        prepareTimeStep, wells/BlackoilWellModel_impl.hpp:1426-1431); update_well_controls sends it back to its BHP limit if it cannot hold it"""
        w = self.wells[k]
        w.rate_control = ("rate", w.rate_control[1], float(target))
        w.control = w.rate_control
        old = self.x[k, w.rate_control[1]]
        new = (-1.0 if w.producer else 1.0) * float(target)
        if old != 0.0:
            self.x[k, :3] *= new / old           # the other components keep their ratio to the controlled one
        else:
            self.x[k, w.rate_control[1]] = new

    def _assemble_wells(self, iq):
        """residuals r_w (nw x 4), D (nw x 4 x 4), per perforation B (4 x 3: d r_w / d cell variables), C (4 x 3: C^T = d r_cell / d x_w),
        source (3) and dsource (3 x 3)"""
        self._rate_dq = None
        pr = self._perf_rates(iq, self.x[:, 3])
        nperf = len(self.cells)
        r = np.zeros((self.nw, 4))
        D = np.zeros((self.nw, 4, 4))
        seg = self.vp[:-1]
        if self.arithmetic == "stated":
            sums, dsums = sequential_sums(pr[:, :, 0], self.vp), sequential_sums(pr[:, :, 4], self.vp)
        else:
            sums, dsums = np.add.reduceat(pr[:, :, 0], seg, axis=0), np.add.reduceat(pr[:, :, 4], seg, axis=0)
        r[:, :3] = self.x[:, :3] - sums          # surface rate - sum of the connection rates
        D[:, [0, 1, 2], [0, 1, 2]] = 1.0
        D[:, :3, 3] = -dsums
        dq = self._rate_dq                       # crossflow: the connection rates answer to the well's own rate unknowns
        if dq is not None:
            flat = dq.reshape(nperf, 9)
            qsums = sequential_sums(flat, self.vp) if self.arithmetic == "stated" else np.add.reduceat(flat, seg, axis=0)
            D[:, :3, :3] = D[:, :3, :3] - qsums.reshape(self.nw, 3, 3)
        if self.vaporised_oil:                   # the dissolved gas and the vaporised oil a producer's rates hold (injectors' perforations: zeros)
            ps = self._perf_solution
            self._solution_rates = sequential_sums(ps, self.vp) if self.arithmetic == "stated" else np.add.reduceat(ps, seg, axis=0)
        else:
            self._solution_rates = np.zeros((self.nw, 2))
        r[:, 3], D[:, 3, :] = self._control_rows()
        # a well none of whose completions flows (its bottom-hole pressure on the wrong side of every completion's pressure) has no rate that
        # answers to its bottom-hole pressure: under a rate target its equations would be singular.  It keeps its bottom-hole pressure for
        # this iteration and its rates go to zero (the reference takes such a well out of operation: checkWellOperability,
        # wells/BlackoilWellModel_impl.hpp:1421-1423)
        for k in np.flatnonzero(np.all(D[:, :3, 3] == 0.0, axis=1) & (D[:, 3, 3] == 0.0)):
            r[k, 3], D[k, 3, :] = 0.0, (0.0, 0.0, 0.0, 1.0)
        B, C = np.zeros((nperf, 4, 3)), np.zeros((nperf, 4, 3))
        B[:, :3, :] = -pr[:, :, 1:4]                 # d r_w[c] / d (Sw, p, X) of the perforated cell
        C[:, 3, :] = -pr[:, :, 4]                    # d r_cell[c] / d bhp = - d(connection rate) / d bhp
        if dq is not None:
            C[:, :3, :] = 0.0 - dq.transpose(0, 2, 1)    # C[j][c]: d r_cell[c] / d q_j
        self.rate_dq = np.zeros((nperf, 3, 3)) if dq is None else dq
        self.last_perf_rates = pr[:, :, 0].copy()    # the connections' component rates of this assemble (tracers.connection_rates)
        return r, D, B, C, pr[:, :, 0], pr[:, :, 1:4]

    def solve_well_equations(self, iq, iterations=20):
        """the well equations alone at a frozen reservoir state (StandardWell::solveWellEqUntilConverged / prepareTimeStep): Newton on the
        4 unknowns of every well"""
        if not self.initialised:
            self.x[:, 3] = self._initial_bhp(iq)
        active = np.ones(self.nw, bool)
        for _ in range(iterations):
            r, D, *_ = self._assemble_wells(iq)
            if self.arithmetic == "stated":      # (a well that has stopped is not looked at again: its x and so its D no longer change)
                dx = np.zeros((self.nw, 4))
                for k in np.flatnonzero(active):
                    dx[k] = row_times_vector(invert4_stated(D[k]), r[k])
            else:
                dx = np.linalg.solve(D, r[:, :, None])[:, :, 0]
            self.x[active] -= dx[active]
            small = (np.abs(dx[:, :3]).max(axis=1) <= 1e-12 * np.maximum(1e-6, np.abs(self.x[:, :3]).max(axis=1))) & (np.abs(dx[:, 3]) <= 1e-3)
            active &= ~small
            if not active.any():
                break
        self.initialised = True

    def assemble(self, iq, ncells=None):
        """-> dict(wells for the C-ABI, res_well, cells / source_cells / dsource_cells: the connection rates per perforated cell, each named once):
        BlackoilWellModel::assemble at the present reservoir and well state.  ncells: also `source` / `dsource` as arrays over the whole grid
        (opmhip_set_source's form)."""
        rw, D, Bn, Cn, src, dsrc = self._assemble_wells(iq)
        self.bhp_from_thp = self._from_thp.copy()
        if self.head_model == "wellbore":        # the well state the next time step's heads start from (StandardWell_impl.hpp:468)
            self.perf_pressure = self.x[:, 3][self.well_of_perf] + self.head
            self.perf_rates = src.copy()
        Dinv = np.array([invert4_stated(d) for d in D]) if self.arithmetic == "stated" else np.linalg.inv(D)
        nu = len(self.ucells)
        source_cells, dsource_cells = np.zeros((nu, 3)), np.zeros((nu, 3, 3))
        np.add.at(source_cells, self.perf_row, src)
        np.add.at(dsource_cells, self.perf_row, dsrc)
        W = dict(numWells=self.nw, val_pointers=self.vp, Ccols=self.cells, Bcols=self.cells.copy(),
                 Cnnzs=np.ascontiguousarray(Cn.reshape(-1)), Bnnzs=np.ascontiguousarray(Bn.reshape(-1)), Dnnzs=np.ascontiguousarray(Dinv.reshape(-1)))
        out = dict(wells=W, res_well=np.ascontiguousarray(rw.reshape(-1)), cells=self.ucells, source_cells=np.ascontiguousarray(source_cells.reshape(-1)),
                   dsource_cells=np.ascontiguousarray(dsource_cells.reshape(-1)))
        if ncells is not None:
            source, dsource = np.zeros((ncells, 3)), np.zeros((ncells, 3, 3))
            source[self.ucells] = source_cells
            dsource[self.ucells] = dsource_cells
            out["source"], out["dsource"] = np.ascontiguousarray(source.reshape(-1)), np.ascontiguousarray(dsource.reshape(-1))
        return out

    def solution_rates(self):
        """(dissolved_gas, vaporised_oil): per well, the sums over a producer's perforations that the last assemble formed - rates into the
        reservoir, production negative; zeros for injectors and with vaporised_oil off (the module's text)"""
        return self._solution_rates[:, 0].copy(), self._solution_rates[:, 1].copy()

    def update(self, xw, relax=1.0):
        """updateWellState: the well unknowns follow their Newton update (x_w = D^-1 (r_w - B x) from the device)"""
        self.x -= relax * np.asarray(xw, float).reshape(self.nw, 4)

    def converged(self, res_well, tol_rate=1e-7, tol_bhp=1.0):
        """getWellConvergence: component equations relative to the largest rate of the well, control equation in its own unit"""
        rw = np.asarray(res_well, float).reshape(self.nw, 4)
        for k, w in enumerate(self.wells):
            scale = max(np.abs(self.x[k, :3]).max(), 1e-9)
            if np.abs(rw[k, :3]).max() > tol_rate * scale:
                return False
            ctl = abs(rw[k, 3])
            in_pressure = w.control[0] in ("bhp", "thp") or (w.control[0] == "grup" and self.group_mode[self.group_of_well[k]] == 0)
            if ctl > (tol_bhp if in_pressure else tol_rate * scale):
                return False
        return True

    def state(self):
        """(x, controls) and, with head_model="wellbore", a third entry: (perforation pressures | None, stored rates, whether the bottom-hole
        pressures have been set) - under that model the bottom-hole pressure is an input of the heads, so a state from before the first
        time step says so and the retry of a given-up first step starts from the cells again"""
        st = self.x.copy(), [w.control for w in self.wells]
        if self.head_model == "wellbore":
            st += ((None if self.perf_pressure is None else self.perf_pressure.copy(), self.perf_rates.copy(), self.initialised),)
        if self.groups:                          # last entry, a dict: the groups' modes and the NUPCOL rates
            st += (dict(group_mode=list(self.group_mode), nupcol_rates=self.nupcol_rates.copy()),)
        return st

    def set_state(self, st):
        self.x = st[0].copy()
        for w, c in zip(self.wells, st[1]):
            w.control = c
        if self.groups and isinstance(st[-1], dict):
            self.group_mode = list(st[-1]["group_mode"])
            self.nupcol_rates = st[-1]["nupcol_rates"].copy()
        if self.head_model == "wellbore" and len(st) > 2:
            self.perf_pressure = None if st[2][0] is None else st[2][0].copy()
            self.perf_rates = st[2][1].copy()
            if len(st[2]) > 2:
                self.initialised = bool(st[2][2])


class DeviceStandardWells:
    """The same wells resident on the device (opmhip_set_std_wells): model is a capi.HipModel whose state is set.  The well unknowns, the
    controls, the heads and the blocks B, C, D^-1 live there; what this object holds of them (x, controls, res_well) is the last read-back
    (fetch).  Wells with allow_crossflow are named to the library (opmhip_set_std_wells_crossflow), further rate limits (Well(limits=)) sent
    with opmhip_set_std_wells_limits, the wet-gas rate model switched on with opmhip_set_std_wells_vaporised_oil, group production control
    (groups=, nupcol=; Well(group=, guide_rate=)) sent with opmhip_set_std_wells_groups.  The arithmetic is StandardWells(arithmetic="stated")'s, bit for bit; newton.BlackoilModelHip takes the branch on_device."""
    on_device = True

    def __init__(self, wells, cell_depth, model, head_model="cell_oil", vfp=None, vaporised_oil=False, matrix_add=False, groups=None, nupcol=NUPCOL_DEFAULT):
        """groups / nupcol: group production control as StandardWells(groups=, nupcol=) - sent (opmhip_set_std_wells_groups) when some
        well names a group, a list without makes the calls it made before;
        matrix_add: the wells are written into the Jacobian every Newton iteration (opmhip_set_std_wells_matrix_add,
        opmhip_std_wells_add_to_matrix) instead of reaching the solver as the operator A - C^T D^-1 B; the model's pattern must hold the wells'
        cliques (decks.with_well_cliques) - ValueError with the library's text when a block is missing;
        vaporised_oil: the wet-gas rate model (opmhip_set_std_wells_vaporised_oil; ValueError on a context whose fluid has no PVTG);
        head_model="wellbore": the heads from the well-bore density (opmhip_set_std_wells_head_model), StandardWells(head_model="wellbore",
        arithmetic="stated")'s with the device's own property functions; vfp: the vfp.VFPTable list the wells' THP limits name - sent to the
        context (opmhip_set_vfp_tables) with the limits (opmhip_set_std_wells_thp) when some well has one"""
        if head_model not in HEAD_MODELS:
            raise ValueError("head_model: 'cell_oil' or 'wellbore'")
        self.wells = list(wells)
        self.nw = len(self.wells)
        self.m = model
        self.head_model = head_model
        self.allow_crossflow = _crossflow_flags(self.wells)
        phase = PHASE_BY_NAME
        depth = np.asarray(cell_depth, float)
        for w in self.wells:
            if w.rate_control[0] != "rate" or (w.control[0] == "bhp" and w.control[1] != w.bhp_limit):
                raise ValueError("DeviceStandardWells: well %s needs a rate target and, under BHP control, its limit as the target" % w.name)
            if w.control[0] == "thp" and w.control[1] != w.thp_limit:
                raise ValueError("DeviceStandardWells: well %s under THP control needs its limit as the target" % w.name)
            if w.control[0] in LIMIT_KINDS and w.control[1] != getattr(w, "limits", {}).get(w.control[0]):
                raise ValueError("DeviceStandardWells: well %s under %s control needs that limit as the target" % (w.name, w.control[0].upper()))
            if not w.producer and w.inj_phase not in phase:
                raise ValueError("DeviceStandardWells: injector %s with unknown phase %r" % (w.name, w.inj_phase))
            if head_model == "wellbore" and w.producer and w.preferred_phase not in phase:
                raise ValueError("DeviceStandardWells: producer %s with unknown preferred phase %r" % (w.name, w.preferred_phase))
        self.thp_tables = _thp_tables(self.wells, vfp)
        _group_lists(self, groups, nupcol)
        self.has_groups = bool(self.groups) and bool((self.group_of_well >= 0).any())
        self.vp = np.concatenate([[0], np.cumsum([len(w.cells) for w in self.wells])]).astype(np.int32)
        self.cells = np.concatenate([w.cells for w in self.wells]).astype(np.int32)
        model.set_std_wells(dict(
            perf_pointers=self.vp, cell=self.cells, tw=np.concatenate([w.tw for w in self.wells]),
            dz=np.concatenate([depth[w.cells] - w.ref_depth for w in self.wells]),
            producer=[int(w.producer) for w in self.wells], inj_phase=[0 if w.producer else phase[w.inj_phase] for w in self.wells],
            rate_component=[w.rate_control[1] for w in self.wells], rate_target=[w.rate_control[2] for w in self.wells],
            bhp_limit=[w.bhp_limit for w in self.wells], control=[int(w.control[0] == "bhp") for w in self.wells], x=None))
        if self.allow_crossflow.any():           # (a list without the switch makes the calls it made before)
            model.set_std_wells_crossflow(self.allow_crossflow.astype(np.int32))
        self.vaporised_oil = bool(vaporised_oil)
        if self.vaporised_oil:                   # (likewise)
            model.set_std_wells_vaporised_oil(True)
        self.matrix_add = bool(matrix_add)
        if self.matrix_add:                      # (likewise)
            model.set_std_wells_matrix_add(True)
        if head_model == "wellbore":
            self._wellbore = dict(perf_depth=depth[self.cells], ref_depth=[w.ref_depth for w in self.wells],
                                  preferred_phase=[phase[w.preferred_phase] if w.producer else PH_O for w in self.wells])
            model.set_std_wells_head_model(self._wellbore)
        if any(t is not None for t in self.thp_tables):     # (a list without a limit makes the calls it made before)
            model.set_vfp_tables(list(vfp))
            model.set_std_wells_thp(dict(vfp_table=[0 if t is None else w.vfp_table for w, t in zip(self.wells, self.thp_tables)],
                                         thp_limit=[0.0 if t is None else w.thp_limit for w, t in zip(self.wells, self.thp_tables)],
                                         alq=[w.alq if t is not None else 0.0 for w, t in zip(self.wells, self.thp_tables)],
                                         dh=[0.0 if t is None else t.datum_depth - w.ref_depth for w, t in zip(self.wells, self.thp_tables)]))
        self.has_limits = any(getattr(w, "limits", None) or not getattr(w, "use_list_target", True) for w in self.wells)
        if self.has_limits:                                  # (a list without further limits makes the calls it made before)
            inf = float("inf")
            kinds = dict(oil_rate="orat", water_rate="wrat", gas_rate="grat", liquid_rate="lrat", resv_rate="resv")
            # a well that starts under one of the new modes is under BHP control until the state call below: its own target may not be a limit
            lim = {field: [w.limits.get(kind, inf) for w in self.wells] for field, kind in kinds.items()}
            lim["use_list_target"] = [int(w.use_list_target) for w in self.wells]
            start = [1 if (w.control[0] in LIMIT_KINDS or w.control[0] in ("thp", "grup")) else CONTROL_CODE[w.control[0]] for w in self.wells]
            if any(s != int(w.control[0] == "bhp") for s, w in zip(start, self.wells)):
                model.set_std_wells_state(None, start, None)
            model.set_std_wells_limits(lim)
        if self.has_groups:                                  # (a list without groups makes the calls it made before)
            T = self.group_target
            model.set_std_wells_groups(dict(num_groups=len(self.groups), well_group=self.group_of_well, oil_target=T[:, 0], water_target=T[:, 1], gas_target=T[:, 2],
                                            liquid_target=T[:, 3], resv_target=T[:, 4], mode=self.group_mode, guide_rate=self.guide, available=self.available,
                                            nupcol=self.nupcol))
        if any(w.control[0] not in ("rate", "bhp") for w in self.wells):   # the list itself starts under the deck's modes: the others through the state call
            model.set_std_wells_state(None, [control_code(w.control) for w in self.wells], None)
        self.x = np.zeros((self.nw, 4))
        self.res_well = np.zeros((self.nw, 4))

    def begin_iteration(self, iteration):
        self.m.std_wells_begin_iteration(iteration)

    def fetch(self):
        """opmhip_get_std_wells: x, the controls in force (onto the Well objects) and r_w of the last assemble; with groups also their
        modes in force (opmhip_get_std_wells_groups): converged() reads them to tell a GRUP well's rate row from its BHP row"""
        self.x, ctl, self.res_well = self.m.get_std_wells()
        if self.has_groups:
            self.group_rates()
        for w, k in zip(self.wells, ctl):
            k = int(k)
            if k == GRUP_CODE:
                w.control = ("grup",)
            else:
                w.control = (w.rate_control, ("bhp", w.bhp_limit), ("thp", w.thp_limit))[k] if k < 3 else (LIMIT_KINDS[k - 3], w.limits[LIMIT_KINDS[k - 3]])
        return self.x

    def update(self, relax=1.0):
        self.m.std_wells_update(relax)

    def converged(self, res_well=None, tol_rate=1e-7, tol_bhp=1.0):
        """getWellConvergence on the last read-back"""
        return StandardWells.converged(self, self.res_well if res_well is None else res_well, tol_rate, tol_bhp)

    def set_rate_target(self, k, target):
        """StandardWells.set_rate_target on the read-back state, sent up again (a report-step event: the read-back does not matter)"""
        self.fetch()
        StandardWells.set_rate_target(self, k, target)
        self._send()

    def _send(self):
        self.m.set_std_wells_state(self.x, [control_code(w.control) for w in self.wells], [w.rate_control[2] for w in self.wells])

    def solution_rates(self):
        """opmhip_get_std_wells_solution_rates: (dissolved_gas, vaporised_oil) per well - StandardWells.solution_rates()"""
        return self.m.std_wells_solution_rates()

    def group_rates(self):
        """opmhip_get_std_wells_groups: StandardWells.group_rates() - dict(mode, rates, voidage, reduction, guide_sum) per group - and
        nupcol_rates (wells, 3); the groups' modes in force are kept on this object too"""
        out = self.m.std_wells_groups()
        self.group_mode = [int(v) for v in out["mode"]]
        return out

    def resv(self):
        """opmhip_get_std_wells_resv: dict(averages, coeff, resv_current) - StandardWells' resv_averages, resv_coeff, resv_current"""
        return self.m.std_wells_resv()

    def thp(self):
        """opmhip_get_std_wells_thp: dict(thp, dp, bhp_from_thp) per well - StandardWells' thp_current, thp_dp, bhp_from_thp"""
        return self.m.std_wells_thp()

    def state(self):
        """as StandardWells.state(); the per-perforation state is read back where the device has one (None before the first heads).  The
        third entry has no "bottom-hole pressures set" flag: the library keeps and rolls back its own (opmhip_update_failed)"""
        self.fetch()
        st = self.x.copy(), [w.control for w in self.wells]
        if self.head_model == "wellbore":
            wb = self.m.std_wells_wellbore()
            st += ((wb["perf_pressure"] if wb["perf_state_set"] else None, wb["perf_rates"]),)
        if self.has_groups:
            g = self.group_rates()
            st += (dict(group_mode=[int(v) for v in g["mode"]], nupcol_rates=g["nupcol_rates"]),)
        return st

    def set_state(self, st):
        """a third entry whose pressures are None ("not yet taken from the cells") sets the head model anew: the library then takes them from
        the cells at the next begin_iteration(0), as the host class does.  (Whether the bottom-hole pressures have been set is the library's
        to keep: it cannot be handed in.)  With groups the last entry's modes go back to the device; its NUPCOL rates do NOT: no entry point
        sets them - the library keeps and rolls back its own (opmhip_advance_time_level / opmhip_update_failed).  A state handed to another
        list, or one older than the last opmhip_advance_time_level, therefore leaves the device's NUPCOL rates as they are: from iteration >=
        nupcol on its reductions differ from those of StandardWells.set_state until the next iteration < nupcol copies the rates anew."""
        self.x = st[0].copy()
        for w, c in zip(self.wells, st[1]):
            w.control = c
        if self.has_groups and isinstance(st[-1], dict):     # the modes first: control 8 is checked against nothing of them, a mode needs its target
            self.group_mode = list(st[-1]["group_mode"])
            self.m.set_std_wells_group_targets(mode=self.group_mode)
        self._send()
        if self.head_model == "wellbore" and len(st) > 2:
            if st[2][0] is None:
                self.m.set_std_wells_head_model(self._wellbore)
            else:
                self.m.set_std_wells_perf_state(st[2][0], st[2][1])
