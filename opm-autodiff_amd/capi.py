"""ctypes binding of libopmhip.so — the same C-ABI a Flow-side shim binds (include/opmhip.h).

No fallback: if the shared library is missing this module raises at import of the library handle, and every
compute entry point returns OPMHIP_NO_DEVICE from opmhip_create when no gfx950 device is visible.
"""
import ctypes as C
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OPMHIP_LIB", os.path.join(HERE, "libopmhip.so"))  # OPMHIP_LIB: tuning variants only
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "opmhip.h")

SUCCESS = 0
ANALYSIS_FAILED, CREATE_PRECONDITIONER_FAILED, UNKNOWN_ERROR = -1, -2, -3
INVALID_ARGUMENT, NOT_READY, DEVICE_ERROR, NO_DEVICE = -4, -5, -6, -7
REORDER = {"level_scheduling": 1, "graph_coloring": 2, "graph_coloring_greedy": 3, "line_coloring": 4, "auto": 5, "distance2": 6}
RELAX = {"post_scale": 0, "in_sweep": 1}
PRECONDITIONER = {"ilu0": 0, "cpr_quasiimpes": 1, "cpr": 2, "cpr_trueimpes": 2}   # opmhip_preconditioner


class OpmHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("opmhip status %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int), ("device_id", C.c_int), ("verbosity", C.c_int), ("maxit", C.c_int),
                ("tolerance", C.c_double), ("ilu_relaxation", C.c_double), ("relax_mode", C.c_int),
                ("reorder", C.c_int), ("zero_diag_fix", C.c_int), ("chain_length", C.c_int), ("spmv_pipe_wgs", C.c_int),
                ("preconditioner", C.c_int), ("cpr_reuse_setup", C.c_int), ("cpr_async_setup", C.c_int), ("cpr_amg_ilu_levels", C.c_int), ("cpr_gather_rows", C.c_int),
                ("half_product", C.c_int), ("pin_host_arrays", C.c_int), ("fused_reductions", C.c_int)]


class Result(C.Structure):
    _fields_ = [("iterations", C.c_int), ("converged", C.c_int), ("reduction", C.c_double),
                ("conv_rate", C.c_double), ("elapsed", C.c_double), ("it", C.c_double), ("t_copy", C.c_double),
                ("t_factor", C.c_double), ("t_solve", C.c_double), ("num_colors", C.c_int),
                ("reserved", C.c_int * 3)]


EPS_FIELDS = ("swl", "swcr", "swu", "sowcr", "sgl", "sgcr", "sgu", "sogcr", "max_pcow", "max_pcgo", "max_krw", "max_krow", "max_krg", "max_krog",
              "krwr", "krorw", "krgr", "krorg")   # OPMHIP_EPS_* order


class EndpointScaling(C.Structure):
    _fields_ = [("sat_scaling", C.c_int), ("three_point_kr", C.c_int), ("krw", C.c_int), ("kro", C.c_int), ("krg", C.c_int),
                ("pcw", C.c_int), ("pcg", C.c_int), ("points", C.c_void_p * 18)]


def endpoint_scaling_struct(es):
    """dict(sat_scaling, three_point_kr, krw, kro, krg, pcw, pcg, <EPS_FIELDS>: per-cell arrays or absent) -> (struct, keep-alive)"""
    s = EndpointScaling()
    for k in ("sat_scaling", "three_point_kr", "krw", "kro", "krg", "pcw", "pcg"):
        setattr(s, k, int(es.get(k, 0)))
    keep = []
    for f, name in enumerate(EPS_FIELDS):
        a = _f64(es.get(name))
        keep.append(a)
        s.points[f] = None if a is None else a.ctypes.data
    return s, keep


MS_APPLY_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double))   # opmhip_ms_apply_fn


class Wells(C.Structure):
    _fields_ = [("num_wells", C.c_int), ("val_pointers", C.c_void_p), ("Ccols", C.c_void_p),
                ("Bcols", C.c_void_p), ("Cnnzs", C.c_void_p), ("Dnnzs", C.c_void_p), ("Bnnzs", C.c_void_p),
                ("num_ms_wells", C.c_int), ("ms_apply", MS_APPLY_FN), ("ms_user", C.c_void_p), ("distributed", C.c_int)]


class MsWells(C.Structure):
    """opmhip_ms_wells: multisegment wells for the device-resident form (opmhip_set_ms_wells)"""
    _fields_ = [("num_ms_wells", C.c_int), ("dim", C.c_int), ("dim_wells", C.c_int), ("Mb_pointers", C.c_void_p), ("Brows", C.c_void_p),
                ("block_pointers", C.c_void_p), ("Bcols", C.c_void_p), ("Bvals", C.c_void_p), ("Cvals", C.c_void_p),
                ("Dcol_pointers", C.c_void_p), ("Drows", C.c_void_p), ("Dvals", C.c_void_p), ("Dnnz_pointers", C.c_void_p)]


class Aquifers(C.Structure):
    """opmhip_aquifers: analytic aquifers for the device-resident form (opmhip_set_aquifers)"""
    _fields_ = [("num_aquifers", C.c_int), ("type", C.c_void_p), ("id", C.c_void_p), ("conn_pointers", C.c_void_p), ("cell", C.c_void_p),
                ("alpha", C.c_void_p), ("time_constant", C.c_void_p), ("water_density", C.c_void_p), ("datum_depth", C.c_void_p),
                ("initial_pressure", C.c_void_p), ("has_initial_pressure", C.c_void_p), ("influx_constant", C.c_void_p),
                ("table_pointers", C.c_void_p), ("td", C.c_void_p), ("pd", C.c_void_p), ("prod_index", C.c_void_p), ("total_compr", C.c_void_p),
                ("initial_watvolume", C.c_void_p), ("has_restart", C.c_void_p), ("restart_W_flux", C.c_void_p), ("restart_pressure", C.c_void_p)]


class BoundaryConditions(C.Structure):
    """opmhip_boundary_conditions: the FREE and RATE faces for the device-resident form (opmhip_set_boundary_conditions)"""
    _fields_ = [("num_faces", C.c_int), ("cell", C.c_void_p), ("direction", C.c_void_p), ("type", C.c_void_p), ("area", C.c_void_p),
                ("trans", C.c_void_p), ("depth", C.c_void_p), ("rate", C.c_void_p)]


class TracerResult(C.Structure):
    """opmhip_tracer_result"""
    _fields_ = [("converged", C.c_int), ("iterations", C.c_double), ("reduction", C.c_double)]


class StdWells(C.Structure):
    """opmhip_std_wells: standard wells for the device-resident form (opmhip_set_std_wells)"""
    _fields_ = [("num_wells", C.c_int), ("perf_pointers", C.c_void_p), ("cell", C.c_void_p), ("tw", C.c_void_p), ("dz", C.c_void_p),
                ("producer", C.c_void_p), ("inj_phase", C.c_void_p), ("rate_component", C.c_void_p), ("rate_target", C.c_void_p),
                ("bhp_limit", C.c_void_p), ("control", C.c_void_p), ("x", C.c_void_p)]


class StdWellsWellbore(C.Structure):
    """opmhip_std_wells_wellbore: what the heads from the well-bore density need beside the list (opmhip_set_std_wells_head_model)"""
    _fields_ = [("perf_depth", C.c_void_p), ("ref_depth", C.c_void_p), ("preferred_phase", C.c_void_p)]


class VfpTables(C.Structure):
    """opmhip_vfp_tables: VFPPROD / VFPINJ tables, SI (opmhip_set_vfp_tables)"""
    _fields_ = [("num_tables", C.c_int), ("kind", C.c_void_p), ("table_num", C.c_void_p), ("flo_type", C.c_void_p), ("wfr_type", C.c_void_p),
                ("gfr_type", C.c_void_p), ("datum_depth", C.c_void_p), ("axis_sizes", C.c_void_p), ("axis_pointers", C.c_void_p), ("axes", C.c_void_p),
                ("value_pointers", C.c_void_p), ("values", C.c_void_p)]


class StdWellsThp(C.Structure):
    """opmhip_std_wells_thp: the THP limits of the resident standard wells (opmhip_set_std_wells_thp)"""
    _fields_ = [("vfp_table", C.c_void_p), ("thp_limit", C.c_void_p), ("alq", C.c_void_p), ("dh", C.c_void_p)]


class StdWellsLimits(C.Structure):
    """opmhip_std_wells_limits: the further rate limits of the resident standard wells (opmhip_set_std_wells_limits)"""
    _fields_ = [("oil_rate", C.c_void_p), ("water_rate", C.c_void_p), ("gas_rate", C.c_void_p), ("liquid_rate", C.c_void_p), ("resv_rate", C.c_void_p),
                ("use_list_target", C.c_void_p)]


def make_std_wells_limits(t, num_wells):
    """dict(any of oil_rate, water_rate, gas_rate, liquid_rate, resv_rate per well, +infinity: no such limit; use_list_target per well) ->
    (StdWellsLimits struct, keep-alive dict); None -> (None, {}).  An absent or None entry is a NULL array."""
    if t is None:
        return None, {}
    arr = {}
    for name, _ in StdWellsLimits._fields_:
        v = t.get(name)
        if v is not None:
            arr[name] = _i32(np.asarray(v).reshape(-1)) if name == "use_list_target" else _f64(np.asarray(v, float).reshape(-1))
            if len(arr[name]) != num_wells:
                raise ValueError("make_std_wells_limits: %s has %d entries for the %d wells set" % (name, len(arr[name]), num_wells))
    s = StdWellsLimits()
    for name, a in arr.items():
        setattr(s, name, a.ctypes.data)
    return s, arr


class StdWellsGroups(C.Structure):
    """opmhip_std_wells_groups: group production control of the resident standard wells (opmhip_set_std_wells_groups)"""
    _fields_ = [("num_groups", C.c_int), ("well_group", C.c_void_p), ("oil_target", C.c_void_p), ("water_target", C.c_void_p), ("gas_target", C.c_void_p),
                ("liquid_target", C.c_void_p), ("resv_target", C.c_void_p), ("mode", C.c_void_p), ("guide_rate", C.c_void_p), ("available", C.c_void_p),
                ("nupcol", C.c_int)]


def make_std_wells_groups(t, num_wells):
    """dict(num_groups, well_group per well, any of oil_target, water_target, gas_target, liquid_target, resv_target per group, mode per
    group, guide_rate (wells, 5), available per well, nupcol) -> (StdWellsGroups struct, keep-alive dict); None -> (None, {}).  An absent
    or None entry is a NULL array."""
    if t is None:
        return None, {}
    ng = int(t["num_groups"])
    arr = {}
    for name, _ in StdWellsGroups._fields_:
        v = t.get(name)
        if name in ("num_groups", "nupcol") or v is None:
            continue
        arr[name] = _i32(np.asarray(v).reshape(-1)) if name in ("well_group", "mode", "available") else _f64(np.asarray(v, float).reshape(-1))
        want = 5 * num_wells if name == "guide_rate" else (num_wells if name in ("well_group", "available") else ng)
        if len(arr[name]) != want:
            raise ValueError("make_std_wells_groups: %s has %d entries, %d expected" % (name, len(arr[name]), want))
    s = StdWellsGroups()
    s.num_groups, s.nupcol = ng, int(t.get("nupcol", 0))
    for name, a in arr.items():
        setattr(s, name, a.ctypes.data)
    return s, arr


def make_vfp_tables(tables):
    """list of vfp.VFPTable (or objects with its attributes: kind, table_num, flo_type, wfr_type, gfr_type, datum_depth, axes in the order flo,
    thp[, wfr, gfr, alq], values with flo fastest) -> (VfpTables struct, keep-alive dict); empty / None -> (None, {})"""
    if not tables:
        return None, {}
    ap, vp, sizes, axes, values = [0], [0], [], [], []
    for t in tables:
        ax = [np.asarray(a, float).reshape(-1) for a in t.axes]
        sizes.append(([len(a) for a in ax] + [1, 1, 1])[:5])
        axes.extend(ax)
        v = np.asarray(t.values, float).reshape(-1)
        values.append(v)
        ap.append(ap[-1] + sum(len(a) for a in ax))
        vp.append(vp[-1] + len(v))
    arr = dict(kind=_i32([t.kind for t in tables]), table_num=_i32([t.table_num for t in tables]), flo_type=_i32([t.flo_type for t in tables]),
               wfr_type=_i32([t.wfr_type for t in tables]), gfr_type=_i32([t.gfr_type for t in tables]), datum_depth=_f64([t.datum_depth for t in tables]),
               axis_sizes=_i32(np.asarray(sizes).reshape(-1)), axis_pointers=_i32(ap), axes=_f64(np.concatenate(axes)), value_pointers=_i32(vp),
               values=_f64(np.concatenate(values)))
    s = VfpTables(len(tables))
    for name, _ in VfpTables._fields_[1:]:
        setattr(s, name, arr[name].ctypes.data)
    return s, arr


def make_std_wells_thp(t, num_wells):
    """dict(vfp_table, thp_limit, alq, dh per well; vfp_table 0: no limit) -> (StdWellsThp struct, keep-alive dict); None -> (None, {})"""
    if t is None:
        return None, {}
    arr = dict(vfp_table=_i32(np.asarray(t["vfp_table"]).reshape(-1)), thp_limit=_f64(np.asarray(t["thp_limit"], float).reshape(-1)),
               alq=_f64(np.asarray(t["alq"], float).reshape(-1)), dh=_f64(np.asarray(t["dh"], float).reshape(-1)))
    if any(len(a) != num_wells for a in arr.values()):
        raise ValueError("make_std_wells_thp: array lengths do not fit the %d wells set" % num_wells)
    s = StdWellsThp()
    for name, _ in StdWellsThp._fields_:
        setattr(s, name, arr[name].ctypes.data)
    return s, arr


def make_std_wells_wellbore(w, num_wells, nperf):
    """dict(perf_depth per perforation; ref_depth, preferred_phase (0 water, 1 oil, 2 gas) per well) for a list of num_wells wells and nperf
    perforations -> (StdWellsWellbore struct, keep-alive dict); None -> (None, {}).  Ragged input raises ValueError."""
    if w is None:
        return None, {}
    arr = dict(perf_depth=_f64(np.asarray(w["perf_depth"], float).reshape(-1)), ref_depth=_f64(np.asarray(w["ref_depth"], float).reshape(-1)),
               preferred_phase=_i32(np.asarray(w["preferred_phase"]).reshape(-1)))
    if len(arr["perf_depth"]) != nperf or len(arr["ref_depth"]) != num_wells or len(arr["preferred_phase"]) != num_wells:
        raise ValueError("make_std_wells_wellbore: array lengths do not fit the list (%d wells, %d perforations)" % (num_wells, nperf))
    s = StdWellsWellbore()
    for name, _ in StdWellsWellbore._fields_:
        setattr(s, name, arr[name].ctypes.data)
    return s, arr


def make_std_wells(w):
    """dict(perf_pointers, cell, tw, dz per perforation; producer, inj_phase, rate_component, rate_target, bhp_limit, control per well;
    x (num_wells x 4) or None) - wells.DeviceStandardWells builds it - -> (StdWells struct, keep-alive dict)"""
    if not w:
        return None, {}
    i32 = ("perf_pointers", "cell", "producer", "inj_phase", "rate_component", "control")
    arr = {k: (_i32(w[k]) if k in i32 else _f64(w[k])) for k in ("perf_pointers", "cell", "tw", "dz", "producer", "inj_phase", "rate_component",
                                                                  "rate_target", "bhp_limit", "control")}
    arr["x"] = _f64(np.asarray(w["x"], float).reshape(-1)) if w.get("x") is not None else None
    nw = len(arr["perf_pointers"]) - 1
    nperf = int(arr["perf_pointers"][-1]) if nw >= 0 else -1
    if nw < 0 or any(len(arr[k]) != nperf for k in ("cell", "tw", "dz")) or any(len(arr[k]) != nw for k in ("producer", "inj_phase", "rate_component",
                                                                                                          "rate_target", "bhp_limit", "control")) \
            or (arr["x"] is not None and len(arr["x"]) != 4 * nw):
        raise ValueError("make_std_wells: array lengths do not fit perf_pointers")
    s = StdWells(nw)
    for name, _ in StdWells._fields_[1:]:
        setattr(s, name, None if arr[name] is None else arr[name].ctypes.data)
    return s, arr


AQUIFER_TYPES = {"carter_tracy": 0, "fetkovich": 1}


def make_aquifers(aquifers):
    """list of per-aquifer dicts (aquifers.carter_tracy / aquifers.fetkovich: type, id, cells, alpha, time_constant, water_density,
    datum_depth, initial_pressure | None = equilibrate, and influx_constant, td, pd or prod_index, total_compr, initial_watvolume,
    restart | None), Carter-Tracy first, cells in natural order -> (Aquifers struct, keep-alive list).
    Ragged input (lengths that do not fit each other, an unknown type, a missing entry) raises ValueError."""
    if not aquifers:
        return None, []
    cp, tp = [0], [0]
    col = {k: [] for k in ("type", "id", "time_constant", "water_density", "datum_depth", "initial_pressure", "has_initial_pressure", "influx_constant",
                           "prod_index", "total_compr", "initial_watvolume", "has_restart", "restart_W_flux", "restart_pressure")}
    cells, alpha, td, pd = [], [], [], []
    for n, a in enumerate(aquifers):
        try:
            kind = AQUIFER_TYPES[a["type"]]
            cl, al = np.asarray(a["cells"]).reshape(-1), np.asarray(a["alpha"], float).reshape(-1)
            if len(cl) != len(al):
                raise ValueError("aquifer %d: %d cells, %d alphas" % (n, len(cl), len(al)))
            for k in ("id", "time_constant", "water_density", "datum_depth"):
                col[k].append(a[k])
            ip = a.get("initial_pressure")
            col["initial_pressure"].append(0.0 if ip is None else float(ip))
            col["has_initial_pressure"].append(int(ip is not None))
            t, p = (np.asarray(a[k], float).reshape(-1) for k in ("td", "pd")) if kind == 0 else (np.zeros(0), np.zeros(0))
            if len(t) != len(p):
                raise ValueError("aquifer %d: influence table with %d times, %d pressures" % (n, len(t), len(p)))
            col["influx_constant"].append(float(a["influx_constant"]) if kind == 0 else 0.0)
            for k in ("prod_index", "total_compr", "initial_watvolume"):
                col[k].append(float(a[k]) if kind == 1 else 0.0)
            rs = a.get("restart")
            col["has_restart"].append(int(rs is not None))
            col["restart_W_flux"].append(float(rs["W_flux"]) if rs is not None else 0.0)
            col["restart_pressure"].append(float(rs.get("pressure", 0.0)) if rs is not None else 0.0)
        except KeyError as e:
            raise ValueError("aquifer %d: missing entry %s" % (n, e))
        col["type"].append(kind)
        cells.append(cl); alpha.append(al); td.append(t); pd.append(p)
        cp.append(cp[-1] + len(cl))
        tp.append(tp[-1] + len(t))
    i32 = ("type", "id", "has_initial_pressure", "has_restart")
    arr = {k: (_i32(v) if k in i32 else _f64(v)) for k, v in col.items()}
    arr.update(conn_pointers=_i32(cp), cell=_i32(np.concatenate(cells)), alpha=_f64(np.concatenate(alpha)), table_pointers=_i32(tp),
               td=_f64(np.concatenate(td)), pd=_f64(np.concatenate(pd)))
    s = Aquifers(len(aquifers))
    for name, _ in Aquifers._fields_[1:]:
        setattr(s, name, arr[name].ctypes.data)
    return s, arr


BOUNDARY_TYPES = {"rate": 0, "free": 1}


def make_boundary_conditions(records):
    """list of face-group dicts (boundary.rate / boundary.free: type, cells, direction, area, trans, depth and, for "rate", rate (n, 3)),
    cells in natural order; the faces are listed in the order of the records -> (BoundaryConditions struct, keep-alive dict).
    Ragged input (lengths that do not fit each other, an unknown type, a missing entry) raises ValueError."""
    if not records:
        return None, {}
    col = {k: [] for k in ("cell", "direction", "type", "area", "trans", "depth", "rate")}
    for n, r in enumerate(records):
        try:
            kind = BOUNDARY_TYPES[r["type"]]
            cl = np.asarray(r["cells"]).reshape(-1)
            m = len(cl)
            per = {k: np.asarray(r[k], float).reshape(-1) for k in ("area", "trans", "depth")}
            per["direction"] = np.asarray(r["direction"]).reshape(-1)
            rt = np.asarray(r["rate"], float).reshape(-1, 3) if kind == 0 else np.zeros((m, 3))
            if any(len(v) != m for v in per.values()) or len(rt) != m:
                raise ValueError("boundary record %d: %d cells, arrays of other lengths" % (n, m))
        except KeyError as e:
            raise ValueError("boundary record %d: missing entry or unknown type %s" % (n, e))
        col["cell"].append(cl); col["type"].append(np.full(m, kind)); col["rate"].append(rt)
        for k, v in per.items():
            col[k].append(v)
    i32 = ("cell", "direction", "type")
    arr = {k: (_i32(np.concatenate(v)) if k in i32 else _f64(np.concatenate(v).reshape(-1))) for k, v in col.items()}
    s = BoundaryConditions(len(arr["cell"]))
    for name, _ in BoundaryConditions._fields_[1:]:
        setattr(s, name, arr[name].ctypes.data)
    return s, arr


def _header_define(name):
    with open(HEADER_PATH) as f:
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, f.read()).group(1))


def ms_wells_caps():
    """(largest M = 4 Mb of one well, KiB of dense D^-1 over the list) the device form takes: OPMHIP_MS_WELLS_MAX_M / _MAX_KIB of the header"""
    return _header_define("OPMHIP_MS_WELLS_MAX_M"), _header_define("OPMHIP_MS_WELLS_MAX_KIB")


MS_WELLS_FORMS = {"dense": 0, "tree": 1, "auto": 2}   # OPMHIP_MS_WELLS_DENSE / _TREE / _AUTO


def ms_wells_tree_cap():
    """the largest number of segments a well may have in the tree form: OPMHIP_MS_WELLS_TREE_MAX_SEGMENTS of the header"""
    return _header_define("OPMHIP_MS_WELLS_TREE_MAX_SEGMENTS")


def make_ms_wells(wells):
    """list of per-well dicts(Brows [Mb+1], Bcols [nblk], Bvals [nblk*12], Cvals [nblk*12], Dcolptr [4 Mb+1], Drows [nnz], Dvals [nnz]) - the
    constructor arguments of Opm::MultisegmentWellContribution, cells in natural order - -> (MsWells struct, keep-alive list).
    Ragged input (lengths that do not fit each other) raises ValueError."""
    if not wells:
        return None, []
    Mbp, blkp, nzp = [0], [0], [0]
    cat = {k: [] for k in ("Brows", "Bcols", "Bvals", "Cvals", "Dcolptr", "Drows", "Dvals")}
    for n, w in enumerate(wells):
        a = {k: np.asarray(w[k]).reshape(-1) for k in cat}
        Mb, nblk, nnz = len(a["Brows"]) - 1, len(a["Bcols"]), len(a["Dvals"])
        if Mb < 1:
            raise ValueError("multisegment well %d: Brows needs Mb + 1 >= 2 entries" % n)
        if a["Brows"][0] != 0 or a["Brows"][-1] != nblk or np.any(np.diff(a["Brows"]) < 0):
            raise ValueError("multisegment well %d: Brows must rise from 0 to the number of blocks (%d)" % (n, nblk))
        if len(a["Bvals"]) != 12 * nblk or len(a["Cvals"]) != 12 * nblk:
            raise ValueError("multisegment well %d: Bvals / Cvals need 12 values per block (%d blocks)" % (n, nblk))
        if len(a["Dcolptr"]) != 4 * Mb + 1:
            raise ValueError("multisegment well %d: Dcolptr needs 4 Mb + 1 = %d entries, has %d" % (n, 4 * Mb + 1, len(a["Dcolptr"])))
        if len(a["Drows"]) != nnz or a["Dcolptr"][0] != 0 or a["Dcolptr"][-1] != nnz or np.any(np.diff(a["Dcolptr"]) < 0):
            raise ValueError("multisegment well %d: Dcolptr must rise from 0 to len(Dvals) = len(Drows)" % n)
        for k in cat:
            cat[k].append(a[k])
        Mbp.append(Mbp[-1] + Mb)
        blkp.append(blkp[-1] + nblk)
        nzp.append(nzp[-1] + nnz)
    keep = [_i32(Mbp), _i32(np.concatenate(cat["Brows"])), _i32(blkp), _i32(np.concatenate(cat["Bcols"])), _f64(np.concatenate(cat["Bvals"])),
            _f64(np.concatenate(cat["Cvals"])), _i32(np.concatenate(cat["Dcolptr"])), _i32(np.concatenate(cat["Drows"])), _f64(np.concatenate(cat["Dvals"])), _i32(nzp)]
    return MsWells(len(wells), 3, 4, *[_ptr(k) for k in keep]), keep


def declared_symbols():
    """Every function name include/opmhip.h declares."""
    with open(HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(opmhip_[a-z0-9_]+)\s*\(", txt)))


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OpmHipError(NO_DEVICE, "libopmhip.so not built (%s); run `make -C %s` or "
                              "__graft_entry__.build() - there is no CPU fallback" % (LIB_PATH, HERE))
        L = C.CDLL(LIB_PATH)
        vp, ip, dp = C.c_void_p, C.c_void_p, C.c_void_p
        L.opmhip_abi_version.restype = C.c_int
        L.opmhip_default_config.argtypes = [C.POINTER(Config)]
        L.opmhip_default_config.restype = None
        L.opmhip_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
        L.opmhip_destroy.argtypes = [vp]
        L.opmhip_destroy.restype = None
        L.opmhip_last_error.argtypes = [vp]
        L.opmhip_last_error.restype = C.c_char_p
        L.opmhip_set_pattern.argtypes = [vp, C.c_int, C.c_int, ip, ip]
        L.opmhip_solve_system.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, ip, ip, dp, C.POINTER(Wells),
                                          C.POINTER(Result)]
        L.opmhip_get_result.argtypes = [vp, dp]
        L.opmhip_get_rhs.argtypes = [vp, dp]
        L.opmhip_add_well_contributions.argtypes = [vp, C.POINTER(Wells)]
        L.opmhip_wells_apply_residual.argtypes = [vp, C.POINTER(Wells), dp]
        L.opmhip_wells_recover_solution.argtypes = [vp, C.POINTER(Wells), dp, dp]
        L.opmhip_upload_system.argtypes = [vp, dp, dp]
        L.opmhip_spmv.argtypes = [vp, dp, dp]
        L.opmhip_ilu0_factor.argtypes = [vp, dp]
        L.opmhip_ilu0_apply.argtypes = [vp, dp, dp]
        L.opmhip_cpr_apply.argtypes = [vp, dp, dp]
        L.opmhip_preconditioned_product.argtypes = [vp, dp, dp, dp]
        L.opmhip_cpr_recreate.argtypes = [vp]
        L.opmhip_set_cpr_weights.argtypes = [vp, dp]
        L.opmhip_get_cpr_weights.argtypes = [vp, dp]
        L.opmhip_get_ordering.argtypes = [vp, ip, ip, ip]
        L.opmhip_get_ordering_info.argtypes = [vp, C.POINTER(C.c_int * 4)]
        L.opmhip_get_product_form.argtypes = [vp, C.POINTER(C.c_int * 4)]
        L.opmhip_get_split_assembly.argtypes = [vp, C.POINTER(C.c_longlong * 4), dp, dp]
        L.opmhip_set_ilu_fillin_level.argtypes = [vp, C.c_int]
        L.opmhip_get_ilu_info.argtypes = [vp, C.POINTER(C.c_int * 4)]
        L.opmhip_set_ms_wells.argtypes = [vp, C.POINTER(MsWells)]
        L.opmhip_get_ms_wells_info.argtypes = [vp, C.POINTER(C.c_int * 4)]
        L.opmhip_set_ms_wells_form.argtypes = [vp, C.c_int]
        L.opmhip_get_ms_wells_form_info.argtypes = [vp, C.POINTER(C.c_int * 6)]
        L.opmhip_get_ilu_factors.argtypes = [vp, ip, ip, ip, ip, ip, dp, dp, dp]
        L.opmhip_time_kernel.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.opmhip_cpr_levels.argtypes = [vp, ip, ip, C.c_int]
        L.opmhip_profile_enable.argtypes = [vp, C.c_int]
        L.opmhip_profile_get.argtypes = [vp, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
        L.opmhip_synchronize.argtypes = [vp]
        L.opmhip_comm_info.argtypes = [vp, ip]
        L.opmhip_comm_selftest.argtypes = [vp, dp]
        L.opmhip_set_vfp_tables.argtypes = [vp, C.POINTER(VfpTables)]
        L.opmhip_vfp_probe.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp]
        _lib = L
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def make_wells(w):
    """dict(numWells, val_pointers, Ccols, Bcols, Cnnzs, Dnnzs, Bnnzs[, numMsWells, ms_apply][, distributed]) -> (Wells struct, keep-alive list).
    numWells counts the standard wells; ms_apply(x, y) - numpy views of the pinned host vectors, natural order - performs
    y -= C^T (D^-1 (B x)) for the numMsWells multisegment wells in place (opmhip_wells.ms_apply)."""
    if not w:
        return None, []
    nstd = int(w.get("numWells", 0))
    if nstd > 0:
        keep = [_i32(w["val_pointers"]), _i32(w["Ccols"]), _i32(w["Bcols"]), _f64(w["Cnnzs"]), _f64(w["Dnnzs"]), _f64(w["Bnnzs"])]
        s = Wells(nstd, *[_ptr(k) for k in keep])
    else:
        keep, s = [], Wells(0)
    nms = int(w.get("numMsWells", 0))
    if nms > 0:
        fn, n = w["ms_apply"], int(w["N"])

        def tramp(_user, hx, hy):
            fn(np.ctypeslib.as_array(hx, shape=(n,)), np.ctypeslib.as_array(hy, shape=(n,)))
        cb = MS_APPLY_FN(tramp)
        keep.append(cb)
        s.num_ms_wells, s.ms_apply = nms, cb
    s.distributed = int(w.get("distributed", 0))   # decomposed runs: the same list on every rank, each with its own perforations (opmhip_wells.distributed)
    return s, keep


class HipSolver:
    """Thin object wrapper over one opmhip context (mirrors how bda::BdaSolver<3> is used:
    ctor(verbosity, maxit, tolerance, deviceID), solve_system(...), get_result(x))."""

    def __init__(self, verbosity=0, maxit=200, tolerance=1e-2, device_id=0, ilu_relaxation=0.9,
                 relax_mode="post_scale", reorder=None, zero_diag_fix=True, chain_length=0, spmv_pipe_wgs=0,
                 preconditioner="ilu0", cpr_reuse_setup=3, cpr_async_setup=0, cpr_amg_ilu_levels=None, cpr_gather_rows=None, half_product=0, pin_host_arrays=0, fused_reductions=0,
                 ilu_fillin_level=0):
        """reorder / cpr_amg_ilu_levels / cpr_gather_rows = None: what opmhip_default_config says (reorder "auto", the library's choice of
        the AMG smoother, the pressure stage across the ranks as the communicator's kind allows).  half_product: ILU0-BiCGStab forms the
        product after M^-1 from the backward sweep's row sums (0 the library's choice, > 0 wherever the pattern allows, < 0 never).
        ilu_fillin_level: --ilu-fillin-level, the n of the block ILU(n) preconditioner (opmhip_set_ilu_fillin_level; ignored with CPR)"""
        L = lib()
        cfg = Config()
        L.opmhip_default_config(C.byref(cfg))
        cfg.verbosity, cfg.maxit, cfg.tolerance, cfg.device_id = verbosity, maxit, tolerance, device_id
        cfg.ilu_relaxation = ilu_relaxation
        cfg.relax_mode = RELAX[relax_mode]
        if reorder is not None:
            cfg.reorder = REORDER[reorder]
        cfg.zero_diag_fix = int(zero_diag_fix)
        cfg.chain_length = int(chain_length)  # line colouring: rows per chain (0: the library's default, 8; 10 with reorder="auto")
        cfg.spmv_pipe_wgs = int(spmv_pipe_wgs)  # pipelined SpMV: workgroups it is sized for (0 default, < 0 off; tests use small values)
        # --linear-solver-configuration (setupPropertyTree.cpp:62-76): "cpr" is short for cpr_trueimpes, as in Flow
        cfg.preconditioner = PRECONDITIONER[preconditioner]
        if cpr_amg_ilu_levels is not None:
            cfg.cpr_amg_ilu_levels = int(cpr_amg_ilu_levels)   # finest levels of the pressure AMG that smooth with ILU0 (0: Jacobi everywhere, < 0: the library's choice)
        if cpr_gather_rows is not None:
            cfg.cpr_gather_rows = int(cpr_gather_rows)         # decomposed runs: the hierarchy is continued across the ranks from the first level this small (0 default, < 0 off)
        cfg.half_product = int(half_product)
        cfg.fused_reductions = int(fused_reductions)   # 1: one reduction (three sums) per BiCGStab half iteration, recurred norms
        self._pin = bool(pin_host_arrays)
        cfg.pin_host_arrays = int(pin_host_arrays)   # 1: vals / b / x keep their addresses (Flow's do): registered for DMA on first sight
        cfg.cpr_async_setup = int(cpr_async_setup)   # mode 2 only: the rebuild on a host thread beside the solves
        cfg.cpr_reuse_setup = int(cpr_reuse_setup)   # --cpr-reuse-setup: 0 every solve, 1 every time step, 2 after > 10 iterations, 3 never
        self._h = C.c_void_p()
        rc = L.opmhip_create(C.byref(cfg), C.byref(self._h))
        if rc != SUCCESS:
            raise OpmHipError(rc, L.opmhip_last_error(None).decode())
        self.Nb = self.nnzb = 0
        if ilu_fillin_level:
            self._check(L.opmhip_set_ilu_fillin_level(self._h, int(ilu_fillin_level)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().opmhip_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def _check(self, rc):
        if rc < 0:
            raise OpmHipError(rc, lib().opmhip_last_error(self._h).decode())
        return rc

    def set_vfp_tables(self, tables):
        """opmhip_set_vfp_tables: the VFPPROD / VFPINJ tables (list of vfp.VFPTable, SI) resident on the device; None or empty clears them.  A
        refused call leaves the previous set in force."""
        vt, keep = make_vfp_tables(tables)
        self._check(lib().opmhip_set_vfp_tables(self._h, C.byref(vt) if vt else None))

    def vfp_probe(self, kind, table_num, aqua, liquid, vapour, thp, alq=0.0, bhp_target=None):
        """opmhip_vfp_probe: the device's VFP functions at given points -> (n, 10): bhp, dthp, dwfr, dgfr, dalq, dflo, d/daqua, d/dliquid, d/dvapour
        and thp(..., bhp_target) (0 without a target) - vfp.probe's columns, bit for bit"""
        vals = (aqua, liquid, vapour, thp, alq) + (() if bhp_target is None else (bhp_target,))
        a = [np.ascontiguousarray(v) for v in np.broadcast_arrays(*(np.atleast_1d(np.asarray(v, np.float64)) for v in vals))]
        n = len(a[0])
        tgt = a.pop() if bhp_target is not None else None
        out = np.zeros((n, 10))
        self._check(lib().opmhip_vfp_probe(self._h, int(kind), int(table_num), n, *[_ptr(v) for v in a], _ptr(tgt), _ptr(out)))
        return out

    def set_pattern(self, Nb, rows, cols):
        rows, cols = _i32(rows), _i32(cols)
        self._check(lib().opmhip_set_pattern(self._h, Nb, len(cols), _ptr(rows), _ptr(cols)))
        self.Nb, self.nnzb = Nb, len(cols)

    def solve_system(self, Nb, rows, cols, vals, b, wells=None):
        """bda::BdaSolver::solve_system; returns the Result struct (check .converged like the reference)."""
        rows, cols, vals, b = _i32(rows), _i32(cols), _f64(vals), _f64(b)
        nnzb = self.nnzb if cols is None else len(cols)
        res = Result()
        ws, keep = make_wells(wells)
        self._check(lib().opmhip_solve_system(self._h, 3 * Nb, 9 * nnzb, 3, _ptr(vals), _ptr(rows), _ptr(cols),
                                              _ptr(b), C.byref(ws) if ws else None, C.byref(res)))
        self.Nb, self.nnzb = Nb, nnzb
        return res

    def get_result(self):
        if getattr(self, "_pin", False):
            # registered arrays must keep their addresses (opmhip_config.pin_host_arrays): one result buffer per context, handed out as a copy
            if getattr(self, "_xbuf", None) is None or len(self._xbuf) != 3 * self.Nb:
                self._xbuf = np.empty(3 * self.Nb)
            self._check(lib().opmhip_get_result(self._h, _ptr(self._xbuf)))
            return self._xbuf.copy()
        x = np.empty(3 * self.Nb)
        self._check(lib().opmhip_get_result(self._h, _ptr(x)))
        return x


    def get_rhs(self):
        """the right-hand side / residual currently on the device, natural order"""
        b = np.empty(3 * self.Nb)
        self._check(lib().opmhip_get_rhs(self._h, _ptr(b)))
        return b

    def add_well_contributions(self, wells):
        """A -= C^T D^-1 B into the device-resident matrix (StandardWell::addWellContributions); the pattern must hold
        the well cliques"""
        ws, keep = make_wells(wells)
        self._check(lib().opmhip_add_well_contributions(self._h, C.byref(ws) if ws else None))

    def wells_apply_residual(self, wells, res_well):
        """r -= C^T (D^-1 resWell) on the device-resident residual (StandardWell::apply(BVector& r))"""
        ws, keep = make_wells(wells)
        rw = _f64(res_well)
        self._check(lib().opmhip_wells_apply_residual(self._h, C.byref(ws) if ws else None, _ptr(rw)))

    def wells_recover_solution(self, wells, res_well):
        """xw = D^-1 (resWell - B x) from the device-resident solution (StandardWell::recoverSolutionWell)"""
        ws, keep = make_wells(wells)
        rw = _f64(res_well)
        xw = np.empty(4 * int(wells["numWells"]))
        self._check(lib().opmhip_wells_recover_solution(self._h, C.byref(ws) if ws else None, _ptr(rw), _ptr(xw)))
        return xw

    def upload_system(self, vals, b=None):
        vals, b = _f64(vals), _f64(b)
        self._check(lib().opmhip_upload_system(self._h, _ptr(vals), _ptr(b)))

    def spmv(self, x):
        x = _f64(x)
        y = np.empty_like(x)
        self._check(lib().opmhip_spmv(self._h, _ptr(x), _ptr(y)))
        return y

    def ilu0_factor(self, want_factors=True):
        lu = np.empty(9 * self.nnzb) if want_factors else None
        self._check(lib().opmhip_ilu0_factor(self._h, _ptr(lu)))
        return lu

    def ilu0_apply(self, d):
        d = _f64(d)
        v = np.empty_like(d)
        self._check(lib().opmhip_ilu0_apply(self._h, _ptr(d), _ptr(v)))
        return v

    def set_cpr_weights(self, w=None):
        """CPR weights from outside (3 per block row, natural order - e.g. Flow's getTrueImpesWeights); None: computed again"""
        w = None if w is None else _f64(np.asarray(w).reshape(-1))
        self._w_keep = w
        self._check(lib().opmhip_set_cpr_weights(self._h, _ptr(w)))

    def cpr_weights(self):
        w = np.empty(3 * self.Nb)
        self._check(lib().opmhip_get_cpr_weights(self._h, _ptr(w)))
        return w.reshape(-1, 3)

    def cpr_recreate(self):
        """the next solve builds the CPR hierarchy's structure anew (the host's ISTLSolverEbos::shouldCreateSolver said so)"""
        self._check(lib().opmhip_cpr_recreate(self._h))

    def cpr_apply(self, d):
        d = _f64(d)
        v = np.empty_like(d)
        self._check(lib().opmhip_cpr_apply(self._h, _ptr(d), _ptr(v)))
        return v

    def preconditioned_product(self, d):
        """(A (M^-1 d), M^-1 d) in the form ILU0-BiCGStab uses inside a solve (opmhip_preconditioned_product)"""
        d = _f64(d)
        t, z = np.empty_like(d), np.empty_like(d)
        self._check(lib().opmhip_preconditioned_product(self._h, _ptr(d), _ptr(t), _ptr(z)))
        return t, z

    def ordering(self):
        to = np.empty(self.Nb, np.int32)
        fr = np.empty(self.Nb, np.int32)
        rpc = np.zeros(self.Nb, np.int32)
        nc = self._check(lib().opmhip_get_ordering(self._h, _ptr(to), _ptr(fr), _ptr(rpc)))
        return to, fr, rpc[:nc].copy()

    def ordering_info(self):
        """what the library's own choices resolved to (opmhip_get_ordering_info)"""
        info = (C.c_int * 4)()
        self._check(lib().opmhip_get_ordering_info(self._h, C.byref(info)))
        names = {v: k for k, v in REORDER.items()}
        return {"ilu_ordering": names[info[0]], "chain_length": int(info[1]), "colors": int(info[2]), "cpr_amg_ilu_levels": int(info[3])}

    def set_ilu_fillin_level(self, n):
        self._check(lib().opmhip_set_ilu_fillin_level(self._h, int(n)))

    def set_ms_wells(self, wells, form="dense"):
        """opmhip_set_ms_wells: the multisegment wells (list of dicts, see make_ms_wells) on the device for every operator application that
        follows; None or an empty list clears them.  form: "dense", "tree" or "auto" (opmhip_set_ms_wells_form, set in front of a list; a
        clearing call leaves the form as it is)"""
        ms, keep = make_ms_wells(wells)
        if ms:
            self._check(lib().opmhip_set_ms_wells_form(self._h, MS_WELLS_FORMS[form] if isinstance(form, str) else int(form)))
        self._check(lib().opmhip_set_ms_wells(self._h, C.byref(ms) if ms else None))

    def ms_wells_form_info(self):
        """opmhip_get_ms_wells_form_info: the form set, the list's wells by form, the largest tree well's segments and depth, KiB of tree blocks"""
        info = (C.c_int * 6)()
        self._check(lib().opmhip_get_ms_wells_form_info(self._h, C.byref(info)))
        names = {v: k for k, v in MS_WELLS_FORMS.items()}
        return {"form": names[int(info[0])], "dense": int(info[1]), "tree": int(info[2]), "tree_max_segments": int(info[3]), "tree_max_depth": int(info[4]),
                "tree_kib": int(info[5])}

    def ms_wells_info(self):
        """opmhip_get_ms_wells_info: wells on the device, largest M = 4 Mb, device KiB held for them, inversions done so far"""
        info = (C.c_int * 4)()
        self._check(lib().opmhip_get_ms_wells_info(self._h, C.byref(info)))
        return {"wells": int(info[0]), "max_m": int(info[1]), "kib": int(info[2]), "factorisations": int(info[3])}

    def ilu_info(self):
        """opmhip_get_ilu_info: fill level in force, blocks of L and U, levels (colours) per sweep"""
        info = (C.c_int * 4)()
        self._check(lib().opmhip_get_ilu_info(self._h, C.byref(info)))
        return {"fill_level": int(info[0]), "nl": int(info[1]), "nu": int(info[2]), "levels": int(info[3])}

    def ilu_factors(self, values=True):
        """opmhip_get_ilu_factors: dict(to, lrowptr, lcol, urowptr, ucol[, L, U, invD]) - internal order, blocks [n, 3, 3]"""
        inf = self.ilu_info()
        Nb, nl, nu = self.Nb, inf["nl"], inf["nu"]
        out = {"to": np.empty(Nb, np.int32), "lrowptr": np.empty(Nb + 1, np.int32), "lcol": np.empty(nl, np.int32),
               "urowptr": np.empty(Nb + 1, np.int32), "ucol": np.empty(nu, np.int32)}
        vals = [None, None, None]
        if values:
            vals = [np.empty((nl, 3, 3)), np.empty((nu, 3, 3)), np.empty((Nb, 3, 3))]
            out.update(L=vals[0], U=vals[1], invD=vals[2])
        self._check(lib().opmhip_get_ilu_factors(self._h, *[_ptr(out[k]) for k in ("to", "lrowptr", "lcol", "urowptr", "ucol")],
                                                 *[_ptr(v) for v in vals]))
        return out

    def product_form(self):
        """what opmhip_config.half_product resolved to (opmhip_get_product_form)"""
        info = (C.c_int * 4)()
        self._check(lib().opmhip_get_product_form(self._h, C.byref(info)))
        return {"half_product": bool(info[0]), "u_is_upper_a": bool(info[1]), "rest_blocks": int(info[2]), "rest_positions": int(info[3])}

    def split_assembly(self, rest=False, matrix=False):
        """opmhip_get_split_assembly: whether opmhip_assemble writes the Jacobian into the arrays the ILU0 solve reads, and how often it did;
        rest / matrix: also the matrix beside its U part (internal order, blocks [nr, 3, 3]) / the matrix in force (natural order, nnzb * 9)"""
        info = (C.c_longlong * 4)()
        r = np.empty((self.product_form()["rest_blocks"], 3, 3)) if rest else None
        m = np.empty(9 * self.nnzb) if matrix else None
        self._check(lib().opmhip_get_split_assembly(self._h, C.byref(info), _ptr(r), _ptr(m)))
        out = {"on": bool(info[0]), "stale": bool(info[1]), "assemblies": int(info[2]), "gathers": int(info[3])}
        if rest:
            out["rest"] = r
        if matrix:
            out["matrix"] = m
        return out

    PROF = ["spmv", "ilu_apply", "ilu_factor", "vector", "assemble", "iq_update", "convergence", "cpr_amg", "spmv_boundary",
            "halo", "allreduce", "cpr_gather"]   # the last three: communication spans of decomposed runs (they overlap the kernel scopes)

    def profile_enable(self, on=True):
        self._check(lib().opmhip_profile_enable(self._h, int(on)))

    def profile(self):
        """-> {class: (launches, total_ms)} from HIP events on the context's stream"""
        out = {}
        for i, name in enumerate(self.PROF):
            n, ms = C.c_longlong(0), C.c_double(0.0)
            self._check(lib().opmhip_profile_get(self._h, i, C.byref(n), C.byref(ms)))
            out[name] = (n.value, ms.value)
        return out

    def cpr_levels(self):
        """(unknowns, entries) of the pressure-AMG levels (preconditioner="cpr", after the first solve)"""
        n, nnz = np.zeros(32, np.int32), np.zeros(32, np.int32)
        L = self._check(lib().opmhip_cpr_levels(self._h, _ptr(n), _ptr(nnz), 32))
        return [int(v) for v in n[:L]], [int(v) for v in nnz[:L]]

    def synchronize(self):
        """everything enqueued on the context's stream is done"""
        self._check(lib().opmhip_synchronize(self._h))

    def comm_info(self):
        """what the communicator itself reports: dict(nranks = ncclCommCount, rank, device, kind)"""
        a = np.zeros(4, np.int32)
        self._check(lib().opmhip_comm_info(self._h, _ptr(a)))
        return {"nranks": int(a[0]), "rank": int(a[1]), "device": int(a[2]), "kind": ["none", "loopback", "rccl"][int(a[3])]}

    def comm_selftest(self):
        """one RCCL all-reduce of (1 + rank, 2): -> (sum over ranks of 1 + rank, 2 * nranks)"""
        a = np.zeros(2)
        self._check(lib().opmhip_comm_selftest(self._h, _ptr(a)))
        return float(a[0]), float(a[1])

    def time_kernel(self, which, reps=20):
        ms = C.c_double()
        self._check(lib().opmhip_time_kernel(self._h, {"spmv": 0, "ilu_apply": 1, "ilu_factor": 2, "vector": 3, "stream_read": 4, "spmv_dot1": 5, "spmv_dot2": 6,
                                                              "rest_product": 7, "rest_product_dot2": 8, "ilu_apply_rowsums": 9}[which],
                                             reps, C.byref(ms)))
        return ms.value


def comm_unique_id():
    """128-byte RCCL unique id (rank 0 creates it, the launcher broadcasts it)."""
    L = lib()
    if not getattr(L, "_asm_bound", False):
        _bind_assembly(L)
        L._asm_bound = True
    buf = C.create_string_buffer(128)
    rc = L.opmhip_comm_unique_id(buf)
    if rc != SUCCESS:
        raise OpmHipError(rc, "opmhip_comm_unique_id failed (librccl not loadable?)")
    return buf.raw


def _bind_assembly(L):
    vp = C.c_void_p
    L.opmhip_set_fluid.argtypes = [vp, vp]
    L.opmhip_set_static.argtypes = [vp] + [vp] * 9
    L.opmhip_set_state.argtypes = [vp, vp, vp]
    L.opmhip_get_state.argtypes = [vp, vp, vp]
    L.opmhip_advance_time_level.argtypes = [vp]
    L.opmhip_update_failed.argtypes = [vp]
    L.opmhip_end_time_step.argtypes = [vp, C.c_double]
    L.opmhip_set_drift_compensation.argtypes = [vp, C.c_int, C.c_double]
    L.opmhip_set_source.argtypes = [vp, vp, vp]
    L.opmhip_assemble.argtypes = [vp, C.c_double, C.c_int, vp, vp]
    L.opmhip_get_iq.argtypes = [vp, vp]
    L.opmhip_get_iq_cells.argtypes = [vp, C.c_int, vp, vp]
    L.opmhip_set_source_cells.argtypes = [vp, C.c_int, vp, vp, vp]
    L.opmhip_convergence.argtypes = [vp, C.c_double, C.c_double, vp]
    L.opmhip_update.argtypes = [vp, vp, C.c_double, C.POINTER(C.c_int)]
    L.opmhip_reservoir_averages.argtypes = [vp, vp]
    L.opmhip_set_fip_regions.argtypes = [vp, C.c_int, vp]
    L.opmhip_fluid_in_place.argtypes = [vp, C.c_int, vp, vp]
    L.opmhip_get_fluid_in_place_initial.argtypes = [vp, C.c_int, vp, vp]
    L.opmhip_get_fluid_in_place_cells.argtypes = [vp, vp]
    L.opmhip_get_fip_info.argtypes = [vp, C.c_int, vp]
    L.opmhip_get_fip_timings.argtypes = [vp, vp]
    L.opmhip_set_pattern_dd.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.opmhip_comm_unique_id.argtypes = [C.c_char_p]
    L.opmhip_comm_init_rccl.argtypes = [vp, C.c_int, C.c_int, C.c_char_p]
    L.opmhip_comm_init_loopback.argtypes = [vp, C.c_int, C.c_int, C.c_char_p]
    L.opmhip_set_halo.argtypes = [vp, C.c_longlong, C.c_int, vp, vp, vp, vp]
    L.opmhip_set_cell_global_ids.argtypes = [vp, vp]
    L.opmhip_fluid_probe.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.opmhip_set_problem_extras.argtypes = [vp, vp, vp, vp]
    L.opmhip_set_pcw.argtypes = [vp, vp]
    L.opmhip_set_endpoint_scaling.argtypes = [vp, vp]
    L.opmhip_set_composition_change_limits.argtypes = [vp, vp, vp, vp]
    L.opmhip_set_irreversible_compaction.argtypes = [vp, C.c_int]
    L.opmhip_begin_time_step.argtypes = [vp, C.c_double]
    L.opmhip_get_trackers.argtypes = [vp, vp, vp, vp, vp]
    L.opmhip_set_vappars.argtypes = [vp, C.c_int, C.c_double, C.c_double]
    L.opmhip_set_water_compaction.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.opmhip_get_max_water_saturation.argtypes = [vp, vp]
    L.opmhip_relative_change.argtypes = [vp, C.POINTER(C.c_double)]
    L.opmhip_sat_end_points.argtypes = [vp, C.c_int, vp]
    L.opmhip_sat_probe.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp]
    L.opmhip_gas_probe.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
    L.opmhip_iq_fields.argtypes = [vp]
    L.opmhip_set_hysteresis.argtypes = [vp, C.c_int, vp, vp]
    L.opmhip_get_hysteresis.argtypes = [vp, vp, vp, vp, vp]
    L.opmhip_set_hysteresis_params.argtypes = [vp, vp, vp]
    L.opmhip_set_aquifers.argtypes = [vp, C.POINTER(Aquifers)]
    L.opmhip_aquifers_begin_time_step.argtypes = [vp, C.c_double, C.c_double]
    L.opmhip_get_aquifers.argtypes = [vp, vp, vp, vp, vp]
    L.opmhip_get_aquifer_rates.argtypes = [vp, vp]
    L.opmhip_set_boundary_conditions.argtypes = [vp, C.POINTER(BoundaryConditions)]
    L.opmhip_get_boundary_rates.argtypes = [vp, vp]
    L.opmhip_set_tracers.argtypes = [vp, C.c_int, vp, vp]
    L.opmhip_set_tracer_solver.argtypes = [vp, C.c_double, C.c_int]
    L.opmhip_set_tracer_connections.argtypes = [vp, C.c_int, vp, vp, vp]
    L.opmhip_tracers_begin_time_step.argtypes = [vp]
    L.opmhip_tracers_end_time_step.argtypes = [vp, C.c_double, C.POINTER(TracerResult)]
    L.opmhip_get_tracers.argtypes = [vp, vp]
    L.opmhip_get_tracer_system.argtypes = [vp, C.c_int, C.c_double, vp, vp]
    L.opmhip_get_tracer_storage.argtypes = [vp, vp, vp]
    L.opmhip_get_tracer_timings.argtypes = [vp, vp, vp]
    L.opmhip_set_std_wells.argtypes = [vp, C.POINTER(StdWells)]
    L.opmhip_std_wells_begin_iteration.argtypes = [vp, C.c_int]
    L.opmhip_std_wells_apply_residual.argtypes = [vp]
    L.opmhip_std_wells_update.argtypes = [vp, C.c_double]
    L.opmhip_get_std_wells.argtypes = [vp, vp, vp, vp]
    L.opmhip_set_std_wells_state.argtypes = [vp, vp, vp, vp]
    L.opmhip_get_std_wells_blocks.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.opmhip_set_std_wells_head_model.argtypes = [vp, C.POINTER(StdWellsWellbore)]
    L.opmhip_get_std_wells_wellbore.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int)]
    L.opmhip_set_std_wells_perf_state.argtypes = [vp, vp, vp]
    L.opmhip_set_std_wells_crossflow.argtypes = [vp, vp]
    L.opmhip_get_std_wells_rate_dq.argtypes = [vp, vp]
    L.opmhip_set_std_wells_vaporised_oil.argtypes = [vp, C.c_int]
    L.opmhip_get_std_wells_solution_rates.argtypes = [vp, vp, vp]
    L.opmhip_set_std_wells_thp.argtypes = [vp, C.POINTER(StdWellsThp)]
    L.opmhip_get_std_wells_thp.argtypes = [vp, vp, vp, vp]
    L.opmhip_set_std_wells_limits.argtypes = [vp, C.POINTER(StdWellsLimits)]
    L.opmhip_get_std_wells_resv.argtypes = [vp, vp, vp, vp]
    L.opmhip_set_std_wells_groups.argtypes = [vp, C.POINTER(StdWellsGroups)]
    L.opmhip_set_std_wells_guide_rates.argtypes = [vp, vp]
    L.opmhip_set_std_wells_group_targets.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.opmhip_get_std_wells_groups.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.opmhip_set_std_wells_matrix_add.argtypes = [vp, C.c_int]
    L.opmhip_std_wells_add_to_matrix.argtypes = [vp]
    L.opmhip_get_std_wells_matrix_add.argtypes = [vp, vp]


class HipFluid(HipSolver):
    """A context that only holds the fluid tables: point evaluation of the device's property functions
    (opmhip_fluid_probe) for host-side setup such as equilibration (equil.py)."""

    COLUMNS = ("invBw", "invBg", "invBo", "rsSat", "pcow", "pcgo", "muo", "mug")

    def __init__(self, fluid, **solver_kw):
        super().__init__(**solver_kw)
        L = lib()
        if not getattr(L, "_asm_bound", False):
            _bind_assembly(L)
            L._asm_bound = True
        self.fluid = fluid
        self._fd = fluid.desc()
        self._check(L.opmhip_set_fluid(self._h, C.addressof(self._fd)))

    def probe(self, p, rs=0.0, sw=0.0, sg=0.0, pvt_region=0, sat_region=0):
        """-> array (n, 8): 1/B_w(p), 1/B_g(p), 1/B_o(p, rs), RsSat(p), pcow(sw), pcgo(sg), mu_o(p, rs), mu_g(p)"""
        p = np.atleast_1d(np.asarray(p, np.float64))
        n = len(p)
        a = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (n,))) for v in (p, rs, sw, sg)]
        out = np.empty((n, 8))
        self._check(lib().opmhip_fluid_probe(self._h, pvt_region, sat_region, n, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), _ptr(out)))
        return out


def _probe_gas(self, p, rv=0.0, pvt_region=0):
    """-> array (n, 3): 1/B_g(p, rv) and mu_g(p, rv) (saturated curve where rv >= RvSat(p)), RvSat(p)"""
    p = np.atleast_1d(np.asarray(p, np.float64))
    n = len(p)
    a = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (n,))) for v in (p, rv)]
    out = np.empty((n, 3))
    self._check(lib().opmhip_gas_probe(self._h, pvt_region, n, _ptr(a[0]), _ptr(a[1]), _ptr(out)))
    return out


HipFluid.probe_gas = _probe_gas


def _sat_end_points(self, sat_region=0):
    """the end points of a saturation region's own tables: dict over capi.EPS_FIELDS (opmhip_sat_end_points)"""
    out = np.empty(18)
    self._check(lib().opmhip_sat_end_points(self._h, sat_region, _ptr(out)))
    return dict(zip(EPS_FIELDS, out.tolist()))


HipFluid.sat_end_points = _sat_end_points


def _sat_probe(self, sw, sg, endscale=None, sat_region=0):
    """(n, 5): krw, kro, krg, pcow, pcgo at (sw, sg); endscale: dict(sat_scaling, three_point_kr, krw, kro, krg, pcw, pcg and any
    of EPS_FIELDS as ONE value each; absent = the table's own end point) or None = unscaled"""
    sw = np.atleast_1d(np.asarray(sw, np.float64))
    n = len(sw)
    sw = np.ascontiguousarray(sw)
    sg = np.ascontiguousarray(np.broadcast_to(np.asarray(sg, np.float64), (n,)))
    out = np.empty(5 * n)
    if endscale is None:
        self._check(lib().opmhip_sat_probe(self._h, sat_region, None, n, _ptr(sw), _ptr(sg), _ptr(out)))
    else:
        es = {k: (np.array([v], np.float64) if k in EPS_FIELDS else v) for k, v in endscale.items()}
        s, keep = endpoint_scaling_struct(es)
        self._check(lib().opmhip_sat_probe(self._h, sat_region, C.byref(s), n, _ptr(sw), _ptr(sg), _ptr(out)))
    return out.reshape(n, 5)


HipFluid.sat_probe = _sat_probe


class HipModel(HipSolver):
    """One context holding the whole per-Newton-iteration path on the device: the call surface follows
    BlackoilModelEbos (assembleReservoir -> getReservoirConvergence -> solveJacobianSystem -> updateSolution,
    opm/simulators/flow/BlackoilModelEbos.hpp:274-392) with every array resident in HBM between the calls."""

    def __init__(self, case, comm=None, **solver_kw):
        """comm (decomposed runs; case from ras.cartesian_subdomain_case / ras.local_problem):
        ("rccl", nranks, rank, id128) or ("loopback", nranks, rank, group_name)."""
        super().__init__(**solver_kw)
        L = lib()
        if not getattr(L, "_asm_bound", False):
            _bind_assembly(L)
            L._asm_bound = True
        self.case = case
        self.Nghost = int(case.get("Nghost", 0))
        if self.Nghost or comm:
            rows, cols = _i32(case["rowptr"]), _i32(case["col"])
            self._check(L.opmhip_set_pattern_dd(self._h, case["Nb"], self.Nghost, len(cols), _ptr(rows), _ptr(cols)))
            self.Nb, self.nnzb = case["Nb"], len(cols)
            if case.get("gids") is not None:
                g64 = np.ascontiguousarray(case["gids"], np.int64)
                self._check(L.opmhip_set_cell_global_ids(self._h, _ptr(g64)))
            if comm:
                kind, nranks, rank, tok = comm
                if kind == "rccl":
                    self._check(L.opmhip_comm_init_rccl(self._h, nranks, rank, tok))
                else:
                    self._check(L.opmhip_comm_init_loopback(self._h, nranks, rank, tok.encode()))
                h = case["halo"]
                keep = [_i32(h["neigh"]), _i32(h["send_ptr"]), _i32(h["send_cells"]), _i32(h["recv_ptr"])]
                self._check(L.opmhip_set_halo(self._h, int(case["global_cells"]), len(keep[0]), *[_ptr(k) for k in keep]))
        else:
            self.set_pattern(case["Nb"], case["rowptr"], case["col"])
        self.Nloc = self.Nb + self.Nghost
        self._fd = case["fluid"].desc()
        self._check(L.opmhip_set_fluid(self._h, C.addressof(self._fd)))
        g = lambda k, f: _ptr(f(case[k])) if case.get(k) is not None else None
        keep = {k: (_f64(case[k]) if k not in ("pvtnum", "satnum") else _i32(case[k]))
                for k in ("trans", "area", "thpres", "poro", "volume", "depth", "pvtnum", "satnum", "rsmax")
                if case.get(k) is not None}
        p = lambda k: _ptr(keep.get(k))
        self._check(L.opmhip_set_static(self._h, p("trans"), p("area"), p("thpres"), p("poro"), p("volume"), p("depth"),
                                        p("pvtnum"), p("satnum"), p("rsmax")))
        if any(case.get(k) is not None for k in ("rvmax", "rocknum", "overburden")):
            self.set_problem_extras(case.get("rvmax"), case.get("rocknum"), case.get("overburden"))
        if case.get("pcw") is not None:
            self.set_pcw(case["pcw"])
        if case.get("endscale") is not None:
            self.set_endpoint_scaling(case["endscale"])

    def set_endpoint_scaling(self, es):
        """saturation end-point scaling (ENDSCALE family): es = dict(sat_scaling, three_point_kr, krw, kro, krg, pcw, pcg and any
        of capi.EPS_FIELDS as per-cell arrays; absent = the end point of the cell's SATNUM tables); None = off.  The fluid needs
        pc_scaling=True."""
        if es is None:
            self._check(lib().opmhip_set_endpoint_scaling(self._h, None))
            return
        s, keep = endpoint_scaling_struct(es)
        self._check(lib().opmhip_set_endpoint_scaling(self._h, C.byref(s)))

    def set_hysteresis(self, kr_model, imbnum=None, imb_endscale=None):
        """relative-permeability hysteresis (SATOPTS HYSTER): kr_model = EHYSTR item 2 (0 | 1; None / negative = off), imbnum = per
        cell imbibition saturation region (0-based), imb_endscale = dict of per-cell scaled end points of the imbibition curves (any
        of capi.EPS_FIELDS, absent = the imbibition tables' own; only with set_endpoint_scaling in force)"""
        if kr_model is None or kr_model < 0:
            self._check(lib().opmhip_set_hysteresis(self._h, -1, None, None))
            return
        imb = _i32(imbnum)
        if imb_endscale is None:
            self._check(lib().opmhip_set_hysteresis(self._h, int(kr_model), _ptr(imb), None))
            return
        s, keep = endpoint_scaling_struct(imb_endscale)
        self._check(lib().opmhip_set_hysteresis(self._h, int(kr_model), _ptr(imb), C.byref(s)))

    def hysteresis(self):
        """(krnSwMdc, deltaSwImbKrn) of the oil-water system, then of the gas-oil system: four per-cell arrays (natural order)"""
        out = [np.empty(self.Nloc) for _ in range(4)]
        self._check(lib().opmhip_get_hysteresis(self._h, *[_ptr(a) for a in out]))
        return tuple(a[:self.Nb] for a in out) if self.Nghost == 0 else tuple(out)

    def set_hysteresis_params(self, sw_ow, sw_go):
        a, b = _f64(sw_ow), _f64(sw_go)
        self._check(lib().opmhip_set_hysteresis_params(self._h, _ptr(a), _ptr(b)))

    def set_pcw(self, pcw):
        """per-cell scaled maximum of the oil-water capillary pressure (PCW, or SWATINIT through equil.equilibrate's pcw_scale
        x the table's pcow(Swl)); None = the tables' own.  The fluid needs pc_scaling=True."""
        a = _f64(pcw)
        self._check(lib().opmhip_set_pcw(self._h, _ptr(a)))

    def set_problem_extras(self, rvmax=None, rocknum=None, overburden=None):
        """DRVDT cap on Rv, rock-table index (ROCKNUM), overburden pressure - per cell, any None"""
        a, b, d = _f64(rvmax), _i32(rocknum), _f64(overburden)
        self._check(lib().opmhip_set_problem_extras(self._h, _ptr(a), _ptr(b), _ptr(d)))

    def set_state(self, pv, meaning):
        pv, meaning = _f64(pv), np.ascontiguousarray(meaning, np.uint8)
        self._check(lib().opmhip_set_state(self._h, _ptr(pv), _ptr(meaning)))

    def get_state(self):
        pv = np.empty(3 * self.Nloc)
        m = np.empty(self.Nloc, np.uint8)
        self._check(lib().opmhip_get_state(self._h, _ptr(pv), _ptr(m)))
        return pv, m

    def advance_time_level(self):
        """solution(1) = solution(0): call when a time step starts (FvBaseDiscretization::advanceTimeLevel)."""
        self._check(lib().opmhip_advance_time_level(self._h))

    def update_failed(self):
        """solution(0) = solution(1) + intensive quantities: the Newton method gave up on this time step."""
        self._check(lib().opmhip_update_failed(self._h))

    def relative_change(self):
        """BlackoilModelEbos::relativeChange: squared change of pressure and saturations since advance_time_level over their
        squared new values (the PID time-step control's error measure); summed over the ranks of a decomposed run."""
        out = C.c_double(0.0)
        self._check(lib().opmhip_relative_change(self._h, C.byref(out)))
        return out.value

    def set_composition_change_limits(self, drsdt=None, drsdt_all_cells=None, drvdt=None):
        """DRSDT / DRVDT: rates per PVT region [1/s] (negative: none), None = keyword not in force; drsdt_all_cells: the OILVAP
        option per region.  After set_state (lastRs / lastRv start from the state now present)."""
        a, b, d = _f64(drsdt), _i32(drsdt_all_cells), _f64(drvdt)
        self._check(lib().opmhip_set_composition_change_limits(self._h, _ptr(a), _ptr(b), _ptr(d)))

    def set_irreversible_compaction(self, enable=True):
        """ROCKCOMP IRREVERS: rock tables read at the lowest oil pressure a cell has seen.  After set_state."""
        self._check(lib().opmhip_set_irreversible_compaction(self._h, int(enable)))

    def begin_time_step(self, dt):
        """EclProblem::beginTimeStep, per-cell part: minimum pressure, DRSDT / DRVDT caps of a step of size dt"""
        self._check(lib().opmhip_begin_time_step(self._h, dt))

    def set_vappars(self, vap1, vap2, enable=True):
        """VAPPARS: exponents on the saturated Rv / Rs below the largest oil saturation seen.  After set_state."""
        self._check(lib().opmhip_set_vappars(self._h, int(enable), float(vap1), float(vap2)))

    def set_water_compaction(self, tables):
        """Water-induced rock compaction (ROCK2D / ROCK2DTR / ROCKWNOD): one dict per rock region with "pressure" [Pa] and "sw"
        nodes (ascending), "pv_mult" [len(pressure) x len(sw)] and optionally "trans_mult" of the same shape (all tables or
        none).  None / []: off.  After set_state."""
        tables = list(tables or [])
        if not tables:
            self._check(lib().opmhip_set_water_compaction(self._h, 0, None, None, None, None, None, None))
            return
        npv = _i32([len(t["pressure"]) for t in tables])
        nsw = _i32([len(t["sw"]) for t in tables])
        pr = _f64(np.concatenate([np.asarray(t["pressure"], float) for t in tables]))
        sw = _f64(np.concatenate([np.asarray(t["sw"], float) for t in tables]))
        shaped = lambda t, k: np.asarray(t[k], float).reshape(len(t["pressure"]), len(t["sw"])).ravel()
        pv = _f64(np.concatenate([shaped(t, "pv_mult") for t in tables]))
        has_tr = [t.get("trans_mult") is not None for t in tables]
        if any(has_tr) and not all(has_tr):
            raise ValueError("set_water_compaction: trans_mult for all tables or for none")
        tr = _f64(np.concatenate([shaped(t, "trans_mult") for t in tables])) if all(has_tr) else None
        self._check(lib().opmhip_set_water_compaction(self._h, len(tables), _ptr(npv), _ptr(nsw), _ptr(pr), _ptr(sw), _ptr(pv), _ptr(tr) if tr is not None else None))

    def max_water_saturation(self):
        """the tracker of the water-induced compaction per cell, natural order (zeros when the feature is off)"""
        a = np.empty(self.Nloc)
        self._check(lib().opmhip_get_max_water_saturation(self._h, _ptr(a)))
        return a

    def trackers(self):
        """-> (lastRs, lastRv, minimum oil pressure, maximum oil saturation) per cell, natural order; zeros where not kept"""
        a, b, d, e = (np.empty(self.Nloc) for _ in range(4))
        self._check(lib().opmhip_get_trackers(self._h, _ptr(a), _ptr(b), _ptr(d), _ptr(e)))
        return a, b, d, e

    def end_time_step(self, dt):
        """EclProblem::endTimeStep (drift part): remember residual * dt of the time step that was just accepted."""
        self._check(lib().opmhip_end_time_step(self._h, dt))

    def set_drift_compensation(self, enable=True, max_compensation=0.1):
        self._check(lib().opmhip_set_drift_compensation(self._h, int(enable), max_compensation))

    def set_aquifers(self, aquifers):
        """opmhip_set_aquifers: the analytic aquifers (list of dicts, see make_aquifers) on the device, initialised from the state now
        present; None or an empty list clears them"""
        aq, keep = make_aquifers(aquifers)
        self._naq = self._naqconn = 0      # a refused call leaves no list set
        self._check(lib().opmhip_set_aquifers(self._h, C.byref(aq) if aq else None))
        if aq:
            self._naq, self._naqconn = aq.num_aquifers, len(keep["cell"])

    def aquifers_begin_time_step(self, time, dt):
        """opmhip_aquifers_begin_time_step: pressure_previous_ and the step's scalars; beside begin_time_step, before every retry too"""
        self._check(lib().opmhip_aquifers_begin_time_step(self._h, float(time), float(dt)))

    def get_aquifers(self):
        """aquiferData() per aquifer: dict(W_flux, pressure, flux_rate, init_pressure) of arrays"""
        n = getattr(self, "_naq", 0)
        out = {k: np.zeros(n) for k in ("W_flux", "pressure", "flux_rate", "init_pressure")}
        self._check(lib().opmhip_get_aquifers(self._h, *[_ptr(out[k]) for k in ("W_flux", "pressure", "flux_rate", "init_pressure")]))
        return out

    def aquifer_rates(self):
        """Qai_ of the last assemble per connection: (connections, 4) = value, d/dSw, d/dp, d/dX"""
        q = np.zeros((getattr(self, "_naqconn", 0), 4))
        self._check(lib().opmhip_get_aquifer_rates(self._h, _ptr(q)))
        return q

    def set_boundary_conditions(self, records):
        """opmhip_set_boundary_conditions: the FREE and RATE faces (list of boundary.free / boundary.rate records, see
        make_boundary_conditions) on the device; the exterior state of the FREE faces is the state now present.  None or an empty list
        clears them"""
        bc, keep = make_boundary_conditions(records)
        self._nbcfaces = 0      # a refused call leaves no list set
        self._check(lib().opmhip_set_boundary_conditions(self._h, C.byref(bc) if bc else None))
        if bc:
            self._nbcfaces = bc.num_faces

    def boundary_rates(self):
        """the last assemble's contribution of every face to its cell's residual, positive out of the cell: (faces, 12) = the three equations
        (oil, water, gas), then their 3 x 3 derivative, row by row"""
        q = np.zeros((getattr(self, "_nbcfaces", 0), 12))
        self._check(lib().opmhip_get_boundary_rates(self._h, _ptr(q)))
        return q

    def _check(self, rc):
        """(a singular D reported by opmhip_get_std_wells / opmhip_solve_system clears the resident list: the sizes kept here follow.
        The words looked for are those of std_wells_check's message in csrc/capi_std_wells.cpp: change both together)"""
        try:
            return HipSolver._check(self, rc)
        except OpmHipError as e:
            if "std_wells" in str(e) and "the list is cleared" in str(e):
                self._nsw = self._nswperf = 0
            raise

    def set_std_wells(self, wells):
        """opmhip_set_std_wells: the standard wells (dict, see make_std_wells) on the device; None clears them"""
        sw, keep = make_std_wells(wells)
        self._nsw = self._nswperf = 0      # a refused call leaves no list set
        self._nswgroups = 0                # replacing the list clears its groups
        self._check(lib().opmhip_set_std_wells(self._h, C.byref(sw) if sw else None))
        if sw:
            self._nsw, self._nswperf = sw.num_wells, len(keep["cell"])

    def set_std_wells_head_model(self, wellbore):
        """opmhip_set_std_wells_head_model: the heads from the well-bore density (dict, see make_std_wells_wellbore); None: back to the
        perforated cell's oil density.  A refused call leaves the model as it was."""
        wb, keep = make_std_wells_wellbore(wellbore, getattr(self, "_nsw", 0), getattr(self, "_nswperf", 0))
        self._check(lib().opmhip_set_std_wells_head_model(self._h, C.byref(wb) if wb else None))

    def set_std_wells_crossflow(self, allow):
        """opmhip_set_std_wells_crossflow: per well 0 / 1 - reversed perforations of that producer inject the well bore's mixture; None or
        all zeros: off.  An injector with the switch is a ValueError; a refused call leaves the flags as they were."""
        a = _i32(allow)
        n = getattr(self, "_nsw", 0)
        if a is not None and a.size != n:
            raise ValueError("set_std_wells_crossflow: %d flags for the %d wells set" % (a.size, n))
        try:
            self._check(lib().opmhip_set_std_wells_crossflow(self._h, _ptr(a)))
        except OpmHipError as e:
            if e.code == INVALID_ARGUMENT and "injector" in str(e):
                raise ValueError(str(e)) from e
            raise

    def set_std_wells_thp(self, thp):
        """opmhip_set_std_wells_thp: the THP limits (dict, see make_std_wells_thp); None switches them off.  A refused call leaves the previous
        values in force."""
        t, keep = make_std_wells_thp(thp, getattr(self, "_nsw", 0))
        self._check(lib().opmhip_set_std_wells_thp(self._h, C.byref(t) if t else None))

    def std_wells_thp(self):
        """opmhip_get_std_wells_thp: dict(thp: what the last begin_iteration formed from the well's state, dp: this time step's hydrostatic
        correction, bhp_from_thp: V - dp of the last assemble) per well; zeros for wells without a limit"""
        n = getattr(self, "_nsw", 0)
        out = dict(thp=np.zeros(n), dp=np.zeros(n), bhp_from_thp=np.zeros(n))
        self._check(lib().opmhip_get_std_wells_thp(self._h, _ptr(out["thp"]), _ptr(out["dp"]), _ptr(out["bhp_from_thp"])))
        return out

    def set_std_wells_limits(self, limits):
        """opmhip_set_std_wells_limits: the further rate limits (dict, see make_std_wells_limits); None switches them off.  A refused call
        leaves the previous values in force."""
        t, keep = make_std_wells_limits(limits, getattr(self, "_nsw", 0))
        self._check(lib().opmhip_set_std_wells_limits(self._h, C.byref(t) if t else None))

    def std_wells_resv(self):
        """opmhip_get_std_wells_resv: dict(averages (5): the field's, as the last begin_iteration(0) with a RESV limit formed them; coeff
        (wells, 3): the RESV control equation's coefficients (oil, water, gas); resv_current: the voidage rate of the last controls pass)"""
        n = getattr(self, "_nsw", 0)
        out = dict(averages=np.zeros(5), coeff=np.zeros((n, 3)), resv_current=np.zeros(n))
        self._check(lib().opmhip_get_std_wells_resv(self._h, _ptr(out["averages"]), _ptr(out["coeff"]), _ptr(out["resv_current"])))
        return out

    def set_std_wells_groups(self, groups):
        """opmhip_set_std_wells_groups: group production control (dict, see make_std_wells_groups); None clears.  A refused call leaves the
        previous values in force."""
        t, keep = make_std_wells_groups(groups, getattr(self, "_nsw", 0))
        self._check(lib().opmhip_set_std_wells_groups(self._h, C.byref(t) if t else None))
        self._nswgroups = 0 if t is None else int(t.num_groups)

    def set_std_wells_guide_rates(self, guide_rate):
        """opmhip_set_std_wells_guide_rates: (wells, 5) - ORAT, WRAT, GRAT, LRAT, RESV per well"""
        g = _f64(np.asarray(guide_rate, float).reshape(-1))
        if g.size != 5 * getattr(self, "_nsw", 0):
            raise ValueError("set_std_wells_guide_rates: %d entries for the %d wells set" % (g.size, getattr(self, "_nsw", 0)))
        self._check(lib().opmhip_set_std_wells_guide_rates(self._h, _ptr(g)))

    def set_std_wells_group_targets(self, oil=None, water=None, gas=None, liquid=None, resv=None, mode=None):
        """opmhip_set_std_wells_group_targets: per group; None = that kind (the modes) stays"""
        ng = getattr(self, "_nswgroups", 0)
        a = [_f64(v) for v in (oil, water, gas, liquid, resv)] + [_i32(mode)]
        if any(v is not None and v.size != ng for v in a):
            raise ValueError("set_std_wells_group_targets: array lengths do not fit the %d groups set" % ng)
        self._check(lib().opmhip_set_std_wells_group_targets(self._h, *[_ptr(v) for v in a]))

    def std_wells_groups(self):
        """opmhip_get_std_wells_groups: dict(mode, rates (groups, 3), voidage, reduction (groups, 3), guide_sum per group as the last group
        data left them, nupcol_rates (wells, 3))"""
        ng, n = getattr(self, "_nswgroups", 0), getattr(self, "_nsw", 0)
        out = dict(mode=np.zeros(ng, np.int32), rates=np.zeros((ng, 3)), voidage=np.zeros(ng), reduction=np.zeros((ng, 3)), guide_sum=np.zeros(ng),
                   nupcol_rates=np.zeros((n, 3)))
        self._check(lib().opmhip_get_std_wells_groups(self._h, *[_ptr(out[k]) for k in ("mode", "rates", "voidage", "reduction", "guide_sum", "nupcol_rates")]))
        return out

    def set_std_wells_vaporised_oil(self, on=True):
        """opmhip_set_std_wells_vaporised_oil: the wet-gas rate model of the resident list - the oil the produced gas carries counts as oil.
        A context whose fluid has no PVTG is a ValueError; a refused call leaves the switch as it was."""
        try:
            self._check(lib().opmhip_set_std_wells_vaporised_oil(self._h, int(on)))
        except OpmHipError as e:
            if e.code == INVALID_ARGUMENT and "no PVTG" in str(e):
                raise ValueError(str(e)) from e
            raise

    def set_std_wells_matrix_add(self, on=True):
        """opmhip_set_std_wells_matrix_add: the resident list goes into the Jacobian (opmhip_std_wells_add_to_matrix) instead of reaching the
        solver as an operator.  The context's pattern must hold every pair of a well's perforated cells (grid.with_well_cliques): a missing
        block is a ValueError with the library's text; a refused call leaves the switch as it was."""
        try:
            self._check(lib().opmhip_set_std_wells_matrix_add(self._h, int(on)))
        except OpmHipError as e:
            if e.code == INVALID_ARGUMENT and "not in the pattern" in str(e):
                raise ValueError(str(e)) from e
            raise

    def std_wells_add_to_matrix(self):
        """opmhip_std_wells_add_to_matrix: A -= C^T D^-1 B with the resident blocks of the last assemble, once per assemble (asynchronous)"""
        self._check(lib().opmhip_std_wells_add_to_matrix(self._h))

    def std_wells_matrix_add_info(self):
        """opmhip_get_std_wells_matrix_add: dict(on, targets: distinct blocks written, pairs: contributions, in_matrix: the last assemble's
        wells are in the matrix)"""
        a = np.zeros(4, np.int32)
        self._check(lib().opmhip_get_std_wells_matrix_add(self._h, _ptr(a)))
        return dict(on=bool(a[0]), targets=int(a[1]), pairs=int(a[2]), in_matrix=bool(a[3]))

    def std_wells_solution_rates(self):
        """opmhip_get_std_wells_solution_rates: (dissolved_gas, vaporised_oil) per well of the last assemble - rates into the reservoir,
        production negative; zeros for injectors and with the switch off"""
        n = getattr(self, "_nsw", 0)
        dis, vap = np.zeros(n), np.zeros(n)
        self._check(lib().opmhip_get_std_wells_solution_rates(self._h, _ptr(dis), _ptr(vap)))
        return dis, vap

    def std_wells_rate_dq(self):
        """for tests: d rate_c / d q_j of the last assemble, (perforations, 3 components, 3 rate unknowns); zeros without crossflow"""
        dq = np.zeros((getattr(self, "_nswperf", 0), 3, 3))
        self._check(lib().opmhip_get_std_wells_rate_dq(self._h, _ptr(dq)))
        return dq

    def std_wells_wellbore(self):
        """for tests and restart files: dict(density, p_avg, mixture (perforations, 3 components), perf_pressure, perf_rates (perforations, 3))
        as the last begin_iteration(0) / assemble left them - zeros without the model - and perf_state_set: whether the perforation
        pressures exist yet (the library's own flag: taken from the cells at the first begin_iteration(0) or handed in; update_failed goes
        back to what advance_time_level saw)"""
        p = getattr(self, "_nswperf", 0)
        out = dict(density=np.zeros(p), p_avg=np.zeros(p), mixture=np.zeros((p, 3)), perf_pressure=np.zeros(p), perf_rates=np.zeros((p, 3)))
        flag = C.c_int(0)
        self._check(lib().opmhip_get_std_wells_wellbore(self._h, *[_ptr(out[k]) for k in ("density", "p_avg", "mixture", "perf_pressure", "perf_rates")],
                                                        C.byref(flag)))
        out["perf_state_set"] = bool(flag.value)
        return out

    def set_std_wells_perf_state(self, perf_pressure=None, perf_rates=None):
        """opmhip_set_std_wells_perf_state: the perforation pressures and the stored component rates; None = that part stays"""
        pp, pr = _f64(perf_pressure), _f64(perf_rates)
        n = getattr(self, "_nswperf", 0)
        if (pp is not None and pp.size != n) or (pr is not None and pr.size != 3 * n):
            raise ValueError("set_std_wells_perf_state: array lengths do not fit the %d perforations set" % n)
        self._check(lib().opmhip_set_std_wells_perf_state(self._h, _ptr(pp), _ptr(pr)))

    def std_wells_begin_iteration(self, iteration):
        """opmhip_std_wells_begin_iteration: wellModel().beginIteration - at iteration 0 the heads and the wells alone, always the controls"""
        self._check(lib().opmhip_std_wells_begin_iteration(self._h, int(iteration)))

    def std_wells_apply_residual(self):
        """opmhip_std_wells_apply_residual: r -= C^T D^-1 r_w with the resident blocks of the last assemble"""
        self._check(lib().opmhip_std_wells_apply_residual(self._h))

    def std_wells_update(self, relax=1.0):
        """opmhip_std_wells_update: x_w = D^-1 (r_w - B x), well unknowns -= relax x_w, on the device"""
        self._check(lib().opmhip_std_wells_update(self._h, float(relax)))

    def get_std_wells(self):
        """the one read-back of a Newton iteration: (x (wells, 4), control (wells) 0 rate / 1 bhp / 2 thp / 3 - 7 orat, wrat, grat, lrat, resv /
        8 grup, r_w (wells, 4))"""
        n = getattr(self, "_nsw", 0)
        x, ctl, rw = np.zeros((n, 4)), np.zeros(n, np.int32), np.zeros((n, 4))
        self._check(lib().opmhip_get_std_wells(self._h, _ptr(x), _ptr(ctl), _ptr(rw)))
        return x, ctl, rw

    def set_std_wells_state(self, x=None, control=None, rate_target=None):
        """opmhip_set_std_wells_state: well unknowns, controls in force, rate targets; None = that part stays"""
        x, control, rate_target = _f64(x), _i32(control), _f64(rate_target)
        n = getattr(self, "_nsw", 0)
        if (x is not None and x.size != 4 * n) or (control is not None and control.size != n) or (rate_target is not None and rate_target.size != n):
            raise ValueError("set_std_wells_state: array lengths do not fit the %d wells set" % n)
        self._check(lib().opmhip_set_std_wells_state(self._h, _ptr(x), _ptr(control), _ptr(rate_target)))

    def std_wells_blocks(self):
        """for tests: dict(head, D, Dinv, B, C, rates, xw) as the last begin_iteration / assemble / update left them"""
        n, p = getattr(self, "_nsw", 0), getattr(self, "_nswperf", 0)
        out = dict(head=np.zeros(p), D=np.zeros((n, 4, 4)), Dinv=np.zeros((n, 4, 4)), B=np.zeros((p, 4, 3)), C=np.zeros((p, 4, 3)), rates=np.zeros((p, 3, 5)),
                   xw=np.zeros((n, 4)))
        self._check(lib().opmhip_get_std_wells_blocks(self._h, *[_ptr(out[k]) for k in ("head", "D", "Dinv", "B", "C", "rates", "xw")]))
        return out

    # ---- passive tracers (opmhip_set_tracers ...; tracers.DeviceTracers) ----
    def set_tracers(self, phase, concentration):
        """phase: per tracer 0 water, 1 oil, 2 gas; concentration (num_tracers, Nb), natural order; no tracers clears.  Ragged input raises
        ValueError; what the library refuses (a gas tracer, an oil tracer on a PVTG fluid, a decomposed context, a value that is not
        finite) raises OpmHipError with its text"""
        ph = _i32(np.asarray(phase).reshape(-1))
        nt = len(ph)
        cc = _f64(np.asarray(concentration, float).reshape(-1)) if nt else _f64(np.zeros(1))
        if nt and len(cc) != nt * self.Nb:
            raise ValueError("set_tracers: concentration needs num_tracers x Nb = %d x %d values, has %d" % (nt, self.Nb, len(cc)))
        self._ntracers = 0     # a refused call leaves none set
        self._check(lib().opmhip_set_tracers(self._h, nt, _ptr(ph) if nt else None, _ptr(cc) if nt else None))
        self._ntracers = nt

    def set_tracer_solver(self, tolerance=1e-2, maxit=100):
        self._check(lib().opmhip_set_tracer_solver(self._h, tolerance, maxit))

    def set_tracer_connections(self, cells, rates, injected):
        """cells [n]; rates [n, 3]: water, oil, gas component surface rates, positive into the reservoir; injected [num_tracers, n]"""
        cl = _i32(np.asarray(cells).reshape(-1))
        n, nt = len(cl), getattr(self, "_ntracers", 0)
        r, j = _f64(np.asarray(rates, float).reshape(-1)), _f64(np.asarray(injected, float).reshape(-1))
        if len(r) != 3 * n or len(j) != nt * n:
            raise ValueError("set_tracer_connections: %d cells need %d rates and %d injected concentrations, got %d and %d" % (n, 3 * n, nt * n, len(r), len(j)))
        self._check(lib().opmhip_set_tracer_connections(self._h, n, _ptr(cl) if n else None, _ptr(r) if n else None, _ptr(j) if n else None))

    def tracers_begin_time_step(self):
        self._check(lib().opmhip_tracers_begin_time_step(self._h))

    def tracers_end_time_step(self, dt):
        """-> per tracer dict(converged, iterations, reduction)"""
        nt = getattr(self, "_ntracers", 0)
        res = (TracerResult * max(nt, 1))()
        self._check(lib().opmhip_tracers_end_time_step(self._h, dt, res))
        return [dict(converged=bool(res[t].converged), iterations=res[t].iterations, reduction=res[t].reduction) for t in range(nt)]

    def get_tracers(self):
        out = np.zeros((getattr(self, "_ntracers", 0), self.Nb))
        self._check(lib().opmhip_get_tracers(self._h, _ptr(out)))
        return out

    def tracer_system(self, phase, dt, num_phase_tracers):
        """for tests: (M [nnzb] in the pattern's order, residual [tracers of the phase, Nb]) at the state now present"""
        M, r = np.zeros(self.nnzb), np.zeros((num_phase_tracers, self.Nb))
        self._check(lib().opmhip_get_tracer_system(self._h, phase, dt, _ptr(M), _ptr(r)))
        return M, r

    def tracer_storage(self):
        """for tests: (storage1, c_initial) of the last tracers_begin_time_step, (num_tracers, Nb) each"""
        nt = getattr(self, "_ntracers", 0)
        s, c0 = np.zeros((nt, self.Nb)), np.zeros((nt, self.Nb))
        self._check(lib().opmhip_get_tracer_storage(self._h, _ptr(s), _ptr(c0)))
        return s, c0

    def tracer_timings(self):
        """device milliseconds of the last tracers_end_time_step: dict(system, factor, solve, levels, launches)"""
        ms, info = np.zeros(3), np.zeros(2, np.int32)
        self._check(lib().opmhip_get_tracer_timings(self._h, _ptr(ms), _ptr(info)))
        return dict(system=ms[0], factor=ms[1], solve=ms[2], levels=int(info[0]), launches=int(info[1]))

    def set_source(self, source, dsource=None):
        s, d = _f64(source), _f64(dsource)
        self._check(lib().opmhip_set_source(self._h, _ptr(s), _ptr(d)))

    def set_source_cells(self, cells, source, dsource=None):
        """the source terms of the cells named (a well model's connection rates), zero everywhere else: opmhip_set_source_cells"""
        cl, s, d = _i32(cells), _f64(source), _f64(dsource)
        self._check(lib().opmhip_set_source_cells(self._h, len(cl), _ptr(cl), _ptr(s), _ptr(d)))

    def assemble(self, dt, iteration, fetch=True):
        """linearizeDomain(); with fetch the Jacobian values and residual are copied back (natural order)."""
        jac = np.empty(9 * self.nnzb) if fetch else None
        res = np.empty(3 * self.Nb) if fetch else None
        self._check(lib().opmhip_assemble(self._h, dt, iteration, _ptr(jac), _ptr(res)))
        return jac, res

    def iq(self):
        nf = self._check(lib().opmhip_iq_fields(self._h))
        out = np.empty(self.Nloc * nf * 4)
        self._check(lib().opmhip_get_iq(self._h, _ptr(out)))
        return out.reshape(self.Nloc, nf, 4)

    def iq_cells(self, cells):
        """the records of the cells named (a well model's perforated cells), gathered on the device: opmhip_get_iq_cells"""
        cl = _i32(cells)
        nf = self._check(lib().opmhip_iq_fields(self._h))
        out = np.empty(len(cl) * nf * 4)
        self._check(lib().opmhip_get_iq_cells(self._h, len(cl), _ptr(cl), _ptr(out)))
        return out.reshape(len(cl), nf, 4)

    def convergence(self, dt, tol_cnv=1e-2):
        out = np.empty(17)
        self._check(lib().opmhip_convergence(self._h, dt, tol_cnv, _ptr(out)))
        return out

    def reservoir_averages(self):
        """opmhip_reservoir_averages: (pressure, rs, rv, pv, 1.0 hydrocarbon weights | 0.0 pore-volume fallback) of the whole field at the
        state now present - RateConverter's defineState, what wells.reservoir_averages(iq, volume) forms by a sequential loop"""
        out = np.empty(5)
        self._check(lib().opmhip_reservoir_averages(self._h, _ptr(out)))
        return out

    # ---- fluids in place per FIP region (opmhip_set_fip_regions ...; fip.py states the arithmetic) ----
    def set_fip_regions(self, regions):
        """regions: {"FIPNUM": ids, "FIPABC": ids, ...}, Nb ids each in the natural cell order; the first name is set 0 ("the field's").
        None or {} releases.  Ragged input raises ValueError; what the library refuses (more than 16 sets, an id above Nb, a decomposed
        context) raises OpmHipError with its text and leaves the sets in force"""
        regions = dict(regions or {})
        keep = [_i32(np.asarray(v).reshape(-1)) for v in regions.values()]
        for name, a in zip(regions, keep):
            if len(a) != self.Nb:
                raise ValueError("set_fip_regions: %s needs Nb = %d ids, has %d" % (name, self.Nb, len(a)))
        ptrs = (C.c_void_p * max(len(keep), 1))(*[a.ctypes.data for a in keep])
        self._check(lib().opmhip_set_fip_regions(self._h, len(keep), ptrs if keep else None))
        self._fip_names = list(regions)

    def _fip_set(self, name):
        names = getattr(self, "_fip_names", [])
        if isinstance(name, str):
            if name not in names:
                raise KeyError("no region set %r (set: %s)" % (name, ", ".join(names) or "none"))
            return names.index(name)
        return int(name)

    def fip_info(self, name="FIPNUM"):
        """dict(max_id, cells, chunks, levels) of a set: its largest id, its cells in regions, its chunks at level 0, its levels"""
        info = np.zeros(4, np.int32)
        self._check(lib().opmhip_get_fip_info(self._h, self._fip_set(name), _ptr(info)))
        return dict(max_id=int(info[0]), cells=int(info[1]), chunks=int(info[2]), levels=int(info[3]))

    def _fip_rows(self, fn, name):
        s = self._fip_set(name)
        info = np.zeros(4, np.int32)
        if lib().opmhip_get_fip_info(self._h, s, _ptr(info)) != SUCCESS:
            info[:] = 0   # no such set: fn refuses below, with its own code and text
        reg, field = np.zeros((int(info[0]), 14)), np.zeros(14)
        self._check(fn(self._h, s, _ptr(reg), _ptr(field)))
        return dict(regions=reg, field=field)

    def fluid_in_place(self, name="FIPNUM"):
        """opmhip_fluid_in_place of one set (a name of set_fip_regions, or its number) at the state now present:
        dict(regions=(max_id, 14), field=(14,)) - the twelve sums in fip.TERMS' order, then RPR / FPR and RPRP / FPRP"""
        if not getattr(self, "_fip_names", []) and isinstance(name, str):
            name = 0   # the library's own status says that no regions are set
        return self._fip_rows(lib().opmhip_fluid_in_place, name)

    def fluid_in_place_initial(self, name="FIPNUM"):
        """the set's first fluid_in_place since set_fip_regions (initialInplace_): what FOE divides by"""
        return self._fip_rows(lib().opmhip_get_fluid_in_place_initial, name)

    def fluid_in_place_cells(self):
        """(12, Nb): the per-cell terms at the state now present, rows as fip.TERMS, natural cell order"""
        out = np.zeros((12, self.Nb))
        self._check(lib().opmhip_get_fluid_in_place_cells(self._h, _ptr(out)))
        return out

    def fip_timings(self):
        """device milliseconds of the last fluid_in_place: dict(cells, reduce)"""
        ms = np.zeros(2)
        self._check(lib().opmhip_get_fip_timings(self._h, _ptr(ms)))
        return dict(cells=float(ms[0]), reduce=float(ms[1]))

    def solve_jacobian_system(self, wells=None):
        """solveJacobianSystem on the device-resident Jacobian and residual (no host copies)."""
        res = Result()
        ws, keep = make_wells(wells)
        self._check(lib().opmhip_solve_system(self._h, 3 * self.Nb, 9 * self.nnzb, 3, None, None, None, None,
                                              C.byref(ws) if ws else None, C.byref(res)))
        return res

    def update(self, dx=None, relax=1.0):
        dx = _f64(dx)
        n = C.c_int(0)
        self._check(lib().opmhip_update(self._h, _ptr(dx), relax, C.byref(n)))
        return n.value
