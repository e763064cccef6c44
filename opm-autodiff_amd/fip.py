"""Fluids in place and region pressures per FIP region - the report Flow forms at every report step - in plain NumPy, on the records of
any model with iq() (capi.HipModel, the oracle binding): the comparator of the device's opmhip_fluid_in_place and the statement of
its arithmetic.

  the per-cell terms (ebos/ecloutputblackoilmodule.hh:610-697, updateFluidInPlace_), values only, in this order (TERMS):
      pv = volume * porosity(record)                   DynamicPoreVolume
      PoreVolume = volume * poro                       (the static, reference porosity)
      hc = S_o + S_g                                   (not 1 - S_w)
      HydroCarbonPV = pv * hc ; PressurePV = p_o * pv ; PressureHydroCarbonPV = PressurePV * hc
      fip_w = (b_w * S_w) * pv ; fip_o = (b_o * S_o) * pv ; fip_g = (b_g * S_g) * pv
      OilInLiquidPhase = fip_o ; GasInGasPhase = fip_g ; GasInLiquidPhase = Rs * fip_o ; OilInGasPhase = Rv * fip_g
      WATER = fip_w ; OIL = fip_o + OilInGasPhase ; GAS = fip_g + GasInLiquidPhase
  the region sums (ebos/eclgenericoutputblackoilmodule.cc:712-737 regionSum; :1412-1427 update): cells with an id <= 0 belong to no
  region and are left out everywhere, field totals included; a field total is the regions' totals added from 0.0 in ascending id; an id
  in 1 .. max that no cell carries gives zeros.  Two arithmetics:
      "sequential"  the reference's loop in cell order;
      "stated"      what the device computes, `reduce256`, applied per region to its cells in ascending natural index:
                    1. the list is cut into chunks of 256 consecutive items (the last may be ragged: a missing item counts as 0.0);
                    2. in a chunk, lane l of one wavefront forms (((0.0 + x[l]) + x[l + 64]) + x[l + 128]) + x[l + 192];
                    3. the 64 lanes are combined by the shuffle-down tree v[l] += v[l + o], o = 32, 16, ..., 1;
                    4. the chunk results, in ascending order, form a new list; the same rule again until one value is left.
                    Its order depends on the region array and the natural cell numbering alone - not on the ordering of a context, the
                    grid of a launch or the call.  On the device one wavefront works on one chunk, a lane carries the twelve
                    accumulators, every level is one launch of k_fip_reduce over descriptors the host prepared, and the field totals
                    are formed by one lane per term (k_fip_totals).
  the pressures (:1240-1250 pressureAverage_): hydrocarbon && HydroCarbonPV > 1e-10 ? PressureHydroCarbonPV / HydroCarbonPV :
  PressurePV / PoreVolume; a region without pore volume gives the reference's 0.0 / 0.0, a NaN.

A result ("inplace") is dict(regions=(max_id, 14), field=(14,)): the twelve sums, then the hydrocarbon-weighted (RPR / FPR) and the
pore-volume-weighted (RPRP / FPRP) pressure - what capi.HipModel.fluid_in_place() returns.
UNVERIFIED: Inplace::add(phase, sum) is opm-common's; whether Flow's field value accumulates over several region sets cannot be read in
the reference tree.  Here every set has field totals of its own."""
import numpy as np

TERMS = ("DynamicPoreVolume", "PoreVolume", "HydroCarbonPV", "PressurePV", "PressureHydroCarbonPV", "OilInLiquidPhase", "GasInGasPhase",
         "GasInLiquidPhase", "OilInGasPhase", "WATER", "OIL", "GAS")
T = {name: i for i, name in enumerate(TERMS)}
ROW = len(TERMS) + 2                       # + RPR, RPRP
HC_PRESSURE, PV_PRESSURE = len(TERMS), len(TERMS) + 1
CHUNK = 256
# EclString (ebos/eclgenericoutputblackoilmodule.cc:48-60): the summary mnemonics behind "F" / "R"
ECL_STRING = {"WATER": "WIP", "OIL": "OIP", "GAS": "GIP", "OilInLiquidPhase": "OIPL", "OilInGasPhase": "OIPG", "GasInLiquidPhase": "GIPL",
              "GasInGasPhase": "GIPG", "PoreVolume": "RPV"}


def cell_terms(iq, volume, poro):
    """iq (cells, 17 | 19 fields, 4) as model.iq() returns it, volume and the reference porosity per cell -> (12, cells), rows as TERMS"""
    iq = np.asarray(iq, float)
    volume, poro = np.asarray(volume, float), np.asarray(poro, float)
    ext = iq.shape[1] == 19
    sw, so, sg = iq[:, 0, 0], iq[:, 1, 0], iq[:, 2, 0]
    po = iq[:, 4, 0]
    bw, bo, bg = iq[:, 6, 0], iq[:, 7, 0], iq[:, 8, 0]
    rs = iq[:, 15, 0]
    rv = iq[:, 16, 0] if ext else np.zeros(len(iq))
    out = np.empty((len(TERMS), len(iq)))
    pv = volume * iq[:, 18 if ext else 16, 0]
    hc = (0.0 + so) + sg
    out[T["DynamicPoreVolume"]] = pv
    out[T["PoreVolume"]] = volume * poro
    out[T["HydroCarbonPV"]] = pv * hc
    out[T["PressurePV"]] = po * pv
    out[T["PressureHydroCarbonPV"]] = out[T["PressurePV"]] * hc
    fip_w, fip_o, fip_g = (bw * sw) * pv, (bo * so) * pv, (bg * sg) * pv
    out[T["OilInLiquidPhase"]] = fip_o
    out[T["GasInGasPhase"]] = fip_g
    out[T["GasInLiquidPhase"]] = rs * fip_o
    out[T["OilInGasPhase"]] = rv * fip_g
    out[T["WATER"]] = fip_w
    out[T["OIL"]] = fip_o + out[T["OilInGasPhase"]]
    out[T["GAS"]] = fip_g + out[T["GasInLiquidPhase"]]
    return out


def reduce256(x):
    """the stated order over the last axis of x: (..., n) -> (...); n = 0 gives zeros"""
    x = np.asarray(x, float)
    if x.shape[-1] == 0:
        return np.zeros(x.shape[:-1])
    while True:
        n = x.shape[-1]
        nch = -(-n // CHUNK)
        c = np.zeros(x.shape[:-1] + (nch * CHUNK,))
        c[..., :n] = x
        c = c.reshape(x.shape[:-1] + (nch, CHUNK // 64, 64))
        v = (((0.0 + c[..., 0, :]) + c[..., 1, :]) + c[..., 2, :]) + c[..., 3, :]
        o = 32
        while o:
            v = v[..., :o] + v[..., o:2 * o]
            o //= 2
        x = v[..., 0]
        if nch == 1:
            return x[..., 0]


def _sequential(x):
    # np.cumsum adds one element after the other in index order (no pairwise blocking): the loop totals[r] += property[j]
    return np.cumsum(x, axis=-1)[..., -1] if x.shape[-1] else np.zeros(x.shape[:-1])


def region_sums(terms, region, arithmetic="sequential"):
    """terms (12, cells), region per cell (natural order) -> (regions (max_id, 12), field (12,))"""
    if arithmetic not in ("sequential", "stated"):
        raise ValueError("region_sums: arithmetic %r, not 'sequential' or 'stated'" % (arithmetic,))
    terms, region = np.asarray(terms, float), np.asarray(region).reshape(-1)
    if terms.shape[1] != len(region):
        raise ValueError("region_sums: %d cells of terms, %d region ids" % (terms.shape[1], len(region)))
    red = _sequential if arithmetic == "sequential" else reduce256
    max_id = max(int(region.max()), 0) if len(region) else 0
    regions = np.zeros((max_id, terms.shape[0]))
    field = np.zeros(terms.shape[0])
    for r in range(1, max_id + 1):
        regions[r - 1] = red(terms[:, region == r])
        field = field + regions[r - 1]
    return regions, field


def averages(sums):
    """pressureAverage_ over rows of twelve sums (..., 12) -> (hydrocarbon = true, hydrocarbon = false)"""
    sums = np.asarray(sums, float)
    with np.errstate(divide="ignore", invalid="ignore"):
        pv_avg = sums[..., T["PressurePV"]] / sums[..., T["PoreVolume"]]
        hc_avg = np.where(sums[..., T["HydroCarbonPV"]] > 1e-10, sums[..., T["PressureHydroCarbonPV"]] / sums[..., T["HydroCarbonPV"]], pv_avg)
    return hc_avg, pv_avg


def inplace(terms, region, arithmetic="sequential"):
    """region_sums + averages -> dict(regions=(max_id, 14), field=(14,)), the form of capi.HipModel.fluid_in_place()"""
    regions, field = region_sums(terms, region, arithmetic)
    rows = np.concatenate([regions, field[None, :]])
    hc, pv = averages(rows)
    rows = np.concatenate([rows, hc[:, None], pv[:, None]], axis=1)
    return dict(regions=rows[:-1], field=rows[-1])


def model_inplace(model, volume, poro, region, arithmetic="sequential"):
    """the same from any model with iq()"""
    iq = model.iq()
    return inplace(cell_terms(iq[:len(np.asarray(volume))], volume, poro), region, arithmetic)


def summary(inplace, initial=None):
    """updateSummaryRegionValues (:1501-1571): the F* keys of the field, the R*:<id> keys of the regions - in place under EclString's
    mnemonics, FPR / FPRP / RPR / RPRP, and FOE = OIL / initial OIL where an "originally in place" record is given (:1514-1517).  SI
    units; unit conversion is the caller's."""
    out = {}
    f, reg = np.asarray(inplace["field"], float), np.asarray(inplace["regions"], float)
    for name, key in ECL_STRING.items():
        out["F" + key] = float(f[T[name]])
        for r in range(len(reg)):
            out["R%s:%d" % (key, r + 1)] = float(reg[r, T[name]])
    out["FPR"], out["FPRP"] = float(f[HC_PRESSURE]), float(f[PV_PRESSURE])
    for r in range(len(reg)):
        out["RPR:%d" % (r + 1)], out["RPRP:%d" % (r + 1)] = float(reg[r, HC_PRESSURE]), float(reg[r, PV_PRESSURE])
    if initial is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            out["FOE"] = float(np.float64(f[T["OIL"]]) / np.float64(np.asarray(initial["field"], float)[T["OIL"]]))
    return out
