// gfx950 kernels of the assembly half of the hot path: black-oil intensive quantities, TPFA flux and storage with
// dense forward AD (value + 3 derivatives), element-centred linearisation straight into block-CSR, convergence
// reductions and the Newton update with primary-variable switching.
//
// Reference behaviour restated (file:line under the reference tree; opm-models / opm-material routines are NOT in that
// tree and are restated from their public 2021.10 sources):
//   ebos/eclfluxmodule.hh:212-357 (TPFA flux), ebos/eclproblem.hh:1430-1486, 1711-1765, 1823-1845 (problem hooks),
//   flow/BlackoilModelEbos.hpp:549-563 (updateSolution), :628-904 (convergence),
//   BlackOilIntensiveQuantities::update, BlackOilLocalResidual::{computeStorage,computeFlux}, FvBaseLocalResidual::eval,
//   FvBaseAdLocalLinearizer, BlackOilNewtonMethod::update_, BlackOilPrimaryVariables::adaptPrimaryVariables.
//
// Mapping: ONE LANE PER BLOCK-CSR ENTRY.  A 256-thread workgroup owns a tile of whole rows with at most
// 256 entries (36 rows of a 7-point stencil: 252/256 lanes busy).  The lane of an off-diagonal entry (I,J) evaluates the
// face flux twice, once with focus I (goes into R_I and the diagonal block) and once with focus J (its derivative is
// the off-diagonal block (I,J), exactly the number the reference's column-wise linearisation writes there); the lane of
// the diagonal entry evaluates the storage term and then sums its row's fluxes out of LDS in ascending column order.
// All 3x3 blocks of the tile are staged in LDS and leave as one contiguous, 16-byte-per-lane coalesced store stream.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "device_blocks.hpp"
#include "fluid_tables.hpp"
#include "internal.hpp"

namespace opmhip {

// ============================== dense AD scalar (DenseAd::Evaluation<double,3>) ==============================
struct Ad {
    double v, d0, d1, d2;
};
__device__ __forceinline__ Ad ad_const(double c) { return Ad{c, 0.0, 0.0, 0.0}; }
__device__ __forceinline__ Ad ad_var(double x, int idx) { return Ad{x, idx == 0 ? 1.0 : 0.0, idx == 1 ? 1.0 : 0.0, idx == 2 ? 1.0 : 0.0}; }
__device__ __forceinline__ Ad operator+(const Ad& a, const Ad& b) { return Ad{a.v + b.v, a.d0 + b.d0, a.d1 + b.d1, a.d2 + b.d2}; }
__device__ __forceinline__ Ad operator-(const Ad& a, const Ad& b) { return Ad{a.v - b.v, a.d0 - b.d0, a.d1 - b.d1, a.d2 - b.d2}; }
__device__ __forceinline__ Ad operator+(const Ad& a, double b) { return Ad{a.v + b, a.d0, a.d1, a.d2}; }
__device__ __forceinline__ Ad operator+(double a, const Ad& b) { return Ad{a + b.v, b.d0, b.d1, b.d2}; }
__device__ __forceinline__ Ad operator-(const Ad& a, double b) { return Ad{a.v - b, a.d0, a.d1, a.d2}; }
__device__ __forceinline__ Ad operator-(double a, const Ad& b) { return Ad{a - b.v, -b.d0, -b.d1, -b.d2}; }
__device__ __forceinline__ Ad operator-(const Ad& a) { return Ad{-a.v, -a.d0, -a.d1, -a.d2}; }
__device__ __forceinline__ Ad operator*(const Ad& a, const Ad& b) {
    const double u = a.v, w = b.v;
    return Ad{u * w, a.d0 * w + b.d0 * u, a.d1 * w + b.d1 * u, a.d2 * w + b.d2 * u};
}
__device__ __forceinline__ Ad operator*(const Ad& a, double b) { return Ad{a.v * b, a.d0 * b, a.d1 * b, a.d2 * b}; }
__device__ __forceinline__ Ad operator*(double a, const Ad& b) { return b * a; }
__device__ __forceinline__ Ad operator/(const Ad& a, const Ad& b) {
    const double u = a.v, w = b.v;
    return Ad{u / w, (w * a.d0 - b.d0 * u) / (w * w), (w * a.d1 - b.d1 * u) / (w * w), (w * a.d2 - b.d2 * u) / (w * w)};
}
__device__ __forceinline__ Ad operator/(const Ad& a, double b) { return Ad{a.v / b, a.d0 / b, a.d1 / b, a.d2 / b}; }
__device__ __forceinline__ Ad operator/(double a, const Ad& b) {
    const double t = -a / (b.v * b.v);
    return Ad{a / b.v, t * b.d0, t * b.d1, t * b.d2};
}
// Opm::pow(Evaluation, Scalar) as oracle/eval.hpp restates it.  The device's pow() and the host's std::pow() agree to an ulp,
// not to the bit: VAPPARS is the one place where device and oracle are compared with a tolerance (tests/test_gpu_vappars.py)
__device__ __forceinline__ Ad epow(const Ad& a, double e) {
    const double px = pow(a.v, e);
    const double df = (a.v == 0.0) ? 0.0 : px / a.v * e;
    return Ad{px, df * a.d0, df * a.d1, df * a.d2};
}
__device__ __forceinline__ double epow(double a, double e) { return pow(a, e); }
__device__ __forceinline__ Ad ad_max(const Ad& a, const Ad& b) { return (a.v > b.v) ? a : b; }
__device__ __forceinline__ Ad ad_min(const Ad& a, const Ad& b) { return (a.v < b.v) ? a : b; }
__device__ __forceinline__ double val(const Ad& a) { return a.v; }
__device__ __forceinline__ double val(double a) { return a; }
template <class E> __device__ __forceinline__ E mk(double x, int idx);
template <> __device__ __forceinline__ Ad mk<Ad>(double x, int idx) { return ad_var(x, idx); }
template <> __device__ __forceinline__ double mk<double>(double x, int) { return x; }
template <class E> __device__ __forceinline__ E cst(double x);
template <> __device__ __forceinline__ Ad cst<Ad>(double x) { return ad_const(x); }
template <> __device__ __forceinline__ double cst<double>(double x) { return x; }
__device__ __forceinline__ double emin(double a, double b) { return (a < b) ? a : b; }
__device__ __forceinline__ Ad emin(const Ad& a, const Ad& b) { return ad_min(a, b); }
__device__ __forceinline__ double emax(double a, double b) { return (a > b) ? a : b; }
__device__ __forceinline__ Ad emax(const Ad& a, const Ad& b) { return ad_max(a, b); }

// ============================== property tables ===============================================================
typedef const double* GlobalTab;                                       // table blob where it lies in HBM (L1/K$-resident)
typedef const __attribute__((address_space(3))) double* LdsTab;        // ... or copied into LDS by the workgroup
template <class DP>
struct TablesT {
    DP dbl;
    const int* idx;
    double rock_pref, rock_cr;
    int ndbl, nidx;   // lengths of the blobs (for the LDS copy of the per-cell kernels)
    int rock_desc, num_rock;   // RockTabDesc array inside the int blob (ROCKTAB), 0 tables = none
    __device__ __forceinline__ const RockTabDesc& rock(int t) const { return reinterpret_cast<const RockTabDesc*>(idx + rock_desc)[t]; }
    __device__ __forceinline__ const PvtRegionDesc& pvt(int r) const { return reinterpret_cast<const PvtRegionDesc*>(idx + 2)[r]; }
    __device__ __forceinline__ const SatRegionDesc& sat(int s) const {
        return reinterpret_cast<const SatRegionDesc*>(idx + 2 + idx[0] * (int)(sizeof(PvtRegionDesc) / sizeof(int)))[s];
    }
};
typedef TablesT<GlobalTab> Tables;
// segment of x in an ascending array with clamping (Tabulated1DFunction / UniformXTabulated2DFunction, extrapolate = true):
// a value that sits exactly on an interior node belongs to the segment on its right
template <class DP> __device__ __forceinline__ int seg_right(DP x, int n, double xv) {
    if (xv <= x[0]) return 0;
    if (xv >= x[n - 1]) return n - 2;
    int lo = 0, hi = n - 1;
    while (lo + 1 < hi) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] <= xv) lo = mid; else hi = mid;
    }
    return lo;
}
template <class E, class DP> __device__ __forceinline__ E tab1(DP x, DP y, int n, const E& xv) {
    const int s = seg_right(x, n, val(xv));
    const double x0 = x[s], x1 = x[s + 1], y0 = y[s], y1 = y[s + 1];
    return y0 + (y1 - y0) * (xv - x0) / (x1 - x0);
}
// plain bilinear interpolation in (x, y) with per-column y grids (UniformXTabulated2DFunction; the policy the Norne PVT
// points select): oil (x = Rs, y = p_o)
struct Tab2Desc { int nx, xs, yoff, ys; };
template <class E, class DP> __device__ __forceinline__ E tab2g(const TablesT<DP>& T, const Tab2Desc& G, int voff, const E& xv, const E& yv) {
    const DP xs = T.dbl + G.xs;
    const int* yo = T.idx + G.yoff;
    const int i = seg_right(xs, G.nx, val(xv));
    const E alpha = (xv - xs[i]) / (xs[i + 1] - xs[i]);
    const DP y1 = T.dbl + G.ys + yo[i];
    const DP y2 = T.dbl + G.ys + yo[i + 1];
    const DP v1 = T.dbl + voff + yo[i];
    const DP v2 = T.dbl + voff + yo[i + 1];
    const int j1 = seg_right(y1, yo[i + 1] - yo[i], val(yv)), j2 = seg_right(y2, yo[i + 2] - yo[i + 1], val(yv));
    const E beta1 = (yv - y1[j1]) / (y1[j1 + 1] - y1[j1]);
    const E beta2 = (yv - y2[j2]) / (y2[j2 + 1] - y2[j2]);
    const E s1 = v1[j1] * (1.0 - beta1) + v1[j1 + 1] * beta1;
    const E s2 = v2[j2] * (1.0 - beta2) + v2[j2 + 1] * beta2;
    return s1 * (1.0 - alpha) + s2 * alpha;
}
template <class E, class DP> __device__ __forceinline__ E tab2(const TablesT<DP>& T, const PvtRegionDesc& D, int voff, const E& xv, const E& yv) {
    return tab2g<E, DP>(T, Tab2Desc{D.o_nx, D.o_xs, D.o_yoff, D.o_ys}, voff, xv, yv);
}
// wet gas (x = p_g, y = Rv): interpolation guided by the columns' LAST samples (the saturated Rv), the shift fading linearly
// to 0 at Rv = 0 - the policy the 16-digit saturations of tests/test_equil.cc DeckWithRSVDAndRVVD / DeckWithPBVDAndPDVD
// select (oracle/fluid.hpp Tab2D, guide = 2); same statements, same order
template <class E, class DP> __device__ __forceinline__ E tab2wg(const TablesT<DP>& T, const PvtRegionDesc& D, int voff, const E& xv, const E& yv) {
    const DP xs = T.dbl + D.wg_xs;
    const int* yo = T.idx + D.wg_yoff;
    const int i = seg_right(xs, D.wg_n, val(xv));
    const E alpha = (xv - xs[i]) / (xs[i + 1] - xs[i]);
    const DP y1 = T.dbl + D.wg_ys + yo[i];
    const DP y2 = T.dbl + D.wg_ys + yo[i + 1];
    const DP v1 = T.dbl + voff + yo[i];
    const DP v2 = T.dbl + voff + yo[i + 1];
    const int n1 = yo[i + 1] - yo[i], n2 = yo[i + 2] - yo[i + 1];
    E yLower = yv, yUpper = yv;
    const double e0 = y1[n1 - 1], e1 = y2[n2 - 1];
    const E yEnd = e0 * (1.0 - alpha) + e1 * alpha;
    if (val(yEnd) > 0.0) {
        const E shift = (e1 - e0) * yv / yEnd;
        yLower = yv - alpha * shift;
        yUpper = yv + shift - alpha * shift;
    }
    const int j1 = seg_right(y1, n1, val(yLower)), j2 = seg_right(y2, n2, val(yUpper));
    const E beta1 = (yLower - y1[j1]) / (y1[j1 + 1] - y1[j1]);
    const E beta2 = (yUpper - y2[j2]) / (y2[j2 + 1] - y2[j2]);
    const E s1 = v1[j1] * (1.0 - beta1) + v1[j1 + 1] * beta1;
    const E s2 = v2[j2] * (1.0 - beta2) + v2[j2 + 1] * beta2;
    return s1 * (1.0 - alpha) + s2 * alpha;
}
// PiecewiseLinearTwoPhaseMaterial: constant outside the table; a value on a node belongs to the segment on its left
// water-induced compaction tables (rockCompPoroMultWc_ / rockCompTransMultWc_: UniformXTabulated2DFunction with the same S_w
// nodes under every pressure node, vertical interpolation, extrapolating) - oracle/fluid.hpp Tab2D::eval with guide 0, same
// statements, same order
template <class E> __device__ __forceinline__ E wc_eval(const int* __restrict__ d, const double* __restrict__ data, int voff, const E& xv, const E& yv) {
    const int ns = d[1];
    const double* xs = data + d[2];
    const double* ys = data + d[3];
    const int i = seg_right(xs, d[0], val(xv));
    const E alpha = (xv - xs[i]) / (xs[i + 1] - xs[i]);
    const double* v1 = data + voff + (size_t)i * ns;
    const double* v2 = v1 + ns;
    const int j1 = seg_right(ys, ns, val(yv)), j2 = j1;
    const E beta1 = (yv - ys[j1]) / (ys[j1 + 1] - ys[j1]);
    const E beta2 = (yv - ys[j2]) / (ys[j2 + 1] - ys[j2]);
    const E s1 = v1[j1] * (1.0 - beta1) + v1[j1 + 1] * beta1;
    const E s2 = v2[j2] * (1.0 - beta2) + v2[j2 + 1] * beta2;
    return s1 * (1.0 - alpha) + s2 * alpha;
}
template <class E, class DP> __device__ __forceinline__ E pwlin(DP x, DP y, int n, const E& xv) {
    const double s = val(xv);
    if (s <= x[0]) return cst<E>(y[0]);
    if (s >= x[n - 1]) return cst<E>(y[n - 1]);
    int lo = 0, hi = n - 1;
    while (lo + 1 < hi) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] < s) lo = mid; else hi = mid;
    }
    const double x0 = x[lo], x1 = x[lo + 1], y0 = y[lo], y1 = y[lo + 1];
    const double m = (y1 - y0) / (x1 - x0);
    return y0 + (xv - x0) * m;
}
template <class DP> __device__ __forceinline__ double rs_sat_value(const TablesT<DP>& T, int pr, double po) {
    const PvtRegionDesc& D = T.pvt(pr);
    return tab1<double, DP>(T.dbl + D.sat_p, T.dbl + D.sat_rs, D.sat_n, po);
}
template <class DP> __device__ __forceinline__ double rv_sat_value(const TablesT<DP>& T, int pr, double pg) {
    const PvtRegionDesc& D = T.pvt(pr);
    return tab1<double, DP>(T.dbl + D.wg_xs, T.dbl + D.wgs_rv, D.wg_n, pg);
}
// EclDefaultMaterial capillary pressures: pC[water] = -pcow(Sw), pC[oil] = 0, pC[gas] = pcgo(1 - Swco - Sg)
template <class E, class DP> __device__ __forceinline__ void cap_pressures(const TablesT<DP>& T, int sr, const E& Sw, const E& Sg, E pC[3]) {
    const SatRegionDesc& Sd = T.sat(sr);
    const DP B = T.dbl;
    const double Swco = B[Sd.swco];
    pC[0] = -pwlin<E, DP>(B + Sd.sw_x, B + Sd.pcow, Sd.nw, Sw);
    pC[1] = cst<E>(0.0);
    pC[2] = pwlin<E, DP>(B + Sd.so_x, B + Sd.pcgo, Sd.ng, 1.0 - Swco - Sg);
}

// ============================== intensive quantities ========================================================
// Record of the intensive-quantity cache: fields x (value + 3 derivatives).  Two layouts, chosen per context when the
// fluid is set: the BASE one (live oil + dry gas + water: 17 fields) and the EXTENDED one (19 fields) for decks with wet
// gas (PVTG: Rv) and / or rock compaction tables (ROCKTAB: transmissibility multiplier).  Kernels are templated on it, so
// that the base instantiation computes bit for bit what it did.
// The cache is stored FIELD-MAJOR: field f of cell c = the four doubles at iq[(f * ncell + c) * 4].  Lanes that walk
// consecutive cells (the per-cell kernels) write and read contiguous memory, and the neighbours a tile of k_assemble
// gathers - runs of consecutive cells of a few z-lines - share cache lines: 3.6x fewer L1 accesses than with per-cell
// records, whose 544-byte stride gave every lane of a gather its own lines.  (F_S .. F_RS, the phases, the equations: internal.hpp)
__device__ __forceinline__ const double* iq_at(const double* iq, int ncell, int f, int c) { return iq + ((size_t)f * ncell + c) * 4; }
__device__ __forceinline__ double* iq_at(double* iq, int ncell, int f, int c) { return iq + ((size_t)f * ncell + c) * 4; }
template <bool EXT> struct Lay {
    static constexpr int F_RV = 16, F_TMULT = 17;                    // EXT only
    static constexpr int F_PORO = EXT ? 18 : 16;
    static constexpr int IQF = EXT ? 19 : 17;                        // fields per cell
    static constexpr int IQS = IQF * 4;                              // doubles per cell
    static constexpr int RQ_F0 = F_P;                                // neighbour fields of the flux: p, 1/B, mobility, density, Rs [, Rv, tmult]
    static constexpr int RQ_NF = (EXT ? F_TMULT : F_RS) - F_P + 1;
};

template <class E>
struct Iq {
    E S[3], p[3], invB[3], mob[3], rho[3], Rs, poro;
    E Rv, tmult;   // extended layout only
};
struct CellStatic {
    const double *poro, *volume, *depth, *rsmax;
    const int *pvtnum, *satnum;
    const double *rvmax, *overburden;   // extended layout: DRVDT cap, overburden pressure (may be NULL)
    const int* rocknum;                 // rock-table index per cell (NULL = table 0)
    const double* pcw;                  // extended layout: scaled maximum of pcow per cell (PCW / SWATINIT; NULL = the tables' own)
    const double* minpo;                // extended layout: minimum oil pressure so far (ROCKCOMP IRREVERS; NULL = reversible compaction)
    const double* maxso;                // extended layout: largest oil saturation seen at the start of a time step (VAPPARS; NULL = not in force)
    double vap1, vap2;                  // VAPPARS: exponent on RvSat / on RsSat
    // extended layout: water-induced compaction (ROCK2D / ROCK2DTR / ROCKWNOD; NULL = off): largest S_w seen at the start of a
    // time step, initial S_w, per table {np, nsw, pressure nodes at, S_w nodes at, pore-volume multipliers at, transmissibility
    // multipliers at (-1: none)} and the tables' doubles (global memory: a handful of nodes, used by few decks)
    const double *maxsw, *sw0;
    const int* wcdesc;
    const double* wcdata;
    const double* eps;                  // extended layout: scaled end points per cell, field-major [EPS_COUNT][ncell] (NULL = no end-point scaling)
    int epscfg;                         // EclEpsConfig: bit 0 saturation scaling, 1 three-point, 2-3 krw, 4-5 kro, 6-7 krg mode, 8 pcw, 9 pcg
    // extended layout: relative-permeability hysteresis (SATOPTS HYSTER; NULL = not in force): per cell the turning point and the
    // imbibition curve's shift of the oil-water and of the gas-oil system, field-major [4][ncell] (krnSwMdc_ow, deltaSwImbKrn_ow,
    // krnSwMdc_go, deltaSwImbKrn_go), the imbibition saturation region (IMBNUM) and, with end-point scaling in force, the
    // scaled end points of the imbibition curves [EPS_COUNT][ncell] (NULL: the imbibition tables' own); hystModel = EHYSTR item 2
    const double* hyst;
    const int* imbnum;
    const double* epsImb;
    int hystModel;
    double* invb;                       // packed 1/b_w, 1/b_o, 1/b_g per cell, written beside the record (convergence check)
    int ncell;                          // cells of the intensive-quantity cache (owned + ghost): the stride between its fields
};

// ---- saturation end-point scaling (EclEpsTwoPhaseLaw; oracle/fluid.hpp eps_*: same statements, same order) ----------------
struct EpsTriple { double s[3]; };
__device__ __forceinline__ EpsTriple eps_pc_ow(const double* e) { return {{e[EPS_SWL], e[EPS_SWU], e[EPS_SWU]}}; }
__device__ __forceinline__ EpsTriple eps_krw_ow(const double* e) { return {{e[EPS_SWCR], 1.0 - e[EPS_SOWCR] - e[EPS_SGL], e[EPS_SWU]}}; }
__device__ __forceinline__ EpsTriple eps_krn_ow(const double* e) { return {{e[EPS_SWL] + e[EPS_SGL], e[EPS_SWCR] + e[EPS_SGL], 1.0 - e[EPS_SOWCR]}}; }
__device__ __forceinline__ EpsTriple eps_pc_go(const double* e) { return {{1.0 - e[EPS_SWL] - e[EPS_SGU], 1.0 - e[EPS_SWL] - e[EPS_SGL], 1.0 - e[EPS_SWL] - e[EPS_SGL]}}; }
__device__ __forceinline__ EpsTriple eps_krw_go(const double* e) { return {{e[EPS_SOGCR], 1.0 - e[EPS_SGCR] - e[EPS_SWL], 1.0 - e[EPS_SWL] - e[EPS_SGL]}}; }
__device__ __forceinline__ EpsTriple eps_krn_go(const double* e) { return {{1.0 - e[EPS_SWL] - e[EPS_SGU], e[EPS_SOGCR], 1.0 - e[EPS_SWL] - e[EPS_SGCR]}}; }
template <class E> __device__ __forceinline__ E eps_sat_two_point(const E& S, const EpsTriple& u, const EpsTriple& sc) {
    return u.s[0] + (S - sc.s[0]) * ((u.s[2] - u.s[0]) / (sc.s[2] - sc.s[0]));
}
template <class E> __device__ __forceinline__ E eps_sat_three_point(const E& S, const EpsTriple& u, const EpsTriple& sc) {
    if (val(S) <= sc.s[0]) return cst<E>(u.s[0]);
    if (val(S) <= sc.s[1]) return u.s[0] + (S - sc.s[0]) * ((u.s[1] - u.s[0]) / (sc.s[1] - sc.s[0]));
    if (u.s[1] == u.s[2]) return cst<E>(u.s[1]);
    if (val(S) <= sc.s[2]) return u.s[1] + (S - sc.s[1]) * ((u.s[2] - u.s[1]) / (sc.s[2] - sc.s[1]));
    return cst<E>(u.s[2]);
}
template <class E> __device__ __forceinline__ E eps_to_unscaled(int cfg, const E& S, const EpsTriple& u, const EpsTriple& sc) {
    if (!(cfg & 1)) return S;
    return (cfg & 2) ? eps_sat_three_point(S, u, sc) : eps_sat_two_point(S, u, sc);
}
template <class E> __device__ __forceinline__ E eps_vertical_krw(int mode, const E& S, const E& kr, const EpsTriple& sc, double fdisp, double fmax, double fr, double fm) {
    if (mode == 0) return kr;
    if (mode == 1) return kr * (fm / fmax);
    const double sm = sc.s[2], sr = emin(sc.s[1], sm);
    if (!(val(S) > sr)) return kr * (fr / fdisp);
    if (fmax > fdisp) { const E t = (kr - fdisp) / (fmax - fdisp); return fr + t * (fm - fr); }
    if (sr < sm) { const E t = (S - sr) / (sm - sr); return fr + t * (fm - fr); }
    return cst<E>(fm);
}
template <class E> __device__ __forceinline__ E eps_vertical_krn(int mode, const E& S, const E& kr, const EpsTriple& sc, double fdisp, double fmax, double fr, double fm) {
    if (mode == 0) return kr;
    if (mode == 1) return kr * (fm / fmax);
    const double sl = sc.s[0], sr = emax(sc.s[1], sl);
    if (!(val(S) < sr)) return kr * (fr / fdisp);
    if (fmax > fdisp) { const E t = (kr - fdisp) / (fmax - fdisp); return fr + t * (fm - fr); }
    if (sr > sl) { const E t = (sr - S) / (sr - sl); return fr + t * (fm - fr); }
    return cst<E>(fm);
}
// the cell's scaled end points out of the field-major array, the region's unscaled ones out of the table blob
template <class DP> __device__ __forceinline__ void eps_load(const CellStatic& C, int c, DP B, const SatRegionDesc& Sd, double* u, double* s) {
#pragma unroll
    for (int f = 0; f < EPS_COUNT; ++f) { u[f] = B[Sd.eps + f]; s[f] = C.eps[(size_t)f * C.ncell + c]; }
}
// capillary pressures of a cell with scaled end points (SatFunc::capillaryPressuresEps)
template <class E, class DP> __device__ __forceinline__ void cap_pressures_eps(DP B, const SatRegionDesc& Sd, int cfg, const double* u, const double* s, const E& Sw, const E& Sg, E pC[3]) {
    const double Swco = B[Sd.swco];
    const double SwcoS = s[EPS_SWL];
    const E SoP = 1.0 - SwcoS - Sg;
    E swU = Sw, soU = SoP;
    if (cfg & 1) {
        swU = eps_sat_two_point(Sw, eps_pc_ow(u), eps_pc_ow(s));
        soU = eps_sat_two_point(SoP, eps_pc_go(u), eps_pc_go(s));
    } else soU = 1.0 - Swco - Sg;
    E pcw = pwlin<E, DP>(B + Sd.sw_x, B + Sd.pcow, Sd.nw, swU), pcg = pwlin<E, DP>(B + Sd.so_x, B + Sd.pcgo, Sd.ng, soU);
    if (cfg & 256) {
        const double sm = s[EPS_MAXPCOW], um = u[EPS_MAXPCOW];
        pcw = pcw * ((sm == um) ? 1.0 : sm / um);
    }
    if (cfg & 512) {
        const double sm = s[EPS_MAXPCGO], um = u[EPS_MAXPCGO];
        pcg = pcg * ((sm == um) ? 1.0 : sm / um);
    }
    pC[0] = -pcw;
    pC[1] = cst<E>(0.0);
    pC[2] = pcg;
}
// relative permeabilities of a cell with scaled end points (SatFunc::relativePermeabilitiesEps)
template <class E, class DP> __device__ __forceinline__ void rel_perms_eps(DP B, const SatRegionDesc& Sd, int cfg, const double* u, const double* s, const E& SwIn, const E& Sg, E kr[3]) {
    const double Swco = B[Sd.swco];
    const double SwcoS = (cfg & 1) ? s[EPS_SWL] : Swco;
    const int mKrw = (cfg >> 2) & 3, mKro = (cfg >> 4) & 3, mKrg = (cfg >> 6) & 3;
    const EpsTriple uKrwOw = eps_krw_ow(u), sKrwOw = eps_krw_ow(s), uKrnOw = eps_krn_ow(u), sKrnOw = eps_krn_ow(s);
    const EpsTriple uKrwGo = eps_krw_go(u), sKrwGo = eps_krw_go(s), uKrnGo = eps_krn_go(u), sKrnGo = eps_krn_go(s);
    kr[0] = eps_vertical_krw(mKrw, SwIn, pwlin<E, DP>(B + Sd.sw_x, B + Sd.krw, Sd.nw, eps_to_unscaled(cfg, SwIn, uKrwOw, sKrwOw)), sKrwOw, u[EPS_KRWR], u[EPS_MAXKRW], s[EPS_KRWR], s[EPS_MAXKRW]);
    const E SoP = 1.0 - SwcoS - Sg;
    kr[2] = eps_vertical_krn(mKrg, SoP, pwlin<E, DP>(B + Sd.so_x, B + Sd.krg, Sd.ng, eps_to_unscaled(cfg, SoP, uKrnGo, sKrnGo)), sKrnGo, u[EPS_KRGR], u[EPS_MAXKRG], s[EPS_KRGR], s[EPS_MAXKRG]);
    const E Sw = emax(cst<E>(SwcoS), SwIn);
    const E Sw_ow = Sg + Sw;
    const E So_go = 1.0 - Sw_ow;
    const E kro_ow = eps_vertical_krn(mKro, Sw_ow, pwlin<E, DP>(B + Sd.sw_x, B + Sd.krow, Sd.nw, eps_to_unscaled(cfg, Sw_ow, uKrnOw, sKrnOw)), sKrnOw, u[EPS_KRORW], u[EPS_MAXKROW], s[EPS_KRORW], s[EPS_MAXKROW]);
    const E kro_go = eps_vertical_krw(mKro, So_go, pwlin<E, DP>(B + Sd.so_x, B + Sd.krog, Sd.ng, eps_to_unscaled(cfg, So_go, uKrwGo, sKrwGo)), sKrwGo, u[EPS_KRORG], u[EPS_MAXKROG], s[EPS_KRORG], s[EPS_MAXKROG]);
    const double eps = 1e-5;
    if (val(Sw_ow) - SwcoS < eps) {
        const E kro2 = (kro_ow + kro_go) / 2.0;
        if (val(Sw_ow) - SwcoS > eps / 2.0) {
            const E kro1 = (Sg * kro_go + (Sw - SwcoS) * kro_ow) / (Sw_ow - SwcoS);
            const E alpha = (eps - (Sw_ow - SwcoS)) / (eps / 2.0);
            kr[1] = kro2 * alpha + kro1 * (1.0 - alpha);
        } else kr[1] = kro2;
    } else kr[1] = (Sg * kro_go + (Sw - SwcoS) * kro_ow) / (Sw_ow - SwcoS);
}
// ---- relative-permeability hysteresis (oracle/fluid.hpp: SatFunc::curve / curveInv / hystSee / relativePermeabilitiesHyst - same
//      statements, same order; EclHysteresisTwoPhaseLaw of opm-material restated, UNVERIFIED vs upstream) -------------------------
enum { KRW_OW = 0, KRN_OW = 1, KRW_GO = 2, KRN_GO = 3 };
// one relative-permeability curve of a saturation region at the (scaled) wetting saturation S of its two-phase system
template <class E, class DP> __device__ __forceinline__ E sat_curve(DP B, const SatRegionDesc& Sd, int kind, const E& S, bool scaled, int cfg, const double* u, const double* s) {
    const DP x = B + (kind <= KRN_OW ? Sd.sw_x : Sd.so_x);
    const DP y = B + (kind == KRW_OW ? Sd.krw : kind == KRN_OW ? Sd.krow : kind == KRW_GO ? Sd.krog : Sd.krg);
    const int n = kind <= KRN_OW ? Sd.nw : Sd.ng;
    if (!scaled) return pwlin<E, DP>(x, y, n, S);
    const EpsTriple ut = kind == KRW_OW ? eps_krw_ow(u) : kind == KRN_OW ? eps_krn_ow(u) : kind == KRW_GO ? eps_krw_go(u) : eps_krn_go(u);
    const EpsTriple st = kind == KRW_OW ? eps_krw_ow(s) : kind == KRN_OW ? eps_krn_ow(s) : kind == KRW_GO ? eps_krw_go(s) : eps_krn_go(s);
    const E k = pwlin<E, DP>(x, y, n, eps_to_unscaled(cfg, S, ut, st));
    if (kind == KRW_OW) return eps_vertical_krw((cfg >> 2) & 3, S, k, st, u[EPS_KRWR], u[EPS_MAXKRW], s[EPS_KRWR], s[EPS_MAXKRW]);
    if (kind == KRN_OW) return eps_vertical_krn((cfg >> 4) & 3, S, k, st, u[EPS_KRORW], u[EPS_MAXKROW], s[EPS_KRORW], s[EPS_MAXKROW]);
    if (kind == KRW_GO) return eps_vertical_krw((cfg >> 4) & 3, S, k, st, u[EPS_KRORG], u[EPS_MAXKROG], s[EPS_KRORG], s[EPS_MAXKROG]);
    return eps_vertical_krn((cfg >> 6) & 3, S, k, st, u[EPS_KRGR], u[EPS_MAXKRG], s[EPS_KRGR], s[EPS_MAXKRG]);
}
// PwLin::inv: the abscissa at which a piecewise-linear curve takes the value yv
template <class DP> __device__ __forceinline__ double pwlin_inv(DP x, DP y, int n, double yv) {
    if (y[0] > y[n - 1]) {
        if (yv >= y[0]) return x[0];
        if (yv <= y[n - 1]) return x[n - 1];
        int lo = 0, hi = n - 1;
        while (lo + 1 < hi) {
            const int mid = (lo + hi) / 2;
            if (y[mid] >= yv) lo = mid; else hi = mid;
        }
        const double m = (x[lo + 1] - x[lo]) / (y[lo + 1] - y[lo]);
        return x[lo] + (yv - y[lo]) * m;
    }
    if (yv <= y[0]) return x[0];
    if (yv >= y[n - 1]) return x[n - 1];
    int lo = 0, hi = n - 1;
    while (lo + 1 < hi) {
        const int mid = (lo + hi) / 2;
        if (y[mid] <= yv) lo = mid; else hi = mid;
    }
    const double m = (x[lo + 1] - x[lo]) / (y[lo + 1] - y[lo]);
    return x[lo] + (yv - y[lo]) * m;
}
// SatFunc::curveInv: the (scaled) wetting saturation at which non-wetting curve `kind` takes the value k
template <class DP> __device__ __forceinline__ double sat_curve_inv(DP B, const SatRegionDesc& Sd, int kind, double k, bool scaled, int cfg, const double* u, const double* s) {
    const double Su = kind == KRN_OW ? pwlin_inv<DP>(B + Sd.sw_x, B + Sd.krow, Sd.nw, k) : pwlin_inv<DP>(B + Sd.so_x, B + Sd.krg, Sd.ng, k);
    if (!scaled || !(cfg & 1)) return Su;
    const EpsTriple ut = kind == KRN_OW ? eps_krn_ow(u) : eps_krn_go(u);
    const EpsTriple st = kind == KRN_OW ? eps_krn_ow(s) : eps_krn_go(s);
    if (cfg & 2) {   // eps_unscaled_to_scaled_three_point
        if (Su <= ut.s[0]) return st.s[0];
        if (Su < ut.s[1]) return st.s[0] + (Su - ut.s[0]) * ((st.s[1] - st.s[0]) / (ut.s[1] - ut.s[0]));
        if (Su < ut.s[2]) return st.s[1] + (Su - ut.s[1]) * ((st.s[2] - st.s[1]) / (ut.s[2] - ut.s[1]));
        return st.s[2];
    }
    return st.s[0] + (Su - ut.s[0]) * ((st.s[2] - st.s[0]) / (ut.s[2] - ut.s[0]));
}
// the imbibition region's end points of cell c: the tables' own and the scaled ones (IS* arrays, else the tables' own)
template <class DP> __device__ __forceinline__ void eps_load_imb(const CellStatic& C, int c, DP B, const SatRegionDesc& Si, double* u, double* s) {
#pragma unroll
    for (int f = 0; f < EPS_COUNT; ++f) { u[f] = B[Si.eps + f]; s[f] = C.epsImb ? C.epsImb[(size_t)f * C.ncell + c] : u[f]; }
}
// SatFunc::relativePermeabilitiesHyst
template <class E, class DP> __device__ __forceinline__ void rel_perms_hyst(const TablesT<DP>& T, const CellStatic& C, int c, const SatRegionDesc& Sd, bool scaled,
                                                                             const double* uD, const double* sD, const E& SwIn, const E& Sg, E kr[3]) {
    const DP B = T.dbl;
    const SatRegionDesc& Si = T.sat(C.imbnum[c]);
    const int cfg = C.epscfg;
    double uI[EPS_COUNT], sI[EPS_COUNT];
    if (scaled) eps_load_imb<DP>(C, c, B, Si, uI, sI);
    const double Swco = B[Sd.swco];
    const double SwcoS = (scaled && (cfg & 1)) ? sD[EPS_SWL] : Swco;
    const size_t N = C.ncell;
    const double mdcOw = C.hyst[c], dOw = C.hyst[N + c], mdcGo = C.hyst[2 * N + c], dGo = C.hyst[3 * N + c];
    const bool wetImb = C.hystModel == 1;
    kr[0] = wetImb ? sat_curve<E, DP>(B, Si, KRW_OW, SwIn, scaled, cfg, uI, sI) : sat_curve<E, DP>(B, Sd, KRW_OW, SwIn, scaled, cfg, uD, sD);
    const E SoP = 1.0 - SwcoS - Sg;
    if (val(SoP) <= mdcGo) kr[2] = sat_curve<E, DP>(B, Sd, KRN_GO, SoP, scaled, cfg, uD, sD);
    else kr[2] = sat_curve<E, DP>(B, Si, KRN_GO, SoP + dGo, scaled, cfg, uI, sI);
    const E Sw = emax(cst<E>(SwcoS), SwIn);
    const E Sw_ow = Sg + Sw;
    const E So_go = 1.0 - Sw_ow;
    E kro_ow;
    if (val(Sw_ow) <= mdcOw) kro_ow = sat_curve<E, DP>(B, Sd, KRN_OW, Sw_ow, scaled, cfg, uD, sD);
    else kro_ow = sat_curve<E, DP>(B, Si, KRN_OW, Sw_ow + dOw, scaled, cfg, uI, sI);
    const E kro_go = wetImb ? sat_curve<E, DP>(B, Si, KRW_GO, So_go, scaled, cfg, uI, sI) : sat_curve<E, DP>(B, Sd, KRW_GO, So_go, scaled, cfg, uD, sD);
    const double eps = 1e-5;
    if (val(Sw_ow) - SwcoS < eps) {
        const E kro2 = (kro_ow + kro_go) / 2.0;
        if (val(Sw_ow) - SwcoS > eps / 2.0) {
            const E kro1 = (Sg * kro_go + (Sw - SwcoS) * kro_ow) / (Sw_ow - SwcoS);
            const E alpha = (eps - (Sw_ow - SwcoS)) / (eps / 2.0);
            kr[1] = kro2 * alpha + kro1 * (1.0 - alpha);
        } else kr[1] = kro2;
    } else kr[1] = (Sg * kro_go + (Sw - SwcoS) * kro_ow) / (Sw_ow - SwcoS);
}
// the capillary pressures of cell c at (Sw, Sg), values only: what the primary-variable switches need
// (computeCapillaryPressures_ of BlackOilPrimaryVariables), with the cell's scaled end points where the deck has them
template <class DP, bool EXT> __device__ __forceinline__ void cell_cap_pressures(const TablesT<DP>& T, const CellStatic& C, int c, int sr, double Sw, double Sg, double pC[3]) {
    if (EXT && C.eps) {
        double u[EPS_COUNT], s[EPS_COUNT];
        eps_load<DP>(C, c, T.dbl, T.sat(sr), u, s);
        cap_pressures_eps<double, DP>(T.dbl, T.sat(sr), C.epscfg, u, s, Sw, Sg, pC);
    } else cap_pressures<double, DP>(T, sr, Sw, Sg, pC);
}

// VAPPARS factor on a saturated Rs / Rv (oracle/blackoil.hpp vappars_factor: same statements)
template <class E> __device__ __forceinline__ E vappars_factor(const E& So, const E& SoMaxIn, double vapPar) {
    const E maxOilSaturation = emin(SoMaxIn, cst<E>(1.0));
    if (vapPar > 0.0 && val(maxOilSaturation) > 0.01 && val(So) < val(maxOilSaturation)) {
        const E S = emax(So, cst<E>(0.001));
        return emax(cst<E>(1e-3), epow(S / maxOilSaturation, vapPar));
    }
    return cst<E>(1.0);
}

// BlackOilIntensiveQuantities::update: live oil + water + dry gas (base) or wet gas / rock compaction tables (EXT)
template <class E, class DP, bool EXT>
__device__ __forceinline__ void update_iq(const TablesT<DP>& T, const CellStatic& C, int c, const double* pv, int meaning, Iq<E>& q) {
    const int pr = C.pvtnum ? C.pvtnum[c] : 0, sr = C.satnum ? C.satnum[c] : 0;
    const double RsMax = C.rsmax ? C.rsmax[c] : DBL_MAX / 2.0;
    const double refPoro = C.poro[c];
    const PvtRegionDesc& D = T.pvt(pr);
    const SatRegionDesc& Sd = T.sat(sr);
    const DP B = T.dbl;
    const bool wet = EXT && D.wg_n > 0;   // FluidSystem::enableVaporizedOil()
    const double Swco = B[Sd.swco];
    const E Sw = mk<E>(pv[0], 0);
    E Sg = cst<E>(0.0);
    if (meaning == OPMHIP_SW_PO_SG) Sg = mk<E>(pv[2], 2);
    else if (EXT && meaning == OPMHIP_SW_PG_RV) Sg = 1.0 - Sw;   // the oil phase is absent
    const E So = 1.0 - Sw - Sg;
    q.S[WATER] = Sw; q.S[GAS] = Sg; q.S[OIL] = So;
    // capillary pressures (EclDefaultMaterial): pC[water] = -pcow(Sw), pC[oil] = 0, pC[gas] = pcgo(1 - Swco - Sg)
    E pC[3];
    const bool scaled = EXT && C.eps;
    double epsU[EXT ? EPS_COUNT : 1], epsS[EXT ? EPS_COUNT : 1];
    if (scaled) {
        eps_load<DP>(C, c, B, Sd, epsU, epsS);
        cap_pressures_eps<E, DP>(B, Sd, C.epscfg, epsU, epsS, Sw, Sg, pC);
    } else {
        pC[0] = -pwlin<E, DP>(B + Sd.sw_x, B + Sd.pcow, Sd.nw, Sw);
        pC[1] = cst<E>(0.0);
        pC[2] = pwlin<E, DP>(B + Sd.so_x, B + Sd.pcgo, Sd.ng, 1.0 - Swco - Sg);
    }
    if (EXT && C.pcw && !scaled) {
        // end-point scaling of the oil-water curve (EclEpsTwoPhaseLaw with enablePcScaling): table value x (scaled max / table max),
        // the table's maximum being its value at the connate saturation (first row of SWOF)
        const double scaledMax = C.pcw[c], tableMax = B[Sd.pcow];
        const double alpha = (scaledMax == tableMax) ? 1.0 : scaledMax / tableMax;
        pC[0] = pC[0] * alpha;
    }
    if (EXT && meaning == OPMHIP_SW_PG_RV) {   // the pressure primary variable is the GAS pressure
        const E pg = mk<E>(pv[1], 1);
        for (int ph = 0; ph < 3; ++ph) q.p[ph] = pg + (pC[ph] - pC[GAS]);
    } else {
        const E po = mk<E>(pv[1], 1);
        for (int ph = 0; ph < 3; ++ph) q.p[ph] = po + (pC[ph] - pC[OIL]);
    }
    // relative permeabilities (stored in mob, divided by viscosity below)
    if (EXT && C.hyst) rel_perms_hyst<E, DP>(T, C, c, Sd, scaled, epsU, epsS, Sw, Sg, q.mob);
    else if (scaled) rel_perms_eps<E, DP>(B, Sd, C.epscfg, epsU, epsS, Sw, Sg, q.mob);
    else {
        q.mob[WATER] = pwlin<E, DP>(B + Sd.sw_x, B + Sd.krw, Sd.nw, Sw);
        q.mob[GAS] = pwlin<E, DP>(B + Sd.so_x, B + Sd.krg, Sd.ng, 1.0 - Swco - Sg);
        const E Swm = emax(cst<E>(Swco), Sw);
        const E Sw_ow = Sg + Swm;
        const E So_go = 1.0 - Sw_ow;
        const E kro_ow = pwlin<E, DP>(B + Sd.sw_x, B + Sd.krow, Sd.nw, Sw_ow);
        const E kro_go = pwlin<E, DP>(B + Sd.so_x, B + Sd.krog, Sd.ng, So_go);
        const double eps = 1e-5;
        if (val(Sw_ow) - Swco < eps) {
            const E kro2 = (kro_ow + kro_go) / 2.0;
            if (val(Sw_ow) - Swco > eps / 2.0) {
                const E kro1 = (Sg * kro_go + (Swm - Swco) * kro_ow) / (Sw_ow - Swco);
                const E alpha = (eps - (Sw_ow - Swco)) / (eps / 2.0);
                q.mob[OIL] = kro2 * alpha + kro1 * (1.0 - alpha);
            } else q.mob[OIL] = kro2;
        } else q.mob[OIL] = (Sg * kro_go + (Swm - Swco) * kro_ow) / (Sw_ow - Swco);
    }
    // Rs / Rv by the meaning of the switching variable, capped by RsMax / RvMax (DRSDT / DRVDT, eclproblem.hh:1711-1754)
    if (EXT) q.Rv = cst<E>(0.0);
    const bool vap = EXT && C.maxso;   // VAPPARS: SoMax = max(So, problem.maxOilSaturation)
    E SoMax = So;
    if (vap) SoMax = emax(So, cst<E>(C.maxso[c]));
    if (meaning == OPMHIP_SW_PO_SG || (EXT && meaning == OPMHIP_SW_PG_RV)) {
        // (Sw_pg_Rv: the oil phase is not present, its "composition" is still needed for the gravity term)
        E RsSat = tab1<E, DP>(B + D.sat_p, B + D.sat_rs, D.sat_n, q.p[OIL]);
        if (vap) RsSat = RsSat * vappars_factor(So, SoMax, C.vap2);
        q.Rs = emin(cst<E>(RsMax), RsSat);
    } else {
        q.Rs = emin(cst<E>(RsMax), mk<E>(pv[2], 2));
    }
    if (EXT && wet) {
        const double RvMax = C.rvmax ? C.rvmax[c] : DBL_MAX / 2.0;
        if (meaning == OPMHIP_SW_PG_RV) q.Rv = emin(cst<E>(RvMax), mk<E>(pv[2], 2));
        else {
            E RvSat = tab1<E, DP>(B + D.wg_xs, B + D.wgs_rv, D.wg_n, q.p[GAS]);
            if (vap) RvSat = RvSat * vappars_factor(So, SoMax, C.vap1);
            q.Rv = emin(cst<E>(RvMax), RvSat);
        }
    }
    // 1/B and viscosity per phase, each at its own phase pressure (BlackOilFluidSystem)
    {
        const bool saturated = val(q.S[GAS]) > 0.0 && val(q.Rs) >= (1.0 - 1e-10) * rs_sat_value(T, pr, val(q.p[OIL]));
        const DP W = B + D.water;  // p_ref, Bw_ref, c_w, mu_ref, c_v
        const E X = W[2] * (q.p[WATER] - W[0]);
        q.invB[WATER] = (1.0 + X * (1.0 + X / 2.0)) / W[1];
        const E Y = (W[2] - W[4]) * (q.p[WATER] - W[0]);
        E mu = (W[3] * W[1]) * q.invB[WATER] / (1.0 + Y * (1.0 + Y / 2.0));
        q.mob[WATER] = q.mob[WATER] / mu;
        if (saturated) {
            q.invB[OIL] = tab1<E, DP>(B + D.sat_p, B + D.sat_invB, D.sat_n, q.p[OIL]);
            mu = tab1<E, DP>(B + D.sat_p, B + D.sat_invB, D.sat_n, q.p[OIL]) / tab1<E, DP>(B + D.sat_p, B + D.sat_invBMu, D.sat_n, q.p[OIL]);
        } else {
            q.invB[OIL] = tab2<E, DP>(T, D, D.o_invB, q.Rs, q.p[OIL]);
            mu = tab2<E, DP>(T, D, D.o_invB, q.Rs, q.p[OIL]) / tab2<E, DP>(T, D, D.o_invBMu, q.Rs, q.p[OIL]);
        }
        q.mob[OIL] = q.mob[OIL] / mu;
        if (EXT && wet) {
            const bool gasSaturated = val(q.S[OIL]) > 0.0 && val(q.Rv) >= (1.0 - 1e-10) * rv_sat_value(T, pr, val(q.p[GAS]));
            if (gasSaturated) {
                q.invB[GAS] = tab1<E, DP>(B + D.wg_xs, B + D.wgs_invB, D.wg_n, q.p[GAS]);
                mu = tab1<E, DP>(B + D.wg_xs, B + D.wgs_invB, D.wg_n, q.p[GAS]) / tab1<E, DP>(B + D.wg_xs, B + D.wgs_invBMu, D.wg_n, q.p[GAS]);
            } else {
                q.invB[GAS] = tab2wg<E, DP>(T, D, D.wg_invB, q.p[GAS], q.Rv);
                mu = tab2wg<E, DP>(T, D, D.wg_invB, q.p[GAS], q.Rv) / tab2wg<E, DP>(T, D, D.wg_invBMu, q.p[GAS], q.Rv);
            }
        } else {
            q.invB[GAS] = tab1<E, DP>(B + D.gas_p, B + D.gas_invB, D.gas_n, q.p[GAS]);
            mu = tab1<E, DP>(B + D.gas_p, B + D.gas_invB, D.gas_n, q.p[GAS]) / tab1<E, DP>(B + D.gas_p, B + D.gas_invBMu, D.gas_n, q.p[GAS]);
        }
        q.mob[GAS] = q.mob[GAS] / mu;
    }
    const DP rr = B + D.density;  // oil, water, gas
    q.rho[WATER] = q.invB[WATER] * rr[1];
    q.rho[GAS] = q.invB[GAS] * rr[2];
    if (EXT && wet) q.rho[GAS] = q.rho[GAS] + q.invB[GAS] * q.Rv * rr[0];   // vaporised oil
    q.rho[OIL] = q.invB[OIL] * rr[0];
    q.rho[OIL] = q.rho[OIL] + q.invB[OIL] * q.Rs * rr[2];
    q.poro = cst<E>(refPoro);
    if (T.rock_cr > 0.0) {
        const E x = T.rock_cr * (q.p[OIL] - T.rock_pref);
        q.poro = q.poro * (1.0 + x + 0.5 * x * x);
    }
    if (EXT) {
        // rock compaction tables: rockCompPoroMultiplier / rockCompTransMultiplier (ebos/eclproblem.hh:1936-2007), reversible form
        q.tmult = cst<E>(1.0);
        if (T.num_rock > 0) {
            const RockTabDesc& R = T.rock(C.rocknum ? C.rocknum[c] : 0);
            E effectiveOilPressure = q.p[OIL];
            if (C.minpo) effectiveOilPressure = emin(q.p[OIL], cst<E>(C.minpo[c]));   // the pore space change is irreversible (eclproblem.hh:1948-1952)
            if (C.overburden) effectiveOilPressure = effectiveOilPressure - C.overburden[c];
            q.poro = q.poro * tab1<E, DP>(B + R.p, B + R.poroMult, R.n, effectiveOilPressure);
            q.tmult = tab1<E, DP>(B + R.p, B + R.transMult, R.n, effectiveOilPressure);
        } else if (C.wcdesc) {   // water compaction (eclproblem.hh:1962-1967, 2001-2005)
            const int* d = C.wcdesc + 6 * (C.rocknum ? C.rocknum[c] : 0);
            E effectiveOilPressure = q.p[OIL];
            if (C.minpo) effectiveOilPressure = emin(q.p[OIL], cst<E>(C.minpo[c]));
            if (C.overburden) effectiveOilPressure = effectiveOilPressure - C.overburden[c];
            const E SwMax = emax(q.S[WATER], cst<E>(C.maxsw[c]));
            const E SwDeltaMax = SwMax - C.sw0[c];
            q.poro = q.poro * wc_eval<E>(d, C.wcdata, d[4], effectiveOilPressure, SwDeltaMax);
            if (d[5] >= 0) q.tmult = wc_eval<E>(d, C.wcdata, d[5], effectiveOilPressure, SwDeltaMax);
        }
    }
}

__device__ __forceinline__ void store_ad(double* o, const Ad& a) {
    *reinterpret_cast<double2*>(o) = make_double2(a.v, a.d0);
    *reinterpret_cast<double2*>(o + 2) = make_double2(a.d1, a.d2);
}
__device__ __forceinline__ Ad load_ad(const double* o) {
    const double2 a = *reinterpret_cast<const double2*>(o), b = *reinterpret_cast<const double2*>(o + 2);
    return Ad{a.x, a.y, b.x, b.y};
}
// the convergence check needs 1/b of the three phases and nothing else of the record (flow/BlackoilModelEbos.hpp:650-664):
// a packed copy (24 B per cell) spares it a 544-byte-strided walk through the cache (PMC: 232 MB of traffic for 56 MB of data)
__device__ __forceinline__ void store_invb(double* invb, int c, const Iq<Ad>& q) {
    invb[(size_t)c * 3] = q.invB[0].v; invb[(size_t)c * 3 + 1] = q.invB[1].v; invb[(size_t)c * 3 + 2] = q.invB[2].v;
}
template <bool EXT>
__device__ __forceinline__ void store_iq(double* iq, int ncell, int c, const Iq<Ad>& q) {
    for (int k = 0; k < 3; ++k) {
        store_ad(iq_at(iq, ncell, F_S + k, c), q.S[k]); store_ad(iq_at(iq, ncell, F_P + k, c), q.p[k]); store_ad(iq_at(iq, ncell, F_B + k, c), q.invB[k]);
        store_ad(iq_at(iq, ncell, F_MOB + k, c), q.mob[k]); store_ad(iq_at(iq, ncell, F_RHO + k, c), q.rho[k]);
    }
    store_ad(iq_at(iq, ncell, F_RS, c), q.Rs);
    if (EXT) { store_ad(iq_at(iq, ncell, Lay<EXT>::F_RV, c), q.Rv); store_ad(iq_at(iq, ncell, Lay<EXT>::F_TMULT, c), q.tmult); }
    store_ad(iq_at(iq, ncell, Lay<EXT>::F_PORO, c), q.poro);
}

// invalidateAndUpdateIntensiveQuantities(0): one lane per cell
// The per-cell kernels walk the property tables with binary searches: ~130 dependent loads per cell, each an L1 round
// trip (PMC: 41 us per wavefront).  The tables are a few KiB, so every workgroup copies the double blob into LDS first
// and searches there with ds_read (LdsTab); tables too large for the LDS budget stay in global memory (GlobalTab).
constexpr int TAB_LDS_DBL = 3072;   // 24 KiB
template <class DP, bool EXT>
__device__ __forceinline__ void iq_update_cell(const TablesT<DP>& T, const CellStatic& C, int c, const double* __restrict__ pv,
                                               const unsigned char* __restrict__ meaning, double* __restrict__ iq) {
    const double x[3] = {pv[(size_t)c * 3], pv[(size_t)c * 3 + 1], pv[(size_t)c * 3 + 2]};
    Iq<Ad> q;
    update_iq<Ad, DP, EXT>(T, C, c, x, meaning[c], q);
    store_iq<EXT>(iq, C.ncell, c, q);
    store_invb(C.invb, c, q);
}
// copies the blob into `s_tab` (workgroup-wide, contains a barrier); true if the tables fit
__device__ __forceinline__ bool tables_to_lds(const Tables& T, double* s_tab) {
    if (T.ndbl > TAB_LDS_DBL) return false;
    for (int i = threadIdx.x; i < T.ndbl; i += blockDim.x) s_tab[i] = T.dbl[i];
    __syncthreads();
    return true;
}
__device__ __forceinline__ TablesT<LdsTab> lds_tables(const Tables& T, double* s_tab) {
    return TablesT<LdsTab>{(LdsTab)s_tab, T.idx, T.rock_pref, T.rock_cr, T.ndbl, T.nidx, T.rock_desc, T.num_rock};
}
// The base layout's two per-cell kernels are held to three wavefronts per SIMD (168 VGPRs; left alone they take 172-174 and
// run two: 0.1865 -> 0.1742 ms on the bench, four waves spill and lose).  The extended layout needs 202 registers and stays free.
#ifndef OPMHIP_IQ_WAVES
#define OPMHIP_IQ_WAVES 3
#endif
#if OPMHIP_IQ_WAVES > 0
#define IQ_OCC __attribute__((amdgpu_waves_per_eu(OPMHIP_IQ_WAVES, OPMHIP_IQ_WAVES)))
#else
#define IQ_OCC
#endif
template <bool EXT>
__device__ __forceinline__ void iq_update_body(int c0, int Nb, const Tables& T, const CellStatic& C, const double* __restrict__ pv,
                                               const unsigned char* __restrict__ meaning, double* __restrict__ iq) {
    __shared__ double s_tab[TAB_LDS_DBL];
    const bool inLds = tables_to_lds(T, s_tab);
    const int c = c0 + blockIdx.x * blockDim.x + threadIdx.x;  // cells [c0, Nb)
    if (c >= Nb) return;
    if (inLds) iq_update_cell<LdsTab, EXT>(lds_tables(T, s_tab), C, c, pv, meaning, iq);
    else iq_update_cell<GlobalTab, EXT>(T, C, c, pv, meaning, iq);
}
template <bool EXT>
__global__ __launch_bounds__(256) void k_iq_update(int c0, int Nb, Tables T, CellStatic C, const double* __restrict__ pv,
                                                   const unsigned char* __restrict__ meaning, double* __restrict__ iq) {
    iq_update_body<EXT>(c0, Nb, T, C, pv, meaning, iq);
}
template <>
__global__ __launch_bounds__(256) IQ_OCC void k_iq_update<false>(int c0, int Nb, Tables T, CellStatic C, const double* __restrict__ pv,
                                                                 const unsigned char* __restrict__ meaning, double* __restrict__ iq) {
    iq_update_body<false>(c0, Nb, T, C, pv, meaning, iq);
}

// BlackOilNewtonMethod::update_ (chopped update) + BlackOilPrimaryVariables::adaptPrimaryVariables + IQ recompute
template <class DP, bool EXT>
__device__ __forceinline__ void newton_update_cell(const TablesT<DP>& T, const CellStatic& C, int c, const double* __restrict__ dx, double relax,
                                                   double* __restrict__ pv, unsigned char* __restrict__ meaning,
                                                   unsigned char* __restrict__ wasSwitched, double* __restrict__ iq,
                                                   int* __restrict__ nswitched) {
    const double dpMaxRel = 0.3, dsMax = 0.2, oscThreshold = 1e-5;
    double x[3] = {pv[(size_t)c * 3], pv[(size_t)c * 3 + 1], pv[(size_t)c * 3 + 2]};
    double u[3] = {dx[(size_t)c * 3], dx[(size_t)c * 3 + 1], dx[(size_t)c * 3 + 2]};
    if (relax != 1.0) { u[0] *= relax; u[1] *= relax; u[2] *= relax; }
    int mng = meaning[c];
    const double deltaSw = u[0];
    double deltaSo = -deltaSw, deltaSg = 0.0;
    if (mng == OPMHIP_SW_PO_SG) { deltaSg = u[2]; deltaSo -= deltaSg; }
    double maxSatDelta = fmax(fabs(deltaSg), fabs(deltaSo));
    maxSatDelta = fmax(maxSatDelta, fabs(deltaSw));
    double satAlpha = 1.0;
    if (maxSatDelta > dsMax) satAlpha = dsMax / maxSatDelta;
    double nx[3];
    {
        double delta = u[0] * satAlpha;
        nx[0] = x[0] - delta;
        delta = u[1];
        if (fabs(delta) > dpMaxRel * x[1]) delta = (delta < 0.0 ? -1.0 : 1.0) * dpMaxRel * x[1];
        nx[1] = x[1] - delta;
        delta = u[2];
        if (mng == OPMHIP_SW_PO_SG) delta *= satAlpha;
        else if (delta > x[2]) delta = x[2];   // Rs / Rv must not become negative
        nx[2] = x[2] - delta;
    }
    x[0] = nx[0]; x[1] = nx[1]; x[2] = nx[2];
    const int pr = C.pvtnum ? C.pvtnum[c] : 0, sr = C.satnum ? C.satnum[c] : 0;
    const double RsMax = C.rsmax ? C.rsmax[c] : DBL_MAX / 2.0;
    const bool wet = EXT && T.pvt(pr).wg_n > 0;
    const double eps = wasSwitched[c] ? oscThreshold : 0.0;
    bool sw = false;
    // VAPPARS in the switches (adaptPrimaryVariables: SoMax = max(So, problem.maxOilSaturation)); 1 where it is not in force
    const bool vap = EXT && C.maxso;
    auto vap_f = [&](double So_, double par) { return vap ? vappars_factor<double>(So_, emax(So_, C.maxso[c]), par) : 1.0; };
    if (x[0] >= 1.0) {   // cells with (almost) only water
        x[0] = 1.0; x[2] = 0.0;
        sw = mng != OPMHIP_SW_PO_SG;
        mng = OPMHIP_SW_PO_SG;
    } else if (mng == OPMHIP_SW_PO_SG) {
        const double So = 1.0 - x[0] - x[2];
        if (x[2] < -eps && So > 0.0) {   // the gas phase disappears
            mng = OPMHIP_SW_PO_RS;
            x[2] = emin(RsMax, rs_sat_value(T, pr, x[1]) * vap_f(So, C.vap2));
            sw = true;
        } else if (EXT && wet && So < -eps && x[2] > 0.0) {   // the oil phase disappears: { Sw, pg, Rv }
            double pC[3];
            cell_cap_pressures<DP, EXT>(T, C, c, sr, x[0], x[2], pC);
            const double pg = x[1] + (pC[GAS] - pC[OIL]);
            const double RvMax = C.rvmax ? C.rvmax[c] : DBL_MAX / 2.0;
            mng = OPMHIP_SW_PG_RV;
            x[1] = pg;
            x[2] = emin(RvMax, rv_sat_value(T, pr, pg) * vap_f(So, C.vap1));
            sw = true;
        }
    } else if (!EXT || mng == OPMHIP_SW_PO_RS) {
        const double RsSat = rs_sat_value(T, pr, x[1]) * vap_f(1.0 - x[0], C.vap2);   // no gas: So = 1 - Sw
        if (x[2] > emin(RsMax, RsSat * (1.0 + eps))) { mng = OPMHIP_SW_PO_SG; x[2] = 0.0; sw = true; }
    } else {   // Sw_pg_Rv: the oil phase appears once the gas holds more oil than saturated gas does
        const double RvMax = C.rvmax ? C.rvmax[c] : DBL_MAX / 2.0;
        const double RvSat = rv_sat_value(T, pr, x[1]) * vap_f(0.0, C.vap1);   // no oil phase: So = 0
        if (x[2] > emin(RvMax, RvSat * (1.0 + eps))) {
            double pC[3];
            cell_cap_pressures<DP, EXT>(T, C, c, sr, x[0], 1.0 - x[0], pC);
            mng = OPMHIP_SW_PO_SG;
            x[1] = x[1] + (pC[OIL] - pC[GAS]);
            x[2] = 1.0 - x[0];
            sw = true;
        }
    }
    wasSwitched[c] = sw ? 1 : 0;
    meaning[c] = (unsigned char)mng;
    pv[(size_t)c * 3] = x[0]; pv[(size_t)c * 3 + 1] = x[1]; pv[(size_t)c * 3 + 2] = x[2];
    if (sw) atomicAdd(nswitched, 1);
    Iq<Ad> q;
    update_iq<Ad, DP, EXT>(T, C, c, x, mng, q);
    store_iq<EXT>(iq, C.ncell, c, q);
    store_invb(C.invb, c, q);
}
template <bool EXT>
__device__ __forceinline__ void newton_update_body(int Nb, const Tables& T, const CellStatic& C, const double* __restrict__ dx, double relax,
                                                   double* __restrict__ pv, unsigned char* __restrict__ meaning,
                                                   unsigned char* __restrict__ wasSwitched, double* __restrict__ iq,
                                                   int* __restrict__ nswitched) {
    __shared__ double s_tab[TAB_LDS_DBL];
    const bool inLds = tables_to_lds(T, s_tab);
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= Nb) return;
    if (inLds) newton_update_cell<LdsTab, EXT>(lds_tables(T, s_tab), C, c, dx, relax, pv, meaning, wasSwitched, iq, nswitched);
    else newton_update_cell<GlobalTab, EXT>(T, C, c, dx, relax, pv, meaning, wasSwitched, iq, nswitched);
}
template <bool EXT>
__global__ __launch_bounds__(256) void k_newton_update(int Nb, Tables T, CellStatic C, const double* __restrict__ dx, double relax,
                                                       double* __restrict__ pv, unsigned char* __restrict__ meaning,
                                                       unsigned char* __restrict__ wasSwitched, double* __restrict__ iq,
                                                       int* __restrict__ nswitched) {
    newton_update_body<EXT>(Nb, T, C, dx, relax, pv, meaning, wasSwitched, iq, nswitched);
}
template <>
__global__ __launch_bounds__(256) IQ_OCC void k_newton_update<false>(int Nb, Tables T, CellStatic C, const double* __restrict__ dx, double relax,
                                                                     double* __restrict__ pv, unsigned char* __restrict__ meaning,
                                                                     unsigned char* __restrict__ wasSwitched, double* __restrict__ iq,
                                                                     int* __restrict__ nswitched) {
    newton_update_body<false>(Nb, T, C, dx, relax, pv, meaning, wasSwitched, iq, nswitched);
}

static Tables tables_of(const opmhip_ctx* c);
// 1/B of the three phases at one point (plain doubles): the one body behind opmhip_fluid_probe / opmhip_gas_probe and the well-bore
// density of the resident standard wells (k_std_wells_wellbore), which therefore carries the probes' bits
__device__ __forceinline__ double pvt_invBw(const Tables& T, const PvtRegionDesc& D, double p) {
    const GlobalTab W = T.dbl + D.water;   // p_ref, Bw_ref, c_w, mu_ref, c_v
    const double X = W[2] * (p - W[0]);
    return (1.0 + X * (1.0 + X / 2.0)) / W[1];
}
__device__ __forceinline__ double pvt_invBo(const Tables& T, int pr, const PvtRegionDesc& D, double p, double rs) {
    const GlobalTab B = T.dbl;
    if (rs >= rs_sat_value(T, pr, p)) return tab1<double, GlobalTab>(B + D.sat_p, B + D.sat_invB, D.sat_n, p);
    return tab2<double, GlobalTab>(T, D, D.o_invB, rs, p);
}
__device__ __forceinline__ double pvt_invBg(const Tables& T, int pr, const PvtRegionDesc& D, double p, double rv) {
    const GlobalTab B = T.dbl;
    if (D.wg_n > 0) {
        if (rv >= rv_sat_value(T, pr, p)) return tab1<double, GlobalTab>(B + D.wg_xs, B + D.wgs_invB, D.wg_n, p);
        return tab2wg<double, GlobalTab>(T, D, D.wg_invB, p, rv);
    }
    return tab1<double, GlobalTab>(B + D.gas_p, B + D.gas_invB, D.gas_n, p);
}
// opmhip_fluid_probe: the property functions of update_iq at given points (plain doubles)
__global__ __launch_bounds__(256) void k_fluid_probe(Tables T, int pr, int sr, int n, const double* __restrict__ p,
                                                     const double* __restrict__ rs, const double* __restrict__ sw,
                                                     const double* __restrict__ sg, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PvtRegionDesc& D = T.pvt(pr);
    const SatRegionDesc& Sd = T.sat(sr);
    const GlobalTab B = T.dbl;
    double* o = out + (size_t)i * 8;
    const double pi = p[i], rsi = rs[i];
    o[0] = pvt_invBw(T, D, pi);
    const bool wetg = D.wg_n > 0;   // PVTG: the saturated curve
    o[1] = wetg ? tab1<double, GlobalTab>(B + D.wg_xs, B + D.wgs_invB, D.wg_n, pi) : tab1<double, GlobalTab>(B + D.gas_p, B + D.gas_invB, D.gas_n, pi);
    const double RsSat = rs_sat_value(T, pr, pi);
    o[3] = RsSat;
    o[2] = pvt_invBo(T, pr, D, pi, rsi);
    if (rsi >= RsSat) o[6] = o[2] / tab1<double, GlobalTab>(B + D.sat_p, B + D.sat_invBMu, D.sat_n, pi);
    else o[6] = o[2] / tab2<double, GlobalTab>(T, D, D.o_invBMu, rsi, pi);
    const double Swco = B[Sd.swco];
    o[4] = pwlin<double, GlobalTab>(B + Sd.sw_x, B + Sd.pcow, Sd.nw, sw[i]);
    o[5] = pwlin<double, GlobalTab>(B + Sd.so_x, B + Sd.pcgo, Sd.ng, 1.0 - Swco - sg[i]);
    o[7] = o[1] / (wetg ? tab1<double, GlobalTab>(B + D.wg_xs, B + D.wgs_invBMu, D.wg_n, pi) : tab1<double, GlobalTab>(B + D.gas_p, B + D.gas_invBMu, D.gas_n, pi));
}
// opmhip_gas_probe: wet-gas functions at (p_g, Rv): 1/B_g and mu_g on the saturated curve where Rv >= RvSat(p_g), else the
// undersaturated 2-D tables; RvSat(p_g).  Dry gas: 1/B_g(p), mu_g(p), 0.
__global__ __launch_bounds__(256) void k_gas_probe(Tables T, int pr, int n, const double* __restrict__ p, const double* __restrict__ rv,
                                                   double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PvtRegionDesc& D = T.pvt(pr);
    const GlobalTab B = T.dbl;
    double* o = out + (size_t)i * 3;
    const double pi = p[i], rvi = rv[i];
    o[0] = pvt_invBg(T, pr, D, pi, rvi);
    if (D.wg_n > 0) {
        const double RvSat = rv_sat_value(T, pr, pi);
        o[2] = RvSat;
        if (rvi >= RvSat) o[1] = o[0] / tab1<double, GlobalTab>(B + D.wg_xs, B + D.wgs_invBMu, D.wg_n, pi);
        else o[1] = o[0] / tab2wg<double, GlobalTab>(T, D, D.wg_invBMu, pi, rvi);
    } else {
        o[1] = o[0] / tab1<double, GlobalTab>(B + D.gas_p, B + D.gas_invBMu, D.gas_n, pi);
        o[2] = 0.0;
    }
}
int launch_gas_probe(opmhip_ctx* c, int pr, int n, const double* d_in, double* d_out) {
    hipLaunchKernelGGL(k_gas_probe, dim3((n + 255) / 256), dim3(256), 0, c->stream, tables_of(c), pr, n, d_in, d_in + n, d_out);
    return OPMHIP_SUCCESS;
}
// opmhip_sat_probe: the saturation functions with one set of scaled end points (eps[EPS_COUNT]; cfg = packed EclEpsConfig) or,
// cfg < 0, the tables' own: out[5 i ..] = krw, kro, krg, pcow, pcgo at (sw, sg) - the functions update_iq evaluates
__global__ __launch_bounds__(256) void k_sat_probe(Tables T, int sr, int cfg, const double* __restrict__ eps, int n, const double* __restrict__ sw,
                                                   const double* __restrict__ sg, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SatRegionDesc& Sd = T.sat(sr);
    const GlobalTab B = T.dbl;
    double u[EPS_COUNT], s[EPS_COUNT];
#pragma unroll
    for (int f = 0; f < EPS_COUNT; ++f) { u[f] = B[Sd.eps + f]; s[f] = cfg >= 0 ? eps[f] : u[f]; }
    double kr[3], pC[3];
    rel_perms_eps<double, GlobalTab>(B, Sd, cfg >= 0 ? cfg : 0, u, s, sw[i], sg[i], kr);
    cap_pressures_eps<double, GlobalTab>(B, Sd, cfg >= 0 ? cfg : 0, u, s, sw[i], sg[i], pC);
    double* o = out + (size_t)i * 5;
    o[0] = kr[0]; o[1] = kr[1]; o[2] = kr[2]; o[3] = -pC[0]; o[4] = pC[2];
}
int launch_sat_probe(opmhip_ctx* c, int sr, int cfg, const double* d_eps, int n, const double* d_in, double* d_out) {
    hipLaunchKernelGGL(k_sat_probe, dim3((n + 255) / 256), dim3(256), 0, c->stream, tables_of(c), sr, cfg, d_eps, n, d_in, d_in + n, d_out);
    return OPMHIP_SUCCESS;
}
int launch_fluid_probe(opmhip_ctx* c, int pr, int sr, int n, const double* d_in, double* d_out) {
    hipLaunchKernelGGL(k_fluid_probe, dim3((n + 255) / 256), dim3(256), 0, c->stream, tables_of(c), pr, sr, n, d_in, d_in + n, d_in + 2 * (size_t)n,
                       d_in + 3 * (size_t)n, d_out);
    return OPMHIP_SUCCESS;
}

// ============================== face flux ===================================================================
// calculateGradients_ + computeFlux for one face: `in` = focus (interior) cell with derivatives, `ex` = exterior cell,
// of which only values enter.  Result: flux[eq] * faceArea.  The two cells come through accessors: PtrQ reads a record
// of the IQ cache where it lies (here: the tile's own rows, staged in LDS), RegQ holds the flux-relevant fields of one
// record in registers (the neighbour cell, fetched with one batch of loads before any of the branchy arithmetic).
struct PtrQ {
    const double* q;
    __device__ __forceinline__ Ad ad(int f) const { return load_ad(q + f * 4); }
    __device__ __forceinline__ double v(int f) const { return q[f * 4]; }
};
template <bool EXT>
struct RegQ {   // fields F_P .. F_RS (.. tmult): p, 1/B, mobility, density (3 phases each), Rs [, Rv, transmissibility multiplier]
    static constexpr int F0 = Lay<EXT>::RQ_F0;
    double r[Lay<EXT>::RQ_NF * 4];
    __device__ __forceinline__ Ad ad(int f) const { return Ad{r[(f - F0) * 4], r[(f - F0) * 4 + 1], r[(f - F0) * 4 + 2], r[(f - F0) * 4 + 3]}; }
    __device__ __forceinline__ double v(int f) const { return r[(f - F0) * 4]; }
};
// keeps a batch of loads together: the values must exist here, so the compiler cannot sink each load into the branch
// that consumes it (where it would cost its own LDS round trip)
__device__ __forceinline__ void pin(Ad& a) { asm volatile("" : "+v"(a.v), "+v"(a.d0), "+v"(a.d1), "+v"(a.d2)); }
__device__ __forceinline__ void pin(double& a) { asm volatile("" : "+v"(a)); }
template <bool EXT, class IN, class EX>
__device__ __forceinline__ void face_flux(const IN& in, const EX& ex, bool wet, double trans, double faceArea,
                                          double thpres, double zIn, double zEx, double Vin, double Vex, bool inLower, Ad flux[3]) {
    flux[0] = flux[1] = flux[2] = ad_const(0.0);
    const double distZ = zIn - zEx;
    const int comp[3] = {EQ_WATER, EQ_OIL, EQ_GAS};
    Ad tmIn = ad_const(1.0);   // transMult = rockCompTransMultiplier of the upstream cell (eclfluxmodule.hh:340-355)
    double tmEx = 1.0;
    if (EXT) { tmIn = in.ad(Lay<EXT>::F_TMULT); tmEx = ex.v(Lay<EXT>::F_TMULT); }
#pragma unroll
    for (int ph = 0; ph < 3; ++ph) {
        // everything this phase may need of the two cells in ONE round of (LDS) loads, before the branches
        Ad mobIn = in.ad(F_MOB + ph), rhoIn = in.ad(F_RHO + ph), pIn = in.ad(F_P + ph), bIn = in.ad(F_B + ph);
        double mobEx = ex.v(F_MOB + ph), rhoEx = ex.v(F_RHO + ph), pEx = ex.v(F_P + ph), bEx = ex.v(F_B + ph);
        Ad rIn = ad_const(0.0);   // Rs with the oil phase, Rv with the gas phase
        double rEx = 0.0;
        if (ph == OIL) { rIn = in.ad(F_RS); rEx = ex.v(F_RS); }
        if (EXT && ph == GAS) { rIn = in.ad(Lay<EXT>::F_RV); rEx = ex.v(Lay<EXT>::F_RV); }
        pin(mobIn); pin(rhoIn); pin(pIn); pin(bIn); pin(mobEx); pin(rhoEx); pin(pEx); pin(bEx);
        if (ph == OIL || (EXT && ph == GAS)) { pin(rIn); pin(rEx); }
        if (mobIn.v <= 0.0 && mobEx <= 0.0) continue;
        const Ad rhoAvg = (rhoIn + rhoEx) / 2.0;
        Ad pressureExterior = ad_const(pEx);
        pressureExterior = pressureExterior + rhoAvg * (distZ * GRAVITY);
        Ad dp = pressureExterior - pIn;
        bool upIn;
        if (dp.v > 0.0) upIn = false;
        else if (dp.v < 0.0) upIn = true;
        else if (Vin > Vex) upIn = true;
        else if (Vin < Vex) upIn = false;
        else upIn = inLower;  // equal pressures and volumes: the lower GLOBAL index is upstream (eclfluxmodule.hh:303-314)
        if (fabs(dp.v) > thpres) {
            if (dp.v < 0.0) dp = dp + thpres; else dp = dp - thpres;
        } else continue;
        Ad volumeFlux, surf;
        if (upIn) {
            volumeFlux = dp * mobIn * (EXT ? tmIn : ad_const(1.0)) * (-trans / faceArea);
            surf = bIn * volumeFlux;
        } else {
            volumeFlux = dp * (mobEx * (EXT ? tmEx : 1.0) * (-trans / faceArea));
            surf = bEx * volumeFlux;
        }
        flux[comp[ph]] = flux[comp[ph]] + surf;
        if (ph == OIL) {
            if (upIn) flux[EQ_GAS] = flux[EQ_GAS] + rIn * surf;
            else flux[EQ_GAS] = flux[EQ_GAS] + rEx * surf;
        } else if (EXT && ph == GAS && wet) {   // vaporised oil carried by the gas phase
            if (upIn) flux[EQ_OIL] = flux[EQ_OIL] + rIn * surf;
            else flux[EQ_OIL] = flux[EQ_OIL] + rEx * surf;
        }
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) flux[e] = flux[e] * faceArea;
}

// ============================== assembly ======================================================================
#ifndef OPMHIP_ASM_THREADS
#define OPMHIP_ASM_THREADS 64
#endif
constexpr int ASM_THREADS = OPMHIP_ASM_THREADS;  // 64: one wavefront per tile (9 rows of a 7-point grid); measured 0.80 ms against 0.84 (128) and 0.88 (256): no cross-wave barrier stalls
static_assert(ASM_THREADS == 64, "k_assemble: one lane per entry of a one-wavefront tile");
constexpr int ASM_MAX_ROWS = ASM_THREADS / 7 + 4;  // rows of one tile (their IQ records are staged in LDS); 36 of 40 on a 7-point grid
int asm_max_rows() { return ASM_MAX_ROWS; }
int asm_threads() { return ASM_THREADS; }
#ifndef OPMHIP_ASM_WAVES
#define OPMHIP_ASM_WAVES 3
#endif
#if OPMHIP_ASM_WAVES > 0
#define ASM_OCC __attribute__((amdgpu_waves_per_eu(OPMHIP_ASM_WAVES, OPMHIP_ASM_WAVES)))
#else
#define ASM_OCC
#endif
struct EntryStatic {
    const double *trans, *area, *thpres;  // per entry, internal order
};
constexpr int ASM_PRE = 10;  // what a diagonal lane fetches ahead for its cell: storageOld[3], source[3], drift[3], reference porosity
// FvBaseLinearizer::linearizeDomain.  One lane per block-CSR entry, one wavefront per tile of whole rows (<= ASM_THREADS
// entries, <= ASM_MAX_ROWS rows).  The kernel is bound by the latency of its dependent load rounds (PMC: waves wait 65 % of
// their life with two waves per SIMD and seven rounds), so there are two of them and room for three waves per SIMD:
//   1  the tile's schedule record (rows, entries) and - found from the workgroup index alone - every lane's entry record
//      (column, entry word: row inside the tile, tie-break flag, natural summation order; capi_asm.cpp)
//   2  own IQ records -> LDS (coalesced), depth / volume of the rows, per lane transmissibility, area, THPRES;
//      off-diagonal lanes: the neighbour's flux fields -> registers; diagonal lanes: storage of the old time level, source,
//      drift (into the same registers, parked in LDS before the arithmetic starts)
// The arithmetic then runs out of LDS / registers.  LDS: the own records are dead once every face is evaluated; the face
// fluxes and the tile's blocks take their place (11 KiB per workgroup instead of 18).
// SPLIT (opmhip_ctx::split_asm): the blocks leave as two runs, the tile's lower and diagonal entries into the rest stream (A = d_R, rows by
// rrowptr) and its upper entries into the U stream (Uout = d_U, rows by urowptr) - the arrays the sweeps and the rest product read.  Every
// lane's place comes with its entry word, the two row pointers of the tile's first row with round 2's loads: no further round.
template <bool EXT, bool SPLIT>
__global__ __launch_bounds__(ASM_THREADS) ASM_OCC void k_assemble(int nsched, const int4* __restrict__ sched, const int2* __restrict__ desc, int wet,
                                                          EntryStatic ES, CellStatic C, const double* __restrict__ iq,
                                                          double* __restrict__ storageOld, const double* __restrict__ source,
                                                          const double* __restrict__ dsource, const double* __restrict__ drift, double maxCompensation,
                                                          double dt, int iteration, double* __restrict__ A, double* __restrict__ resid,
                                                          double* __restrict__ Uout, const int* __restrict__ rrowptr, const int* __restrict__ urowptr) {
    constexpr int IQS = Lay<EXT>::IQS, RQ_F0 = Lay<EXT>::RQ_F0, RQ_NF = Lay<EXT>::RQ_NF, F_PORO = Lay<EXT>::F_PORO;
    constexpr int N_OWN = ASM_MAX_ROWS * IQS, N_FLUX = ASM_THREADS * 12, N_OUT = N_FLUX + (ASM_THREADS + 2) * BB;
    __shared__ __attribute__((aligned(16))) double sU[N_OWN > N_OUT ? N_OWN : N_OUT];
    double* const sI = sU;              // until the faces are evaluated: IQ records of the tile's rows
    double* const sflux = sU;           // then: face flux seen from the row's cell, 3 equations x (value, 3 derivatives) per entry
    double* const sblk = sU + N_FLUX;   //       and the tile's blocks, streamed out at the end
    __shared__ double sgeo[2 * ASM_MAX_ROWS];
    __shared__ double spre[ASM_MAX_ROWS * ASM_PRE];
    __shared__ unsigned char snat[ASM_THREADS];
    __shared__ short sfirst[ASM_MAX_ROWS + 1];
    static_assert(RQ_NF >= ASM_PRE, "the diagonal lane borrows the value slots of the neighbour record");
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= nsched) return;
    // ---- round 1: the tile's schedule record and, independent of it, the lane's entry (column, entry word)
    const int4 S = sched[blockIdx.x];
    const int2 jm = desc[(size_t)blockIdx.x * ASM_THREADS + tid];
    const int r0 = S.x, k0 = S.z, nent = S.w - S.z, nrows = S.y - S.x;
    const int k0e = k0 & ~1;  // 16-byte aligned start of the output stream
    const bool act = tid < nent;
    const int k = act ? k0 + tid : k0;
    const int J = jm.x;
    const unsigned m = (unsigned)jm.y;
    {   // ---- round 2.  Own records: per field one contiguous run of nrows x 32 bytes of the cache, into per-row records in LDS
        const int n2r = nrows * 2;                              // 16-byte pieces per field
        const unsigned inv = n2r > 0 ? (65536u + n2r - 1) / n2r : 0u;  // i / n2r == (i * inv) >> 16 for the few hundred i of a tile
        const int n2 = n2r * Lay<EXT>::IQF;
        const double2* g2 = reinterpret_cast<const double2*>(iq);
        double2* s2 = reinterpret_cast<double2*>(sI);
        for (int i = tid; i < n2; i += ASM_THREADS) {
            const int fld = (int)(((unsigned)i * inv) >> 16), j = i - fld * n2r;
            s2[(j >> 1) * (IQS / 2) + fld * 2 + (j & 1)] = g2[((size_t)fld * C.ncell + r0) * 2 + j];
        }
    }
    if (tid < nrows) { sgeo[tid] = C.depth[r0 + tid]; sgeo[ASM_MAX_ROWS + tid] = C.volume[r0 + tid]; }
    const double trans = ES.trans[k], area = ES.area[k], thp = ES.thpres ? ES.thpres[k] : 0.0;
    // SPLIT: the tile's runs of the two streams, [rb0, rb1) and [ub0, ub1), and where they stand in sblk - each with the parity of its
    // first double in memory, so that 16-byte pieces of LDS are 16-byte pieces of the stream
    int rb0 = 0, ub0 = 0, nR = 0, nU = 0;
    if (SPLIT) { rb0 = rrowptr[r0]; ub0 = urowptr[r0]; nR = rrowptr[r0 + nrows] - rb0; nU = urowptr[r0 + nrows] - ub0; }
    const int ldsR = (rb0 & 1) * BB;
    const int ldsU = SPLIT ? ldsR + nR * BB + (((ldsR + nR * BB) ^ (ub0 * BB)) & 1) : 0;
    // the lane's block in sblk (doubles): by its entry in the matrix, or by its place in its stream
    const int bofs = SPLIT ? (((m >> 16) & 1u) ? ldsU : ldsR) + (int)((m >> 17) & 127u) * BB : (k - k0e) * BB;
    const int lrow = m & 63;
    const bool lowI = ((m >> 6) & 1u) != 0;
    const int I = r0 + lrow;
    const bool isDiag = act && I == J, isOff = act && I != J;
    snat[tid] = (unsigned char)(m >> 8);
    {
        const int prevRow = __shfl_up(lrow, 1);
        if (act && (tid == 0 || prevRow != lrow)) sfirst[lrow] = (short)tid;
        if (tid == 0) sfirst[nrows] = (short)nent;
    }
    RegQ<EXT> qJ;
    double zJ = 0.0, VJ = 0.0;
    if (isOff) {
        const double2* g2 = reinterpret_cast<const double2*>(iq) + (size_t)J * 2;
#pragma unroll
        for (int i = 0; i < RQ_NF; ++i) {
            const double2 a = g2[(size_t)(RQ_F0 + i) * C.ncell * 2], b = g2[(size_t)(RQ_F0 + i) * C.ncell * 2 + 1];
            qJ.r[4 * i] = a.x; qJ.r[4 * i + 1] = a.y; qJ.r[4 * i + 2] = b.x; qJ.r[4 * i + 3] = b.y;
        }
        zJ = C.depth[J]; VJ = C.volume[J];
    } else if (isDiag) {
        const size_t o = (size_t)I * 3;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            qJ.r[4 * e] = (iteration == 0) ? 0.0 : storageOld[o + e];
            qJ.r[4 * (3 + e)] = source ? source[o + e] : 0.0;
            qJ.r[4 * (6 + e)] = drift ? drift[o + e] : 0.0;
        }
        qJ.r[4 * 9] = drift ? C.poro[I] : 1.0;   // referencePorosity
    }
    __syncthreads();
    const double zI = sgeo[lrow], VI = sgeo[ASM_MAX_ROWS + lrow];
    Ad f[3];         // off-diagonal lane: face flux seen from cell I; diagonal lane: storage term
    double blk[BB];  // off-diagonal lane: block (I,J)
    const PtrQ qI{sI + lrow * IQS};
    if (isOff) {
        face_flux<EXT>(qJ, qI, wet != 0, trans, area, thp, zJ, zI, VJ, VI, !lowI, f);  // focus J: residual[I] -= flux  ->  block (I,J)
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const Ad mm = ad_const(0.0) - f[e];
            blk[e * 3 + 0] = mm.d0; blk[e * 3 + 1] = mm.d1; blk[e * 3 + 2] = mm.d2;
        }
        face_flux<EXT>(qI, qJ, wet != 0, trans, area, thp, zI, zJ, VI, VJ, lowI, f);   // focus I: contribution to R_I
    } else if (isDiag) {
#pragma unroll
        for (int i = 0; i < ASM_PRE; ++i) spre[lrow * ASM_PRE + i] = qJ.r[4 * i];
        // computeStorage: surface volumes per bulk volume
        const Ad poro = qI.ad(F_PORO), Rs = qI.ad(F_RS);
        f[0] = f[1] = f[2] = ad_const(0.0);
        const int comp[3] = {EQ_WATER, EQ_OIL, EQ_GAS};
#pragma unroll
        for (int ph = 0; ph < 3; ++ph) {
            const Ad surfaceVolume = qI.ad(F_S + ph) * qI.ad(F_B + ph) * poro;
            f[comp[ph]] = f[comp[ph]] + surfaceVolume;
            if (ph == OIL) f[EQ_GAS] = f[EQ_GAS] + Rs * surfaceVolume;
            if (EXT && ph == GAS && wet) f[EQ_OIL] = f[EQ_OIL] + qI.ad(Lay<EXT>::F_RV) * surfaceVolume;   // vaporised oil
        }
    }
    __syncthreads();   // every read of the own records is done: their LDS becomes sflux / sblk
    if (isOff) {
#pragma unroll
        for (int e = 0; e < 3; ++e) store_ad(&sflux[tid * 12 + e * 4], f[e]);
        double* b = &sblk[bofs];
#pragma unroll
        for (int q = 0; q < BB; ++q) b[q] = blk[q];
    }
    __syncthreads();
    if (isDiag) {
        Ad R[3] = {ad_const(0.0), ad_const(0.0), ad_const(0.0)};
        // flux terms first (FvBaseLocalResidual::eval), faces in ascending NATURAL neighbour order whatever the
        // internal ordering is, so that the sum is the one the natural-order CPU path forms
        const int e0 = sfirst[lrow], e1 = sfirst[lrow + 1];
        // the next face's flux is read from LDS while the present one is added
        auto face_of = [&](int i) { const int q = e0 + snat[i < e1 ? i : e1 - 1]; return q; };
        Ad nx[3];
        int qn = face_of(e0);
        for (int e = 0; e < 3; ++e) nx[e] = load_ad(&sflux[qn * 12 + e * 4]);
        for (int i = e0; i < e1; ++i) {
            const int q = qn;
            Ad cur[3] = {nx[0], nx[1], nx[2]};
            qn = face_of(i + 1);
            for (int e = 0; e < 3; ++e) nx[e] = load_ad(&sflux[qn * 12 + e * 4]);
            if (q == tid) continue;   // the diagonal entry itself
            for (int e = 0; e < 3; ++e) R[e] = R[e] + cur[e];
        }
        const double V = VI;
        const double* pre = &spre[lrow * ASM_PRE];
        for (int e = 0; e < 3; ++e) {
            double old;
            if (iteration == 0) { old = f[e].v; storageOld[(size_t)I * 3 + e] = old; } else old = pre[e];
            Ad tt = f[e] - old;
            tt = tt * (V / dt);
            R[e] = R[e] + tt;
        }
        // drift compensation (ebos/eclproblem.hh:1847-1875): what the last accepted time step left unconverged in this
        // cell (residual * dt, opmhip_end_time_step) goes back in as a rate, capped at maxCompensation of the pore volume
        double dofDriftRate[3] = {0.0, 0.0, 0.0};
        if (drift) {
            const double poro = pre[9];   // referencePorosity
#pragma unroll
            for (int e = 0; e < 3; ++e) dofDriftRate[e] = pre[6 + e] / (dt * V);
            double totalDriftRate = 0.0;
#pragma unroll
            for (int e = 0; e < 3; ++e) totalDriftRate += fabs(dofDriftRate[e]) * dt * 1.0 / poro;   // eqWeight = 1 (UNVERIFIED, see oracle)
            if (totalDriftRate > maxCompensation) {
#pragma unroll
                for (int e = 0; e < 3; ++e) dofDriftRate[e] *= maxCompensation / totalDriftRate;
            }
        }
        for (int e = 0; e < 3; ++e) {
            Ad s = ad_const(pre[3 + e]);
            if (dsource) { s.d0 = dsource[(size_t)I * 9 + e * 3]; s.d1 = dsource[(size_t)I * 9 + e * 3 + 1]; s.d2 = dsource[(size_t)I * 9 + e * 3 + 2]; }
            s = s / V;
            if (drift) s = s - dofDriftRate[e];
            s = s * V;
            R[e] = R[e] - s;
        }
        double* b = &sblk[bofs];
        for (int e = 0; e < 3; ++e) {
            resid[(size_t)I * 3 + e] = R[e].v;
            b[e * 3 + 0] = R[e].d0; b[e * 3 + 1] = R[e].d1; b[e * 3 + 2] = R[e].d2;
        }
    }
    __syncthreads();
    // stream the tile's blocks out: contiguous range [k0, k1) x 72 B; SPLIT: one such range in either stream
    // (sblk[i] goes to dst[i]: dst is the stream's address moved back by the run's offset in sblk, an even number of doubles)
    auto stream_out = [&](double* dst, int b, int e) {
        // unaligned head / tail doubles go out one by one, the body as double2
        if (e <= b) return;   // (an empty run: the last rows own no upper entry)
        if ((b & 1) && tid == 0) dst[b] = sblk[b];
        if ((e & 1) && tid == 0) dst[e - 1] = sblk[e - 1];
        b = (b + 1) & ~1;
        e = e & ~1;
        const double2* s2 = reinterpret_cast<const double2*>(sblk);
        double2* d2 = reinterpret_cast<double2*>(dst);
        // nontemporal: the Jacobian leaves for good (500 MB), the intensive-quantity records the neighbouring tiles gather stay in L2
        // (0.607 -> 0.601 ms in alternation, profiles/r06_nt_operands_ab.txt)
        typedef double v2d_a __attribute__((ext_vector_type(2)));
        for (int i = (b >> 1) + tid; i < (e >> 1); i += ASM_THREADS) {
            const double2 t = s2[i];
            v2d_a v; v.x = t.x; v.y = t.y;
            __builtin_nontemporal_store(v, reinterpret_cast<v2d_a*>(&d2[i]));
        }
    };
    if (SPLIT) {
        stream_out(A + ((ptrdiff_t)rb0 * BB - ldsR), ldsR, ldsR + nR * BB);
        stream_out(Uout + ((ptrdiff_t)ub0 * BB - ldsU), ldsU, ldsU + nU * BB);
    } else {
        const int head = (k0 - k0e) * BB;      // doubles to skip at the front (0 or 9)
        stream_out(A + (size_t)k0e * BB, head, head + nent * BB);
    }
}

// ============================== convergence ===================================================================
// pass 1 partials per block: R_sum[3], maxCoeff[3], sum(1/b)[3], pvSum ; pass 2: cnvErrorPv
__global__ __launch_bounds__(256) void k_conv_pass1(int Nb, CellStatic C, const double* __restrict__ resid, double* __restrict__ part) {
    __shared__ double sh[10][4];
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    double a[10];
    for (int i = 0; i < 10; ++i) a[i] = (i >= 3 && i < 6) ? -DBL_MAX : 0.0;
    if (c < Nb) {
        const double pvValue = C.poro[c] * C.volume[c];
        const int comp[3] = {EQ_WATER, EQ_OIL, EQ_GAS};
        for (int ph = 0; ph < 3; ++ph) {
            const int e = comp[ph];
            a[6 + e] = 1.0 / C.invb[(size_t)c * 3 + ph];
            const double R2 = resid[(size_t)c * 3 + e];
            a[e] = R2;
            a[3 + e] = fabs(R2) / pvValue;
        }
        a[9] = pvValue;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int i = 0; i < 10; ++i) {
        double v = a[i];
        for (int o = 32; o > 0; o >>= 1) {
            const double w = __shfl_down(v, o, 64);
            v = (i >= 3 && i < 6) ? fmax(v, w) : v + w;
        }
        if (lane == 0) sh[i][wv] = v;
    }
    __syncthreads();
    if (threadIdx.x < 10) {
        const int i = threadIdx.x;
        double v = sh[i][0];
        for (int w = 1; w < 4; ++w) v = (i >= 3 && i < 6) ? fmax(v, sh[i][w]) : v + sh[i][w];
        part[(size_t)blockIdx.x * 10 + i] = v;
    }
}
// one workgroup: reduce the block partials in a fixed order; out[0..9] as above with B_avg divided by Nb
// decomposed runs: the local results are combined over the ranks (sum of R_sum, sum(1/b), pvSum; max of maxCoeff:
// convergenceReduction, flow/BlackoilModelEbos.hpp:572-625) before B_avg is formed with the GLOBAL cell count (:722-727)
__global__ void k_conv_pack(const double* __restrict__ out, double* __restrict__ red) {
    if (threadIdx.x < 3) { red[threadIdx.x] = out[threadIdx.x]; red[3 + threadIdx.x] = out[6 + threadIdx.x]; red[8 + threadIdx.x] = out[3 + threadIdx.x]; }
    if (threadIdx.x == 0) red[6] = out[9];
}
__global__ void k_conv_unpack(const double* __restrict__ red, double global_cells, double* __restrict__ out) {
    if (threadIdx.x < 3) { out[threadIdx.x] = red[threadIdx.x]; out[6 + threadIdx.x] = red[3 + threadIdx.x] / global_cells; out[3 + threadIdx.x] = red[8 + threadIdx.x]; }
    if (threadIdx.x == 0) out[9] = red[6];
}
__global__ __launch_bounds__(256) void k_conv_final1(int nblocks, int Nb, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double sh[10][256];
    double a[10];
    for (int i = 0; i < 10; ++i) a[i] = (i >= 3 && i < 6) ? -DBL_MAX : 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256)
        for (int i = 0; i < 10; ++i) {
            const double v = part[(size_t)b * 10 + i];
            a[i] = (i >= 3 && i < 6) ? fmax(a[i], v) : a[i] + v;
        }
    for (int i = 0; i < 10; ++i) sh[i][threadIdx.x] = a[i];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int i = 0; i < 10; ++i) {
                const double v = sh[i][threadIdx.x + o];
                sh[i][threadIdx.x] = (i >= 3 && i < 6) ? fmax(sh[i][threadIdx.x], v) : sh[i][threadIdx.x] + v;
            }
        __syncthreads();
    }
    if (threadIdx.x < 10) {
        double v = sh[threadIdx.x][0];
        if (threadIdx.x >= 6 && threadIdx.x < 9 && Nb > 0) v /= (double)Nb;  // Nb <= 0: keep the raw sum (decomposed run)
        out[threadIdx.x] = v;
    }
}
__global__ __launch_bounds__(256) void k_conv_pass2(int Nb, CellStatic C, const double* __restrict__ resid, const double* __restrict__ out1,
                                                    double dt, double tol_cnv, double* __restrict__ part) {
    __shared__ double sh[4];
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    double v = 0.0;
    if (c < Nb) {
        const double pvValue = C.poro[c] * C.volume[c];
        bool violated = false;
        for (int e = 0; e < 3; ++e) {
            const double CNV = resid[(size_t)c * 3 + e] * dt * out1[6 + e] / pvValue;
            violated = violated || (fabs(CNV) > tol_cnv);
        }
        if (violated) v = pvValue;
    }
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ __launch_bounds__(256) void k_conv_final2(int nblocks, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double sh[256];
    double a = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) a += part[b];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[10] = sh[0];
}

// ============================== reservoir averages ============================================================
// RateConverter::SurfaceToReservoirVoidage::defineState (wells/RateConverter.hpp:433-554) for the one region Flow uses (every cell in
// region 0): pore-volume-weighted sums of p_o, Rs, Rv over the cells, once weighted by the hydrocarbon pore volume, once by the pore volume.
// Eight sums: [0..4) = sum hpv, sum p_o hpv, sum Rs hpv, sum Rv hpv over the cells with hpv > 0; [4..8) the same with pv_cell over the cells
// with pv_cell > 0.  Two stages in the manner of k_conv_pass1 / k_conv_final1, no atomics: a lane adds its cells (grid stride) in ascending
// order, the wave's lanes by shuffles, the four waves in order, one final workgroup the partials in a fixed order - the grid depends on the
// cell count alone, so two runs over one state give the same bits.  Value loads only (element 0 of the AD records).
constexpr int RESV_SUMS = 8;
template <bool EXT>
__global__ __launch_bounds__(256) void k_resv_avg_part(int Nb, int ncell, const double* __restrict__ iq, const double* __restrict__ volume,
                                                       double* __restrict__ part) {
    __shared__ double sh[RESV_SUMS][4];
    double a[RESV_SUMS];
    for (int i = 0; i < RESV_SUMS; ++i) a[i] = 0.0;
    for (size_t c = (size_t)blockIdx.x * 256 + threadIdx.x; c < (size_t)Nb; c += (size_t)gridDim.x * 256) {
        const int ci = (int)c;
        const double pv_cell = volume[ci] * iq_at(iq, ncell, Lay<EXT>::F_PORO, ci)[0];
        double hydrocarbon = 1.0;
        hydrocarbon -= iq_at(iq, ncell, F_S + WATER, ci)[0];
        const double po = iq_at(iq, ncell, F_P + OIL, ci)[0], Rs = iq_at(iq, ncell, F_RS, ci)[0];
        const double Rv = EXT ? iq_at(iq, ncell, Lay<EXT>::F_RV, ci)[0] : 0.0;
        const double hpv = pv_cell * hydrocarbon;
        if (hpv > 0.0) { a[0] += hpv; a[1] += po * hpv; a[2] += Rs * hpv; a[3] += Rv * hpv; }
        if (pv_cell > 0.0) { a[4] += pv_cell; a[5] += po * pv_cell; a[6] += Rs * pv_cell; a[7] += Rv * pv_cell; }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int i = 0; i < RESV_SUMS; ++i) {
        double v = a[i];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) sh[i][wv] = v;
    }
    __syncthreads();
    if (threadIdx.x < RESV_SUMS) {
        const int i = threadIdx.x;
        part[(size_t)blockIdx.x * RESV_SUMS + i] = ((sh[i][0] + sh[i][1]) + sh[i][2]) + sh[i][3];
    }
}
// one workgroup: the partials in a fixed order, then the averages - out[0..5) = pressure, rs, rv, pv, 1.0 where the hydrocarbon weights
// were used / 0.0 for the pore-volume fallback; out[5] = sum pv (the host refuses a field without pore volume instead of dividing)
__global__ __launch_bounds__(RESV_FINAL_THREADS) void k_resv_avg_final(int nblocks, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double sh[RESV_SUMS][RESV_FINAL_THREADS];
    double a[RESV_SUMS];
    for (int i = 0; i < RESV_SUMS; ++i) a[i] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += RESV_FINAL_THREADS)
        for (int i = 0; i < RESV_SUMS; ++i) a[i] += part[(size_t)b * RESV_SUMS + i];
    for (int i = 0; i < RESV_SUMS; ++i) sh[i][threadIdx.x] = a[i];
    __syncthreads();
    for (int o = RESV_FINAL_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int i = 0; i < RESV_SUMS; ++i) sh[i][threadIdx.x] += sh[i][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double hpv_sum = sh[0][0], pv_sum = sh[4][0];
        const int k = hpv_sum > 0.0 ? 0 : 4;
        const double w = sh[k][0];
        const bool ok = hpv_sum > 0.0 || pv_sum > 0.0;
        out[0] = ok ? sh[k + 1][0] / w : 0.0;
        out[1] = ok ? sh[k + 2][0] / w : 0.0;
        out[2] = ok ? sh[k + 3][0] / w : 0.0;
        out[3] = w;
        out[4] = k == 0 ? 1.0 : 0.0;
        out[5] = pv_sum;
    }
}

// EclProblem::endTimeStep, drift part (ebos/eclproblem.hh:1126-1135): drift = residual * dt of the accepted step
__global__ void k_drift_update(int n, const double* __restrict__ resid, double dt, double* __restrict__ drift) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) drift[e] = resid[e] * dt;
}
// ---- EclProblem's per-cell bookkeeping between time steps ---------------------------------------------------------------
// updateCompositionChangeLimits_ (ebos/eclproblem.hh:2010-2107): lastRs = Rs where the DRSDT limit binds (all cells of the
// region, or those with free gas: Sg > freeGasMinSaturation_ = 1e-7, :2073, 2877), else infinity; lastRv = Rv
template <bool EXT>
__global__ __launch_bounds__(256) void k_last_rs_rv(int N, const int* __restrict__ pvtnum, const int* __restrict__ drsdt_all, const double* __restrict__ iq,
                                                    double* __restrict__ lastRs, double* __restrict__ lastRv) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    if (lastRs) {
        const int pr = pvtnum ? pvtnum[c] : 0;
        const double Sg = iq_at(iq, N, F_S + GAS, c)[0];
        lastRs[c] = (drsdt_all[pr] || Sg > 1e-7) ? iq_at(iq, N, F_RS, c)[0] : INFINITY;
    }
    if (EXT && lastRv) lastRv[c] = iq_at(iq, N, Lay<EXT>::F_RV, c)[0];
}
// maxGasDissolutionFactor / maxOilVaporizationFactor (:1711-1754) of time level 0 (dt > 0: lastRs + DRSDT * dt,
// eclgenericproblem.cc: maxDRs_ = DRSDT * timeStepSize) or of time level 1 (dt = 0)
__global__ __launch_bounds__(256) void k_set_limits(int N, double dt, const int* __restrict__ pvtnum, const double* __restrict__ drsdt, const double* __restrict__ drvdt,
                                                    const double* __restrict__ lastRs, const double* __restrict__ lastRv, double* __restrict__ rsmax, double* __restrict__ rvmax) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const int pr = pvtnum ? pvtnum[c] : 0;
    if (drsdt) rsmax[c] = (drsdt[pr] < 0.0) ? DBL_MAX / 2.0 : lastRs[c] + drsdt[pr] * dt;
    if (drvdt) rvmax[c] = (drvdt[pr] < 0.0) ? DBL_MAX / 2.0 : lastRv[c] + drvdt[pr] * dt;
}
// updateMinPressure_ (:2172-2197); init: minOilPressure_ = min(1e99, p_o of the initial state) (eclgenericproblem.cc:165, :2293-2294)
__global__ __launch_bounds__(256) void k_min_pressure(int N, int init, const double* __restrict__ iq, double* __restrict__ minpo) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const double po = iq_at(iq, N, F_P + OIL, c)[0];
    const double old = init ? 1e99 : minpo[c];
    minpo[c] = (po < old) ? po : old;
}
// updateMaxOilSaturation_ (:2110-2141); init: maxOilSaturation_ = max(0, S_o of the initial state) (:2291-2292)
__global__ __launch_bounds__(256) void k_max_oil_saturation(int N, int init, const double* __restrict__ iq, double* __restrict__ maxso) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const double So = iq_at(iq, N, F_S + OIL, c)[0];
    const double old = init ? 0.0 : maxso[c];
    maxso[c] = (old > So) ? old : So;   // std::max(old, So)
}
// updateMaxWaterSaturation_ (:2144-2169); init: maxWaterSaturation_ = max(0, S_w of the initial state) (:2289-2290) and the
// initial saturation itself (initialFluidStates_).  The statement :2150 in front of the reference's loop (cell 1 takes over
// cell 0's stored maximum) is launch_max_water_saturation's copy
__global__ void k_copy_entry(double* __restrict__ a, int to, int from) { a[to] = a[from]; }
__global__ __launch_bounds__(256) void k_max_water_saturation(int N, int init, const double* __restrict__ iq, double* __restrict__ maxsw, double* __restrict__ sw0) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const double Sw = iq_at(iq, N, F_S + WATER, c)[0];
    const double old = init ? 0.0 : maxsw[c];
    maxsw[c] = (old > Sw) ? old : Sw;   // std::max(old, Sw)
    if (init) sw0[c] = Sw;
}
// updateHysteresis_ (:2603-2626) -> EclDefaultMaterial::updateHysteresis (its default "inconsistent" form): the oil-water system sees
// 1 - So, the gas-oil system 1 - Sg (Sg clamped to [0, 1]); a system whose wetting saturation falls below its turning point moves
// the turning point and recomputes the imbibition curve's shift (EclHysteresisTwoPhaseLawParams::update / updateDynamicParams_;
// oracle/fluid.hpp SatFunc::hystSee, same statements).  sw_ow / sw_go != NULL: restart (initHysteresisParams) - the turning
// points handed in (cell order of the device), starting from "nothing seen"
__global__ __launch_bounds__(256) void k_hyst_update(int N, Tables T, CellStatic C, const double* __restrict__ iq, double* __restrict__ hyst,
                                                     const double* __restrict__ sw_ow, const double* __restrict__ sw_go) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const GlobalTab B = T.dbl;
    const SatRegionDesc& Sd = T.sat(C.satnum ? C.satnum[c] : 0);
    const SatRegionDesc& Si = T.sat(C.imbnum[c]);
    const bool scaled = C.eps != nullptr;
    const int cfg = C.epscfg;
    double uD[EPS_COUNT], sD[EPS_COUNT], uI[EPS_COUNT], sI[EPS_COUNT];
    if (scaled) { eps_load<GlobalTab>(C, c, B, Sd, uD, sD); eps_load_imb<GlobalTab>(C, c, B, Si, uI, sI); }
    double mdcOw = 2.0, dOw = 0.0, mdcGo = 2.0, dGo = 0.0, sOw, sGo;
    if (sw_ow) { sOw = sw_ow[c]; sGo = sw_go[c]; }
    else {
        mdcOw = hyst[c]; dOw = hyst[(size_t)N + c]; mdcGo = hyst[(size_t)2 * N + c]; dGo = hyst[(size_t)3 * N + c];
        const double So = iq_at(iq, N, F_S + OIL, c)[0];
        double Sg = iq_at(iq, N, F_S + GAS, c)[0];
        Sg = emin(1.0, emax(0.0, Sg));
        sOw = 1.0 - So;
        sGo = 1.0 - Sg;
    }
    if (sOw < mdcOw) {
        mdcOw = sOw;
        const double krnMdcDrainage = sat_curve<double, GlobalTab>(B, Sd, KRN_OW, sOw, scaled, cfg, uD, sD);
        const double SwKrnMdcImbibition = sat_curve_inv<GlobalTab>(B, Si, KRN_OW, krnMdcDrainage, scaled, cfg, uI, sI);
        dOw = SwKrnMdcImbibition - sOw;
    }
    if (sGo < mdcGo) {
        mdcGo = sGo;
        const double krnMdcDrainage = sat_curve<double, GlobalTab>(B, Sd, KRN_GO, sGo, scaled, cfg, uD, sD);
        const double SwKrnMdcImbibition = sat_curve_inv<GlobalTab>(B, Si, KRN_GO, krnMdcDrainage, scaled, cfg, uI, sI);
        dGo = SwKrnMdcImbibition - sGo;
    }
    hyst[c] = mdcOw; hyst[(size_t)N + c] = dOw; hyst[(size_t)2 * N + c] = mdcGo; hyst[(size_t)3 * N + c] = dGo;
}
// the storage term of the cached intensive quantities, values only (computeStorage; the statements of k_assemble's diagonal
// lane): the old time level's storage where the first iteration's cannot be recycled (:1758-1765)
template <bool EXT>
__global__ __launch_bounds__(256) void k_storage_old(int Nb, int N, int wet, const double* __restrict__ iq, double* __restrict__ storageOld) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= Nb) return;
    const double poro = iq_at(iq, N, Lay<EXT>::F_PORO, c)[0], Rs = iq_at(iq, N, F_RS, c)[0];
    double f[3] = {0.0, 0.0, 0.0};
    const int comp[3] = {EQ_WATER, EQ_OIL, EQ_GAS};
#pragma unroll
    for (int ph = 0; ph < 3; ++ph) {
        const double surfaceVolume = iq_at(iq, N, F_S + ph, c)[0] * iq_at(iq, N, F_B + ph, c)[0] * poro;
        f[comp[ph]] = f[comp[ph]] + surfaceVolume;
        if (ph == OIL) f[EQ_GAS] = f[EQ_GAS] + Rs * surfaceVolume;
        if (EXT && ph == GAS && wet) f[EQ_OIL] = f[EQ_OIL] + iq_at(iq, N, Lay<EXT>::F_RV, c)[0] * surfaceVolume;
    }
    for (int e = 0; e < 3; ++e) storageOld[(size_t)c * 3 + e] = f[e];
}
void launch_drift_update(opmhip_ctx* c, double dt) {
    const int n = c->pat.Nb * 3;
    hipLaunchKernelGGL(k_drift_update, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, c->d_b, dt, c->asmb.d_drift);
}

// ============================== analytic aquifers (opmhip_set_aquifers) =======================================
// AquiferInterface::addToSource (opm/simulators/aquifers/AquiferInterface.hpp:130-153) with calculateInflowRate of
// AquiferCarterTracy.hpp:135-169 and AquiferFetkovich.hpp:112-148, statement by statement (the library is built with
// -ffp-contract=off: the expression trees below are the ones a NumPy restatement has to copy to get the same bits).
// Plain wave64 kernels, one lane per connected cell / connection / aquifer; no atomics.
struct AqArrays {
    const int *of, *pos;                        // per connection: aquifer, cell (internal position)
    const double *alpha, *pprev;                // per connection: alphai_, pressure_previous_
    const double *par, *step, *state;           // per aquifer: AQ_PAR constants, AQ_STEP scalars of the time step, AQ_STATE state
};
__device__ __forceinline__ Ad aquifer_rate(const double* __restrict__ par, const double* __restrict__ step, const double* __restrict__ state,
                                           double alpha, double cellDepth, double pprev, const Ad& pcur) {
    const double gdz = GRAVITY * (cellDepth - par[AQ_DATUM]);
    if (par[AQ_TYPE] == 0.0) {   // Carter-Tracy: dpai, calculateEqnConstants, Eq 5.7
        const double dpai = par[AQ_PA0] + par[AQ_RHOW] * gdz - pprev;
        const double denom = par[AQ_TC] * (step[AQ_PITD] - step[AQ_TD] * step[AQ_PITDPRIME]);
        const double a = (par[AQ_BETA] * dpai - state[AQ_AUX] * step[AQ_PITDPRIME]) / denom;
        const double b = par[AQ_BETA] / denom;
        return alpha * (a - b * (pcur - pprev));
    }
    // Fetkovich: dpai carries the derivative, Eq 5.14
    const Ad dpai = (state[AQ_AUX] + par[AQ_RHOW] * gdz) - pcur;
    return (step[AQ_COEF] * alpha * par[AQ_PI]) * dpai;
}
// AquiferInterface::beginTimeStep: pressure_previous_ of every connection
__global__ __launch_bounds__(64) void k_aquifer_begin(int nc, int ncell, const int* __restrict__ pos, const double* __restrict__ iq, double* __restrict__ pprev) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < nc) pprev[i] = iq_at(iq, ncell, F_P + WATER, pos[i])[0];
}
// In front of k_assemble, one lane per DISTINCT connected cell: Qai_ of the cell's connections (stored for opmhip_end_time_step and the
// tests) added, in aquifer order, to the water row of the cell's source and its derivative; what the caller had there is kept in `save`
__global__ __launch_bounds__(64) void k_aquifer_apply(int nd, int ncell, AqArrays Q, const int* __restrict__ cpos, const int* __restrict__ cptr,
                                                      const int* __restrict__ cconn, const double* __restrict__ iq, const double* __restrict__ depth,
                                                      double* __restrict__ source, double* __restrict__ dsource, double* __restrict__ save, double* __restrict__ q4) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= nd) return;
    const int c = cpos[t];
    const Ad pw = load_ad(iq_at(iq, ncell, F_P + WATER, c));
    const double z = depth[c];
    double* s = source + (size_t)c * 3 + EQ_WATER;
    double* ds = dsource + (size_t)c * 9 + EQ_WATER * 3;
    Ad w{*s, ds[0], ds[1], ds[2]};
    store_ad(save + (size_t)4 * t, w);
    for (int k = cptr[t]; k < cptr[t + 1]; ++k) {
        const int i = cconn[k], a = Q.of[i];
        const Ad q = aquifer_rate(Q.par + (size_t)a * AQ_PAR, Q.step + (size_t)a * AQ_STEP, Q.state + (size_t)a * AQ_STATE, Q.alpha[i], z, Q.pprev[i], pw);
        store_ad(q4 + (size_t)4 * i, q);
        w = w + q;
    }
    *s = w.v; ds[0] = w.d0; ds[1] = w.d1; ds[2] = w.d2;
}
// behind k_assemble: the caller's rows back
__global__ __launch_bounds__(64) void k_aquifer_restore(int nd, const int* __restrict__ cpos, const double* __restrict__ save, double* __restrict__ source,
                                                        double* __restrict__ dsource) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= nd) return;
    const int c = cpos[t];
    const Ad w = load_ad(save + (size_t)4 * t);
    double* ds = dsource + (size_t)c * 9 + EQ_WATER * 3;
    source[(size_t)c * 3 + EQ_WATER] = w.v; ds[0] = w.d0; ds[1] = w.d1; ds[2] = w.d2;
}
// endTimeStep of both classes (AquiferCarterTracy.hpp:62-70, AquiferFetkovich.hpp:64-70, 122-133), one lane per aquifer: the reference's
// loop over Qai_ in connection order, left to right - once per time step, a serial sum is the sum to the bit
__global__ __launch_bounds__(64) void k_aquifer_end(int na, double dt, const int* __restrict__ ptr, const double* __restrict__ par, const double* __restrict__ q4,
                                                    double* __restrict__ state) {
    const int a = blockIdx.x * 64 + threadIdx.x;
    if (a >= na) return;
    double W = state[(size_t)a * AQ_STATE + AQ_WFLUX];
    for (int i = ptr[a]; i < ptr[a + 1]; ++i) W += q4[(size_t)4 * i] * dt;
    state[(size_t)a * AQ_STATE + AQ_WFLUX] = W;
    const double* p = par + (size_t)a * AQ_PAR;
    state[(size_t)a * AQ_STATE + AQ_AUX] = p[AQ_TYPE] == 0.0 ? W : p[AQ_PA0] - (W / p[AQ_CV]);
}
static AqArrays aquifer_arrays(const AquifersDev& Q) { return AqArrays{Q.d_of, Q.d_pos, Q.d_alpha, Q.d_pprev, Q.d_par, Q.d_step, Q.d_state}; }
void launch_aquifer_begin(opmhip_ctx* c) {
    const AquifersDev& Q = c->asmb.aq;
    hipLaunchKernelGGL(k_aquifer_begin, dim3((Q.nc + 63) / 64), dim3(64), 0, c->stream, Q.nc, c->pat.Nloc, Q.d_pos, c->asmb.d_iq, Q.d_pprev);
}
void launch_aquifer_apply(opmhip_ctx* c) {
    const AquifersDev& Q = c->asmb.aq;
    hipLaunchKernelGGL(k_aquifer_apply, dim3((Q.nd + 63) / 64), dim3(64), 0, c->stream, Q.nd, c->pat.Nloc, aquifer_arrays(Q), Q.d_cpos, Q.d_cptr, Q.d_cconn,
                       c->asmb.d_iq, c->asmb.d_depth, c->asmb.d_source, c->asmb.d_dsource, Q.d_save, Q.d_q);
}
void launch_aquifer_restore(opmhip_ctx* c) {
    const AquifersDev& Q = c->asmb.aq;
    hipLaunchKernelGGL(k_aquifer_restore, dim3((Q.nd + 63) / 64), dim3(64), 0, c->stream, Q.nd, Q.d_cpos, Q.d_save, c->asmb.d_source, c->asmb.d_dsource);
}
void launch_aquifer_end(opmhip_ctx* c, double dt) {
    const AquifersDev& Q = c->asmb.aq;
    hipLaunchKernelGGL(k_aquifer_end, dim3((Q.num + 63) / 64), dim3(64), 0, c->stream, Q.num, dt, Q.d_ptr, Q.d_par, Q.d_q, Q.d_state);
}

// ============================== VFP tables (opmhip_set_vfp_tables) ==============================================
// wells/VFPHelpers.cpp - findInterpData (:81-145), interpolate (:181-287, :289-341), bhp (:343-385), findTHP (:387-499), findX (:40-66),
// getFlo / getWFR / getGFR (:501-590) -, the AD forms of bhp (VFPProdProperties.cpp:142-172, VFPInjProperties.cpp:88-112) and thp
// (VFPProdProperties.cpp:37-82, VFPInjProperties.cpp:47-74) in the statement order of vfp.py: one body for opmhip_vfp_probe and for the
// wells' THP control.  No contraction (the library's build), plain loads: the 32 corners are a gather from a table of a few tens of KB
// that lives in L2.  UNVERIFIED, as vfp.py says: a chop or a threshold that binds, ties included, has derivative zero.
struct VfpTab { const int* desc; const double* dbl; };   // one table's descriptor (vfp_tables.hpp), the set's doubles
struct VfpInterp { int i0, i1; double inv, fac; };
struct VfpVar { double v, d[3]; };                        // a value and its derivatives by (aqua, liquid, vapour)
__device__ __forceinline__ const double* vfp_axis(const VfpTab T, int a) { return T.dbl + T.desc[VFP_AXIS + a]; }
__device__ VfpInterp vfp_find_interp(double value_in, const double* __restrict__ axis, int n) {
    VfpInterp r{0, 0, 0.0, 0.0};
    const double value = value_in < 0.0 ? 0.0 : value_in;   // no extrapolation towards negative ranges
    if (n == 1) return r;
    if (value < axis[0]) r.i1 = 1;
    else if (value >= axis[n - 1]) r.i1 = n - 1;
    else {
        r.i1 = n - 1;   // (a NaN finds nothing: the last interval)
        for (int i = 1; i < n; ++i)
            if (axis[i] >= value) { r.i1 = i; break; }
    }
    r.i0 = r.i1 - 1;
    const double start = axis[r.i0], end = axis[r.i1];
    if (end > start) { r.inv = 1.0 / (end - start); r.fac = (value - start) * r.inv; }
    if (r.fac > 3.0) r.fac = 3.0;
    return r;
}
// c[2^N], the corner of the axis reduced first in the lowest bit: N reductions (t1 * a) + (t2 * b), t2 = fac[s], t1 = 1.0 - t2
template <int N>
__device__ __forceinline__ double vfp_reduce(double* c, const double* fac) {
#pragma unroll
    for (int s = 0; s < N; ++s) {
        const double t2 = fac[s], t1 = 1.0 - t2;
#pragma unroll
        for (int k = 0; k < (1 << (N - 1 - s)); ++k) c[k] = (t1 * c[2 * k]) + (t2 * c[2 * k + 1]);
    }
    return c[0];
}
// VFPPROD: out[0] = value and, DERIV, out[1..5] = dthp, dwfr, dgfr, dalq, dflo.  Corner index t * 16 + w * 8 + g * 4 + a * 2 + f; every
// derivative (hi - lo) * inv_dist per corner pair, the same at both ends; all fields reduced along flo, alq, gfr, wfr, thp
template <bool DERIV>
__device__ void vfp_interp_prod(const VfpTab T, const VfpInterp& fl, const VfpInterp& th, const VfpInterp& wf, const VfpInterp& gf, const VfpInterp& al, double* out) {
    const int* d = T.desc;
    const double* __restrict__ val = T.dbl + d[VFP_VALUES];
    const size_t nf = d[VFP_N], nw = d[VFP_N + 2], ng = d[VFP_N + 3], na = d[VFP_N + 4];
    double v[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const size_t ti = (i & 16) ? th.i1 : th.i0, wi = (i & 8) ? wf.i1 : wf.i0, gi = (i & 4) ? gf.i1 : gf.i0, ai = (i & 2) ? al.i1 : al.i0, fi = (i & 1) ? fl.i1 : fl.i0;
        v[i] = val[(((ti * nw + wi) * ng + gi) * na + ai) * nf + fi];
    }
    const double fac[5] = {fl.fac, al.fac, gf.fac, wf.fac, th.fac};
    if (DERIV) {
        const double inv[5] = {th.inv, wf.inv, gf.inv, al.inv, fl.inv};
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int b = 16 >> k;
            double dd[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) dd[i] = (v[i | b] - v[i & ~b]) * inv[k];
            out[1 + k] = vfp_reduce<5>(dd, fac);
        }
    }
    out[0] = vfp_reduce<5>(v, fac);
}
// VFPINJ: out[0] = value and, DERIV, out[1] = dthp, out[2] = dflo.  Corner index t * 2 + f; reduced along flo, then thp
template <bool DERIV>
__device__ void vfp_interp_inj(const VfpTab T, const VfpInterp& fl, const VfpInterp& th, double* out) {
    const double* __restrict__ val = T.dbl + T.desc[VFP_VALUES];
    const size_t nf = T.desc[VFP_N];
    double v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = val[(size_t)((i & 2) ? th.i1 : th.i0) * nf + ((i & 1) ? fl.i1 : fl.i0)];
    const double fac[2] = {fl.fac, th.fac};
    if (DERIV) {
        const double inv[2] = {th.inv, fl.inv};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int b = 2 >> k;
            double dd[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) dd[i] = (v[i | b] - v[i & ~b]) * inv[k];
            out[1 + k] = vfp_reduce<2>(dd, fac);
        }
    }
    out[0] = vfp_reduce<2>(v, fac);
}
__device__ __forceinline__ VfpVar vfp_var(double v, double da, double dl, double dv) { return VfpVar{v, {da, dl, dv}}; }
__device__ __forceinline__ VfpVar vfp_chop(VfpVar x) {   // chopNegativeValues: max(0, x), std::max's way
    if (!(0.0 < x.v)) x = vfp_var(0.0, 0.0, 0.0, 0.0);
    return x;
}
// chop(a) / max(1e-12, chop(c)); the quotient rule as (a' - v * b') / b with v = a / b
__device__ VfpVar vfp_quotient(VfpVar a, VfpVar c) {
    a = vfp_chop(a);
    c = vfp_chop(c);
    if (!(1e-12 < c.v)) c = vfp_var(1e-12, 0.0, 0.0, 0.0);
    VfpVar o;
    o.v = a.v / c.v;
#pragma unroll
    for (int j = 0; j < 3; ++j) o.d[j] = (a.d[j] - o.v * c.d[j]) / c.v;
    return o;
}
__device__ VfpVar vfp_flo(const int* desc, double aq, double li, double va) {   // getFlo: the sign of the rates kept
    const int type = desc[VFP_FLO_TYPE];
    if (type == 0) return vfp_var(li, 0.0, 1.0, 0.0);
    if (type == 2) return vfp_var(va, 0.0, 0.0, 1.0);
    return desc[VFP_KIND] == 0 ? vfp_var(aq + li, 1.0, 1.0, 0.0) : vfp_var(aq, 1.0, 0.0, 0.0);   // LIQ / WAT
}
__device__ VfpVar vfp_wfr(const int* desc, double aq, double li, double va) {
    const int type = desc[VFP_WFR_TYPE];
    const VfpVar num = vfp_var(-aq, -1.0, 0.0, 0.0);
    if (type == 0) return vfp_quotient(num, vfp_var(-li, 0.0, -1.0, 0.0));          // WOR
    if (type == 1) return vfp_quotient(num, vfp_var(-aq - li, -1.0, -1.0, 0.0));    // WCT
    return vfp_quotient(num, vfp_var(-va, 0.0, 0.0, -1.0));                         // WGR
}
__device__ VfpVar vfp_gfr(const int* desc, double aq, double li, double va) {
    const int type = desc[VFP_GFR_TYPE];
    if (type == 0) return vfp_quotient(vfp_var(-va, 0.0, 0.0, -1.0), vfp_var(-li, 0.0, -1.0, 0.0));          // GOR
    if (type == 1) return vfp_quotient(vfp_var(-va, 0.0, 0.0, -1.0), vfp_var(-li - aq, -1.0, -1.0, 0.0));    // GLR
    return vfp_quotient(vfp_var(-li, 0.0, -1.0, 0.0), vfp_var(-va, 0.0, 0.0, -1.0));                         // OGR
}
// out[9]: bhp, dthp, dwfr, dgfr, dalq, dflo, d/daqua, d/dliquid, d/dvapour (an injector's dwfr, dgfr, dalq: 0)
__device__ void vfp_bhp(const VfpTab T, double aq, double li, double va, double thp, double alq, double* out) {
    const int* d = T.desc;
    const VfpVar f = vfp_flo(d, aq, li, va);
    const VfpInterp th = vfp_find_interp(thp, vfp_axis(T, 1), d[VFP_N + 1]);
    if (d[VFP_KIND] == 0) {
        const VfpVar w = vfp_wfr(d, aq, li, va), g = vfp_gfr(d, aq, li, va);
        const VfpInterp fl = vfp_find_interp(-f.v, vfp_axis(T, 0), d[VFP_N]), wf = vfp_find_interp(w.v, vfp_axis(T, 2), d[VFP_N + 2]),
                        gf = vfp_find_interp(g.v, vfp_axis(T, 3), d[VFP_N + 3]), al = vfp_find_interp(alq, vfp_axis(T, 4), d[VFP_N + 4]);
        vfp_interp_prod<true>(T, fl, th, wf, gf, al, out);
#pragma unroll
        for (int j = 0; j < 3; ++j) out[6 + j] = ((out[2] * w.d[j]) + (out[3] * g.d[j])) - (out[5] * f.d[j]);
    } else {
        double r[3];
        vfp_interp_inj<true>(T, vfp_find_interp(f.v, vfp_axis(T, 0), d[VFP_N]), th, r);
        out[0] = r[0]; out[1] = r[1]; out[2] = 0.0; out[3] = 0.0; out[4] = 0.0; out[5] = r[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) out[6 + j] = r[2] * f.d[j];
    }
}
__device__ __forceinline__ double vfp_find_x(double x0, double x1, double y0, double y1, double y) {
    const double dx = x1 - x0, dy = y1 - y0;
    return dy != 0.0 ? x0 + (y - y0) * (dx / dy) : x1;
}
// The inverse look-up: the table's BHP at every entry of its THP axis for these rates, then findTHP - in one pass over the axis, which
// keeps what findTHP can ask for: whether the values are sorted, the first and the last interval, the first interval with y0 < bhp <= y1.
// -1e100 where the reference throws; 0 for a THP axis of fewer than two entries (refused where it matters: opmhip_set_std_wells_thp)
__device__ double vfp_thp(const VfpTab T, double aq, double li, double va, double bhp, double alq) {
    const int* d = T.desc;
    const int nthp = d[VFP_N + 1];
    if (nthp < 2) return 0.0;
    const bool prod = d[VFP_KIND] == 0;
    const double* __restrict__ taxis = vfp_axis(T, 1);
    double flo = vfp_flo(d, aq, li, va).v;
    VfpInterp wf{0, 0, 0.0, 0.0}, gf = wf, al = wf;
    if (prod) {
        double wfr = 0.0, gfr = 0.0;
        if (aq == 0.0 && li == 0.0 && va == 0.0) flo = vfp_axis(T, 0)[0];   // likely the initial state: no extrapolation, zero fractions
        else { flo = -flo; wfr = vfp_wfr(d, aq, li, va).v; gfr = vfp_gfr(d, aq, li, va).v; }
        wf = vfp_find_interp(wfr, vfp_axis(T, 2), d[VFP_N + 2]);
        gf = vfp_find_interp(gfr, vfp_axis(T, 3), d[VFP_N + 3]);
        al = vfp_find_interp(alq, vfp_axis(T, 4), d[VFP_N + 4]);
    }
    const VfpInterp fl = vfp_find_interp(flo, vfp_axis(T, 0), d[VFP_N]);
    bool sorted = true;
    int in = -1;
    double b0 = 0.0, b1 = 0.0, bm = 0.0, bl = 0.0, iy0 = 0.0, iy1 = 0.0;   // the first two, the last two, the interval found
    for (int i = 0; i < nthp; ++i) {
        const VfpInterp th = vfp_find_interp(taxis[i], taxis, nthp);
        double b;
        if (prod) vfp_interp_prod<false>(T, fl, th, wf, gf, al, &b);
        else vfp_interp_inj<false>(T, fl, th, &b);
        if (i == 0) b0 = b;
        else {
            if (i == 1) b1 = b;
            if (b < bl) sorted = false;
            if (in < 0 && bl < bhp && bhp <= b) { in = i - 1; iy0 = bl; iy1 = b; }
        }
        bm = bl;
        bl = b;
    }
    const int where = bhp <= b0 ? 0 : (bhp > bl ? 1 : 2);   // below, above, neither
    if (in >= 0 && (!sorted || where == 2)) return vfp_find_x(taxis[in], taxis[in + 1], iy0, iy1, bhp);
    if (where == 0) return vfp_find_x(taxis[0], taxis[1], b0, b1, bhp);
    if (where == 1) return vfp_find_x(taxis[nthp - 2], taxis[nthp - 1], bm, bl, bhp);
    return -1e100;
}
// opmhip_vfp_probe: one lane per point; in: aqua | liquid | vapour | thp | alq | bhp_target, n each
__global__ __launch_bounds__(64) void k_vfp_probe(VfpTab T, int n, const double* __restrict__ in, int has_target, double* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const size_t N = n;
    const double aq = in[i], li = in[N + i], va = in[2 * N + i], alq = in[4 * N + i];
    double o[10];
    vfp_bhp(T, aq, li, va, in[3 * N + i], alq, o);
    o[9] = has_target ? vfp_thp(T, aq, li, va, in[5 * N + i], alq) : 0.0;
#pragma unroll
    for (int k = 0; k < 10; ++k) out[(size_t)10 * i + k] = o[k];
}
int launch_vfp_probe(opmhip_ctx* c, int table, int n, const double* d_in, bool has_target, double* d_out) {
    const VfpDev& V = c->asmb.vfp;
    hipLaunchKernelGGL(k_vfp_probe, dim3((n + 63) / 64), dim3(64), 0, c->stream, VfpTab{V.d_desc + (size_t)table * VFP_DESC, V.d_dbl}, n, d_in, has_target ? 1 : 0, d_out);
    return OPMHIP_SUCCESS;
}

// ============================== standard wells on the device (opmhip_set_std_wells) ===========================
// computePerfRate and assembleWellEqWithoutIteration (wells/StandardWell_impl.hpp:195-420, 516-640) in the minimal form and in the
// operation order of wells.py StandardWells(arithmetic="stated") - the library is built with -ffp-contract=off, so that every
// expression below rounds where its NumPy counterpart rounds.  SwAd<5>: value, d/dSw, d/dp, d/dX of the perforated cell, d/dbhp.
// Plain wave64 kernels; no atomics; every sum over perforations is added by one lane in perforation order.
//
// Crossflow in producers (opmhip_set_std_wells_crossflow, per well, off by default): the injecting branch of
// StandardWellEval::computePerfRate with allow_cf (wells/StandardWellEval.cpp:1023-1090).  A perforation of such a producer whose
// drawdown dd = p_o - (bhp + head) is not > 0 puts the well bore's mixture back into the formation.  q = the well's rate unknowns:
//     p_c = -q_c where q_c < 0, else 0;  P = (p_o + p_w) + p_g;  cmix_c = p_c / P          (wellSurfaceVolumeFraction, :233-243)
//     d cmix_c / d q_j = -((delta_cj - cmix_c) / P) where q_j < 0, else 0
//     cqt_i = -tw * (((mob_w + mob_o) + mob_g) * dd)
//     volumeRatio = (cmix_w / b_w + cmix_o / b_o) + (cmix_g - rs * cmix_o) / b_g            (b = 1/B of the perforated cell)
//     cqt_is = cqt_i / volumeRatio;  rate_c = cmix_c * cqt_is
// on SwAd<8> = value, d/dSw, d/dp, d/dX, d/dbhp, d/dq_o, d/dq_w, d/dq_g: a product is sw_mul (a0 b0; a0 b_i + b0 a_i), a quotient sw_div
// (v = a0 / b0; (a_i - v b_i) / b0), sums and differences entry by entry, in the order written.  P not > 0 (the well has not flowed
// yet) or volumeRatio not > 0: the perforation stays closed for that evaluation - nothing is divided by zero or a negative.  Then
// D[c][j] = delta_cj - sum_p d rate_c / d q_j and C[j][c] = 0 - d rate_c / d q_j; perforations with dd > 0 and wells without the switch
// take the expressions below unchanged.  By default the rate model is the dry-gas one (rv = 0, d = 1, tmp_oil = cmix_o).  Left out:
// openCrossFlowAvoidSingularity.  Injectors are refused: this parametrisation fixes the injected composition, where the reference
// re-injects what crosses in.
//
// Vaporised oil (opmhip_set_std_wells_vaporised_oil, per list, off by default; the VO instantiations): the rs / rv terms of computePerfRate
// (wells/StandardWellEval.cpp:999-1021, 1055-1073, 1092-1112) with rv = the record's F_RV.  surf[ph] = b_ph * (-tw * (mob_ph * dd)):
//     dd > 0 (N = 5):  rate_o = surf_o + rv * surf_g;  rate_g = surf_g + rs * surf_o;  rate_w = surf_w
//                      a producer's perf_dis_gas = (rs * surf_o).value, perf_vap_oil = (rv * surf_g).value
//     reversed, CF (N = 8):  d = 1 - rv * rs;  tmp_oil = (cmix_o - rv * cmix_g) / d;  tmp_gas = (cmix_g - rs * cmix_o) / d
//                      volumeRatio = (cmix_w / b_w + tmp_oil / b_o) + tmp_gas / b_g;  d not > 0: closed, like volumeRatio not > 0
//                      on values: perf_vap_oil = rv * (q_g - rs * q_o) / d;  perf_dis_gas = rs * (q_o - rv * q_g) / d
// Injectors keep their branch.  The two split values join the per-well sums in LDS (NS + 2); lane 0 leaves their sums per well.
template <int N> struct SwAd { double v[N]; };
template <int N> __device__ __forceinline__ SwAd<N> sw_load(const double* __restrict__ p) {   // a field of the record: no d/dbhp, no d/dq
    SwAd<N> o;
#pragma unroll
    for (int i = 0; i < N; ++i) o.v[i] = i < 4 ? p[i] : 0.0;
    return o;
}
template <int N> __device__ __forceinline__ SwAd<N> sw_mul(const SwAd<N>& a, const SwAd<N>& b) {   // the product rule of wells.py's `mul`
    SwAd<N> o;
    o.v[0] = a.v[0] * b.v[0];
#pragma unroll
    for (int i = 1; i < N; ++i) o.v[i] = a.v[0] * b.v[i] + b.v[0] * a.v[i];
    return o;
}
template <int N> __device__ __forceinline__ SwAd<N> sw_div(const SwAd<N>& a, const SwAd<N>& b) {   // wells.py's `div`
    SwAd<N> o;
    o.v[0] = a.v[0] / b.v[0];
#pragma unroll
    for (int i = 1; i < N; ++i) o.v[i] = (a.v[i] - o.v[0] * b.v[i]) / b.v[0];
    return o;
}
template <int N> __device__ __forceinline__ SwAd<N> sw_scale(double s, const SwAd<N>& a) {
    SwAd<N> o;
#pragma unroll
    for (int i = 0; i < N; ++i) o.v[i] = s * a.v[i];
    return o;
}
template <int N> __device__ __forceinline__ SwAd<N> sw_add(const SwAd<N>& a, const SwAd<N>& b) {
    SwAd<N> o;
#pragma unroll
    for (int i = 0; i < N; ++i) o.v[i] = a.v[i] + b.v[i];
    return o;
}
template <int N> __device__ __forceinline__ SwAd<N> sw_sub(const SwAd<N>& a, const SwAd<N>& b) {
    SwAd<N> o;
#pragma unroll
    for (int i = 0; i < N; ++i) o.v[i] = a.v[i] - b.v[i];
    return o;
}
template <int N> __device__ __forceinline__ void sw_store5(double* o, const SwAd<N>& a) {
#pragma unroll
    for (int i = 0; i < 5; ++i) o[i] = a.v[i];
}
// the drawdown p_o - (bhp + head) with its derivatives, from the cell's oil pressure and the value dd0
template <int N> __device__ __forceinline__ SwAd<N> sw_drawdown(const double* __restrict__ po, double dd0) {
    SwAd<N> dd = sw_load<N>(po);
    dd.v[0] = dd0;
    dd.v[4] = -1.0;
    return dd;
}
// the well bore's surface-volume fractions from the well's rate unknowns, mix[component * 4 + (value, d/dq_o, d/dq_w, d/dq_g)]
// -> whether the well flows (P > 0)
__device__ bool sw_wellbore_fractions(const double* x, double* mix) {
    bool s[3];
    double p[3];
    for (int c = 0; c < 3; ++c) { s[c] = x[c] < 0.0; p[c] = s[c] ? -x[c] : 0.0; }
    const double P = (p[EQ_OIL] + p[EQ_WATER]) + p[EQ_GAS];
    for (int i = 0; i < 12; ++i) mix[i] = 0.0;
    if (!(P > 0.0)) return false;
    for (int c = 0; c < 3; ++c) {
        const double m = p[c] / P;
        mix[c * 4] = m;
        for (int j = 0; j < 3; ++j)
            if (s[j]) mix[c * 4 + 1 + j] = -(((c == j ? 1.0 : 0.0) - m) / P);
    }
    return true;
}
// The connection rates of one perforation into the reservoir, out[component * 5 + (value, d/dSw, d/dp, d/dX, d/dbhp)], and under CF
// dq[component * 3 + (d/dq_o, d/dq_w, d/dq_g)].  The drawdown decides, once: a perforation that flows the way of its well takes the
// N = 5 arithmetic (dq = 0); one that does not stays closed - unless it is a producer's and `reverse` holds (the well has the crossflow
// switch and flows: mix are its fractions), which takes the N = 8 branch, closed still where the volume ratio is not positive.
// VO: the wet-gas rate model (the extended record: F_RV); sol[0] = perf_dis_gas, sol[1] = perf_vap_oil of a producer's perforation.
template <bool CF, bool VO>
__device__ __forceinline__ void sw_perf_rates(const double* __restrict__ iq, int ncell, int c, double tw, double bhp, double head, bool producer, int injPhase,
                                              bool reverse, const double* mix, double* out, double* dq, double* sol) {
#pragma unroll
    for (int i = 0; i < 15; ++i) out[i] = 0.0;
    if (VO) { sol[0] = 0.0; sol[1] = 0.0; }
    if (CF) {
#pragma unroll
        for (int i = 0; i < 9; ++i) dq[i] = 0.0;
    }
    const double* po = iq_at(iq, ncell, F_P + OIL, c);
    const double dd0 = po[0] - (bhp + head);   // the head between the reference depth and the completion is explicit
    const double ntw = -tw;
    if (producer ? dd0 > 0.0 : dd0 < 0.0) {
        const SwAd<5> dd = sw_drawdown<5>(po, dd0);
        if (producer) {   // phase rate = -Tw mob drawdown, surface volumes through 1/B, dissolved gas with the oil
            SwAd<5> surf[3];
#pragma unroll
            for (int ph = 0; ph < 3; ++ph)
                surf[ph] = sw_mul(sw_load<5>(iq_at(iq, ncell, F_B + ph, c)), sw_scale(ntw, sw_mul(sw_load<5>(iq_at(iq, ncell, F_MOB + ph, c)), dd)));
            if (VO) {     // the oil the gas carries counts as oil; both products from the surf values before either sum
                const SwAd<5> dis = sw_mul(sw_load<5>(iq_at(iq, ncell, F_RS, c)), surf[OIL]);
                const SwAd<5> vap = sw_mul(sw_load<5>(iq_at(iq, ncell, Lay<true>::F_RV, c)), surf[GAS]);
                sw_store5(out + EQ_OIL * 5, sw_add(surf[OIL], vap));
                sw_store5(out + EQ_WATER * 5, surf[WATER]);
                sw_store5(out + EQ_GAS * 5, sw_add(surf[GAS], dis));
                sol[0] = dis.v[0];
                sol[1] = vap.v[0];
            } else {
                sw_store5(out + EQ_OIL * 5, surf[OIL]);
                sw_store5(out + EQ_WATER * 5, surf[WATER]);
                sw_store5(out + EQ_GAS * 5, sw_add(surf[GAS], sw_mul(sw_load<5>(iq_at(iq, ncell, F_RS, c)), surf[OIL])));
            }
        } else {          // total mobility, the injected phase's 1/B
            const SwAd<5> tot = sw_add(sw_add(sw_load<5>(iq_at(iq, ncell, F_MOB + 0, c)), sw_load<5>(iq_at(iq, ncell, F_MOB + 1, c))), sw_load<5>(iq_at(iq, ncell, F_MOB + 2, c)));
            const SwAd<5> vol = sw_scale(ntw, sw_mul(tot, dd));
            const int comp = injPhase == GAS ? EQ_GAS : (injPhase == WATER ? EQ_WATER : EQ_OIL);
            sw_store5(out + comp * 5, sw_mul(sw_load<5>(iq_at(iq, ncell, F_B + injPhase, c)), vol));
        }
    } else if (CF && producer && reverse) {
        typedef SwAd<8> A8;   // value, d/dSw, d/dp, d/dX, d/dbhp, d/dq_o, d/dq_w, d/dq_g
        const A8 dd = sw_drawdown<8>(po, dd0);
        A8 cm[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) cm[k] = A8{{mix[k * 4], 0.0, 0.0, 0.0, 0.0, mix[k * 4 + 1], mix[k * 4 + 2], mix[k * 4 + 3]}};
        const A8 tot = sw_add(sw_add(sw_load<8>(iq_at(iq, ncell, F_MOB + WATER, c)), sw_load<8>(iq_at(iq, ncell, F_MOB + OIL, c))), sw_load<8>(iq_at(iq, ncell, F_MOB + GAS, c)));
        const A8 cqt_i = sw_scale(ntw, sw_mul(tot, dd));
        A8 ratio;
        double rs0 = 0.0, rv0 = 0.0, d0 = 1.0;
        if (VO) {
            const A8 rs = sw_load<8>(iq_at(iq, ncell, F_RS, c)), rv = sw_load<8>(iq_at(iq, ncell, Lay<true>::F_RV, c));
            const A8 d = sw_sub(A8{{1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}}, sw_mul(rv, rs));
            if (!(d.v[0] > 0.0)) return;   // (the reference throws where d == 0)
            const A8 tmp_oil = sw_div(sw_sub(cm[EQ_OIL], sw_mul(rv, cm[EQ_GAS])), d);
            const A8 tmp_gas = sw_div(sw_sub(cm[EQ_GAS], sw_mul(rs, cm[EQ_OIL])), d);
            ratio = sw_add(sw_add(sw_div(cm[EQ_WATER], sw_load<8>(iq_at(iq, ncell, F_B + WATER, c))), sw_div(tmp_oil, sw_load<8>(iq_at(iq, ncell, F_B + OIL, c)))),
                           sw_div(tmp_gas, sw_load<8>(iq_at(iq, ncell, F_B + GAS, c))));
            rs0 = rs.v[0]; rv0 = rv.v[0]; d0 = d.v[0];
        } else
            ratio = sw_add(sw_add(sw_div(cm[EQ_WATER], sw_load<8>(iq_at(iq, ncell, F_B + WATER, c))), sw_div(cm[EQ_OIL], sw_load<8>(iq_at(iq, ncell, F_B + OIL, c)))),
                           sw_div(sw_sub(cm[EQ_GAS], sw_mul(sw_load<8>(iq_at(iq, ncell, F_RS, c)), cm[EQ_OIL])), sw_load<8>(iq_at(iq, ncell, F_B + GAS, c))));
        if (!(ratio.v[0] > 0.0)) return;
        const A8 cqt_is = sw_div(cqt_i, ratio);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const A8 r = sw_mul(cm[k], cqt_is);
            sw_store5(out + k * 5, r);
#pragma unroll
            for (int j = 0; j < 3; ++j) dq[k * 3 + j] = r.v[5 + j];
        }
        if (VO) {   // the split, on values only (:1105-1111)
            sol[1] = rv0 * (out[EQ_GAS * 5] - rs0 * out[EQ_OIL * 5]) / d0;
            sol[0] = rs0 * (out[EQ_OIL * 5] - rv0 * out[EQ_GAS * 5]) / d0;
        }
    }
}
struct SwArrays {
    int num;
    const int *vp, *cell, *wi;                  // perforation ranges, perforated cells (internal positions), per well: producer, injected phase, rate component
    const double *wd, *tw, *dz;                 // per well: rate target, bhp limit; per perforation
    double *head, *pr, *x, *Dmat, *B, *C, *Dinv;   // x: the well unknowns, 4 per well
    int wellbore, nperf;                        // the heads come from the well-bore density (k_std_wells_wellbore); all perforations of the list
    double* wbstate;                            // then: p_perf [nperf] | the rates of the last assembly [nperf * 3]
    const int* cf;                              // per well: crossflow allowed (read by the CF instantiations only; NULL without a flag)
    double* dq;                                 // then: d rate_c / d q_j of the last assembly [nperf * 9]
    double* sol;                                // the VO instantiations': per well dissolved gas [num] | vaporised oil [num] of the last assembly
    double *control, *rw, *flag;                // d_pack's other fields: per well 0.0 rate / 1.0 bhp / 2.0 thp; r_w, 4 per well; the zero-pivot flag
};
// THP limits (opmhip_set_std_wells_thp; read by the THP instantiations only).  table: per well the index of its VFP table, -1: no limit; wd:
// per well limit, alq, dh; out: thp of the last controls [num] | dp of this time step [num] | V - dp of the last assembly [num]; wbdens: the
// well-bore densities per perforation under that head model
struct SwThp {
    const int* table;
    const double* wd;
    double* out;
    const int* desc;
    const double* dbl;
    const double* wbdens;
};
__device__ __forceinline__ VfpTab sw_thp_table(const SwThp& H, int w) { return VfpTab{H.desc + (size_t)H.table[w] * VFP_DESC, H.dbl}; }
__device__ __forceinline__ int wb_component(int phase);   // the component of a phase (below, with the well-bore heads)
// Further rate limits (opmhip_set_std_wells_limits; read by the LIM instantiations only).  lim: per well oil, water, gas, liquid, resv
// (+infinity: no such limit) - control value 3 + k names lim[5 w + k]; use: per well, the list's own target is a limit; out: coeff [3 num] |
// resv_current [num] | the averages of this time step [5]
struct SwLim {
    const double* lim;
    const int* use;
    double* out;
};
// Group production control (opmhip_set_std_wells_groups; read by the GRP instantiations only).  ptr / idx: per group its producers, wells
// ascending; of / avail: per well its group (-1: none), available for group control; guide: per well ORAT, WRAT, GRAT, LRAT, RESV; target:
// per group the same five (+infinity: none); mode: per group 0.0 NONE, 1.0 .. 5.0; nupcol: per well the three NUPCOL rates; rec: per group
// rates [3] | voidage | reduction [3] | guide_sum of the last group data (k_std_wells_groups), read frozen by everything else
struct SwGrp {
    int ng, nupcol_n;
    const int *ptr, *idx, *of, *avail;
    const double *guide, *target;
    double *mode, *nupcol, *rec;
};
constexpr int GRP_REC = 8, GRP_VOID = 3, GRP_RED = 4, GRP_GSUM = 7;
// TargetCalculator::calcModeRateFromRates (wells/TargetCalculator.cpp:53-90) for group mode 1 .. 5 on three values v (oil, water, gas); cf: the
// well's calcCoeff
__device__ __forceinline__ double grp_mode_rate(int mode, const double* v, const double* cf) {
    if (mode <= 3) return v[mode - 1];
    if (mode == 4) return v[EQ_OIL] + v[EQ_WATER];
    return (cf[EQ_WATER] * v[EQ_WATER] + cf[EQ_OIL] * v[EQ_OIL]) + cf[EQ_GAS] * v[EQ_GAS];
}
// RateConverter::calcCoeff / calcInjCoeff / calcReservoirVoidageRates (wells/RateConverter.hpp:592-777) in the statement order of wells.py
// calc_coeff / calc_inj_coeff / calc_reservoir_voidage_rates; components oil, water, gas; avg: pressure, rs, rv
__device__ __forceinline__ void rc_calc_coeff(const Tables& T, int pr, const double* avg, double* coeff) {
    const PvtRegionDesc& D = T.pvt(pr);
    const double p = avg[0], Rs = avg[1], Rv = avg[2];
    const double bw = pvt_invBw(T, D, p), bo = pvt_invBo(T, pr, D, p, Rs), bg = pvt_invBg(T, pr, D, p, Rv);
    coeff[EQ_OIL] = 0.0; coeff[EQ_WATER] = 0.0; coeff[EQ_GAS] = 0.0;
    coeff[EQ_WATER] = 1.0 / bw;
    const double detR = 1.0 - (Rs * Rv);
    double den = bo * detR;
    coeff[EQ_OIL] += 1.0 / den;
    coeff[EQ_GAS] -= Rv / den;
    den = bg * detR;
    coeff[EQ_GAS] += 1.0 / den;
    coeff[EQ_OIL] -= Rs / den;
}
__device__ __forceinline__ void rc_calc_inj_coeff(const Tables& T, int pr, const double* avg, double* coeff) {
    const PvtRegionDesc& D = T.pvt(pr);
    const double p = avg[0];
    const double bw = pvt_invBw(T, D, p), bo = pvt_invBo(T, pr, D, p, 0.0), bg = pvt_invBg(T, pr, D, p, 0.0);
    coeff[EQ_OIL] = 0.0; coeff[EQ_WATER] = 0.0; coeff[EQ_GAS] = 0.0;
    coeff[EQ_WATER] = 1.0 / bw;
    coeff[EQ_OIL] += 1.0 / bo;
    coeff[EQ_GAS] += 1.0 / bg;
}
// the sum of the voidage rates of the surface rates x (oil, water, gas): positive for what a producer takes out / an injector puts in
// (wells/WellInterfaceFluidSystem.cpp:145-152, 217-226)
__device__ __forceinline__ double rc_resv_current(const Tables& T, int pr, const double* avg, const double* x, bool producer) {
    const PvtRegionDesc& D = T.pvt(pr);
    const double p = avg[0];
    const double qo = x[EQ_OIL], qw = x[EQ_WATER], qg = x[EQ_GAS];
    double a = avg[1];
    double b = qg / (qo + 1.0e-15);
    const double Rs = b < a ? b : a;
    a = avg[2];
    b = qo / (qg + 1.0e-15);
    const double Rv = b < a ? b : a;
    const double bw = pvt_invBw(T, D, p), bo = pvt_invBo(T, pr, D, p, Rs), bg = pvt_invBg(T, pr, D, p, Rv);
    const double vw = qw / bw;
    const double detR = 1.0 - (Rs * Rv);
    double den = bo * detR;
    double v = qo;
    v -= Rv * qg;
    const double vo = v / den;
    den = bg * detR;
    v = qg;
    v -= Rs * qo;
    const double vg = v / den;
    double cur = 0.0;
    if (producer) { cur -= vw; cur -= vo; cur -= vg; }
    else { cur += vw; cur += vo; cur += vg; }
    return cur;
}
// At opmhip_std_wells_begin_iteration(0), behind k_resv_avg_final, one lane per well: this time step's averages are kept beside the
// coefficients (a later opmhip_reservoir_averages does not change them); the coefficients of every well with a RESV limit, at the PVT
// region of its first perforated cell.  grp_resv (NULL without groups): per well, a producer of a group with a RESV target - it gets its
// coefficients too; M.lim is NULL for a list with groups and without further limits
__global__ __launch_bounds__(64) void k_std_wells_resv_coeff(int num, const int* __restrict__ wi, const int* __restrict__ vp, const int* __restrict__ cell,
                                                             const int* __restrict__ pvtnum, Tables T, SwLim M, const double* __restrict__ avg,
                                                             const int* __restrict__ grp_resv) {
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= num) return;
    if (w == 0)
        for (int i = 0; i < 5; ++i) M.out[(size_t)4 * num + i] = avg[i];
    double coeff[3] = {0.0, 0.0, 0.0};
    if (((M.lim && M.lim[5 * w + 4] < INFINITY) || (grp_resv && grp_resv[w] != 0)) && avg[5] > 0.0) {   // (a field without pore volume: zeros, nothing is divided)
        const int pr = pvtnum ? pvtnum[cell[vp[w]]] : 0;
        if (wi[3 * w] != 0) rc_calc_coeff(T, pr, avg, coeff);
        else rc_calc_inj_coeff(T, pr, avg, coeff);
    }
    for (int i = 0; i < 3; ++i) M.out[(size_t)3 * w + i] = coeff[i];
}
// One wavefront per well.  Lanes take the well's perforations 64 at a time: rates with their five derivatives, B, C and the rates to
// global memory, what the per-well sums need to LDS; lane 0 adds the sums in perforation order and forms r_w, D, the guard of a well
// without a flowing completion, and D^-1.  SOLVE: the well alone against the frozen reservoir (StandardWells.solve_well_equations) - the
// heads first, then that body in a loop of at most 20 with the well's own stopping test, x -= D^-1 r_w in between; nothing but x, the
// heads and the flag is written.  CF: the list has a well with crossflow (launched in place of the other instantiation, for all its
// wells): 15 sums per lane - the 9 d rate / d q beside the 6 -, the full D, C's first three rows; the well bore's fractions are formed
// by lane 0 once per evaluation from x in LDS.  A well without the switch, or without a reversed perforation, gets today's bits.
// THP: the list has a well with a THP limit (launched in place of the other instantiation, for all its wells).  SOLVE then sets, after the
// heads, dp = (rho g) dh of every such well - rho what the head model uses for the first perforation (WellHelpers.hpp:149-155) -; under
// control 2 the control row is bhp - (V - dp) with V = vfp_bhp at the limit (control_eq = bhp - bhp_from_thp, WellInterfaceEval.cpp:351-354,
// 433-436, 463-504); the assembling form also leaves V - dp of every well with a limit.  Every other well gets today's bits.
// LIM: the list has further rate limits (launched in place of the other instantiation, for all its wells): under control 3 .. 7 the control
// row is that limit's (include/opmhip.h, opmhip_set_std_wells_limits); every other control gets today's bits.
// VO: the list has the vaporised-oil switch (launched in place of the other instantiation): the wet-gas rate model of sw_perf_rates, two
// more sums per lane - a perforation's dissolved gas and vaporised oil -, which the assembling form leaves per well in W.sol.
// GRP: the list has groups (launched in place of the other instantiation, for all its wells): under control 8 the control row is the
// group mode's with target_rate = max(0, (target - mode(reduction)) (g_w / guide_sum)) in the limit's place, the BHP row for a group of mode
// NONE (WellInterfaceEval.cpp:178-266); the group record is read as the last k_std_wells_groups left it.  Every other control gets today's bits.
template <bool SOLVE, bool CF, bool THP, bool LIM, bool VO, bool GRP>
__global__ __launch_bounds__(64) void k_std_wells_eq(SwArrays W, SwThp H, SwLim M, SwGrp G, int ncell, const double* __restrict__ iq, int first) {
    constexpr int NS = (CF ? 15 : 6) + (VO ? 2 : 0), SOL = CF ? 15 : 6;   // SOL: where the two split values sit
    __shared__ double sums[64 * NS];
    __shared__ double xs[4];
    __shared__ double s_mix[12];
    __shared__ int s_active, s_flows;
    const bool crossflow = CF && W.cf[blockIdx.x] != 0;   // uniform: the well's
    const int w = blockIdx.x, lane = threadIdx.x;
    const int pb = W.vp[w], pe = W.vp[w + 1];
    const bool producer = W.wi[3 * w] != 0;
    const int injPhase = W.wi[3 * w + 1], comp = W.wi[3 * w + 2];
    double* x = W.x + (size_t)4 * w;
    double* flag = W.flag + w;
    if (SOLVE && !W.wellbore)   // calculate_explicit_quantities: (rho_o g) dz, constant through the time step; lane l owns perforations pb + l + 64 k here and below
        for (int p = pb + lane; p < pe; p += 64) W.head[p] = (iq_at(iq, ncell, F_RHO + OIL, W.cell[p])[0] * GRAVITY) * W.dz[p];
    const bool limited = THP && H.table[w] >= 0;   // uniform: the well's
    double dp = 0.0;                               // lane 0's
    if (lane == 0) {
        for (int i = 0; i < 4; ++i) xs[i] = x[i];
        if (SOLVE && first) xs[3] = iq_at(iq, ncell, F_P + OIL, W.cell[pb])[0] + (producer ? -1e5 : 1e5);
        s_active = 1;
        if (limited) {
            if (SOLVE) {
                const double rho = W.wellbore ? H.wbdens[pb] : iq_at(iq, ncell, F_RHO + OIL, W.cell[pb])[0];
                dp = (rho * GRAVITY) * H.wd[3 * w + 2];
                H.out[(size_t)W.num + w] = dp;
            } else dp = H.out[(size_t)W.num + w];
        }
    }
    __syncthreads();
    for (int it = 0; it < (SOLVE ? 20 : 1); ++it) {
        if (crossflow) {
            if (lane == 0) s_flows = sw_wellbore_fractions(xs, s_mix) ? 1 : 0;
            __syncthreads();
        }
        const double bhp = xs[3];
        double S[NS];   // lane 0: sums of the rates, of d/dbhp and (CF) of d/dq
        for (int k = 0; k < NS; ++k) S[k] = 0.0;
        for (int p0 = pb; p0 < pe; p0 += 64) {
            const int p = p0 + lane;
            if (p < pe) {
                double q[15], dq[CF ? 9 : 1], sol[VO ? 2 : 1];
                sw_perf_rates<CF, VO>(iq, ncell, W.cell[p], W.tw[p], bhp, W.head[p], producer, injPhase, crossflow && s_flows, s_mix, q, dq, sol);
                if (VO) { sums[lane * NS + SOL] = sol[0]; sums[lane * NS + SOL + 1] = sol[1]; }
                if (CF) {
#pragma unroll
                    for (int i = 0; i < 9; ++i) sums[lane * NS + 6 + i] = dq[i];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) { sums[lane * NS + c] = q[c * 5]; sums[lane * NS + 3 + c] = q[c * 5 + 4]; }
                if (!SOLVE) {
                    double* pr = W.pr + (size_t)15 * p;
                    double* B = W.B + (size_t)12 * p;
                    double* C = W.C + (size_t)12 * p;
#pragma unroll
                    for (int i = 0; i < 15; ++i) pr[i] = q[i];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        for (int v = 0; v < 3; ++v) { B[c * 3 + v] = -q[c * 5 + 1 + v]; C[c * 3 + v] = CF ? 0.0 - dq[v * 3 + c] : 0.0; }
                        B[9 + c] = 0.0;
                        C[9 + c] = -q[c * 5 + 4];
                    }
                    if (CF) {
#pragma unroll
                        for (int i = 0; i < 9; ++i) W.dq[(size_t)9 * p + i] = dq[i];
                    }
                    if (W.wellbore) {   // the well state the next time step's heads start from (StandardWell_impl.hpp:468 and the rates of computePerfRate)
                        W.wbstate[p] = bhp + W.head[p];
#pragma unroll
                        for (int c = 0; c < 3; ++c) W.wbstate[(size_t)W.nperf + 3 * (size_t)p + c] = q[c * 5];
                    }
                }
            }
            __syncthreads();
            if (lane == 0) {
                const int m = pe - p0 < 64 ? pe - p0 : 64;
                for (int j = 0; j < m; ++j)
                    for (int k = 0; k < NS; ++k) S[k] = (p0 == pb && j == 0) ? sums[k] : S[k] + sums[j * NS + k];
            }
            __syncthreads();
        }
        if (lane == 0) {
            double r[4], D[16], inv[16];
            for (int i = 0; i < 16; ++i) { D[i] = 0.0; inv[i] = 0.0; }
            for (int c = 0; c < 3; ++c) { r[c] = xs[c] - S[c]; D[c * 4 + c] = 1.0; D[c * 4 + 3] = -S[3 + c]; }
            if (CF)
                for (int c = 0; c < 3; ++c)
                    for (int j = 0; j < 3; ++j) D[c * 4 + j] = D[c * 4 + j] - S[6 + c * 3 + j];
            const bool thp = limited && W.control[w] == 2.0;
            double V[9] = {0.0}, fromThp = 0.0;
            if (limited && (thp || !SOLVE)) {   // the table's bhp at the limit and the rates now present, brought to the reference depth
                vfp_bhp(sw_thp_table(H, w), xs[EQ_WATER], xs[EQ_OIL], xs[EQ_GAS], H.wd[3 * w], H.wd[3 * w + 1], V);
                fromThp = V[0] - dp;
                if (!SOLVE) H.out[(size_t)2 * W.num + w] = fromThp;
            }
            if (thp) {
                r[3] = xs[3] - fromThp;
                D[12 + EQ_OIL] = 0.0 - V[7]; D[12 + EQ_WATER] = 0.0 - V[6]; D[12 + EQ_GAS] = 0.0 - V[8];
                D[15] = 1.0;
            }
            else if (GRP && W.control[w] == 8.0) {
                const int g = G.of[w], mode = (int)G.mode[g];
                if (mode == 0) { r[3] = xs[3] - W.wd[2 * w + 1]; D[15] = 1.0; }
                else {
                    const double* rec = G.rec + (size_t)GRP_REC * g;
                    const double* cf = M.out + (size_t)3 * w;
                    const double gsum = rec[GRP_GSUM];
                    const double frac = gsum > 1e-12 ? G.guide[5 * w + mode - 1] / gsum : 0.0;
                    const double t = (G.target[5 * g + mode - 1] - grp_mode_rate(mode, rec + GRP_RED, cf)) * frac;
                    const double targetRate = t > 0.0 ? t : 0.0;
                    r[3] = grp_mode_rate(mode, xs, cf) + targetRate;
                    if (mode <= 3) D[12 + mode - 1] = 1.0;
                    else if (mode == 4) { D[12 + EQ_OIL] = 1.0; D[12 + EQ_WATER] = 1.0; }
                    else
                        for (int j = 0; j < 3; ++j) D[12 + j] = cf[j];
                }
            }
            else if (LIM && W.control[w] >= 3.0) {
                const int k = (int)W.control[w] - 3;
                const double L = M.lim[5 * w + k];
                if (k < 3) { r[3] = xs[k] + L; D[12 + k] = 1.0; }   // ORAT, WRAT, GRAT: the components' order is the equations'
                else if (k == 3) { r[3] = (xs[EQ_OIL] + xs[EQ_WATER]) + L; D[12 + EQ_OIL] = 1.0; D[12 + EQ_WATER] = 1.0; }
                else {
                    const double* cf = M.out + (size_t)3 * w;
                    if (producer) {
                        r[3] = ((cf[EQ_WATER] * xs[EQ_WATER] + cf[EQ_OIL] * xs[EQ_OIL]) + cf[EQ_GAS] * xs[EQ_GAS]) + L;
                        for (int j = 0; j < 3; ++j) D[12 + j] = cf[j];
                    } else {
                        const int ic = wb_component(injPhase);
                        r[3] = cf[ic] * xs[ic] - L;
                        D[12 + ic] = cf[ic];
                    }
                }
            }
            else if (W.control[w] != 0.0) { r[3] = xs[3] - W.wd[2 * w + 1]; D[15] = 1.0; }
            else { r[3] = xs[comp] - (producer ? -1.0 : 1.0) * W.wd[2 * w]; D[12 + comp] = 1.0; }
            // a well none of whose completions flows has no rate that answers to its bottom-hole pressure: it keeps the pressure
            if (D[3] == 0.0 && D[7] == 0.0 && D[11] == 0.0 && D[15] == 0.0) { r[3] = 0.0; D[12] = D[13] = D[14] = 0.0; D[15] = 1.0; }
            const int sing = invert4_stated(D, inv);
            if (sing) *flag = (double)sing;   // sticky: cleared by the host once it has looked
            if (SOLVE) {
                s_active = 0;
                if (!sing) {
                    double dx[4];
                    for (int i = 0; i < 4; ++i) {
                        double s = inv[i * 4] * r[0];
                        for (int j = 1; j < 4; ++j) s += inv[i * 4 + j] * r[j];
                        dx[i] = s;
                        xs[i] = xs[i] - s;
                    }
                    const double mdx = fmax(fmax(fabs(dx[0]), fabs(dx[1])), fabs(dx[2])), mx = fmax(fmax(fabs(xs[0]), fabs(xs[1])), fabs(xs[2]));
                    const bool small = mdx <= 1e-12 * fmax(1e-6, mx) && fabs(dx[3]) <= 1e-3;
                    s_active = small ? 0 : 1;
                }
            } else {
                for (int i = 0; i < 4; ++i) W.rw[(size_t)4 * w + i] = r[i];
                if (VO) { W.sol[w] = S[SOL]; W.sol[(size_t)W.num + w] = S[SOL + 1]; }
                for (int i = 0; i < 16; ++i) { W.Dmat[(size_t)16 * w + i] = D[i]; W.Dinv[(size_t)16 * w + i] = inv[i]; }   // a singular D: zeros, never NaNs
            }
        }
        __syncthreads();
        if (!SOLVE || !s_active) break;   // uniform: s_active is the workgroup's
    }
    if (SOLVE && lane == 0)
        for (int i = 0; i < 4; ++i) x[i] = xs[i];
}
// ---- the heads from the well-bore density (opmhip_set_std_wells_head_model) ----------------------------------------------------
// StandardWell::computeWellConnectionPressures (wells/StandardWell_impl.hpp:899-1012, 1124-1210), StandardWellEval::computeConnectionDensities
// (wells/StandardWellEval.cpp:814-960) and StandardWellGeneric::computeConnectionPressureDelta (wells/StandardWellGeneric.cpp:158-193) in
// the statement order of wells.py StandardWells(head_model="wellbore", arithmetic="stated").  Components (the equations' order) oil,
// water, gas; phases (the record's order) water, oil, gas: phase ph belongs to component (EQ_WATER, EQ_OIL, EQ_GAS)[ph].
// (1/B_w, 1/B_o, 1/B_g: pvt_invBw / pvt_invBo / pvt_invBg, the one body the probes run too)
__device__ __forceinline__ int wb_component(int phase) { return phase == GAS ? EQ_GAS : (phase == WATER ? EQ_WATER : EQ_OIL); }
struct WbArrays {
    const double *depth, *ref;   // per perforation: its depth; per well: the reference depth
    const int* pref;             // per well: the preferred phase
    double *out, *scratch;       // density [nperf] | p_avg [nperf] | mixture [nperf * 3]; 8 doubles per perforation
};
enum { WB_B = 0, WB_RSMAX = 3, WB_RVMAX = 4, WB_Q = 5, WB_REC = 8 };   // the record of a perforation between the passes: 1/B and q per component
// One wavefront per well, in front of the solving k_std_wells_eq.  Lanes take the perforations 64 at a time for the gathers and the table
// look-ups - p_avg, 1/B_w, RsSat, RvSat, 1/B_g, 1/B_o, the rates that count - and leave a record per perforation in LDS (a well of at
// most 64 perforations) or in global scratch.  Lane 0 then runs the two dependent passes in perforation order: the flow past every
// perforation from the last to the first, and from the first to the last the mixture, its corrected form x (which a perforation
// without flow hands to the next), the density and the head's running sum.  No atomics, no transcendental functions; what a lane
// computes depends on its perforation alone.  first: the bottom-hole pressure is the one the solving k_std_wells_eq is about to start from;
// init: the perforation pressures are the perforated cells' oil pressures and the stored rates zero (wells/WellState.cpp:298).
__global__ __launch_bounds__(64) void k_std_wells_wellbore(SwArrays W, WbArrays Q, Tables T, const int* __restrict__ pvtnum, int ncell,
                                                           const double* __restrict__ iq, int first, int init) {
    __shared__ double rec[64 * WB_REC];
    __shared__ double s_tw;
    const int w = blockIdx.x, lane = threadIdx.x;
    const int pb = W.vp[w], pe = W.vp[w + 1];
    const size_t np = W.nperf;
    const bool producer = W.wi[3 * w] != 0;
    const int injPhase = W.wi[3 * w + 1];
    const double* x = W.x + (size_t)4 * w;
    double* pp = W.wbstate;
    double* qs = W.wbstate + np;
    double* sc = pe - pb <= 64 ? rec : Q.scratch + (size_t)WB_REC * pb;
    if (init) {
        for (int p = pb + lane; p < pe; p += 64) {
            pp[p] = iq_at(iq, ncell, F_P + OIL, W.cell[p])[0];
            qs[3 * (size_t)p] = 0.0; qs[3 * (size_t)p + 1] = 0.0; qs[3 * (size_t)p + 2] = 0.0;
        }
        __syncthreads();
    }
    const double bhp = first ? iq_at(iq, ncell, F_P + OIL, W.cell[pb])[0] + (producer ? -1e5 : 1e5) : x[3];
    const double oilrate = fabs(x[EQ_OIL]), gasrate = fabs(x[EQ_GAS]);   // the well unknowns now present
    // a producer all of whose stored rates are exactly zero: the mixture by mobility ratio, the perforations weighted by tw (:1154-1184)
    int nonzero = 0;
    for (int p = pb + lane; p < pe; p += 64) nonzero |= (qs[3 * (size_t)p] != 0.0 || qs[3 * (size_t)p + 1] != 0.0 || qs[3 * (size_t)p + 2] != 0.0) ? 1 : 0;
    const bool fallback = !__syncthreads_or(nonzero) && producer;   // uniform
    if (fallback) {
        if (lane == 0) {
            double t = 0.0;
            for (int p = pb; p < pe; ++p) t += W.tw[p];
            s_tw = t;
        }
        __syncthreads();
    }
    for (int p = pb + lane; p < pe; p += 64) {
        const int c = W.cell[p];
        const int pr = pvtnum ? pvtnum[c] : 0;
        const PvtRegionDesc& D = T.pvt(pr);
        const double pAbove = p == pb ? bhp : pp[p - 1];
        const double pAvg = (pp[p] + pAbove) / 2.0;
        double* s = sc + (size_t)WB_REC * (p - pb);
        s[WB_B + EQ_WATER] = pvt_invBw(T, D, pAvg);
        const double rvmax = D.wg_n > 0 ? rv_sat_value(T, pr, pAvg) : 0.0;
        if (oilrate > 0.0) {
            double rv = 0.0;
            if (gasrate > 0.0) rv = oilrate / gasrate;
            rv = rvmax < rv ? rvmax : rv;
            s[WB_B + EQ_GAS] = pvt_invBg(T, pr, D, pAvg, rv);
        } else s[WB_B + EQ_GAS] = pvt_invBg(T, pr, D, pAvg, rvmax);   // the saturated curve
        const double rsmax = rs_sat_value(T, pr, pAvg);
        if (gasrate > 0.0) {
            double rs = 0.0;
            if (oilrate > 0.0) rs = gasrate / oilrate;
            rs = rsmax < rs ? rsmax : rs;
            s[WB_B + EQ_OIL] = pvt_invBo(T, pr, D, pAvg, rs);
        } else s[WB_B + EQ_OIL] = pvt_invBo(T, pr, D, pAvg, rsmax);
        s[WB_RSMAX] = rsmax;
        s[WB_RVMAX] = rvmax;
        if (fallback) {
            const double frac = W.tw[p] / s_tw;
            double mob[3], tm = 0.0;
            for (int ph = 0; ph < 3; ++ph) {
                mob[ph] = iq_at(iq, ncell, F_MOB + ph, c)[0];
                tm += iq_at(iq, ncell, F_B + ph, c)[0] * mob[ph];
            }
            for (int ph = 0; ph < 3; ++ph) s[WB_Q + wb_component(ph)] = frac * mob[ph] / tm;
        } else {
            for (int k = 0; k < 3; ++k) s[WB_Q + k] = qs[3 * (size_t)p + k];
        }
        Q.out[np + p] = pAvg;
    }
    __syncthreads();
    if (lane != 0) return;
    // 1. the flow up the well bore past every perforation, in place of the rates: from below minus what leaves through the perforation
    for (int p = pe - 1; p >= pb; --p) {
        double* s = sc + (size_t)WB_REC * (p - pb);
        for (int k = 0; k < 3; ++k) {
            double q = p == pe - 1 ? 0.0 : s[WB_REC + WB_Q + k];
            q -= s[WB_Q + k];
            s[WB_Q + k] = q;
        }
    }
    // 2. mixture, volume ratio, density; the head
    double xm[3] = {0.0, 0.0, 0.0}, head = 0.0;
    for (int p = pb; p < pe; ++p) {
        const double* s = sc + (size_t)WB_REC * (p - pb);
        const double tot = ((0.0 + s[WB_Q]) + s[WB_Q + 1]) + s[WB_Q + 2];
        double mix[3] = {0.0, 0.0, 0.0};
        if (tot != 0.0) {
            for (int k = 0; k < 3; ++k) mix[k] = fabs(s[WB_Q + k] / tot);
        } else if (!producer) mix[wb_component(injPhase)] = 1.0;
        else if (p == pb) mix[wb_component(Q.pref[w])] = 1.0;
        else { mix[0] = xm[0]; mix[1] = xm[1]; mix[2] = xm[2]; }   // x, not mix, of the perforation above: as the reference has it
        xm[0] = mix[0]; xm[1] = mix[1]; xm[2] = mix[2];
        double rs = 0.0, rv = 0.0;
        if (mix[EQ_OIL] > 1e-12) { const double r = mix[EQ_GAS] / mix[EQ_OIL]; rs = s[WB_RSMAX] < r ? s[WB_RSMAX] : r; }
        if (mix[EQ_GAS] > 1e-12) { const double r = mix[EQ_OIL] / mix[EQ_GAS]; rv = s[WB_RVMAX] < r ? s[WB_RVMAX] : r; }
        if (rs != 0.0) xm[EQ_GAS] = (mix[EQ_GAS] - mix[EQ_OIL] * rs) / (1.0 - rs * rv);
        if (rv != 0.0) xm[EQ_OIL] = (mix[EQ_OIL] - mix[EQ_GAS] * rv) / (1.0 - rs * rv);
        const GlobalTab rho = T.dbl + T.pvt(pvtnum ? pvtnum[W.cell[p]] : 0).density;   // surface densities: oil, water, gas
        double volrat = 0.0, sd = 0.0;
        for (int k = 0; k < 3; ++k) volrat += xm[k] / s[WB_B + k];
        for (int k = 0; k < 3; ++k) sd += rho[k] * mix[k];
        const double density = sd / volrat;
        const double dz = Q.depth[p] - (p == pb ? Q.ref[w] : Q.depth[p - 1]);
        const double dp = dz * density * GRAVITY;
        head = p == pb ? dp : head + dp;
        W.head[p] = head;
        Q.out[p] = density;
        for (int k = 0; k < 3; ++k) Q.out[2 * np + 3 * (size_t)p + k] = mix[k];
    }
}
// update_well_controls, one lane per well.  THP (the list has a well with a THP limit): the limits in the reference's order
// (WellInterfaceFluidSystem.cpp:170-268, :100-166), the first that is violated and is not the control in force wins - BHP, the rate
// target, THP: current = thp(table, q_w, q_o, q_g, bhp + dp, alq) (StandardWellGeneric.cpp:116-156, StandardWellEval.cpp:546-583), a
// producer switches when its limit > current, an injector when its limit < current, to control 2 with bhp = V - dp at the rates at hand
// (updateWellStateWithTarget's THP case, WellInterface_impl.hpp:659-667, 882-890).  A well without a limit takes today's two branches.
// LIM (the list has further rate limits): producers BHP, ORAT, WRAT, GRAT, LRAT, RESV, THP; injectors BHP, RATE, RESV, THP; the list's own
// target at its component's place; RESV's current rate from rc_resv_current at the rates at hand.  A switch to a rate-type mode leaves x.
// GRP (the list has groups): the well's group check comes first (WellInterfaceFluidSystem.cpp:363-432, WellGroupHelpers.cpp:1055-1180) - a
// producer not under GRUP, available, in a group whose mode is not NONE, whose current = -mode(x) exceeds target_rate = max(1e-12, ((target -
// mode(reduction)) + current) g_w / (guide_sum + g_w)) goes under control 8 with its rates scaled by target_rate / current, and is not looked at
// individually.  It reads the group record frozen (k_std_wells_groups ran in front), so the lanes are independent, as the reference's loop is.
template <bool THP, bool LIM, bool GRP>
__global__ __launch_bounds__(64) void k_std_wells_controls(int num, const int* __restrict__ wi, const double* __restrict__ wd, double* __restrict__ xs,
                                                           double* __restrict__ controls, SwThp H, SwLim M, Tables T, const int* __restrict__ vp,
                                                           const int* __restrict__ cell, const int* __restrict__ pvtnum, SwGrp G) {
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= num) return;
    const bool producer = wi[3 * w] != 0;
    const int comp = wi[3 * w + 2];
    const double target = wd[2 * w], limit = wd[2 * w + 1];
    double* x = xs + (size_t)4 * w;
    double* control = controls + w;
    if (GRP) {
        const int g = G.of[w];
        if (producer && *control != 8.0 && G.avail[w] != 0 && g >= 0 && G.mode[g] != 0.0) {
            const int mode = (int)G.mode[g];
            const double* rec = G.rec + (size_t)GRP_REC * g;
            const double* cf = M.out + (size_t)3 * w;
            const double cur = -grp_mode_rate(mode, x, cf);
            const double gw = G.guide[5 * w + mode - 1];
            const double gsum = rec[GRP_GSUM] + gw;
            const double frac = gsum > 1e-12 ? gw / gsum : 0.0;
            double t = G.target[5 * g + mode - 1] - grp_mode_rate(mode, rec + GRP_RED, cf);
            t = t + cur;
            t = t * frac;
            const double targetRate = t > 1e-12 ? t : 1e-12;
            if (cur > targetRate) {
                *control = 8.0;
                const double scale = cur > 1e-12 ? targetRate / cur : 1.0;
                for (int i = 0; i < 3; ++i) x[i] = x[i] * scale;
                return;
            }
        }
    }
    const bool limited = THP && H.table[w] >= 0;
    double current = 0.0;
    if (THP) {
        if (limited) current = vfp_thp(sw_thp_table(H, w), x[EQ_WATER], x[EQ_OIL], x[EQ_GAS], x[3] + H.out[(size_t)num + w], H.wd[3 * w + 1]);
        H.out[w] = current;
    }
    if (LIM) {
        const double* lim = M.lim + (size_t)5 * w;
        double resv = 0.0;
        if (lim[4] < INFINITY) {
            resv = rc_resv_current(T, pvtnum ? pvtnum[cell[vp[w]]] : 0, M.out + (size_t)4 * num, x, producer);
            M.out[(size_t)3 * num + w] = resv;
        }
        if (*control != 1.0 && ((producer && x[3] < limit) || (!producer && x[3] > limit))) { *control = 1.0; x[3] = limit; return; }
        const double ctl = *control;
        const int own = M.use[w] ? comp : -1;
        if (producer) {
            for (int k = 0; k < 5; ++k) {
                if (k < 3 && k == own) {
                    if (ctl != 0.0 && -1.0 * x[k] > target) { *control = 0.0; return; }
                    continue;
                }
                if (!(lim[k] < INFINITY) || ctl == 3.0 + k) continue;
                double cur;
                if (k < 3) cur = -x[k];
                else if (k == 3) { cur = -x[EQ_OIL]; cur -= x[EQ_WATER]; }
                else cur = resv;
                if (lim[k] < cur) { *control = 3.0 + k; return; }
            }
        } else {
            if (own >= 0 && ctl != 0.0 && 1.0 * x[comp] > target) { *control = 0.0; return; }
            if (lim[4] < INFINITY && ctl != 7.0 && lim[4] < resv) { *control = 7.0; return; }
        }
        if (limited && ctl != 2.0 && (producer ? H.wd[3 * w] > current : H.wd[3 * w] < current)) {
            double V[9];
            vfp_bhp(sw_thp_table(H, w), x[EQ_WATER], x[EQ_OIL], x[EQ_GAS], H.wd[3 * w], H.wd[3 * w + 1], V);
            *control = 2.0;
            x[3] = V[0] - H.out[(size_t)num + w];
        }
        return;
    }
    if (*control != 1.0 && ((producer && x[3] < limit) || (!producer && x[3] > limit))) { *control = 1.0; x[3] = limit; }
    else if (*control != 0.0 && (producer ? -1.0 : 1.0) * x[comp] > target) *control = 0.0;
    else if (limited && *control != 2.0 && (producer ? H.wd[3 * w] > current : H.wd[3 * w] < current)) {
        double V[9];
        vfp_bhp(sw_thp_table(H, w), x[EQ_WATER], x[EQ_OIL], x[EQ_GAS], H.wd[3 * w], H.wd[3 * w + 1], V);
        *control = 2.0;
        x[3] = V[0] - H.out[(size_t)num + w];
    }
}
// Group data and the groups' check, one lane per group, walking the group's producers in list order: every sum is sequential from 0, so it
// equals wells.py StandardWells._group_sums / _group_data / _group_check to the bit (no atomics).  CHECK (in front of the controls kernel,
// while iteration <= nupcol; BlackoilWellModelGeneric.cpp:537-650, 888-943): ORAT, WRAT, GRAT, LRAT, RESV, the first target that is < current
// and is not the mode in force wins; on a switch the rates of the group's wells under GRUP are multiplied by target / current when current >
// 1e-12 (WellGroupHelpers.cpp:429-).  Then, always, the data (BlackoilWellModelGeneric.cpp:1494-1539, WellGroupHelpers.cpp:300-427): the
// NUPCOL copy while iteration < nupcol, the reduction from the NUPCOL rates of the producers not under GRUP, the mode's guide-rate sum of those
// under GRUP, the present rates' sums and - groups with a RESV target - the voidage sum, into the group's record.
template <bool CHECK>
__global__ __launch_bounds__(64) void k_std_wells_groups(SwGrp G, int num, int iteration, double* __restrict__ xs, const double* __restrict__ controls, SwLim M,
                                                         Tables T, const int* __restrict__ vp, const int* __restrict__ cell, const int* __restrict__ pvtnum) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= G.ng) return;
    const int kb = G.ptr[g], ke = G.ptr[g + 1];
    const double* target = G.target + (size_t)5 * g;
    const bool hasResv = target[4] < INFINITY;
    const double* avg = M.out + (size_t)4 * num;
    if (CHECK && iteration <= G.nupcol_n) {
        double s[3] = {0.0, 0.0, 0.0}, voidage = 0.0;
        for (int k = kb; k < ke; ++k) {
            const int w = G.idx[k];
            const double* x = xs + (size_t)4 * w;
            for (int c = 0; c < 3; ++c) s[c] -= x[c];
            if (hasResv) voidage += rc_resv_current(T, pvtnum ? pvtnum[cell[vp[w]]] : 0, avg, x, true);
        }
        const int inForce = (int)G.mode[g];
        for (int mode = 1; mode <= 5; ++mode) {
            const double tg = target[mode - 1];
            if (!(tg < INFINITY) || inForce == mode) continue;
            const double cur = mode <= 3 ? s[mode - 1] : (mode == 4 ? s[EQ_OIL] + s[EQ_WATER] : voidage);
            if (tg < cur) {
                G.mode[g] = (double)mode;
                if (cur > 1e-12) {
                    const double scale = tg / cur;
                    for (int k = kb; k < ke; ++k) {
                        const int w = G.idx[k];
                        if (controls[w] == 8.0)
                            for (int c = 0; c < 3; ++c) xs[(size_t)4 * w + c] = xs[(size_t)4 * w + c] * scale;
                    }
                }
                break;
            }
        }
    }
    const int mode = (int)G.mode[g];
    double s[3] = {0.0, 0.0, 0.0}, red[3] = {0.0, 0.0, 0.0}, voidage = 0.0, gsum = 0.0;
    for (int k = kb; k < ke; ++k) {
        const int w = G.idx[k];
        const double* x = xs + (size_t)4 * w;
        double* nup = G.nupcol + (size_t)3 * w;
        if (iteration < G.nupcol_n)
            for (int c = 0; c < 3; ++c) nup[c] = x[c];
        if (controls[w] == 8.0) {
            if (mode != 0) gsum += G.guide[5 * w + mode - 1];
        } else
            for (int c = 0; c < 3; ++c) red[c] -= nup[c];
        for (int c = 0; c < 3; ++c) s[c] -= x[c];
        if (hasResv) voidage += rc_resv_current(T, pvtnum ? pvtnum[cell[vp[w]]] : 0, avg, x, true);
    }
    double* rec = G.rec + (size_t)GRP_REC * g;
    for (int c = 0; c < 3; ++c) { rec[c] = s[c]; rec[GRP_RED + c] = red[c]; }
    rec[GRP_VOID] = voidage;
    rec[GRP_GSUM] = gsum;
}
// In front of k_assemble (and of k_aquifer_apply), one lane per DISTINCT perforated cell: the caller's source and dsource rows are kept in
// `save`, the rates of the cell's perforations are added in perforation order (computeTotalRatesForDof)
__global__ __launch_bounds__(64) void k_std_wells_source(int nd, const int* __restrict__ cpos, const int* __restrict__ cptr, const int* __restrict__ cperf,
                                                         const double* __restrict__ pr, double* __restrict__ source, double* __restrict__ dsource, double* __restrict__ save) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= nd) return;
    const int c = cpos[t];
    double* s = source + (size_t)c * 3;
    double* ds = dsource + (size_t)c * 9;
    double v[12];
    for (int i = 0; i < 3; ++i) v[i] = s[i];
    for (int i = 0; i < 9; ++i) v[3 + i] = ds[i];
    for (int i = 0; i < 12; ++i) save[(size_t)12 * t + i] = v[i];
    for (int k = cptr[t]; k < cptr[t + 1]; ++k) {
        const double* q = pr + (size_t)15 * cperf[k];
        for (int e = 0; e < 3; ++e) {
            v[e] += q[e * 5];
            for (int d = 0; d < 3; ++d) v[3 + e * 3 + d] += q[e * 5 + 1 + d];
        }
    }
    for (int i = 0; i < 3; ++i) s[i] = v[i];
    for (int i = 0; i < 9; ++i) ds[i] = v[3 + i];
}
__global__ __launch_bounds__(64) void k_std_wells_restore(int nd, const int* __restrict__ cpos, const double* __restrict__ save, double* __restrict__ source,
                                                          double* __restrict__ dsource) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= nd) return;
    const int c = cpos[t];
    for (int i = 0; i < 3; ++i) source[(size_t)c * 3 + i] = save[(size_t)12 * t + i];
    for (int i = 0; i < 9; ++i) dsource[(size_t)c * 9 + i] = save[(size_t)12 * t + 3 + i];
}
// updateWellState: x -= relax * x_w
__global__ __launch_bounds__(64) void k_std_wells_axpy(int n, double relax, const double* __restrict__ xw, double* __restrict__ x) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) x[i] = x[i] - relax * xw[i];
}
static SwThp std_wells_thp(opmhip_ctx* c) {
    const StdWellsDev& S = c->wells.sw;
    const VfpDev& V = c->asmb.vfp;
    return SwThp{S.d_thp_table, S.d_thp_wd, S.d_thp_out, V.d_desc, V.d_dbl, S.d_wbout};
}
static SwLim std_wells_lim(opmhip_ctx* c) {
    const StdWellsDev& S = c->wells.sw;
    return SwLim{S.d_lim, S.d_lim_use, S.limits ? S.d_lim_out : S.d_grp_out};   // (a list with groups and without limits keeps the coefficients and the averages in its own array)
}
static SwGrp std_wells_grp(opmhip_ctx* c) {
    const StdWellsDev& S = c->wells.sw;
    return SwGrp{S.grp_num, S.grp_nupcol, S.d_grp_ptr, S.d_grp_idx, S.d_grp_of, S.d_grp_avail, S.d_grp_guide, S.d_grp_target,
                 S.d_grp_state, S.d_grp_state ? S.d_grp_state + S.grp_num : nullptr, S.d_grp_rec};
}
// the instantiation of k_std_wells_eq a list runs: one per combination of crossflow, THP limits, further rate limits and the vaporised-oil
// switch (a list without the feature runs the code it ran before; the number of launches is the same)
template <bool SOLVE, bool VO, bool GRP>
static auto std_wells_eq_kernel_of(const StdWellsDev& S) -> decltype(&k_std_wells_eq<SOLVE, false, false, false, VO, GRP>) {
    if (S.limits)
        return S.thp ? (S.crossflow ? k_std_wells_eq<SOLVE, true, true, true, VO, GRP> : k_std_wells_eq<SOLVE, false, true, true, VO, GRP>)
                     : (S.crossflow ? k_std_wells_eq<SOLVE, true, false, true, VO, GRP> : k_std_wells_eq<SOLVE, false, false, true, VO, GRP>);
    return S.thp ? (S.crossflow ? k_std_wells_eq<SOLVE, true, true, false, VO, GRP> : k_std_wells_eq<SOLVE, false, true, false, VO, GRP>)
                 : (S.crossflow ? k_std_wells_eq<SOLVE, true, false, false, VO, GRP> : k_std_wells_eq<SOLVE, false, false, false, VO, GRP>);
}
template <bool SOLVE>
static auto std_wells_eq_kernel(const StdWellsDev& S) -> decltype(&k_std_wells_eq<SOLVE, false, false, false, false, false>) {
    if (S.groups) return S.vaporised_oil ? std_wells_eq_kernel_of<SOLVE, true, true>(S) : std_wells_eq_kernel_of<SOLVE, false, true>(S);
    return S.vaporised_oil ? std_wells_eq_kernel_of<SOLVE, true, false>(S) : std_wells_eq_kernel_of<SOLVE, false, false>(S);
}
static SwArrays std_wells_arrays(const WellsDev& W) {
    const StdWellsDev& S = W.sw;
    return SwArrays{S.num, W.d_val_pointers, W.d_Ccols, S.d_wi, S.d_wd, S.d_tw, S.d_dz, S.d_head, S.d_pr, S.x(), S.d_Dmat, W.d_B, W.d_C, W.d_D,
                    S.wellbore ? 1 : 0, S.nperf, S.d_wbstate, S.d_cf, S.d_dq, S.d_sol, S.control(), S.rw(), S.flag()};
}
// (booked under the profile's assembly class, one scope per function: a context with a list shows them in opmhip_profile_get)
void launch_std_wells_solve(opmhip_ctx* c, bool first) {
    const int ps = prof_begin(c, PROF_ASSEMBLE);
    // (a list with a crossflow well runs the CF instantiation in place of the other: the number of launches is the same)
    // (... and one with a THP limit the THP instantiation)
    const StdWellsDev& S = c->wells.sw;
    hipLaunchKernelGGL(std_wells_eq_kernel<true>(S), dim3(S.num), dim3(64), 0, c->stream, std_wells_arrays(c->wells), std_wells_thp(c), std_wells_lim(c), std_wells_grp(c), c->pat.Nloc,
                       c->asmb.d_iq, first ? 1 : 0);
    prof_end(c, ps);
}
void launch_std_wells_wellbore(opmhip_ctx* c, bool first, bool init) {
    const StdWellsDev& S = c->wells.sw;
    const int ps = prof_begin(c, PROF_ASSEMBLE);
    hipLaunchKernelGGL(k_std_wells_wellbore, dim3(S.num), dim3(64), 0, c->stream, std_wells_arrays(c->wells),
                       WbArrays{S.d_wbdepth, S.d_wbref, S.d_wbpref, S.d_wbout, S.d_wbscratch}, tables_of(c), c->asmb.d_pvtnum, c->pat.Nloc, c->asmb.d_iq,
                       first ? 1 : 0, init ? 1 : 0);
    prof_end(c, ps);
}
void launch_std_wells_controls(opmhip_ctx* c) {
    const StdWellsDev& S = c->wells.sw;
    const int ps = prof_begin(c, PROF_ASSEMBLE);
    const auto plain = S.limits ? (S.thp ? k_std_wells_controls<true, true, false> : k_std_wells_controls<false, true, false>)
                                : (S.thp ? k_std_wells_controls<true, false, false> : k_std_wells_controls<false, false, false>);
    const auto grouped = S.limits ? (S.thp ? k_std_wells_controls<true, true, true> : k_std_wells_controls<false, true, true>)
                                  : (S.thp ? k_std_wells_controls<true, false, true> : k_std_wells_controls<false, false, true>);
    hipLaunchKernelGGL(S.groups ? grouped : plain, dim3((S.num + 63) / 64), dim3(64), 0, c->stream, S.num, S.d_wi, S.d_wd, S.x(), S.control(), std_wells_thp(c),
                       std_wells_lim(c), tables_of(c), c->wells.d_val_pointers, c->wells.d_Ccols, c->asmb.d_pvtnum, std_wells_grp(c));
    prof_end(c, ps);
}
void launch_std_wells_groups(opmhip_ctx* c, int iteration, bool check) {
    const StdWellsDev& S = c->wells.sw;
    const int ps = prof_begin(c, PROF_ASSEMBLE);
    hipLaunchKernelGGL(check ? k_std_wells_groups<true> : k_std_wells_groups<false>, dim3((S.grp_num + 63) / 64), dim3(64), 0, c->stream, std_wells_grp(c), S.num,
                       iteration, S.x(), S.control(), std_wells_lim(c), tables_of(c), c->wells.d_val_pointers, c->wells.d_Ccols, c->asmb.d_pvtnum);
    prof_end(c, ps);
}
void launch_std_wells_assemble(opmhip_ctx* c) {
    const StdWellsDev& S = c->wells.sw;
    const int ps = prof_begin(c, PROF_ASSEMBLE);
    hipLaunchKernelGGL(std_wells_eq_kernel<false>(S), dim3(S.num), dim3(64), 0, c->stream, std_wells_arrays(c->wells), std_wells_thp(c), std_wells_lim(c), std_wells_grp(c), c->pat.Nloc,
                       c->asmb.d_iq, 0);
    hipLaunchKernelGGL(k_std_wells_source, dim3((S.nd + 63) / 64), dim3(64), 0, c->stream, S.nd, S.d_cpos, S.d_cptr, S.d_cperf, S.d_pr, c->asmb.d_source,
                       c->asmb.d_dsource, S.d_save);
    prof_end(c, ps);
}
void launch_std_wells_restore(opmhip_ctx* c) {
    const StdWellsDev& S = c->wells.sw;
    const int ps = prof_begin(c, PROF_ASSEMBLE);
    hipLaunchKernelGGL(k_std_wells_restore, dim3((S.nd + 63) / 64), dim3(64), 0, c->stream, S.nd, S.d_cpos, S.d_save, c->asmb.d_source, c->asmb.d_dsource);
    prof_end(c, ps);
}
void launch_std_wells_axpy(opmhip_ctx* c, double relax) {
    const StdWellsDev& S = c->wells.sw;
    const int ps = prof_begin(c, PROF_ASSEMBLE);
    hipLaunchKernelGGL(k_std_wells_axpy, dim3((4 * S.num + 63) / 64), dim3(64), 0, c->stream, 4 * S.num, relax, c->wells.d_xw, S.x());
    prof_end(c, ps);
}

// ============================== small permutation helpers =====================================================
__global__ void k_cellvec_to_internal_u8(int Nb, const int* __restrict__ fromOrder, const unsigned char* __restrict__ nat, unsigned char* __restrict__ internal) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < Nb) internal[p] = nat[fromOrder[p]];
}
__global__ void k_cellvec_to_natural_u8(int Nb, const int* __restrict__ toOrder, const unsigned char* __restrict__ internal, unsigned char* __restrict__ nat) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Nb) nat[i] = internal[toOrder[i]];
}
__global__ void k_iq_to_natural(int Nb, int IQS, const int* __restrict__ toOrder, const double* __restrict__ internal, double* __restrict__ nat) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)Nb * IQS) return;
    const int i = (int)(e / IQS), q = (int)(e % IQS);
    nat[e] = internal[((size_t)(q >> 2) * Nb + toOrder[i]) * 4 + (q & 3)];   // field-major cache -> per-cell records
}
// records of n named cells out of the field-major cache (opmhip_get_iq_cells)
__global__ void k_iq_gather(int n, int IQS, int Nb, const int* __restrict__ pos, const double* __restrict__ internal, double* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)n * IQS) return;
    const int i = (int)(e / IQS), q = (int)(e % IQS);
    out[e] = internal[((size_t)(q >> 2) * Nb + pos[i]) * 4 + (q & 3)];
}
// source terms of n DISTINCT cells into the (zeroed) per-cell arrays (opmhip_set_source_cells)
__global__ void k_source_scatter(int n, const int* __restrict__ pos, const double* __restrict__ src, const double* __restrict__ dsrc,
                                 double* __restrict__ source, double* __restrict__ dsource) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * 12) return;
    const int i = e / 12, q = e % 12;
    if (q < 3) source[(size_t)pos[i] * 3 + q] = src[(size_t)i * 3 + q];
    else if (dsrc) dsource[(size_t)pos[i] * 9 + (q - 3)] = dsrc[(size_t)i * 9 + (q - 3)];
}
__global__ void k_unpermute_blocks(int nnzb, const int* __restrict__ nnzMap, const double* __restrict__ internal, double* __restrict__ nat) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)nnzb * BB) return;
    const int k = (int)(e / BB), q = (int)(e % BB);
    nat[(size_t)nnzMap[k] * BB + q] = internal[e];
}

// ============================== launchers ====================================================================
static inline int cdiv(size_t a, size_t b) { return (int)((a + b - 1) / b); }
static Tables tables_of(const opmhip_ctx* c) {
    return Tables{c->asmb.d_tab_dbl, c->asmb.d_tab_idx, c->asmb.rock_pref, c->asmb.rock_cr, c->asmb.tab_ndbl, c->asmb.tab_nidx, c->asmb.rock_desc, c->asmb.num_rock};
}
static CellStatic cells_of(const opmhip_ctx* c) {
    return CellStatic{c->asmb.d_poro, c->asmb.d_volume, c->asmb.d_depth, c->asmb.d_rsmax, c->asmb.d_pvtnum, c->asmb.d_satnum,
                      c->asmb.d_rvmax, c->asmb.d_overburden, c->asmb.d_rocknum, c->asmb.d_pcw, c->asmb.d_minpo, c->asmb.d_maxso, c->asmb.vap1, c->asmb.vap2,
                      c->asmb.d_maxsw, c->asmb.d_sw0, c->asmb.d_wcdesc, c->asmb.d_wcdata, c->asmb.d_eps, c->asmb.epscfg,
                      c->asmb.d_hyst, c->asmb.d_imbnum, c->asmb.d_eps_imb, c->asmb.hyst_model, c->asmb.d_invb, c->pat.Nloc};
}
// sw_ow / sw_go (device, internal order, Nloc each) or NULL: from the intensive quantities of the state at hand
void launch_hyst_update(opmhip_ctx* c, const double* d_sw_ow, const double* d_sw_go) {
    const int N = c->pat.Nloc;   // all cells, the ghost ones too ("to avoid desynchronization of the processes", :2608-2609)
    hipLaunchKernelGGL(k_hyst_update, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, tables_of(c), cells_of(c), c->asmb.d_iq, c->asmb.d_hyst, d_sw_ow, d_sw_go);
}
// the context's record layout: extended when the fluid has PVTG or ROCKTAB tables
#define OPMHIP_LAYOUT(c, call_base, call_ext) do { if ((c)->asmb.ext) { call_ext; } else { call_base; } } while (0)

void launch_iq_update(opmhip_ctx* c) {
    const int Nb = c->pat.Nloc;  // ghost cells too: their intensive quantities feed the faces towards them
    const int ps = prof_begin(c, PROF_IQ_UPDATE);
    OPMHIP_LAYOUT(c,
        hipLaunchKernelGGL(k_iq_update<false>, dim3(cdiv(Nb, 256)), dim3(256), 0, c->stream, 0, Nb, tables_of(c), cells_of(c), c->asmb.d_pv, c->asmb.d_meaning, c->asmb.d_iq),
        hipLaunchKernelGGL(k_iq_update<true>, dim3(cdiv(Nb, 256)), dim3(256), 0, c->stream, 0, Nb, tables_of(c), cells_of(c), c->asmb.d_pv, c->asmb.d_meaning, c->asmb.d_iq));
    prof_end(c, ps);
}
// after a Newton update in a decomposed run: ghost primary variables come from their owners, then their IQs are redone
int launch_ghost_refresh(opmhip_ctx* c) {
    if (c->comm.nranks <= 1 || c->pat.Nghost == 0) return OPMHIP_SUCCESS;
    int rc;
    if ((rc = comm_halo_f64(c, c->asmb.d_pv, 3))) return rc;
    if ((rc = comm_halo_u8(c, c->asmb.d_meaning))) return rc;
    const int Nb = c->pat.Nb, Nloc = c->pat.Nloc;
    OPMHIP_LAYOUT(c,
        hipLaunchKernelGGL(k_iq_update<false>, dim3(cdiv(Nloc - Nb, 256)), dim3(256), 0, c->stream, Nb, Nloc, tables_of(c), cells_of(c), c->asmb.d_pv, c->asmb.d_meaning, c->asmb.d_iq),
        hipLaunchKernelGGL(k_iq_update<true>, dim3(cdiv(Nloc - Nb, 256)), dim3(256), 0, c->stream, Nb, Nloc, tables_of(c), cells_of(c), c->asmb.d_pv, c->asmb.d_meaning, c->asmb.d_iq));
    return OPMHIP_SUCCESS;
}
void launch_newton_update(opmhip_ctx* c, const double* d_dx, double relax) {
    const int Nb = c->pat.Nb;
    (void)hipMemsetAsync(c->asmb.d_nswitched, 0, sizeof(int), c->stream);
    const int ps = prof_begin(c, PROF_IQ_UPDATE);
    OPMHIP_LAYOUT(c,
        hipLaunchKernelGGL(k_newton_update<false>, dim3(cdiv(Nb, 256)), dim3(256), 0, c->stream, Nb, tables_of(c), cells_of(c), d_dx, relax, c->asmb.d_pv,
                           c->asmb.d_meaning, c->asmb.d_wasSwitched, c->asmb.d_iq, c->asmb.d_nswitched),
        hipLaunchKernelGGL(k_newton_update<true>, dim3(cdiv(Nb, 256)), dim3(256), 0, c->stream, Nb, tables_of(c), cells_of(c), d_dx, relax, c->asmb.d_pv,
                           c->asmb.d_meaning, c->asmb.d_wasSwitched, c->asmb.d_iq, c->asmb.d_nswitched));
    prof_end(c, ps);
}
void launch_assemble(opmhip_ctx* c, double dt, int iteration) {
    EntryStatic ES{c->asmb.d_trans, c->asmb.d_area, c->asmb.d_thpres};
    const int ps = prof_begin(c, PROF_ASSEMBLE);
    const double* drift = c->asmb.drift_enabled ? c->asmb.d_drift : (const double*)nullptr;
    const int grid = c->asmb.nsched;
    if (iteration == 0 && c->asmb.storage_frozen) iteration = 1;   // the old time level's storage was formed by opmhip_begin_time_step
    // split assembly: the Jacobian goes where the ILU0 solve reads it (d_R, d_U) and d_A is left alone - unless a well list is to be
    // added to the matrix afterwards, which works on d_A
    const bool split = c->split_asm && c->asmb.split_ok && !c->wells.sw.matrix_add;
#define OPMHIP_ASM_LAUNCH(EXT, SPL, WET)                                                                                                                                   \
    hipLaunchKernelGGL((k_assemble<EXT, SPL>), dim3(grid), dim3(ASM_THREADS), 0, c->stream, c->asmb.nsched, reinterpret_cast<const int4*>(c->asmb.d_asm_sched),                \
                       reinterpret_cast<const int2*>(c->asmb.d_asm_desc), WET, ES, cells_of(c), c->asmb.d_iq, c->asmb.d_storageOld, c->asmb.d_source, c->asmb.d_dsource, drift, \
                       c->asmb.max_compensation, dt, iteration, SPL ? c->d_R : c->d_A, c->d_b, c->d_U, c->pat.d_rrowptr, c->pat.d_urowptr)
    if (split) { OPMHIP_LAYOUT(c, OPMHIP_ASM_LAUNCH(false, true, 0), OPMHIP_ASM_LAUNCH(true, true, c->asmb.wet_gas ? 1 : 0)); }
    else { OPMHIP_LAYOUT(c, OPMHIP_ASM_LAUNCH(false, false, 0), OPMHIP_ASM_LAUNCH(true, false, c->asmb.wet_gas ? 1 : 0)); }
#undef OPMHIP_ASM_LAUNCH
    c->A_stale = split;
    if (split) c->split_assemblies++;
    prof_end(c, ps);
}
void launch_last_rs_rv(opmhip_ctx* c) {
    const AsmDev& A = c->asmb;
    const int N = c->pat.Nloc;
    OPMHIP_LAYOUT(c, hipLaunchKernelGGL(k_last_rs_rv<false>, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, A.d_pvtnum, A.d_drsdt_all, A.d_iq, A.drsdt_on ? A.d_lastRs : nullptr, (double*)nullptr),
                  hipLaunchKernelGGL(k_last_rs_rv<true>, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, A.d_pvtnum, A.d_drsdt_all, A.d_iq, A.drsdt_on ? A.d_lastRs : nullptr, A.drvdt_on ? A.d_lastRv : nullptr));
}
void launch_set_limits(opmhip_ctx* c, double dt) {
    const AsmDev& A = c->asmb;
    const int N = c->pat.Nloc;
    hipLaunchKernelGGL(k_set_limits, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, dt, A.d_pvtnum, A.drsdt_on ? A.d_drsdt : nullptr, A.drvdt_on ? A.d_drvdt : nullptr,
                       A.d_lastRs, A.d_lastRv, A.d_rsmax, A.d_rvmax);
}
void launch_min_pressure(opmhip_ctx* c, bool init) {
    const int N = c->pat.Nloc;
    hipLaunchKernelGGL(k_min_pressure, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, init ? 1 : 0, c->asmb.d_iq, c->asmb.d_minpo);
}
void launch_max_oil_saturation(opmhip_ctx* c, bool init) {
    const int N = c->pat.Nloc;
    hipLaunchKernelGGL(k_max_oil_saturation, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, init ? 1 : 0, c->asmb.d_iq, c->asmb.d_maxso);
}
void launch_max_water_saturation(opmhip_ctx* c, bool init) {
    const Pattern& P = c->pat;
    const int N = P.Nloc;
    // eclproblem.hh:2150: the cell with index 1 takes over the stored maximum of the cell with index 0 (natural numbering)
    if (!init && N > 1) hipLaunchKernelGGL(k_copy_entry, dim3(1), dim3(1), 0, c->stream, c->asmb.d_maxsw, P.toOrder[1], P.toOrder[0]);
    hipLaunchKernelGGL(k_max_water_saturation, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, init ? 1 : 0, c->asmb.d_iq, c->asmb.d_maxsw, c->asmb.d_sw0);
}
void launch_storage_old(opmhip_ctx* c) {
    const AsmDev& A = c->asmb;
    const int Nb = c->pat.Nb, N = c->pat.Nloc;
    OPMHIP_LAYOUT(c, hipLaunchKernelGGL(k_storage_old<false>, dim3((Nb + 255) / 256), dim3(256), 0, c->stream, Nb, N, 0, A.d_iq, A.d_storageOld),
                  hipLaunchKernelGGL(k_storage_old<true>, dim3((Nb + 255) / 256), dim3(256), 0, c->stream, Nb, N, A.wet_gas ? 1 : 0, A.d_iq, A.d_storageOld));
}

// BlackoilModelEbos::relativeChange (flow/BlackoilModelEbos.hpp:431-510): sum over the owned cells of (p_new - p_old)^2 and of
// the squared saturation changes, over the sum of p_new^2 and the squared new saturations - what the PID time-step control
// calls the error of a time step (timestepping/TimeStepControl.cpp:127-161).  solution(0) = the state, solution(1) = the
// time level opmhip_advance_time_level kept.  Per cell the terms are added in the reference's order (pressure, then water,
// oil, gas); the cells are summed by a fixed tree (a sequential sum over 10^6 cells is not what a GPU does), so the result
// agrees with the reference's sequential sum to rounding, not to the bit.
constexpr int RC_PARTS = 256;
__global__ __launch_bounds__(256) void k_relative_change_part(int Nb, const double* __restrict__ pv, const unsigned char* __restrict__ mg,
                                                              const double* __restrict__ pvOld, const unsigned char* __restrict__ mgOld,
                                                              double* __restrict__ part) {
    __shared__ double sd[256], sn[256];
    double delta = 0.0, denom = 0.0;
    for (int c = blockIdx.x * 256 + threadIdx.x; c < Nb; c += RC_PARTS * 256) {
        const double* a = &pv[(size_t)c * 3];
        const double* b = &pvOld[(size_t)c * 3];
        double sN[3] = {0.0, 0.0, 0.0}, sO[3] = {0.0, 0.0, 0.0};
        double oilN = 1.0, oilO = 1.0;
        sN[WATER] = a[0]; oilN -= sN[WATER];
        if (mg[c] == OPMHIP_SW_PO_SG) { sN[GAS] = a[2]; oilN -= sN[GAS]; }
        sN[OIL] = oilN;
        const double tmp = a[1] - b[1];
        double d = tmp * tmp, q = a[1] * a[1];
        sO[WATER] = b[0]; oilO -= sO[WATER];
        if (mgOld[c] == OPMHIP_SW_PO_SG) { sO[GAS] = b[2]; oilO -= sO[GAS]; }
        sO[OIL] = oilO;
#pragma unroll
        for (int ph = 0; ph < 3; ++ph) {
            const double t = sN[ph] - sO[ph];
            d += t * t;
            q += sN[ph] * sN[ph];
        }
        delta += d;
        denom += q;
    }
    sd[threadIdx.x] = delta; sn[threadIdx.x] = denom;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) { sd[threadIdx.x] += sd[threadIdx.x + h]; sn[threadIdx.x] += sn[threadIdx.x + h]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[blockIdx.x] = sd[0]; part[RC_PARTS + blockIdx.x] = sn[0]; }
}
__global__ __launch_bounds__(64) void k_relative_change_final(const double* __restrict__ part, double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    double d = 0.0, q = 0.0;
    for (int i = 0; i < RC_PARTS; ++i) { d += part[i]; q += part[RC_PARTS + i]; }
    out[0] = d; out[1] = q;
}
// -> d_rc[2 * RC_PARTS .. + 2): (resultDelta, resultDenom), summed over the ranks of a decomposed run (gridView.comm().sum)
int launch_relative_change(opmhip_ctx* c) {
    const AsmDev& A = c->asmb;
    double* part = A.d_rc;
    double* out = A.d_rc + 2 * RC_PARTS;
    hipLaunchKernelGGL(k_relative_change_part, dim3(RC_PARTS), dim3(256), 0, c->stream, c->pat.Nb, A.d_pv, A.d_meaning, A.d_pv_prev, A.d_meaning_prev, part);
    hipLaunchKernelGGL(k_relative_change_final, dim3(1), dim3(64), 0, c->stream, part, out);
    if (c->comm.nranks > 1) return comm_allreduce(c, out, 2, 0);
    return OPMHIP_SUCCESS;
}

int launch_convergence(opmhip_ctx* c, double dt, double tol_cnv) {
    const int Nb = c->pat.Nb, nb = cdiv(Nb, 256);
    const int ps = prof_begin(c, PROF_CONVERGENCE);
    hipLaunchKernelGGL(k_conv_pass1, dim3(nb), dim3(256), 0, c->stream, Nb, cells_of(c), c->d_b, c->asmb.d_conv_part);
    const bool dd = c->comm.nranks > 1;
    hipLaunchKernelGGL(k_conv_final1, dim3(1), dim3(256), 0, c->stream, nb, dd ? 0 : Nb, c->asmb.d_conv_part, c->asmb.d_conv_out);
    if (dd) {
        hipLaunchKernelGGL(k_conv_pack, dim3(1), dim3(64), 0, c->stream, c->asmb.d_conv_out, c->comm.d_red);
        int rc;  // a failed reduction must not be read as "converged": report it
        if ((rc = comm_allreduce(c, c->comm.d_red, 7, 0))) return rc;
        if ((rc = comm_allreduce(c, c->comm.d_red + 8, 3, 1))) return rc;
        hipLaunchKernelGGL(k_conv_unpack, dim3(1), dim3(64), 0, c->stream, c->comm.d_red, (double)c->comm.global_cells, c->asmb.d_conv_out);
    }
    hipLaunchKernelGGL(k_conv_pass2, dim3(nb), dim3(256), 0, c->stream, Nb, cells_of(c), c->d_b, c->asmb.d_conv_out, dt, tol_cnv, c->asmb.d_conv_part);
    hipLaunchKernelGGL(k_conv_final2, dim3(1), dim3(256), 0, c->stream, nb, c->asmb.d_conv_part, c->asmb.d_conv_out);
    if (dd) {
        const int rc = comm_allreduce(c, c->asmb.d_conv_out + 10, 1, 0);
        if (rc) return rc;
    }
    prof_end(c, ps);
    return OPMHIP_SUCCESS;
}
// the two kernels of the reservoir averages: asmb.d_resv = the partials, then the RESV_OUT results
static double* resv_avg_kernels(opmhip_ctx* c) {
    const int Nb = c->pat.Nb, nb = cdiv(Nb, 256) < RESV_MAX_PARTS ? cdiv(Nb, 256) : RESV_MAX_PARTS;
    double* part = c->asmb.d_resv;
    double* avg = part + (size_t)RESV_MAX_PARTS * RESV_SUMS;
    OPMHIP_LAYOUT(c,
        hipLaunchKernelGGL(k_resv_avg_part<false>, dim3(nb), dim3(256), 0, c->stream, Nb, c->pat.Nloc, c->asmb.d_iq, c->asmb.d_volume, part),
        hipLaunchKernelGGL(k_resv_avg_part<true>, dim3(nb), dim3(256), 0, c->stream, Nb, c->pat.Nloc, c->asmb.d_iq, c->asmb.d_volume, part));
    hipLaunchKernelGGL(k_resv_avg_final, dim3(1), dim3(RESV_FINAL_THREADS), 0, c->stream, nb, part, avg);
    return avg;
}
// (one scope: a time step of a list with a RESV limit shows one more entry of the assembly class than one without)
void launch_std_wells_resv(opmhip_ctx* c) {
    const StdWellsDev& S = c->wells.sw;
    const int ps = prof_begin(c, PROF_ASSEMBLE);
    const double* avg = resv_avg_kernels(c);
    hipLaunchKernelGGL(k_std_wells_resv_coeff, dim3((S.num + 63) / 64), dim3(64), 0, c->stream, S.num, S.d_wi, c->wells.d_val_pointers, c->wells.d_Ccols, c->asmb.d_pvtnum,
                       tables_of(c), std_wells_lim(c), avg, S.grp_resv ? S.d_grp_resv : nullptr);
    prof_end(c, ps);
}
void launch_reservoir_averages(opmhip_ctx* c) {
    const int ps = prof_begin(c, PROF_ASSEMBLE);   // (the well model's, as the standard wells' launches: one span per call)
    resv_avg_kernels(c);
    prof_end(c, ps);
}
void launch_u8_to_internal(opmhip_ctx* c, const unsigned char* nat, unsigned char* internal) {
    hipLaunchKernelGGL(k_cellvec_to_internal_u8, dim3(cdiv(c->pat.Nloc, 256)), dim3(256), 0, c->stream, c->pat.Nloc, c->pat.d_fromOrder, nat, internal);
}
void launch_u8_to_natural(opmhip_ctx* c, const unsigned char* internal, unsigned char* nat) {
    hipLaunchKernelGGL(k_cellvec_to_natural_u8, dim3(cdiv(c->pat.Nloc, 256)), dim3(256), 0, c->stream, c->pat.Nloc, c->pat.d_toOrder, internal, nat);
}
void launch_iq_to_natural(opmhip_ctx* c, double* d_nat) {
    const size_t n = (size_t)c->pat.Nloc * iq_doubles_per_cell(c);
    hipLaunchKernelGGL(k_iq_to_natural, dim3(cdiv(n, 256)), dim3(256), 0, c->stream, c->pat.Nloc, iq_doubles_per_cell(c), c->pat.d_toOrder, c->asmb.d_iq, d_nat);
}
void launch_iq_gather(opmhip_ctx* c, int n, const int* d_pos, double* d_out) {
    const int IQS = iq_doubles_per_cell(c);
    hipLaunchKernelGGL(k_iq_gather, dim3(cdiv((size_t)n * IQS, 256)), dim3(256), 0, c->stream, n, IQS, c->pat.Nloc, d_pos, c->asmb.d_iq, d_out);
}
void launch_source_scatter(opmhip_ctx* c, int n, const int* d_pos, const double* d_src, const double* d_dsrc) {
    hipLaunchKernelGGL(k_source_scatter, dim3(cdiv((size_t)n * 12, 256)), dim3(256), 0, c->stream, n, d_pos, d_src, d_dsrc, c->asmb.d_source, c->asmb.d_dsource);
}
void launch_unpermute_blocks(opmhip_ctx* c, const double* internal, double* nat) {
    const size_t n = (size_t)c->pat.nnzb * BB;
    hipLaunchKernelGGL(k_unpermute_blocks, dim3(cdiv(n, 256)), dim3(256), 0, c->stream, c->pat.nnzb, c->pat.d_nnzMap, internal, nat);
}
int iq_doubles_per_cell(const opmhip_ctx* c) { return c->asmb.ext ? Lay<true>::IQS : Lay<false>::IQS; }

}  // namespace opmhip
