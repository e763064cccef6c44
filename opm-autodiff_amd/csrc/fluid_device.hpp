// One copy of the device-side fluid arithmetic that more than one unit states: the dense AD scalar the lookups are written over, the
// property-table types and lookups, the layout of the intensive-quantity cache and 1/B of the three phases.  assemble.hip (the
// reservoir) and std_wells.hip (the resident standard wells) both read the tables and the cache through these, so a well-bore density
// carries the bits of the fluid probes.  HIP units only.
#pragma once
#include <hip/hip_runtime.h>

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
__device__ __forceinline__ void set_val(Ad& a, double v) { a.v = v; }
__device__ __forceinline__ void set_val(double& a, double v) { a = v; }
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
    E r = y0 + (y1 - y0) * (xv - x0) / (x1 - x0);
    // the right end of a segment is met only on the table's last node (an interior node belongs to the segment on its right); there
    // the product and the sum above can miss the sample by an ulp, so the value is the sample itself and the slope stays the segment's
    if (val(xv) == x1) set_val(r, y1);
    return r;
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

// ============================== intensive-quantity cache ======================================================
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
// one field (value + 3 derivatives, 16-byte aligned) as two 16-byte accesses
__device__ __forceinline__ void store_ad(double* o, const Ad& a) {
    *reinterpret_cast<double2*>(o) = make_double2(a.v, a.d0);
    *reinterpret_cast<double2*>(o + 2) = make_double2(a.d1, a.d2);
}
__device__ __forceinline__ Ad load_ad(const double* o) {
    const double2 a = *reinterpret_cast<const double2*>(o), b = *reinterpret_cast<const double2*>(o + 2);
    return Ad{a.x, a.y, b.x, b.y};
}
template <bool EXT> struct Lay {
    static constexpr int F_RV = 16, F_TMULT = 17;                    // EXT only
    static constexpr int F_PORO = EXT ? 18 : 16;
    static constexpr int IQF = EXT ? 19 : 17;                        // fields per cell
    static constexpr int IQS = IQF * 4;                              // doubles per cell
    static constexpr int RQ_F0 = F_P;                                // neighbour fields of the flux: p, 1/B, mobility, density, Rs [, Rv, tmult]
    static constexpr int RQ_NF = (EXT ? F_TMULT : F_RS) - F_P + 1;
};
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
inline Tables tables_of(const opmhip_ctx* c) {
    return Tables{c->asmb.d_tab_dbl, c->asmb.d_tab_idx, c->asmb.rock_pref, c->asmb.rock_cr, c->asmb.tab_ndbl, c->asmb.tab_nidx, c->asmb.rock_desc, c->asmb.num_rock};
}

}  // namespace opmhip
