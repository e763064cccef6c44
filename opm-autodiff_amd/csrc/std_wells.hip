// gfx950 kernels of the device-resident standard wells (opmhip_set_std_wells) and of the VFP tables their THP control reads
// (opmhip_set_vfp_tables): VFP interpolation, the well equations with their controls, limits and groups, the well-bore heads, and the
// launchers.  The fluid tables and the intensive-quantity cache are read through fluid_device.hpp, as assemble.hip reads them.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "device_blocks.hpp"
#include "fluid_device.hpp"

namespace opmhip {

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
    return SwThp{S.thp.d_table, S.thp.d_wd, S.thp.d_out, V.d_desc, V.d_dbl, S.wb.d_out};
}
static SwLim std_wells_lim(opmhip_ctx* c) {
    const StdWellsDev& S = c->wells.sw;
    return SwLim{S.lim.d_lim, S.lim.d_use, S.lim.on ? S.lim.d_out : S.grp.d_out};   // (a list with groups and without limits keeps the coefficients and the averages in its own array)
}
static SwGrp std_wells_grp(opmhip_ctx* c) {
    const SwGroupsDev& G = c->wells.sw.grp;
    return SwGrp{G.num, G.nupcol, G.d_ptr, G.d_idx, G.d_of, G.d_avail, G.d_guide, G.d_target, G.d_state, G.d_state ? G.d_state + G.num : nullptr, G.d_rec};
}
// the instantiation of k_std_wells_eq a list runs: one per combination of crossflow, THP limits, further rate limits and the vaporised-oil
// switch (a list without the feature runs the code it ran before; the number of launches is the same)
template <bool SOLVE, bool VO, bool GRP>
static auto std_wells_eq_kernel_of(const StdWellsDev& S) -> decltype(&k_std_wells_eq<SOLVE, false, false, false, VO, GRP>) {
    if (S.lim.on)
        return S.thp.on ? (S.cf.on ? k_std_wells_eq<SOLVE, true, true, true, VO, GRP> : k_std_wells_eq<SOLVE, false, true, true, VO, GRP>)
                     : (S.cf.on ? k_std_wells_eq<SOLVE, true, false, true, VO, GRP> : k_std_wells_eq<SOLVE, false, false, true, VO, GRP>);
    return S.thp.on ? (S.cf.on ? k_std_wells_eq<SOLVE, true, true, false, VO, GRP> : k_std_wells_eq<SOLVE, false, true, false, VO, GRP>)
                 : (S.cf.on ? k_std_wells_eq<SOLVE, true, false, false, VO, GRP> : k_std_wells_eq<SOLVE, false, false, false, VO, GRP>);
}
template <bool SOLVE>
static auto std_wells_eq_kernel(const StdWellsDev& S) -> decltype(&k_std_wells_eq<SOLVE, false, false, false, false, false>) {
    if (S.grp.on) return S.vo.on ? std_wells_eq_kernel_of<SOLVE, true, true>(S) : std_wells_eq_kernel_of<SOLVE, false, true>(S);
    return S.vo.on ? std_wells_eq_kernel_of<SOLVE, true, false>(S) : std_wells_eq_kernel_of<SOLVE, false, false>(S);
}
static SwArrays std_wells_arrays(const WellsDev& W) {
    const StdWellsDev& S = W.sw;
    return SwArrays{S.num, W.d_val_pointers, W.d_Ccols, S.d_wi, S.d_wd, S.d_tw, S.d_dz, S.d_head, S.d_pr, S.x(), S.d_Dmat, W.d_B, W.d_C, W.d_D,
                    S.wb.on ? 1 : 0, S.nperf, S.wb.d_state, S.cf.d_allow, S.cf.d_dq, S.vo.d_sol, S.control(), S.rw(), S.flag()};
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
                       WbArrays{S.wb.d_depth, S.wb.d_ref, S.wb.d_pref, S.wb.d_out, S.wb.d_scratch}, tables_of(c), c->asmb.d_pvtnum, c->pat.Nloc, c->asmb.d_iq,
                       first ? 1 : 0, init ? 1 : 0);
    prof_end(c, ps);
}
void launch_std_wells_controls(opmhip_ctx* c) {
    const StdWellsDev& S = c->wells.sw;
    const int ps = prof_begin(c, PROF_ASSEMBLE);
    const auto plain = S.lim.on ? (S.thp.on ? k_std_wells_controls<true, true, false> : k_std_wells_controls<false, true, false>)
                                : (S.thp.on ? k_std_wells_controls<true, false, false> : k_std_wells_controls<false, false, false>);
    const auto grouped = S.lim.on ? (S.thp.on ? k_std_wells_controls<true, true, true> : k_std_wells_controls<false, true, true>)
                                  : (S.thp.on ? k_std_wells_controls<true, false, true> : k_std_wells_controls<false, false, true>);
    hipLaunchKernelGGL(S.grp.on ? grouped : plain, dim3((S.num + 63) / 64), dim3(64), 0, c->stream, S.num, S.d_wi, S.d_wd, S.x(), S.control(), std_wells_thp(c),
                       std_wells_lim(c), tables_of(c), c->wells.d_val_pointers, c->wells.d_Ccols, c->asmb.d_pvtnum, std_wells_grp(c));
    prof_end(c, ps);
}
void launch_std_wells_groups(opmhip_ctx* c, int iteration, bool check) {
    const StdWellsDev& S = c->wells.sw;
    const int ps = prof_begin(c, PROF_ASSEMBLE);
    hipLaunchKernelGGL(check ? k_std_wells_groups<true> : k_std_wells_groups<false>, dim3((S.grp.num + 63) / 64), dim3(64), 0, c->stream, std_wells_grp(c), S.num,
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
// (one scope: a time step of a list with a RESV limit shows one more entry of the assembly class than one without)
void launch_std_wells_resv(opmhip_ctx* c) {
    const StdWellsDev& S = c->wells.sw;
    const int ps = prof_begin(c, PROF_ASSEMBLE);
    const double* avg = resv_avg_kernels(c);
    hipLaunchKernelGGL(k_std_wells_resv_coeff, dim3((S.num + 63) / 64), dim3(64), 0, c->stream, S.num, S.d_wi, c->wells.d_val_pointers, c->wells.d_Ccols, c->asmb.d_pvtnum,
                       tables_of(c), std_wells_lim(c), avg, S.grp.resv ? S.grp.d_resv : nullptr);
    prof_end(c, ps);
}

}  // namespace opmhip
