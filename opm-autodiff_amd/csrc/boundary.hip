// Open boundaries on the device (opmhip_set_boundary_conditions): FREE and RATE faces of the BC keyword.
// EclProblem::boundary (ebos/eclproblem.hh:1602-1671) with calculateBoundaryGradients_ (ebos/eclfluxmodule.hh:362-468) statement by
// statement in Ad arithmetic (the library is built with -ffp-contract=off: the expression trees below are the ones boundary.py's
// HostBoundary copies to get the same bits).  The step from phase volume fluxes to the three equations -
// BlackOilBoundaryRateVector::setFreeFlow / setMassRate, evalPhaseFluxes_ - is opm-models' and not in the reference tree: restated from
// its published form, UNVERIFIED (include/opmhip.h "open boundaries" says what was decided).
// Plain wave64 kernels, one lane per distinct boundary cell / exterior record; no atomics, no LDS: a cell has at most six faces and
// every array is read once.
#include "fluid_device.hpp"
#include "internal.hpp"

namespace opmhip {

// initialFluidStates_[globalDofIdx] of the cells with a FREE face: the values of the interior cell's own record, now
template <bool EXT>
__global__ __launch_bounds__(64) void k_boundary_capture(int nfc, int ncell, const int* __restrict__ fcell, const int* __restrict__ cpos,
                                                         const double* __restrict__ iq, double* __restrict__ ext) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= nfc) return;
    const int c = cpos[fcell[s]];
    double* x = ext + (size_t)s * BC_EXT;
    for (int ph = 0; ph < 3; ++ph) {
        x[BX_P + ph] = iq_at(iq, ncell, F_P + ph, c)[0];
        x[BX_RHO + ph] = iq_at(iq, ncell, F_RHO + ph, c)[0];
        x[BX_MOB + ph] = iq_at(iq, ncell, F_MOB + ph, c)[0];
        x[BX_B + ph] = iq_at(iq, ncell, F_B + ph, c)[0];
    }
    x[BX_RS] = iq_at(iq, ncell, F_RS, c)[0];
    x[BX_RV] = EXT ? iq_at(iq, ncell, Lay<EXT>::F_RV, c)[0] : 0.0;
}

// setFreeFlow on one face: r[3] per unit area times the area, positive out of the cell
template <bool EXT>
__device__ __forceinline__ void boundary_free_flow(const double* __restrict__ iq, int ncell, int c, bool wet, const double* __restrict__ x,
                                                   double trans, double faceArea, double zIn, double zEx, Ad r[3]) {
    r[0] = r[1] = r[2] = ad_const(0.0);
    const double distZ = zIn - zEx;
    const int comp[3] = {EQ_WATER, EQ_OIL, EQ_GAS};
    for (int ph = 0; ph < 3; ++ph) {
        const Ad rhoIn = load_ad(iq_at(iq, ncell, F_RHO + ph, c)), pIn = load_ad(iq_at(iq, ncell, F_P + ph, c));
        // calculateBoundaryGradients_ (:401-467)
        const Ad rhoAvg = (rhoIn + x[BX_RHO + ph]) / 2.0;
        Ad pressureExterior = ad_const(x[BX_P + ph]);
        pressureExterior = pressureExterior + rhoAvg * (distZ * GRAVITY);
        const Ad dp = pressureExterior - pIn;
        Ad volumeFlux;
        if (dp.v > 0.0) {   // the exterior is upstream: its mobility, a plain number
            volumeFlux = (dp * x[BX_MOB + ph]) * (-trans / faceArea);
        } else {            // rockCompTransMultiplier<double> of the interior cell: the ROCKTAB multiplier's value
            double transModified = trans;
            if (EXT) transModified = transModified * iq_at(iq, ncell, Lay<EXT>::F_TMULT, c)[0];
            volumeFlux = (dp * load_ad(iq_at(iq, ncell, F_MOB + ph, c))) * (-transModified / faceArea);
        }
        // setFreeFlow / evalPhaseFluxes_ (UNVERIFIED): the raw phase pressures choose whose 1/B, Rs and Rv the flux carries
        const double pBoundary = x[BX_P + ph];
        Ad surf;
        if (pBoundary < pIn.v) {          // outflux: the interior's, with derivatives
            surf = load_ad(iq_at(iq, ncell, F_B + ph, c)) * volumeFlux;
            r[comp[ph]] = r[comp[ph]] + surf;
            if (ph == OIL) r[EQ_GAS] = r[EQ_GAS] + load_ad(iq_at(iq, ncell, F_RS, c)) * surf;
            if (EXT && ph == GAS && wet) r[EQ_OIL] = r[EQ_OIL] + load_ad(iq_at(iq, ncell, Lay<EXT>::F_RV, c)) * surf;
        } else if (pBoundary > pIn.v) {   // influx: the captured state's, plain numbers
            surf = x[BX_B + ph] * volumeFlux;
            r[comp[ph]] = r[comp[ph]] + surf;
            if (ph == OIL) r[EQ_GAS] = r[EQ_GAS] + x[BX_RS] * surf;
            if (EXT && ph == GAS && wet) r[EQ_OIL] = r[EQ_OIL] + x[BX_RV] * surf;
        }                                 // equal: the phase adds nothing
    }
    for (int e = 0; e < 3; ++e) r[e] = r[e] * faceArea;   // evalBoundary_: the rate per area times scvf.area()
}

struct BcArrays {
    const int *type, *cpos, *cptr, *cconn, *slot;
    const double *geo, *rate, *ext;
};
// In front of k_assemble (behind the wells' and the aquifers' apply), one lane per DISTINCT boundary cell: the caller's source row and
// dsource block are kept in `save`; the cell's faces in list order, each face's 12 numbers stored for opmhip_get_boundary_rates and
// subtracted from the cell's source and derivative (the boundary rate is positive out of the cell, the source a rate into it)
template <bool EXT>
__global__ __launch_bounds__(64) void k_boundary_apply(int nd, int ncell, BcArrays B, Tables T, const int* __restrict__ pvtnum, int wet,
                                                       const double* __restrict__ iq, const double* __restrict__ depth, double* __restrict__ source,
                                                       double* __restrict__ dsource, double* __restrict__ save, double* __restrict__ q12) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= nd) return;
    const int c = B.cpos[t];
    double* s = source + (size_t)c * 3;
    double* ds = dsource + (size_t)c * 9;
    double* sv = save + (size_t)t * BC_Q;
    Ad S[3];
    for (int e = 0; e < 3; ++e) {
        S[e] = Ad{s[e], ds[3 * e], ds[3 * e + 1], ds[3 * e + 2]};
        sv[e] = S[e].v; sv[3 + 3 * e] = S[e].d0; sv[3 + 3 * e + 1] = S[e].d1; sv[3 + 3 * e + 2] = S[e].d2;
    }
    const double zIn = depth[c];
    for (int k = B.cptr[t]; k < B.cptr[t + 1]; ++k) {
        const int f = B.cconn[k];
        const double* g = B.geo + (size_t)f * BC_GEO;
        Ad r[3];
        if (B.type[f] == OPMHIP_BC_FREE) {
            boundary_free_flow<EXT>(iq, ncell, c, wet != 0, B.ext + (size_t)B.slot[t] * BC_EXT, g[BC_TRANS], g[BC_AREA], zIn, g[BC_DEPTH], r);
        } else {   // setMassRate (UNVERIFIED): mass rate / reference density of the component in the cell's PVT region, times the area
            const GlobalTab rhoRef = T.dbl + T.pvt(pvtnum ? pvtnum[c] : 0).density;   // oil, water, gas: the equations' order
            for (int e = 0; e < 3; ++e) r[e] = ad_const((B.rate[(size_t)f * 3 + e] / rhoRef[e]) * g[BC_AREA]);
        }
        double* q = q12 + (size_t)f * BC_Q;
        for (int e = 0; e < 3; ++e) {
            q[e] = r[e].v; q[3 + 3 * e] = r[e].d0; q[3 + 3 * e + 1] = r[e].d1; q[3 + 3 * e + 2] = r[e].d2;
            S[e] = S[e] - r[e];
        }
    }
    for (int e = 0; e < 3; ++e) { s[e] = S[e].v; ds[3 * e] = S[e].d0; ds[3 * e + 1] = S[e].d1; ds[3 * e + 2] = S[e].d2; }
}
// behind k_assemble (ahead of the aquifers' and the wells' restores: the save areas nest): the caller's row and block back
__global__ __launch_bounds__(64) void k_boundary_restore(int nd, const int* __restrict__ cpos, const double* __restrict__ save, double* __restrict__ source,
                                                         double* __restrict__ dsource) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= nd) return;
    const int c = cpos[t];
    const double* sv = save + (size_t)t * BC_Q;
    for (int e = 0; e < 3; ++e) source[(size_t)c * 3 + e] = sv[e];
    for (int k = 0; k < 9; ++k) dsource[(size_t)c * 9 + k] = sv[3 + k];
}

void launch_boundary_capture(opmhip_ctx* c) {
    const BoundaryDev& B = c->asmb.bc;
    const dim3 grid((B.nfc + 63) / 64), block(64);
    if (c->asmb.ext) hipLaunchKernelGGL(k_boundary_capture<true>, grid, block, 0, c->stream, B.nfc, c->pat.Nloc, B.d_fcell, B.d_cpos, c->asmb.d_iq, B.d_ext);
    else hipLaunchKernelGGL(k_boundary_capture<false>, grid, block, 0, c->stream, B.nfc, c->pat.Nloc, B.d_fcell, B.d_cpos, c->asmb.d_iq, B.d_ext);
}
void launch_boundary_apply(opmhip_ctx* c) {
    const BoundaryDev& B = c->asmb.bc;
    const AsmDev& A = c->asmb;
    const BcArrays arr{B.d_type, B.d_cpos, B.d_cptr, B.d_cconn, B.d_slot, B.d_geo, B.d_rate, B.d_ext};
    const dim3 grid((B.nd + 63) / 64), block(64);
    if (A.ext)
        hipLaunchKernelGGL(k_boundary_apply<true>, grid, block, 0, c->stream, B.nd, c->pat.Nloc, arr, tables_of(c), A.d_pvtnum, A.wet_gas ? 1 : 0, A.d_iq, A.d_depth,
                           A.d_source, A.d_dsource, B.d_save, B.d_q);
    else
        hipLaunchKernelGGL(k_boundary_apply<false>, grid, block, 0, c->stream, B.nd, c->pat.Nloc, arr, tables_of(c), A.d_pvtnum, 0, A.d_iq, A.d_depth,
                           A.d_source, A.d_dsource, B.d_save, B.d_q);
}
void launch_boundary_restore(opmhip_ctx* c) {
    const BoundaryDev& B = c->asmb.bc;
    hipLaunchKernelGGL(k_boundary_restore, dim3((B.nd + 63) / 64), dim3(64), 0, c->stream, B.nd, B.d_cpos, B.d_save, c->asmb.d_source, c->asmb.d_dsource);
}

}  // namespace opmhip
