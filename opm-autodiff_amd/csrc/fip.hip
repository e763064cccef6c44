// Fluids in place and region pressures per FIP region (include/opmhip.h "fluids in place"; host set-up and the stated order of the
// sums: fip_setup.hpp; entry points: capi_fip.cpp).  Three kernels, all on the context's stream, no floating-point atomics:
//   k_fip_cells   one lane per cell, internal order: the twelve terms of ebos/ecloutputblackoilmodule.hh:610-697 from the values of the
//                 cached intensive quantities, field-major into d_terms[FIP_TERMS][Nloc]
//   k_fip_reduce  one launch per level of `reduce256`: one wavefront per chunk of 256 items, a lane carries the twelve accumulators
//                 of its four items, the lanes are combined by the shuffle-down tree, lane 0 stores the chunk's twelve results
//   k_fip_totals  the regions' sums out of their result slots (zeros for an id no cell carries) and, per term, one lane's sum of them
//                 from 0.0 in ascending id (update, ebos/eclgenericoutputblackoilmodule.cc:1420-1426)
// The build has -ffp-contract=off: every statement below is the rounding it reads as.
#include "fip_setup.hpp"
#include "fluid_device.hpp"
#include "internal.hpp"

namespace opmhip {

namespace {

template <bool EXT>
__global__ __launch_bounds__(256) void k_fip_cells(int Nb, int ncell, const double* __restrict__ iq, const double* __restrict__ volume,
                                                   const double* __restrict__ poro, double* __restrict__ terms) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= Nb) return;
    const double Sw = iq_at(iq, ncell, F_S + WATER, c)[0], So = iq_at(iq, ncell, F_S + OIL, c)[0], Sg = iq_at(iq, ncell, F_S + GAS, c)[0];
    const double bw = iq_at(iq, ncell, F_B + WATER, c)[0], bo = iq_at(iq, ncell, F_B + OIL, c)[0], bg = iq_at(iq, ncell, F_B + GAS, c)[0];
    const double po = iq_at(iq, ncell, F_P + OIL, c)[0], Rs = iq_at(iq, ncell, F_RS, c)[0];
    const double Rv = EXT ? iq_at(iq, ncell, Lay<EXT>::F_RV, c)[0] : 0.0;
    const double totVolume = volume[c];
    const double pv = totVolume * iq_at(iq, ncell, Lay<EXT>::F_PORO, c)[0];
    double hydrocarbon = 0.0;
    hydrocarbon += So;
    hydrocarbon += Sg;
    const double pressurePv = po * pv;
    const double fip_w = bw * Sw * pv, fip_o = bo * So * pv, fip_g = bg * Sg * pv;
    const double gasInPlaceLiquid = Rs * fip_o;
    const double oilInPlaceGas = Rv * fip_g;
    double* t = terms + c;
    const size_t n = (size_t)ncell;
    t[FIP_DYNAMIC_PV * n] = pv;
    t[FIP_PORE_VOLUME * n] = totVolume * poro[c];
    t[FIP_HC_PV * n] = pv * hydrocarbon;
    t[FIP_PRESSURE_PV * n] = pressurePv;
    t[FIP_PRESSURE_HC_PV * n] = pressurePv * hydrocarbon;
    t[FIP_OIL_IN_LIQUID * n] = fip_o;
    t[FIP_GAS_IN_GAS * n] = fip_g;
    t[FIP_GAS_IN_LIQUID * n] = gasInPlaceLiquid;
    t[FIP_OIL_IN_GAS * n] = oilInPlaceGas;
    t[FIP_WATER * n] = fip_w;
    t[FIP_OIL * n] = fip_o + oilInPlaceGas;
    t[FIP_GAS * n] = fip_g + gasInPlaceLiquid;
}

// Chunks [chunk0, chunk0 + nchunks) of one level.  GATHER (level 0): item i of the list is cell items[i], its terms at src[f * stride +
// items[i]]; otherwise (a later level) item i is slot i of the partial sums, src == part and stride == npart.  A level reads only slots
// the levels before it wrote and writes only its own chunks' slots.
template <bool GATHER>
__global__ __launch_bounds__(256) void k_fip_reduce(int chunk0, int nchunks, const int* __restrict__ desc, const int* __restrict__ items,
                                                    const double* src, size_t stride, double* part, size_t npart) {
    const int lane = threadIdx.x & 63;
    const int ch = blockIdx.x * 4 + (threadIdx.x >> 6);   // one wavefront, one chunk: the whole wavefront leaves together
    if (ch >= nchunks) return;
    const int* d = desc + (size_t)(chunk0 + ch) * 3;
    const int first = d[0], count = d[1], dest = d[2];
    double a[FIP_TERMS];
#pragma unroll
    for (int f = 0; f < FIP_TERMS; ++f) a[f] = 0.0;
#pragma unroll
    for (int k = 0; k < FIP_CHUNK / 64; ++k) {
        const int i = lane + 64 * k;
        const bool in = i < count;
        size_t at = 0;
        if (in) at = GATHER ? (size_t)items[first + i] : (size_t)(first + i);
#pragma unroll
        for (int f = 0; f < FIP_TERMS; ++f) {
            const double x = in ? src[f * stride + at] : 0.0;
            a[f] = a[f] + x;
        }
    }
#pragma unroll
    for (int f = 0; f < FIP_TERMS; ++f) {
        double v = a[f];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) part[f * npart + dest] = v;
    }
}

__global__ __launch_bounds__(64) void k_fip_totals(int max_id, const int* __restrict__ result, const double* __restrict__ part, size_t npart,
                                                   double* __restrict__ out) {
    const int f = threadIdx.x;
    if (f >= FIP_TERMS) return;
    double sum = 0.0;
    for (int r = 0; r < max_id; ++r) {
        const int s = result[r];
        const double rval = s >= 0 ? part[f * npart + s] : 0.0;
        out[(size_t)r * FIP_TERMS + f] = rval;
        sum += rval;
    }
    out[(size_t)max_id * FIP_TERMS + f] = sum;
}

}  // namespace

void launch_fip_cells(opmhip_ctx* c) {
    const AsmDev& A = c->asmb;
    const int Nb = c->pat.Nb, nb = (Nb + 255) / 256;
    if (nb == 0) return;
    if (A.ext)
        hipLaunchKernelGGL(k_fip_cells<true>, dim3(nb), dim3(256), 0, c->stream, Nb, c->pat.Nloc, A.d_iq, A.d_volume, A.d_poro, A.fip.d_terms);
    else
        hipLaunchKernelGGL(k_fip_cells<false>, dim3(nb), dim3(256), 0, c->stream, Nb, c->pat.Nloc, A.d_iq, A.d_volume, A.d_poro, A.fip.d_terms);
}

void launch_fip_reduce(opmhip_ctx* c, const FipSetDev& S) {
    const FipDev& F = c->asmb.fip;
    const size_t np = (size_t)F.npart;
    for (int level = 0; level + 1 < (int)S.level_ptr.size(); ++level) {
        const int c0 = S.level_ptr[level], n = S.level_ptr[level + 1] - c0;
        if (level == 0)
            hipLaunchKernelGGL(k_fip_reduce<true>, dim3((n + 3) / 4), dim3(256), 0, c->stream, c0, n, S.d_desc, S.d_items, F.d_terms, (size_t)c->pat.Nloc,
                               F.d_part, np);
        else
            hipLaunchKernelGGL(k_fip_reduce<false>, dim3((n + 3) / 4), dim3(256), 0, c->stream, c0, n, S.d_desc, S.d_items, F.d_part, np, F.d_part, np);
    }
    hipLaunchKernelGGL(k_fip_totals, dim3(1), dim3(64), 0, c->stream, S.max_id, S.d_result, F.d_part, np, F.d_out);
}

}  // namespace opmhip
