// gfx950 kernels of the passive tracers (opmhip_set_tracers ... opmhip_tracers_end_time_step): the phase volume and the storage cache, the
// scalar transport system of one phase batch, an exact scalar ILU0 in the context's ordering scheduled by level sets, and a BiCGStab
// that advances all tracers of the batch in lock step.
//
// Reference behaviour restated (file:line under the reference tree):
//   ebos/ecltracermodel.hh:158-179 (computeVolume_), :182-213 (computeFlux_), :216-337 (assembleTracerEquations_), :340-359
//   (updateStorageCache), :362-383 (advanceTracerFields); ebos/eclgenerictracermodel.cc:248-281 (linearSolve_, linearSolveBatchwise_);
//   ebos/eclfluxmodule.hh:212-357 (the volume flux: the value arithmetic of face_flux in assemble.hip);
//   bda/cusparseSolverBackend.cu:60-184 (the BiCGStab recurrence: Dune's BiCGSTABSolver is not in the tree, iteration counts UNVERIFIED).
//
// Mapping: ONE LANE PER ROW everywhere (plain wave64 kernels, 64 lanes per workgroup, no LDS, no atomics).  A row has seven entries and
// every kernel here is a stream over arrays that are read once, so there is nothing to share inside a workgroup; the row's sums run
// sequentially in the lane, in the order the host form states.  The per-cell vectors of a batch are interleaved [cell][tracer]: a
// neighbour gather fetches all tracers from one line, and a matrix or factor entry is read once for TR_CH tracers at a time (the
// accumulators live in registers; a batch of more than TR_CH tracers takes one pass per TR_CH).
// The library is built with -ffp-contract=off: the expression trees below are the ones tracers.py's HostTracers copies to get the same bits.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cfloat>
#include <chrono>

#include "fluid_device.hpp"

namespace opmhip {

constexpr int TR_CH = 8;     // tracers whose accumulators a lane holds at a time
constexpr int TR_WG = 64;
// per-tracer BiCGStab scalars on the device (double d_sc[TS_COUNT] per tracer of the batch)
enum { TS_RHO = 0, TS_RHOP, TS_ALPHA, TS_OMEGA, TS_BETA, TS_NORM, TS_NORM0, TS_DONE, TS_HALVES, TS_CONV, TS_COUNT = 16 };
enum { FIN_TR_INIT = 0, FIN_TR_RHO, FIN_TR_RHO_FIRST, FIN_TR_ALPHA, FIN_TR_OMEGA, FIN_TR_NORM };

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- the phase volume (computeVolume_, ecltracermodel.hh:158-179) --------------------------------------------------------------------
template <bool EXT>
__device__ __forceinline__ double tracer_volume(const double* __restrict__ iq, int N, int ph, int c) {
    const double phaseVolume = iq_at(iq, N, F_S + ph, c)[0] * iq_at(iq, N, F_B + ph, c)[0] * iq_at(iq, N, Lay<EXT>::F_PORO, c)[0];
    return phaseVolume > 1e-10 ? phaseVolume : 1e-10;   // "avoid singular matrix if no water is present"
}
// updateStorageCache (:340-359), one lane per cell
template <bool EXT>
__global__ __launch_bounds__(TR_WG) void k_tracer_volume(int Nb, int N, int ph, int nt, const double* __restrict__ iq, const double* __restrict__ c,
                                                         double* __restrict__ c0, double* __restrict__ s1) {
    const int p = blockIdx.x * TR_WG + threadIdx.x;
    if (p >= Nb) return;
    const double vol = tracer_volume<EXT>(iq, N, ph, p);
    for (int t = 0; t < nt; ++t) {
        const double ci = c[(size_t)p * nt + t];
        c0[(size_t)p * nt + t] = ci;
        s1[(size_t)p * nt + t] = vol * ci;
    }
}

// ---- the face (computeFlux_, :182-213) -----------------------------------------------------------------------------------------------
// f = A v b_up of one phase with `in` as the interior cell: the VALUE arithmetic of face_flux (assemble.hip) for that phase, statement by
// statement - gravity with the averaged density, THPRES, the upwind rule with its volume and global-index tie-breaks, the rock
// transmissibility multiplier of the extended record - and no derivatives.  up: `in` is upstream.  A face face_flux skips (no mobile
// phase on either side, |dp| within the threshold) carries f = 0.
struct TracerFace {
    double f;
    bool up;
};
template <bool EXT>
__device__ __forceinline__ TracerFace tracer_face(const double* __restrict__ iq, int N, int ph, int in, int ex, double trans, double faceArea,
                                                  double thpres, double zIn, double zEx, double Vin, double Vex, bool inLower) {
    const double mobIn = iq_at(iq, N, F_MOB + ph, in)[0], rhoIn = iq_at(iq, N, F_RHO + ph, in)[0], pIn = iq_at(iq, N, F_P + ph, in)[0],
                 bIn = iq_at(iq, N, F_B + ph, in)[0];
    const double mobEx = iq_at(iq, N, F_MOB + ph, ex)[0], rhoEx = iq_at(iq, N, F_RHO + ph, ex)[0], pEx = iq_at(iq, N, F_P + ph, ex)[0],
                 bEx = iq_at(iq, N, F_B + ph, ex)[0];
    double tmIn = 1.0, tmEx = 1.0;
    if (EXT) { tmIn = iq_at(iq, N, Lay<EXT>::F_TMULT, in)[0]; tmEx = iq_at(iq, N, Lay<EXT>::F_TMULT, ex)[0]; }
    if (mobIn <= 0.0 && mobEx <= 0.0) return TracerFace{0.0, false};
    const double distZ = zIn - zEx;
    const double rhoAvg = (rhoIn + rhoEx) / 2.0;
    const double pressureExterior = pEx + rhoAvg * (distZ * GRAVITY);
    double dp = pressureExterior - pIn;
    bool upIn;
    if (dp > 0.0) upIn = false;
    else if (dp < 0.0) upIn = true;
    else if (Vin > Vex) upIn = true;
    else if (Vin < Vex) upIn = false;
    else upIn = inLower;
    if (fabs(dp) > thpres) {
        if (dp < 0.0) dp = dp + thpres; else dp = dp - thpres;
    } else return TracerFace{0.0, false};
    double surf;
    if (upIn) {
        const double volumeFlux = dp * mobIn * tmIn * (-trans / faceArea);
        surf = bIn * volumeFlux;
    } else {
        const double volumeFlux = dp * (mobEx * tmEx * (-trans / faceArea));
        surf = bEx * volumeFlux;
    }
    return TracerFace{(0.0 + surf) * faceArea, upIn};
}

// ---- the system (assembleTracerEquations_, :216-291), one lane per row ------------------------------------------------------------------
// Row I: storage, then the faces in ascending natural column order (ford), each evaluated twice - with I as the interior cell for the
// residual and the diagonal, with J as the interior cell for the entry (I, J), which belongs to J's visit in the reference (:285-288).
// The two evaluations are not bitwise antisymmetric, so neither is derived from the other.
template <bool EXT>
__global__ __launch_bounds__(TR_WG) void k_tracer_system(int Nb, int N, int ph, int nt, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                         const int* __restrict__ diag, const int* __restrict__ ford, const int* __restrict__ fromOrder,
                                                         const double* __restrict__ iq, const double* __restrict__ trans, const double* __restrict__ area,
                                                         const double* __restrict__ thpres, const double* __restrict__ depth,
                                                         const double* __restrict__ volume, double dt, const double* __restrict__ c,
                                                         const double* __restrict__ s1, double* __restrict__ M, double* __restrict__ res) {
    const int I = blockIdx.x * TR_WG + threadIdx.x;
    if (I >= Nb) return;
    const double vol = tracer_volume<EXT>(iq, N, ph, I);
    const double V = volume[I], zI = depth[I];
    const int natI = fromOrder[I];
    const int kb = rowptr[I], ke = rowptr[I + 1];
    for (int t0 = 0; t0 < nt; t0 += TR_CH) {
        double acc[TR_CH];
#pragma unroll
        for (int u = 0; u < TR_CH; ++u)
            if (t0 + u < nt) acc[u] = (vol * c[(size_t)I * nt + t0 + u] - s1[(size_t)I * nt + t0 + u]) * V / dt;
        double dg = vol * V / dt;   // fVolume.derivative(0) * scvVolume / dt (:271)
        for (int q = kb; q < ke; ++q) {
            const int k = ford[q], J = col[k];
            if (J == I) continue;
            const double tr = trans[k], ar = area[k], th = thpres ? thpres[k] : 0.0;
            const double zJ = depth[J], VJ = volume[J];
            const bool lowI = natI < fromOrder[J];
            const TracerFace fI = tracer_face<EXT>(iq, N, ph, I, J, tr, ar, th, zI, zJ, V, VJ, lowI);
            const int up = fI.up ? I : J;
#pragma unroll
            for (int u = 0; u < TR_CH; ++u)
                if (t0 + u < nt) acc[u] = acc[u] + fI.f * c[(size_t)up * nt + t0 + u];
            if (fI.up) dg = dg + fI.f;
            if (t0 == 0) {
                const TracerFace fJ = tracer_face<EXT>(iq, N, ph, J, I, tr, ar, th, zJ, zI, VJ, V, !lowI);
                M[k] = fJ.up ? -fJ.f : 0.0;
            }
        }
        if (t0 == 0) M[diag[I]] = dg;
#pragma unroll
        for (int u = 0; u < TR_CH; ++u)
            if (t0 + u < nt) res[(size_t)I * nt + t0 + u] = acc[u];
    }
}
// The wells' terms (:293-336) behind it, one lane per DISTINCT connected cell, the cell's connections in list order (as k_aquifer_apply
// does): q > 0: r_t -= q c_inj[t]; q < 0: r_t -= q c_t and M_II -= q
__global__ __launch_bounds__(TR_WG) void k_tracer_wells(int nd, int ph, int nt, int nconn, TracerMembers mem, const int* __restrict__ cpos,
                                                        const int* __restrict__ cptr, const int* __restrict__ cconn, const double* __restrict__ rate,
                                                        const double* __restrict__ inj, const int* __restrict__ diag, const double* __restrict__ c,
                                                        double* __restrict__ M, double* __restrict__ res) {
    const int d = blockIdx.x * TR_WG + threadIdx.x;
    if (d >= nd) return;
    const int I = cpos[d];
    double dg = M[diag[I]];
    for (int k = cptr[d]; k < cptr[d + 1]; ++k) {
        const double q = rate[(size_t)3 * cconn[k] + ph];
        if (q < 0.0) dg = dg - q;
    }
    M[diag[I]] = dg;
    for (int t = 0; t < nt; ++t) {
        double r = res[(size_t)I * nt + t];
        const double ci = c[(size_t)I * nt + t];
        for (int k = cptr[d]; k < cptr[d + 1]; ++k) {
            const int i = cconn[k];
            const double q = rate[(size_t)3 * i + ph];
            if (q > 0.0) r = r - q * inj[(size_t)mem.g[t] * nconn + i];
            else if (q < 0.0) r = r - q * ci;
        }
        res[(size_t)I * nt + t] = r;
    }
}

// ---- scalar ILU0 in the context's ordering (SeqILU(M, 0, 1), eclgenerictracermodel.cc:256-258) ------------------------------------------
// One launch per level of the lower triangle (tracers_setup.hpp: tracer_levels), one lane per row: the row-wise (IKJ) elimination on the
// matrix's own pattern, the multipliers L_ij = a_ij * (1 / u_jj) left in the lower part, the inverse pivots in invd.  A pivot that is zero
// or not finite raises the flag and is replaced by 1: nothing that is not finite is stored because of it.
__global__ __launch_bounds__(TR_WG) void k_tracer_copy(int n, const double* __restrict__ a, double* __restrict__ b, int* __restrict__ flag) {
    const int i = blockIdx.x * TR_WG + threadIdx.x;
    if (i == 0) *flag = 0;   // the pivot flag of the factorisation that follows
    if (i < n) b[i] = a[i];
}
__global__ __launch_bounds__(TR_WG) void k_tracer_ilu_level(int nrows, const int* __restrict__ rows, const int* __restrict__ rowptr,
                                                            const int* __restrict__ col, const int* __restrict__ diag, double* __restrict__ LU,
                                                            double* __restrict__ invd, int* __restrict__ flag) {
    const int q = blockIdx.x * TR_WG + threadIdx.x;
    if (q >= nrows) return;
    const int i = rows[q];
    const int kd = diag[i], ke = rowptr[i + 1];
    for (int k = rowptr[i]; k < kd; ++k) {
        const int j = col[k];
        const double l = LU[k] * invd[j];
        LU[k] = l;
        int kk = k + 1;
        for (int m = diag[j] + 1; m < rowptr[j + 1]; ++m) {
            const int cj = col[m];
            while (kk < ke && col[kk] < cj) ++kk;
            if (kk < ke && col[kk] == cj) LU[kk] = LU[kk] - l * LU[m];
        }
    }
    double d = LU[kd];
    if (!(fabs(d) <= DBL_MAX) || d == 0.0) { *flag = 1; d = 1.0; LU[kd] = d; }
    invd[i] = 1.0 / d;
}
// y_i = d_i - sum_{j < i} L_ij y_j over the row's lower entries in ascending column order
__global__ __launch_bounds__(TR_WG) void k_tracer_lower(int nrows, const int* __restrict__ rows, int nt, const int* __restrict__ rowptr,
                                                        const int* __restrict__ col, const int* __restrict__ diag, const double* __restrict__ LU,
                                                        const double* __restrict__ d, double* __restrict__ y) {
    const int q = blockIdx.x * TR_WG + threadIdx.x;
    if (q >= nrows) return;
    const int i = rows[q];
    const int kb = rowptr[i], kd = diag[i];
    for (int t0 = 0; t0 < nt; t0 += TR_CH) {
        double acc[TR_CH];
#pragma unroll
        for (int u = 0; u < TR_CH; ++u)
            if (t0 + u < nt) acc[u] = d[(size_t)i * nt + t0 + u];
        for (int k = kb; k < kd; ++k) {
            const double l = LU[k];
            const size_t o = (size_t)col[k] * nt + t0;
#pragma unroll
            for (int u = 0; u < TR_CH; ++u)
                if (t0 + u < nt) acc[u] = acc[u] - l * y[o + u];
        }
#pragma unroll
        for (int u = 0; u < TR_CH; ++u)
            if (t0 + u < nt) y[(size_t)i * nt + t0 + u] = acc[u];
    }
}
// z_i = (y_i - sum_{j > i} U_ij z_j) * (1 / u_ii)
__global__ __launch_bounds__(TR_WG) void k_tracer_upper(int nrows, const int* __restrict__ rows, int nt, const int* __restrict__ rowptr,
                                                        const int* __restrict__ col, const int* __restrict__ diag, const double* __restrict__ LU,
                                                        const double* __restrict__ invd, const double* __restrict__ y, double* __restrict__ z) {
    const int q = blockIdx.x * TR_WG + threadIdx.x;
    if (q >= nrows) return;
    const int i = rows[q];
    const int kd = diag[i], ke = rowptr[i + 1];
    const double di = invd[i];
    for (int t0 = 0; t0 < nt; t0 += TR_CH) {
        double acc[TR_CH];
#pragma unroll
        for (int u = 0; u < TR_CH; ++u)
            if (t0 + u < nt) acc[u] = y[(size_t)i * nt + t0 + u];
        for (int k = kd + 1; k < ke; ++k) {
            const double a = LU[k];
            const size_t o = (size_t)col[k] * nt + t0;
#pragma unroll
            for (int u = 0; u < TR_CH; ++u)
                if (t0 + u < nt) acc[u] = acc[u] - a * z[o + u];
        }
#pragma unroll
        for (int u = 0; u < TR_CH; ++u)
            if (t0 + u < nt) z[(size_t)i * nt + t0 + u] = acc[u] * di;
    }
}
// y = M x, the row's entries in ascending (internal) column order
__global__ __launch_bounds__(TR_WG) void k_tracer_spmv(int Nb, int nt, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                       const double* __restrict__ M, const double* __restrict__ x, double* __restrict__ y) {
    const int i = blockIdx.x * TR_WG + threadIdx.x;
    if (i >= Nb) return;
    const int kb = rowptr[i], ke = rowptr[i + 1];
    for (int t0 = 0; t0 < nt; t0 += TR_CH) {
        double acc[TR_CH];
#pragma unroll
        for (int u = 0; u < TR_CH; ++u) acc[u] = 0.0;
        for (int k = kb; k < ke; ++k) {
            const double a = M[k];
            const size_t o = (size_t)col[k] * nt + t0;
#pragma unroll
            for (int u = 0; u < TR_CH; ++u)
                if (t0 + u < nt) acc[u] = acc[u] + a * x[o + u];
        }
#pragma unroll
        for (int u = 0; u < TR_CH; ++u)
            if (t0 + u < nt) y[(size_t)i * nt + t0 + u] = acc[u];
    }
}

// ---- reductions: fixed-order two-stage sums, no floating-point atomics ------------------------------------------------------------------
// Stage 1: workgroup b sums the cells [b cells, (b + 1) cells) of up to two scalar products per tracer.  A lane walks the workgroup's
// flat range with a stride that is a multiple of nt, so it stays with one tracer; the lanes of a tracer are then added in lane order.
constexpr int TR_RED = 256;
__global__ __launch_bounds__(TR_RED) void k_tracer_dot(int Nb, int nt, int cells, int nblk, const double* __restrict__ a0, const double* __restrict__ b0,
                                                       const double* __restrict__ a1, const double* __restrict__ b1, double* __restrict__ part) {
    __shared__ double s0[TR_RED], s1[TR_RED];
    const int tid = threadIdx.x;
    const int W = TR_RED - TR_RED % nt;
    const int c0 = blockIdx.x * cells, c1 = min(Nb, c0 + cells);
    double x0 = 0.0, x1 = 0.0;
    if (tid < W) {
        const size_t e1 = (size_t)c1 * nt;
        for (size_t e = (size_t)c0 * nt + tid; e < e1; e += W) {
            x0 = x0 + a0[e] * b0[e];
            if (a1) x1 = x1 + a1[e] * b1[e];
        }
    }
    s0[tid] = x0; s1[tid] = x1;
    __syncthreads();
    if (tid < nt) {
        double y0 = 0.0, y1 = 0.0;
        for (int j = tid; j < W; j += nt) { y0 = y0 + s0[j]; y1 = y1 + s1[j]; }
        part[(size_t)blockIdx.x * nt + tid] = y0;
        part[((size_t)nblk + blockIdx.x) * nt + tid] = y1;
    }
}
// Stage 2 and the scalar stage: one workgroup, lane t sums tracer t's partial sums in workgroup order and forms the scalar the mode
// names.  A tracer that has met its tolerance is frozen: its scalars are left alone.  After a norm the number of tracers done goes to
// the pinned record and, system-scope release, the record's sequence number, which the host polls.
__global__ __launch_bounds__(TR_WG) void k_tracer_finalize(int mode, int nt, int nblk, const double* __restrict__ part, double* __restrict__ sc, double tol,
                                                           double* __restrict__ rec, double seq) {
    __shared__ int sdone[TR_WG];
    const int t = threadIdx.x;
    int done = 1;
    if (t < nt) {
        double* S = sc + (size_t)t * TS_COUNT;
        if (mode == FIN_TR_INIT) S[TS_DONE] = 0.0;
        if (S[TS_DONE] == 0.0) {
            double a = 0.0, b = 0.0;
            for (int q = 0; q < nblk; ++q) { a = a + part[(size_t)q * nt + t]; b = b + part[((size_t)nblk + q) * nt + t]; }
            if (mode == FIN_TR_INIT) {
                const double n0 = sqrt(a);
                S[TS_NORM0] = n0; S[TS_NORM] = n0; S[TS_RHO] = 1.0; S[TS_RHOP] = 1.0; S[TS_ALPHA] = 0.0; S[TS_OMEGA] = 0.0; S[TS_BETA] = 0.0;
                S[TS_HALVES] = 0.0;
                const double z = (n0 == 0.0) ? 1.0 : 0.0;   // a zero right-hand side: x = 0 is the solution
                S[TS_DONE] = z; S[TS_CONV] = z;
            } else if (mode == FIN_TR_RHO || mode == FIN_TR_RHO_FIRST) {
                const double rhop = S[TS_RHO];
                S[TS_RHOP] = rhop; S[TS_RHO] = a;
                if (mode == FIN_TR_RHO) S[TS_BETA] = (a / rhop) * (S[TS_ALPHA] / S[TS_OMEGA]);
            } else if (mode == FIN_TR_ALPHA) {
                S[TS_ALPHA] = S[TS_RHO] / a;
            } else if (mode == FIN_TR_OMEGA) {
                S[TS_OMEGA] = a / b;
            } else {
                const double norm = sqrt(a);
                S[TS_NORM] = norm;
                S[TS_HALVES] = S[TS_HALVES] + 1.0;
                if (norm < tol * S[TS_NORM0]) { S[TS_DONE] = 1.0; S[TS_CONV] = 1.0; }
            }
        }
        done = S[TS_DONE] != 0.0 ? 1 : 0;
    }
    if (!rec) return;
    sdone[t] = done;
    __syncthreads();
    if (t == 0) {
        int n = 0;
        for (int u = 0; u < nt; ++u) n += sdone[u];
        rec[0] = (double)n;
        __hip_atomic_store(&rec[3], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // the host polls this one
    }
}

// ---- vector updates: one lane per element of the interleaved vectors; a frozen tracer's elements are left alone --------------------------
__global__ __launch_bounds__(256) void k_tracer_init(size_t n, const double* __restrict__ b, double* __restrict__ x, double* __restrict__ r,
                                                     double* __restrict__ rw, double* __restrict__ p) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const double v = b[e];   // x = 0: r = b - M x = b
    x[e] = 0.0; r[e] = v; rw[e] = v; p[e] = v;
}
// p = beta (p - omega v) + r (bda/cusparseSolverBackend.cu:95-99)
__global__ __launch_bounds__(256) void k_tracer_pupdate(size_t n, int nt, const double* __restrict__ sc, const double* __restrict__ v,
                                                        const double* __restrict__ r, double* __restrict__ p) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const double* S = sc + (e % nt) * TS_COUNT;
    if (S[TS_DONE] != 0.0) return;
    const double nomega = -S[TS_OMEGA];
    p[e] = S[TS_BETA] * (p[e] + nomega * v[e]) + r[e];
}
// r -= alpha v, x += alpha pw (:121-124)
__global__ __launch_bounds__(256) void k_tracer_update1(size_t n, int nt, const double* __restrict__ sc, const double* __restrict__ v,
                                                        const double* __restrict__ pw, double* __restrict__ r, double* __restrict__ x) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const double* S = sc + (e % nt) * TS_COUNT;
    if (S[TS_DONE] != 0.0) return;
    const double alpha = S[TS_ALPHA], nalpha = -alpha;
    r[e] = r[e] + nalpha * v[e];
    x[e] = x[e] + alpha * pw[e];
}
// x += omega s, r -= omega t (:153-156)
__global__ __launch_bounds__(256) void k_tracer_update2(size_t n, int nt, const double* __restrict__ sc, const double* __restrict__ s,
                                                        const double* __restrict__ t, double* __restrict__ r, double* __restrict__ x) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const double* S = sc + (e % nt) * TS_COUNT;
    if (S[TS_DONE] != 0.0) return;
    const double omega = S[TS_OMEGA], nomega = -omega;
    x[e] = x[e] + omega * s[e];
    r[e] = r[e] + nomega * t[e];
}
// concentration_ -= dx (ecltracermodel.hh:379-380)
__global__ __launch_bounds__(256) void k_tracer_apply(size_t n, const double* __restrict__ x, double* __restrict__ c) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) c[e] = c[e] - x[e];
}

// ============================== launchers =================================================================================================
void launch_tracer_begin(opmhip_ctx* c, int phase) {
    const TracersDev& T = c->asmb.tr;
    const TracerBatchDev& B = T.b[phase];
    const int Nb = c->pat.Nb;
    if (B.nt == 0 || Nb == 0) return;
    if (c->asmb.ext)
        hipLaunchKernelGGL(k_tracer_volume<true>, dim3(cdiv(Nb, TR_WG)), dim3(TR_WG), 0, c->stream, Nb, c->pat.Nloc, phase, B.nt, c->asmb.d_iq, B.d_c, B.d_c0, B.d_s1);
    else
        hipLaunchKernelGGL(k_tracer_volume<false>, dim3(cdiv(Nb, TR_WG)), dim3(TR_WG), 0, c->stream, Nb, c->pat.Nloc, phase, B.nt, c->asmb.d_iq, B.d_c, B.d_c0, B.d_s1);
}
void launch_tracer_system(opmhip_ctx* c, int phase, double dt) {
    const TracersDev& T = c->asmb.tr;
    const TracerBatchDev& B = T.b[phase];
    const Pattern& P = c->pat;
    const AsmDev& A = c->asmb;
    if (B.nt == 0 || P.Nb == 0) return;
    if (A.ext)
        hipLaunchKernelGGL(k_tracer_system<true>, dim3(cdiv(P.Nb, TR_WG)), dim3(TR_WG), 0, c->stream, P.Nb, P.Nloc, phase, B.nt, P.d_rowptr, P.d_col, P.d_diag,
                           T.d_ford, P.d_fromOrder, A.d_iq, A.d_trans, A.d_area, A.d_thpres, A.d_depth, A.d_volume, dt, B.d_c, B.d_s1, T.d_M, T.d_res);
    else
        hipLaunchKernelGGL(k_tracer_system<false>, dim3(cdiv(P.Nb, TR_WG)), dim3(TR_WG), 0, c->stream, P.Nb, P.Nloc, phase, B.nt, P.d_rowptr, P.d_col, P.d_diag,
                           T.d_ford, P.d_fromOrder, A.d_iq, A.d_trans, A.d_area, A.d_thpres, A.d_depth, A.d_volume, dt, B.d_c, B.d_s1, T.d_M, T.d_res);
    if (T.nd > 0)
        hipLaunchKernelGGL(k_tracer_wells, dim3(cdiv(T.nd, TR_WG)), dim3(TR_WG), 0, c->stream, T.nd, phase, B.nt, T.nconn, B.members, T.d_cpos, T.d_cptr, T.d_cconn,
                           T.d_rate, T.d_inj, P.d_diag, B.d_c, T.d_M, T.d_res);
}

namespace {
// the host's side of the pinned record: spin on the sequence number (as the block solver's wait_half does)
int tracer_wait(opmhip_ctx* c, double want, int* ndone) {
    const volatile double* rec = c->asmb.tr.h_rec;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned long spin = 1;; ++spin) {
        if (rec[3] == want) break;
        if ((spin & 0xFFFFu) == 0) {   // every ~65k polls: is the stream still alive?
            const hipError_t e = hipStreamQuery(c->stream);
            if (e == hipSuccess) {
                if (rec[3] == want) break;
                return fail(c, OPMHIP_DEVICE_ERROR, "tracers: the stream drained without the stopping-rule record");
            }
            if (e != hipErrorNotReady) return fail(c, OPMHIP_DEVICE_ERROR, "tracers: %s", hipGetErrorString(e));
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120))
                return fail(c, OPMHIP_DEVICE_ERROR, "tracers: no stopping-rule record after 120 s");
        }
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    *ndone = (int)rec[0];
    return OPMHIP_SUCCESS;
}
struct TracerSolve {
    opmhip_ctx* c;
    TracersDev& T;
    const Pattern& P;
    int nt;
    size_t n;
    int nlev() const { return (int)T.lvptr.size() - 1; }
    void dot(const double* a0, const double* b0, const double* a1, const double* b1) {
        hipLaunchKernelGGL(k_tracer_dot, dim3(T.nblk), dim3(TR_RED), 0, c->stream, P.Nb, nt, T.cellsPerBlock, T.nblk, a0, b0, a1, b1, T.d_part);
        T.launches++;
    }
    double finalize(int mode, bool record) {
        const double seq = record ? (T.seq += 1.0) : 0.0;
        hipLaunchKernelGGL(k_tracer_finalize, dim3(1), dim3(TR_WG), 0, c->stream, mode, nt, T.nblk, T.d_part, T.d_sc, T.tol, record ? T.d_rec : nullptr, seq);
        T.launches++;
        return seq;
    }
    void factor() {
        hipLaunchKernelGGL(k_tracer_copy, dim3(cdiv(P.nnzb, TR_WG)), dim3(TR_WG), 0, c->stream, P.nnzb, T.d_M, T.d_LU, T.d_flag);
        for (int l = 0; l < nlev(); ++l) {
            const int nr = T.lvptr[l + 1] - T.lvptr[l];
            hipLaunchKernelGGL(k_tracer_ilu_level, dim3(cdiv(nr, TR_WG)), dim3(TR_WG), 0, c->stream, nr, T.d_lvrows + T.lvptr[l], P.d_rowptr, P.d_col, P.d_diag,
                               T.d_LU, T.d_invd, T.d_flag);
        }
    }
    void apply(const double* d, double* z) {   // z = U^-1 L^-1 d, through d_y
        for (int l = 0; l < nlev(); ++l) {
            const int nr = T.lvptr[l + 1] - T.lvptr[l];
            hipLaunchKernelGGL(k_tracer_lower, dim3(cdiv(nr, TR_WG)), dim3(TR_WG), 0, c->stream, nr, T.d_lvrows + T.lvptr[l], nt, P.d_rowptr, P.d_col, P.d_diag,
                               T.d_LU, d, T.d_y);
        }
        for (int l = nlev() - 1; l >= 0; --l) {
            const int nr = T.lvptr[l + 1] - T.lvptr[l];
            hipLaunchKernelGGL(k_tracer_upper, dim3(cdiv(nr, TR_WG)), dim3(TR_WG), 0, c->stream, nr, T.d_lvrows + T.lvptr[l], nt, P.d_rowptr, P.d_col, P.d_diag,
                               T.d_LU, T.d_invd, T.d_y, z);
        }
        T.launches += 2 * nlev();
    }
    void spmv(const double* x, double* y) {
        hipLaunchKernelGGL(k_tracer_spmv, dim3(cdiv(P.Nb, TR_WG)), dim3(TR_WG), 0, c->stream, P.Nb, nt, P.d_rowptr, P.d_col, T.d_M, x, y);
        T.launches++;
    }
};
}  // namespace

// linearSolveBatchwise_ for one batch: M dx_t = r_t from x = 0 for all its tracers in lock step, then c_t -= dx_t.  The matrix and the
// residuals are in d_M / d_res (launch_tracer_system).  The host waits for the record of every half iteration before it enqueues the next.
int tracer_solve_batch(opmhip_ctx* c, int phase, opmhip_tracer_result* out, bool* pivot_failed) {
    TracersDev& T = c->asmb.tr;
    TracerBatchDev& B = T.b[phase];
    const Pattern& P = c->pat;
    *pivot_failed = false;
    if (B.nt == 0 || P.Nb == 0) return OPMHIP_SUCCESS;
    const int nt = B.nt;
    const size_t n = (size_t)P.Nb * nt;
    const int nb = (int)((n + 255) / 256);
    TracerSolve S{c, T, P, nt, n};
    int rc, ndone = 0;
    OPMHIP_HIP(c, hipEventRecord(T.ev[1], c->stream));
    S.factor();
    OPMHIP_HIP(c, hipEventRecord(T.ev[2], c->stream));
    hipLaunchKernelGGL(k_tracer_init, dim3(nb), dim3(256), 0, c->stream, n, T.d_res, T.d_x, T.d_r, T.d_rw, T.d_p);
    S.dot(T.d_r, T.d_r, nullptr, nullptr);
    double want = S.finalize(FIN_TR_INIT, true);
    OPMHIP_HIP(c, hipGetLastError());
    if ((rc = tracer_wait(c, want, &ndone))) return rc;
    for (int it = 1; it <= T.maxit && ndone < nt; ++it) {
        // first half (bda/cusparseSolverBackend.cu:91-129)
        S.dot(T.d_rw, T.d_r, nullptr, nullptr);
        S.finalize(it > 1 ? FIN_TR_RHO : FIN_TR_RHO_FIRST, false);
        if (it > 1) { hipLaunchKernelGGL(k_tracer_pupdate, dim3(nb), dim3(256), 0, c->stream, n, nt, T.d_sc, T.d_v, T.d_r, T.d_p); T.launches++; }
        S.apply(T.d_p, T.d_pw);
        S.spmv(T.d_pw, T.d_v);
        S.dot(T.d_rw, T.d_v, nullptr, nullptr);
        S.finalize(FIN_TR_ALPHA, false);
        hipLaunchKernelGGL(k_tracer_update1, dim3(nb), dim3(256), 0, c->stream, n, nt, T.d_sc, T.d_v, T.d_pw, T.d_r, T.d_x);
        T.launches++;
        S.dot(T.d_r, T.d_r, nullptr, nullptr);
        want = S.finalize(FIN_TR_NORM, true);
        OPMHIP_HIP(c, hipGetLastError());
        if ((rc = tracer_wait(c, want, &ndone))) return rc;
        if (ndone >= nt) break;
        // second half (:131-163)
        S.apply(T.d_r, T.d_s);
        S.spmv(T.d_s, T.d_t);
        S.dot(T.d_t, T.d_r, T.d_t, T.d_t);
        S.finalize(FIN_TR_OMEGA, false);
        hipLaunchKernelGGL(k_tracer_update2, dim3(nb), dim3(256), 0, c->stream, n, nt, T.d_sc, T.d_s, T.d_t, T.d_r, T.d_x);
        S.dot(T.d_r, T.d_r, nullptr, nullptr);
        want = S.finalize(FIN_TR_NORM, true);
        T.launches++;
        OPMHIP_HIP(c, hipGetLastError());
        if ((rc = tracer_wait(c, want, &ndone))) return rc;
    }
    hipLaunchKernelGGL(k_tracer_apply, dim3(nb), dim3(256), 0, c->stream, n, T.d_x, B.d_c);
    OPMHIP_HIP(c, hipEventRecord(T.ev[3], c->stream));
    OPMHIP_HIP(c, hipGetLastError());
    // the per-tracer outcome and the pivot flag: one small read-back per batch and time step
    std::vector<double> sc((size_t)nt * TS_COUNT);
    int flag = 0;
    OPMHIP_HIP(c, hipMemcpyAsync(sc.data(), T.d_sc, sc.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    OPMHIP_HIP(c, hipMemcpyAsync(&flag, T.d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
    *pivot_failed = flag != 0;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, T.ev[0], T.ev[1]) == hipSuccess) T.ms[0] += ms;
    if (hipEventElapsedTime(&ms, T.ev[1], T.ev[2]) == hipSuccess) T.ms[1] += ms;
    if (hipEventElapsedTime(&ms, T.ev[2], T.ev[3]) == hipSuccess) T.ms[2] += ms;
    if (out)
        for (int t = 0; t < nt; ++t) {
            const double* s = &sc[(size_t)t * TS_COUNT];
            opmhip_tracer_result& R = out[t];
            R.converged = (s[TS_CONV] != 0.0 && flag == 0) ? 1 : 0;
            R.iterations = s[TS_CONV] != 0.0 ? 0.5 * s[TS_HALVES] : (double)T.maxit;   // min(it, maxit) (bda/cusparseSolverBackend.cu:172)
            R.reduction = s[TS_NORM0] > 0.0 ? s[TS_NORM] / s[TS_NORM0] : 0.0;
        }
    return OPMHIP_SUCCESS;
}

}  // namespace opmhip
