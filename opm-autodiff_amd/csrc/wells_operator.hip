// gfx950 kernels and launchers of the well operator y -= C^T (D^-1 (B x)): the standard wells of a solve's list (opmhip_wells), the
// device-resident multisegment wells in their dense and tree forms (opmhip_set_ms_wells), the host-callback round trip, and the wells
// added to the matrix.  solver.hip's launch_spmv calls in here through internal.hpp; nothing here uses the solver's tiles or schedules.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "device_blocks.hpp"
#include "internal.hpp"

namespace opmhip {

// ============================== standard wells ===========================================================
// y -= C^T (D^-1 (B x)) per well (bda/WellContributions.cu:36-126); one wavefront per well, any number of
// perforations (the CUDA kernel's 32-lane masks assume <= 2 blocks per warp pass, :82).
// (B x)_w added to (SUB: subtracted from) s on lanes 0..3, one well equation each, in the order of the CPU's per-perforation loop
// (wells/StandardWell_impl.hpp:1254-1275).  Walking the perforations one by one on four lanes costs a round trip to memory per
// perforation (100 completions: ~50 us per application, twice per BiCGStab iteration); here every lane forms the twelve products of one
// perforation - 64 perforations' loads in flight together - and lanes 0..3 then add the products up out of LDS in that same order: the
// same products, the same additions, the same bits.
template <bool SUB>
__device__ __forceinline__ double well_Bx(double s, int pb, int pe, const int* __restrict__ Bcols, const double* __restrict__ B,
                                          const double* __restrict__ x, double xs, int lane, double* prod /* LDS, 64 x 12 */) {
    for (int p0 = pb; p0 < pe; p0 += 64) {
        const int p = p0 + lane;
        if (p < pe) {
            const double* xb = &x[(size_t)Bcols[p] * 3];
            const double x0 = xs * xb[0], x1 = xs * xb[1], x2 = xs * xb[2];
            const double* Bp = &B[(size_t)p * 12];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                prod[lane * 12 + q * 3] = Bp[q * 3] * x0;
                prod[lane * 12 + q * 3 + 1] = Bp[q * 3 + 1] * x1;
                prod[lane * 12 + q * 3 + 2] = Bp[q * 3 + 2] * x2;
            }
        }
        __syncthreads();
        if (lane < 4) {
            const int m = pe - p0 < 64 ? pe - p0 : 64;
            for (int j = 0; j < m; ++j) {
                const double* pj = &prod[j * 12 + lane * 3];
                if (SUB) { s -= pj[0]; s -= pj[1]; s -= pj[2]; }
                else { s += pj[0]; s += pj[1]; s += pj[2]; }
            }
        }
        __syncthreads();
    }
    return s;
}
__global__ __launch_bounds__(64) void k_wells_apply(const int* __restrict__ vp, const int* __restrict__ Ccols,
                                                    const int* __restrict__ Bcols, const double* __restrict__ C,
                                                    const double* __restrict__ D, const double* __restrict__ B,
                                                    const double* __restrict__ x, double* __restrict__ y, double xs) {
    __shared__ double z1[4], z2[4], prod[64 * 12];
    const int w = blockIdx.x, lane = threadIdx.x;
    const int pb = vp[w], pe = vp[w + 1];
    // z1 = B x : lanes 0..3 own one well equation each
    const double bx = well_Bx<false>(0.0, pb, pe, Bcols, B, x, xs, lane, prod);
    if (lane < 4) z1[lane] = bx;
    __syncthreads();
    if (lane < 4) {
        double s = 0.0;
        for (int q = 0; q < 4; ++q) s += D[(size_t)w * 16 + lane * 4 + q] * z1[q];
        z2[lane] = s;
    }
    __syncthreads();
    for (int e = pb * 3 + lane; e < pe * 3; e += 64) {
        const int p = e / 3, c = e % 3;
        double s = 0.0;
        for (int j = 0; j < 4; ++j) s += C[(size_t)p * 12 + j * 3 + c] * z2[j];
        // wells do not normally share a cell; if two do, their workgroups meet here: add atomically (one add per
        // well and entry - the same bits as a plain update whenever the cell has a single well)
        atomicAdd(&y[(size_t)Ccols[p] * 3 + c], -s);
    }
}

// this rank's part of B x of every well, 4 doubles per well, for the sum over the ranks (distributed wells); the sums of k_wells_apply
__global__ __launch_bounds__(64) void k_wells_bx(const int* __restrict__ vp, const int* __restrict__ Bcols, const double* __restrict__ B,
                                                 const double* __restrict__ x, double xs, double* __restrict__ bx) {
    __shared__ double prod[64 * 12];
    const int w = blockIdx.x, lane = threadIdx.x;
    const double s = well_Bx<false>(0.0, vp[w], vp[w + 1], Bcols, B, x, xs, lane, prod);
    if (lane < 4) bx[(size_t)w * 4 + lane] = s;
}

// r -= C^T (D^-1 resWell) (StandardWell::apply(BVector& r), wells/StandardWell_impl.hpp:1283-1296) and
// xw = D^-1 (resWell - B x) (recoverSolutionWell, :1298-1311); one wavefront per well, sums in the CPU's order
__global__ __launch_bounds__(64) void k_wells_residual(const int* __restrict__ vp, const int* __restrict__ Ccols,
                                                       const double* __restrict__ C, const double* __restrict__ D,
                                                       const double* __restrict__ resWell, double* __restrict__ r) {
    __shared__ double z2[4];
    const int w = blockIdx.x, lane = threadIdx.x;
    const int pb = vp[w], pe = vp[w + 1];
    if (lane < 4) {
        double s = 0.0;
        for (int q = 0; q < 4; ++q) s += D[(size_t)w * 16 + lane * 4 + q] * resWell[(size_t)w * 4 + q];
        z2[lane] = s;
    }
    __syncthreads();
    for (int e = pb * 3 + lane; e < pe * 3; e += 64) {
        const int p = e / 3, c = e % 3;
        double s = 0.0;
        for (int j = 0; j < 4; ++j) s += C[(size_t)p * 12 + j * 3 + c] * z2[j];
        atomicAdd(&r[(size_t)Ccols[p] * 3 + c], -s);  // see k_wells_apply
    }
}
__global__ __launch_bounds__(64) void k_wells_recover(const int* __restrict__ vp, const int* __restrict__ Bcols,
                                                      const double* __restrict__ B, const double* __restrict__ D,
                                                      const double* __restrict__ resWell, const double* __restrict__ x,
                                                      const double* __restrict__ bxAll, double* __restrict__ xw) {
    __shared__ double z1[4];
    __shared__ double prod[64 * 12];
    const int w = blockIdx.x, lane = threadIdx.x;
    const int pb = vp[w], pe = vp[w + 1];
    double s = lane < 4 ? resWell[(size_t)w * 4 + lane] : 0.0;   // resWell -= B x, perforation by perforation (BCRSMatrix::mmv)
    if (bxAll) { if (lane < 4) s -= bxAll[(size_t)w * 4 + lane]; }   // a well shared by several ranks: the product summed over them, subtracted as a whole
    else s = well_Bx<true>(s, pb, pe, Bcols, B, x, 1.0, lane, prod);
    if (lane < 4) z1[lane] = s;
    __syncthreads();
    if (lane < 4) {
        double s = 0.0;
        for (int q = 0; q < 4; ++q) s += D[(size_t)w * 16 + lane * 4 + q] * z1[q];
        xw[(size_t)w * 4 + lane] = s;
    }
}

// ---- multisegment wells on the device (opmhip_set_ms_wells) ----
// D -> D^-1, one workgroup per well: D is scattered from its CSC form into the well's dense M x M array (column-major, M = 4 Mb <= MSW_MAX_M),
// eliminated in place by Gauss-Jordan steps with partial pivoting - the pivot of step k is the largest entry of column k in rows k .. M - 1,
// the smaller row number where two are equal - and the columns are put back in the reverse order of the row exchanges, which leaves the
// explicit inverse.  Per step: column k to LDS (the multipliers), the pivot search by the first wavefront, the pivot row scaled to LDS while
// the old row k moves to its place, then every entry's update - wavefronts over the columns, lanes down a column.  A zero (or non-finite)
// pivot ends the well's elimination: flag[well] = 1 + k, read by the host where it synchronises next; 0 otherwise.
constexpr int MSW_MAX_M = OPMHIP_MS_WELLS_MAX_M;
constexpr int MSW_FACTOR_THREADS = 512, MSW_APPLY_THREADS = 1024;
static_assert(MSW_MAX_M % 64 == 0 && MSW_MAX_M <= MSW_APPLY_THREADS, "k_ms_wells_apply: one thread per well equation and part of the columns");
__global__ __launch_bounds__(MSW_FACTOR_THREADS) void k_ms_wells_factor(const MsWellDesc* __restrict__ desc, const int* __restrict__ Dcolp,
                                                                        const int* __restrict__ Drows, const double* __restrict__ Dvals,
                                                                        double* __restrict__ inv, int* __restrict__ flag) {
    __shared__ double col[MSW_MAX_M], rs[MSW_MAX_M];
    __shared__ int piv[MSW_MAX_M];
    __shared__ int s_p;
    const MsWellDesc d = desc[blockIdx.x];
    const int M = 4 * d.Mb, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    constexpr int T = MSW_FACTOR_THREADS, WAVES = MSW_FACTOR_THREADS / 64;
    double* W = inv + d.inv0;
    for (int e = t; e < M * M; e += T) W[e] = 0.0;
    __syncthreads();
    for (int c = t; c < M; c += T) {   // one thread per column: entries that name the same place are added in their order
        const int* cp = Dcolp + d.dcol0;
        for (int k = cp[c]; k < cp[c + 1]; ++k) W[c * M + Drows[d.dnz0 + k]] += Dvals[d.dnz0 + k];
    }
    __syncthreads();
    for (int k = 0; k < M; ++k) {
        for (int i = t; i < M; i += T) col[i] = W[k * M + i];
        __syncthreads();
        if (wave == 0) {
            double best = -1.0;
            int bi = M;
            for (int i = k + lane; i < M; i += 64) {
                const double a = fabs(col[i]);
                if (a > best) { best = a; bi = i; }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const double ob = __shfl_xor(best, off);
                const int oi = __shfl_xor(bi, off);
                if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            if (lane == 0) s_p = (best > 0.0 && best <= 1.7976931348623157e308) ? bi : -1;
        }
        __syncthreads();
        const int p = s_p;
        if (p < 0) {   // (the same for every thread)
            if (t == 0) flag[d.well] = k + 1;
            return;
        }
        const double pv = col[p];
        for (int j = t; j < M; j += T) {
            const double a = W[j * M + p];
            rs[j] = (j == k) ? 1.0 / pv : a / pv;
            if (p != k) W[j * M + p] = W[j * M + k];
        }
        if (t == 0) piv[k] = p;
        __syncthreads();
        const double rk = rs[k];
        for (int j = wave; j < M; j += WAVES) {
            const double rj = rs[j];
            for (int i = lane; i < M; i += 64) {
                double* w = W + j * M + i;
                if (i == k) { *w = rj; continue; }
                const double f = (i == p) ? col[k] : col[i];   // (the row that stands at p now is the old row k)
                *w = (j == k) ? -(f * rk) : *w - f * rj;
            }
        }
        __syncthreads();
    }
    for (int k = M - 1; k >= 0; --k) {   // thread i touches row i alone: no barrier between the exchanges
        const int p = piv[k];
        if (p == k) continue;
        for (int i = t; i < M; i += T) {
            const double a = W[k * M + i];
            W[k * M + i] = W[p * M + i];
            W[p * M + i] = a;
        }
    }
    if (t == 0) flag[d.well] = 0;
}
// y -= C^T (D^-1 (B (xs x))) for the wells of the list, one workgroup per well, z1 and z2 in LDS:
// z1 = B (xs x): per segment row its blocks in ascending order, each block's sum over k formed first (MultisegmentWellContribution.cpp:78-90);
// z2 = D^-1 z1: thread i forms row i's sum over one part of the columns (the parts: MSW_APPLY_THREADS / (M rounded up to 64) equal ranges,
//      so that a well of any size keeps every wavefront loading), the parts are added in their order;
// y[cell] -= C^T z2 per block (:97-108).  ATOMIC: a cell is shared between two blocks of the list - their updates meet: atomic adds.
template <bool ATOMIC>
__global__ __launch_bounds__(MSW_APPLY_THREADS) void k_ms_wells_apply(const MsWellDesc* __restrict__ desc, const int* __restrict__ Brows,
                                                                      const int* __restrict__ cell, const int* __restrict__ blkrow,
                                                                      const double* __restrict__ B, const double* __restrict__ C,
                                                                      const double* __restrict__ inv, const double* __restrict__ x,
                                                                      double* __restrict__ y, double xs) {
    __shared__ double z1[MSW_MAX_M], z2[MSW_MAX_M], part[MSW_APPLY_THREADS];
    const MsWellDesc d = desc[blockIdx.x];
    const int M = 4 * d.Mb, t = threadIdx.x;
    if (t < M) {
        const int row = t >> 2, j = t & 3;
        const int* br = Brows + d.seg0;
        double z = 0.0;
        for (int blk = d.blk0 + br[row]; blk < d.blk0 + br[row + 1]; ++blk) {
            const double* xb = x + (size_t)cell[blk] * 3;
            double temp = 0.0;
            for (int k = 0; k < 3; ++k) temp += B[(size_t)blk * 12 + j * 3 + k] * (xs * xb[k]);
            z += temp;
        }
        z1[t] = z;
    }
    __syncthreads();
    const int M64 = (M + 63) & ~63, nsplit = MSW_APPLY_THREADS / M64, chunk = (M + nsplit - 1) / nsplit;
    const int sp = t / M64, i = t - sp * M64;
    if (sp < nsplit && i < M) {
        const double* W = inv + d.inv0 + i;
        const int j0 = sp * chunk, j1 = min(M, j0 + chunk);
        double s = 0.0;
        for (int j = j0; j < j1; ++j) s += W[j * M] * z1[j];
        part[sp * M64 + i] = s;
    }
    __syncthreads();
    if (t < M) {
        double s = part[t];
        for (int q = 1; q < nsplit; ++q) s += part[q * M64 + t];
        z2[t] = s;
    }
    __syncthreads();
    for (int e = t; e < d.nblk * 3; e += MSW_APPLY_THREADS) {
        const int blk = d.blk0 + e / 3, j = e % 3;
        const double* zz = z2 + blkrow[blk] * 4;
        double temp = 0.0;
        for (int k = 0; k < 4; ++k) temp += C[(size_t)blk * 12 + j + k * 3] * zz[k];
        double* yp = y + (size_t)cell[blk] * 3 + j;
        if (ATOMIC) atomicAdd(yp, -temp);
        else *yp -= temp;
    }
}

// ---- the tree form of the same list (opmhip_set_ms_wells_form; ms_wells_setup.hpp; mswells.py tree_solve states the arithmetic) ----
// D is block-sparse over the segment tree: 4 x 4 blocks on the diagonal and between a segment i and its parent p.  Eliminating the leaves
// first leaves no fill: per segment S_i = D_ii - sum_c E_c D_ci over the children c of i, E_i = D_pi S_i^-1.  One workgroup per well, one
// lane per segment of a level, levels separated by barriers; every sum in a stated order (the children ascending, inside a block
// product k ascending from 0.0), no floating-point atomics.  The blocks live in global memory, 48 doubles per segment:
// S_i^-1 | E_i | D_ip.  Pivoting stays INSIDE a segment's block (invert4_stated): a block without a non-zero finite pivot sets
// flag[well] = 1 + the lowest such segment (an integer minimum in LDS: the same whatever the lanes' order).
constexpr int MSW_TREE_THREADS = 256;
constexpr int MSW_TREE_MAX_M = 4 * OPMHIP_MS_WELLS_TREE_MAX_SEGMENTS;
constexpr int MSW_SEG = opmhip::MS_TREE_SEG, MSW_UP = opmhip::MS_TREE_UP, MSW_DOWN = opmhip::MS_TREE_DOWN;
static_assert(MSW_TREE_MAX_M * sizeof(double) <= 32768, "k_ms_wells_tree_apply: the well's z stays in LDS, half of the static limit");
__global__ __launch_bounds__(MSW_TREE_THREADS) void k_ms_wells_tree_factor(const MsTreeDesc* __restrict__ desc, const int* __restrict__ Dcolp,
                                                                           const int* __restrict__ tint, const double* __restrict__ Dvals,
                                                                           double* facAll, int* __restrict__ flag) {
    __shared__ int s_bad;
    const MsTreeDesc d = desc[blockIdx.x];
    const int M = 4 * d.Mb, t = threadIdx.x;
    constexpr int T = MSW_TREE_THREADS;
    double* fac = facAll + d.fac0;
    const int *parent = tint + d.par0, *cptr = tint + d.cptr0, *child = tint + d.child0, *lptr = tint + d.lptr0, *lseg = tint + d.lseg0, *dest = tint + d.dest0;
    if (t == 0) s_bad = INT_MAX;
    for (int e = t; e < MSW_SEG * d.Mb; e += T) fac[e] = 0.0;
    __syncthreads();
    const int* cp = Dcolp + d.dcol0;
    for (int c = t; c < M; c += T)   // one thread per column (two columns never share a place): entries that name the same place are added in their order
        for (int k = cp[c]; k < cp[c + 1]; ++k) fac[dest[k]] += Dvals[d.dnz0 + k];
    __syncthreads();
    for (int l = d.depth - 1; l >= 0; --l) {
        for (int q = lptr[l] + t; q < lptr[l + 1]; q += T) {
            const int i = lseg[q];
            double* F = fac + (size_t)i * MSW_SEG;
            double S[16], Si[16];
            for (int e = 0; e < 16; ++e) S[e] = F[e];
            for (int k = cptr[i]; k < cptr[i + 1]; ++k) {   // S_i -= E_c D_ci, the children ascending
                const double* G = fac + (size_t)child[k] * MSW_SEG;
                for (int r = 0; r < 4; ++r)
                    for (int c = 0; c < 4; ++c) {
                        double p = 0.0;
                        for (int m = 0; m < 4; ++m) p += G[MSW_UP + r * 4 + m] * G[MSW_DOWN + m * 4 + c];
                        S[r * 4 + c] = S[r * 4 + c] - p;
                    }
            }
            bool ok = invert4_stated(S, Si) == 0;
            if (ok)
                for (int e = 0; e < 16; ++e) ok = ok && fabs(Si[e]) <= 1.7976931348623157e308;
            if (!ok) { atomicMin(&s_bad, i + 1); continue; }
            for (int e = 0; e < 16; ++e) F[e] = Si[e];
            if (parent[i] >= 0) {   // E_i = D_pi S_i^-1
                double U[16];
                for (int e = 0; e < 16; ++e) U[e] = F[MSW_UP + e];
                for (int r = 0; r < 4; ++r)
                    for (int c = 0; c < 4; ++c) {
                        double p = 0.0;
                        for (int m = 0; m < 4; ++m) p += U[r * 4 + m] * Si[m * 4 + c];
                        F[MSW_UP + r * 4 + c] = p;
                    }
            }
        }
        __syncthreads();
    }
    if (t == 0) flag[d.well] = s_bad == INT_MAX ? 0 : s_bad;
}
// The two sweeps of z2 = D^-1 z1 over the tree, z in LDS, in place.  Forward, from the deepest parents up: z_p -= E_c z_c over p's
// children, ascending (pull: lane p alone writes z_p).  Backward, from the roots down: x_i = S_i^-1 (z_i - D_ip x_p).  A chain is
// 2 x depth dependent steps, so what a step costs beside its arithmetic decides:
//   - the tree's index lists (`ti`) are in LDS: a step's chain level -> segment -> children -> block is four dependent reads;
//   - the blocks (`fac`) are in LDS too where the well's fit (STAGED; otherwise each step waits for global memory once);
//   - WAVE - no level is wider than a wavefront - lets the first wavefront alone walk the levels, ordered by the LDS' own in-order
//     execution (a wavefront-scope fence keeps the compiler from moving the accesses; no s_barrier); otherwise the whole workgroup
//     does, with a barrier per level.
template <bool WAVE>
__device__ __forceinline__ void msw_tree_level_end() {
    if (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}
template <bool WAVE>
__device__ __forceinline__ void msw_tree_sweeps(const MsTreeDesc& d, const int* ti, const double* fac, double* z, int t) {
    constexpr int T = WAVE ? 64 : MSW_TREE_THREADS;
    const int *parent = ti, *cptr = ti + (d.cptr0 - d.par0), *child = ti + (d.child0 - d.par0), *lptr = ti + (d.lptr0 - d.par0), *lseg = ti + (d.lseg0 - d.par0);
    for (int l = d.depth - 2; l >= 0; --l) {
        for (int q = lptr[l] + t; q < lptr[l + 1]; q += T) {
            const int i = lseg[q], k0 = cptr[i], k1 = cptr[i + 1];
            if (k0 == k1) continue;
            double zp[4];
            for (int r = 0; r < 4; ++r) zp[r] = z[4 * i + r];
            for (int k = k0; k < k1; ++k) {
                const int c = child[k];
                const double* E = fac + (size_t)c * MSW_SEG + MSW_UP;
                for (int r = 0; r < 4; ++r) {
                    double s = 0.0;
                    for (int m = 0; m < 4; ++m) s += E[r * 4 + m] * z[4 * c + m];
                    zp[r] = zp[r] - s;
                }
            }
            for (int r = 0; r < 4; ++r) z[4 * i + r] = zp[r];
        }
        msw_tree_level_end<WAVE>();
    }
    for (int l = 0; l < d.depth; ++l) {
        for (int q = lptr[l] + t; q < lptr[l + 1]; q += T) {
            const int i = lseg[q], p = parent[i];
            const double* F = fac + (size_t)i * MSW_SEG;
            double v[4], x[4];
            for (int r = 0; r < 4; ++r) v[r] = z[4 * i + r];
            if (p >= 0)
                for (int r = 0; r < 4; ++r) {
                    double s = 0.0;
                    for (int m = 0; m < 4; ++m) s += F[MSW_DOWN + r * 4 + m] * z[4 * p + m];
                    v[r] = v[r] - s;
                }
            for (int r = 0; r < 4; ++r) {
                double s = 0.0;
                for (int m = 0; m < 4; ++m) s += F[r * 4 + m] * v[m];
                x[r] = s;
            }
            for (int r = 0; r < 4; ++r) z[4 * i + r] = x[r];
        }
        msw_tree_level_end<WAVE>();
    }
}
// y -= C^T (D^-1 (B (xs x))) for the tree wells of the list, one workgroup per well: z1 and y's update as k_ms_wells_apply forms them
// (a well of more equations than threads loops), z2 by the sweeps above.  Dynamic LDS, ldsDoubles doubles: z [4 Mb] | the tree's index
// lists [nint ints] | the well's blocks [48 Mb], the last only where they fit (msw_tree_lds_doubles: the host sizes the launch by it).
__host__ __device__ inline size_t msw_tree_lds_doubles(int Mb, int nint, bool staged) {
    return (size_t)4 * Mb + (size_t)(nint + 1) / 2 + (staged ? (size_t)MSW_SEG * Mb : 0);
}
template <bool ATOMIC>
__global__ __launch_bounds__(MSW_TREE_THREADS) void k_ms_wells_tree_apply(const MsTreeDesc* __restrict__ desc, const int* __restrict__ Brows,
                                                                          const int* __restrict__ cell, const int* __restrict__ blkrow,
                                                                          const double* __restrict__ B, const double* __restrict__ C,
                                                                          const int* __restrict__ tint, const double* __restrict__ facAll,
                                                                          const double* __restrict__ x, double* __restrict__ y, double xs, int ldsDoubles) {
    extern __shared__ double msw_lds[];
    const MsTreeDesc d = desc[blockIdx.x];
    const int M = 4 * d.Mb, t = threadIdx.x, nint = d.dest0 - d.par0;
    const bool staged = msw_tree_lds_doubles(d.Mb, nint, true) <= (size_t)ldsDoubles;   // (the same for every thread)
    double* z = msw_lds;
    int* ti = reinterpret_cast<int*>(msw_lds + M);
    double* sfac = msw_lds + M + (nint + 1) / 2;
    for (int e = t; e < nint; e += MSW_TREE_THREADS) ti[e] = tint[d.par0 + e];
    if (staged)
        for (int e = t; e < MSW_SEG * d.Mb; e += MSW_TREE_THREADS) sfac[e] = facAll[d.fac0 + e];
    const int* br = Brows + d.seg0;
    for (int e = t; e < M; e += MSW_TREE_THREADS) {
        const int row = e >> 2, j = e & 3;
        double s = 0.0;
        for (int blk = d.blk0 + br[row]; blk < d.blk0 + br[row + 1]; ++blk) {
            const double* xb = x + (size_t)cell[blk] * 3;
            double temp = 0.0;
            for (int k = 0; k < 3; ++k) temp += B[(size_t)blk * 12 + j * 3 + k] * (xs * xb[k]);
            s += temp;
        }
        z[e] = s;
    }
    __syncthreads();
    if (d.width <= 64) {
        if (t < 64) {
            if (staged) msw_tree_sweeps<true>(d, ti, sfac, z, t);
            else msw_tree_sweeps<true>(d, ti, facAll + d.fac0, z, t);
        }
        __syncthreads();
    } else {
        if (staged) msw_tree_sweeps<false>(d, ti, sfac, z, t);
        else msw_tree_sweeps<false>(d, ti, facAll + d.fac0, z, t);
    }
    for (int e = t; e < d.nblk * 3; e += MSW_TREE_THREADS) {
        const int blk = d.blk0 + e / 3, j = e % 3;
        const double* zz = z + blkrow[blk] * 4;
        double temp = 0.0;
        for (int k = 0; k < 4; ++k) temp += C[(size_t)blk * 12 + j + k * 3] * zz[k];
        double* yp = y + (size_t)cell[blk] * 3 + j;
        if (ATOMIC) atomicAdd(yp, -temp);
        else *yp -= temp;
    }
}

// blk += -C_c^T (D^-1 B_b) for one perforation pair: tmp = D^-1 B_b (4 x 3), then s = sum_k C_c[k][i] tmp[k][j], every sum ascending in k
// from 0.0 (Detail::multMatrix and Detail::negativeMultMatrixTransposed, linalg/MatrixBlock.hpp:496-570).  The one copy of the
// arithmetic of both matrix-add kernels below.
__device__ __forceinline__ void wells_pair_add(const double* __restrict__ Cc, const double* __restrict__ Dw, const double* __restrict__ Bb, double* blk) {
    double tmp[4][3];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += Dw[i * 4 + k] * Bb[k * 3 + j];
            tmp[i][j] = s;
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += Cc[k * 3 + i] * tmp[k][j];
            blk[i * 3 + j] += -s;
        }
}

// A(Ccols[c], Bcols[b]) += -C_c^T (D^-1 B_b) for every perforation pair (c, b) of well w0 + blockIdx.x
// (StandardWell::addWellContributions, wells/StandardWell_impl.hpp:1688-1712).  entry[] holds, per pair, the position of
// the block in the device's block-CSR (found on the host).
// serial != 0: the well has two perforations in one cell, i.e. several of its pairs hit the same block - one lane then
// adds all pairs in the perforation order of the CPU loop (no race, same bits).
__global__ __launch_bounds__(64) void k_wells_add_to_matrix(int w0, int serial, const int* __restrict__ vp, const double* __restrict__ C,
                                                            const double* __restrict__ D, const double* __restrict__ B,
                                                            const int* __restrict__ pair_ptr, const int* __restrict__ entry,
                                                            double* __restrict__ A) {
    const int w = w0 + blockIdx.x;
    const int pb = vp[w], np = vp[w + 1] - pb;
    if (serial && threadIdx.x != 0) return;
    for (int q = serial ? 0 : (int)threadIdx.x; q < np * np; q += serial ? 1 : 64) {
        const int c = q / np, b = q % np;
        const double* Bb = &B[(size_t)(pb + b) * 12];
        const double* Cc = &C[(size_t)(pb + c) * 12];
        const double* Dw = &D[(size_t)w * 16];
        wells_pair_add(Cc, Dw, Bb, &A[(size_t)entry[pair_ptr[w] + q] * BB]);
    }
}

// The same for the resident standard wells (opmhip_set_std_wells_matrix_add), by the schedule source_lists.cpp built once: one lane per
// distinct block of the matrix; the lane adds that block's contributions (well, a, b) one after the other in list order - by well, then
// by a * np + b, the order of the kernel above across its launches and inside its serial case.  Two wells in one cell and a well with
// two perforations in one cell are then ordinary entries of one list: one launch, no atomics, no LDS.  B, C and D^-1 are a few KB (L2).
__global__ __launch_bounds__(64) void k_std_wells_add_to_matrix(int nt, const int* __restrict__ target, const int* __restrict__ tptr,
                                                                const int* __restrict__ contrib, const int* __restrict__ vp,
                                                                const double* __restrict__ C, const double* __restrict__ D,
                                                                const double* __restrict__ B, double* __restrict__ A) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= nt) return;
    double* blk = &A[(size_t)target[t] * BB];
    for (int k = tptr[t]; k < tptr[t + 1]; ++k) {
        const int w = contrib[3 * k], pb = vp[w];
        wells_pair_add(&C[(size_t)(pb + contrib[3 * k + 1]) * 12], &D[(size_t)w * 16], &B[(size_t)(pb + contrib[3 * k + 2]) * 12], blk);
    }
}

void launch_ms_wells_factor(opmhip_ctx* c) {
    MsWellsDev& S = c->wells.ms;
    if (S.num_dense > 0)
        hipLaunchKernelGGL(k_ms_wells_factor, dim3(S.num_dense), dim3(MSW_FACTOR_THREADS), 0, c->stream, S.d_desc, S.d_Dcolp, S.d_Drows, S.d_Dvals, S.d_inv, S.d_flag);
    if (S.num_tree > 0)
        hipLaunchKernelGGL(k_ms_wells_tree_factor, dim3(S.num_tree), dim3(MSW_TREE_THREADS), 0, c->stream, S.d_tdesc, S.d_Dcolp, S.d_tint, S.d_Dvals, S.d_fac, S.d_flag);
    (void)hipMemcpyAsync(S.h_flag, S.d_flag, (size_t)S.num * sizeof(int), hipMemcpyDeviceToHost, c->stream);
    S.flag_pending = true;
    S.factorisations++;
}
// the device-resident multisegment wells, in the place of the host round trip: no copy, no synchronisation
void launch_ms_wells_apply(opmhip_ctx* c, const double* x, double* y, double xs) {
    const MsWellsDev& S = c->wells.ms;
    if (S.num_dense > 0) {
        if (S.atomic)
            hipLaunchKernelGGL(k_ms_wells_apply<true>, dim3(S.num_dense), dim3(MSW_APPLY_THREADS), 0, c->stream, S.d_desc, S.d_Brows, S.d_cell, S.d_blkrow, S.d_B, S.d_C, S.d_inv, x, y, xs);
        else
            hipLaunchKernelGGL(k_ms_wells_apply<false>, dim3(S.num_dense), dim3(MSW_APPLY_THREADS), 0, c->stream, S.d_desc, S.d_Brows, S.d_cell, S.d_blkrow, S.d_B, S.d_C, S.d_inv, x, y, xs);
    }
    if (S.num_tree > 0) {
        const size_t lds = (size_t)S.tree_lds_doubles * sizeof(double);
        if (S.atomic)
            hipLaunchKernelGGL(k_ms_wells_tree_apply<true>, dim3(S.num_tree), dim3(MSW_TREE_THREADS), lds, c->stream, S.d_tdesc, S.d_Brows, S.d_cell, S.d_blkrow, S.d_B, S.d_C, S.d_tint, S.d_fac, x, y, xs, S.tree_lds_doubles);
        else
            hipLaunchKernelGGL(k_ms_wells_tree_apply<false>, dim3(S.num_tree), dim3(MSW_TREE_THREADS), lds, c->stream, S.d_tdesc, S.d_Brows, S.d_cell, S.d_blkrow, S.d_B, S.d_C, S.d_tint, S.d_fac, x, y, xs, S.tree_lds_doubles);
    }
}
// The dynamic LDS of k_ms_wells_tree_apply for a list of tree wells: every well's z and index lists, and the blocks of the largest well
// whose blocks fit beside them (wells that fit stage their blocks, the others read them from global memory).  More than 64 KiB per
// workgroup has to be asked for; where the runtime declines, 64 KiB is the limit.
void ms_wells_tree_plan(opmhip_ctx* c, const std::vector<MsTreeDesc>& tdesc) {
    MsWellsDev& S = c->wells.ms;
    S.tree_lds_doubles = 0;
    if (tdesc.empty()) return;
    constexpr int LARGE = 160 * 1024, SMALL = 64 * 1024;
    const bool large = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ms_wells_tree_apply<true>), hipFuncAttributeMaxDynamicSharedMemorySize, LARGE) == hipSuccess &&
                       hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ms_wells_tree_apply<false>), hipFuncAttributeMaxDynamicSharedMemorySize, LARGE) == hipSuccess;
    if (!large) (void)hipGetLastError();
    const size_t cap = (size_t)(large ? LARGE : SMALL) / sizeof(double);
    size_t need = 0;
    for (const MsTreeDesc& d : tdesc) {
        const size_t plain = msw_tree_lds_doubles(d.Mb, d.dest0 - d.par0, false), staged = msw_tree_lds_doubles(d.Mb, d.dest0 - d.par0, true);
        need = std::max(need, staged <= cap ? staged : plain);
    }
    S.tree_lds_doubles = (int)need;
}
int launch_wells_apply(opmhip_ctx* c, const double* x, double* y, double xs) {
    const WellsDev& W = c->wells;
    if (W.num_wells <= 0) return OPMHIP_SUCCESS;
    if (W.distributed) {
        // a well shared by several subdomains: this rank's perforations give its part of B x, the parts are summed over the ranks, D^-1 and
        // C^T follow on every rank for its own cells (ParallelStandardWellB::mv, wells/WellHelpers.hpp:68-123; StandardWell::apply,
        // wells/StandardWell_impl.hpp:1254-1280)
        hipLaunchKernelGGL(k_wells_bx, dim3(W.num_wells), dim3(64), 0, c->stream, W.d_val_pointers, W.d_Bcols, W.d_B, x, xs, W.d_bx);
        const int rc = comm_allreduce(c, W.d_bx, W.num_wells * 4, 0);
        if (rc) return rc;
        hipLaunchKernelGGL(k_wells_residual, dim3(W.num_wells), dim3(64), 0, c->stream, W.d_val_pointers, W.d_Ccols, W.d_C, W.d_D, W.d_bx, y);
        return OPMHIP_SUCCESS;
    }
    hipLaunchKernelGGL(k_wells_apply, dim3(W.num_wells), dim3(64), 0, c->stream, W.d_val_pointers, W.d_Ccols, W.d_Bcols, W.d_C, W.d_D,
                       W.d_B, x, y, xs);
    return OPMHIP_SUCCESS;
}
void launch_wells_add_to_matrix(opmhip_ctx* c, int w0, int nw, int serial, const int* d_pair_ptr, const int* d_entry) {
    const WellsDev& W = c->wells;
    ensure_A(c);   // the wells are added to the matrix itself; the factorisation that follows reads it and rewrites the two streams
    hipLaunchKernelGGL(k_wells_add_to_matrix, dim3(nw), dim3(64), 0, c->stream, w0, serial, W.d_val_pointers, W.d_C, W.d_D, W.d_B, d_pair_ptr, d_entry, c->d_A);
}
void launch_std_wells_add_to_matrix(opmhip_ctx* c) {
    const WellsDev& W = c->wells;
    const SwMatrixAddDev& M = W.sw.ma;
    ensure_A(c);
    const int ps = prof_begin(c, PROF_ASSEMBLE);   // (the well model's, as the standard wells' other launches: one scope)
    hipLaunchKernelGGL(k_std_wells_add_to_matrix, dim3((M.targets + 63) / 64), dim3(64), 0, c->stream, M.targets, M.d_target, M.d_tptr, M.d_contrib,
                       W.d_val_pointers, W.d_C, W.d_D, W.d_B, c->d_A);
    prof_end(c, ps);
}
void launch_wells_residual(opmhip_ctx* c, const double* d_resWell, double* r) {
    const WellsDev& W = c->wells;
    if (W.num_wells <= 0) return;
    hipLaunchKernelGGL(k_wells_residual, dim3(W.num_wells), dim3(64), 0, c->stream, W.d_val_pointers, W.d_Ccols, W.d_C, W.d_D, d_resWell, r);
}
int launch_wells_recover(opmhip_ctx* c, const double* d_resWell, const double* x, double* d_xw) {
    const WellsDev& W = c->wells;
    if (W.num_wells <= 0) return OPMHIP_SUCCESS;
    if (W.distributed) {   // resWell - (sum over the ranks of B x): ParallelStandardWellB::mmv's branch for a shared well, wells/WellHelpers.hpp:136-141
        hipLaunchKernelGGL(k_wells_bx, dim3(W.num_wells), dim3(64), 0, c->stream, W.d_val_pointers, W.d_Bcols, W.d_B, x, 1.0, W.d_bx);
        const int rc = comm_allreduce(c, W.d_bx, W.num_wells * 4, 0);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_wells_recover, dim3(W.num_wells), dim3(64), 0, c->stream, W.d_val_pointers, W.d_Bcols, W.d_B, W.d_D, d_resWell, x,
                       W.distributed ? W.d_bx : nullptr, d_xw);
    return OPMHIP_SUCCESS;
}
// Multisegment wells: y -= C^T (D^-1 (B (xs x))) on the HOST, by the caller's objects (opmhip_wells.ms_apply) - x and y to pinned memory in
// the natural order, the callback, y back: the round trip the reference's back-ends make after every product
// (bda/WellContributions.cu:160-187; MultisegmentWellContribution::apply, bda/MultisegmentWellContribution.cpp:70-110).  The stream is
// drained twice per product: a deck whose multisegment wells come this way pays what it pays in the reference.  The alternative is the
// device-resident list of opmhip_set_ms_wells (k_ms_wells_factor / k_ms_wells_apply): the same operator with no host in the loop.
int ms_wells_apply_callback(opmhip_ctx* c, const double* x, double* y, double xs) {
    WellsDev& W = c->wells;
    const size_t n = (size_t)c->pat.Nb * BS;
    launch_vec_to_natural(c, x, c->d_stageV);
    OPMHIP_HIP(c, hipMemcpyAsync(W.h_x, c->d_stageV, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    launch_vec_to_natural(c, y, c->d_stageV);
    OPMHIP_HIP(c, hipMemcpyAsync(W.h_y, c->d_stageV, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
    if (xs != 1.0)   // x arrives without the relaxation factor of M^-1 (launch_ilu_apply's `unscaled`): one rounded product per entry, as on the device
        for (size_t i = 0; i < n; ++i) W.h_x[i] *= xs;
    W.ms_apply(W.ms_user, W.h_x, W.h_y);
    OPMHIP_HIP(c, hipMemcpyAsync(c->d_stageV, W.h_y, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    launch_vec_to_internal(c, c->d_stageV, y);
    OPMHIP_HIP(c, hipStreamSynchronize(c->stream));   // h_y may be written again by the next product
    return OPMHIP_SUCCESS;
}

}  // namespace opmhip
