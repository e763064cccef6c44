// Device functions more than one translation unit states: one copy of the arithmetic, so that the units cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

// wells.py invert4_stated: Gauss-Jordan on [D | I], partial pivoting (largest |entry| of the column, lowest row on ties), the pivot row
// divided by the pivot, every other row updated as a - f * b.  -> 0, or 1 + the column without a pivot (inv is then left alone)
__device__ inline int invert4_stated(const double* D, double* inv) {
    double a[4][8];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) { a[i][j] = D[i * 4 + j]; a[i][4 + j] = i == j ? 1.0 : 0.0; }
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        for (int r = col + 1; r < 4; ++r)
            if (fabs(a[r][col]) > fabs(a[piv][col])) piv = r;
        if (!(fabs(a[piv][col]) > 0.0)) return 1 + col;
        if (piv != col)
            for (int j = 0; j < 8; ++j) { const double t = a[col][j]; a[col][j] = a[piv][j]; a[piv][j] = t; }
        const double p = a[col][col];
        for (int j = 0; j < 8; ++j) a[col][j] = a[col][j] / p;
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const double f = a[r][col];
            for (int j = 0; j < 8; ++j) a[r][j] = a[r][j] - f * a[col][j];
        }
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) inv[i * 4 + j] = a[i][4 + j];
    return 0;
}

// ---- 3 x 3 block arithmetic of the linear solver and of CPR (solver.hip, cpr.hip) ------------------------------------------------
namespace opmhip {
// y -= A x, y += A x, y = A x in dune-common DenseMatrix order (row outer, column inner)
__device__ __forceinline__ void blk_mmv(const double* A, const double x0, const double x1, const double x2, double* y) {
    y[0] -= A[0] * x0; y[0] -= A[1] * x1; y[0] -= A[2] * x2;
    y[1] -= A[3] * x0; y[1] -= A[4] * x1; y[1] -= A[5] * x2;
    y[2] -= A[6] * x0; y[2] -= A[7] * x1; y[2] -= A[8] * x2;
}
// The same with the block known to live in LDS.  The pointer carries its address space in its type, so that the compiler
// can neither treat it as "flat" nor merge this path with the global-memory one behind a single flat pointer (it does
// that to two branches that differ in nothing but the pointer): a flat load makes the wavefront wait for EVERY outstanding
// memory access - in the pipelined sweeps that is the prefetch of the next step.
typedef __attribute__((address_space(3))) const double lds_cdouble;
__device__ __forceinline__ void blk_mmv_lds(const double* Agen, const double x0, const double x1, const double x2, double* y) {
    lds_cdouble* A = (lds_cdouble*)Agen;
    y[0] -= A[0] * x0; y[0] -= A[1] * x1; y[0] -= A[2] * x2;
    y[1] -= A[3] * x0; y[1] -= A[4] * x1; y[1] -= A[5] * x2;
    y[2] -= A[6] * x0; y[2] -= A[7] * x1; y[2] -= A[8] * x2;
}
// y -= A x and, beside it, u += A x from the SAME rounded products: the backward sweep's row sums u_i = sum_{j>i} U_ij x_j (Pattern::ualias)
__device__ __forceinline__ void blk_mmv_u(const double* A, const double x0, const double x1, const double x2, double* y, double* u) {
    double p;
    p = A[0] * x0; y[0] -= p; u[0] += p; p = A[1] * x1; y[0] -= p; u[0] += p; p = A[2] * x2; y[0] -= p; u[0] += p;
    p = A[3] * x0; y[1] -= p; u[1] += p; p = A[4] * x1; y[1] -= p; u[1] += p; p = A[5] * x2; y[1] -= p; u[1] += p;
    p = A[6] * x0; y[2] -= p; u[2] += p; p = A[7] * x1; y[2] -= p; u[2] += p; p = A[8] * x2; y[2] -= p; u[2] += p;
}
__device__ __forceinline__ void blk_mmv_lds_u(const double* Agen, const double x0, const double x1, const double x2, double* y, double* u) {
    lds_cdouble* A = (lds_cdouble*)Agen;
    double p;
    p = A[0] * x0; y[0] -= p; u[0] += p; p = A[1] * x1; y[0] -= p; u[0] += p; p = A[2] * x2; y[0] -= p; u[0] += p;
    p = A[3] * x0; y[1] -= p; u[1] += p; p = A[4] * x1; y[1] -= p; u[1] += p; p = A[5] * x2; y[1] -= p; u[1] += p;
    p = A[6] * x0; y[2] -= p; u[2] += p; p = A[7] * x1; y[2] -= p; u[2] += p; p = A[8] * x2; y[2] -= p; u[2] += p;
}
__device__ __forceinline__ void blk_umv_lds(const double* Agen, const double x0, const double x1, const double x2, double* y) {
    lds_cdouble* A = (lds_cdouble*)Agen;
    y[0] += A[0] * x0; y[0] += A[1] * x1; y[0] += A[2] * x2;
    y[1] += A[3] * x0; y[1] += A[4] * x1; y[1] += A[5] * x2;
    y[2] += A[6] * x0; y[2] += A[7] * x1; y[2] += A[8] * x2;
}
__device__ __forceinline__ void blk_umv(const double* A, const double x0, const double x1, const double x2, double* y) {
    y[0] += A[0] * x0; y[0] += A[1] * x1; y[0] += A[2] * x2;
    y[1] += A[3] * x0; y[1] += A[4] * x1; y[1] += A[5] * x2;
    y[2] += A[6] * x0; y[2] += A[7] * x1; y[2] += A[8] * x2;
}
// C = A * B with the inner sum starting from 0.0 (DenseMatrix::rightmultiply / leftmultiply)
__device__ __forceinline__ void blk_mul(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            s += A[i * 3 + 0] * B[0 * 3 + j];
            s += A[i * 3 + 1] * B[1 * 3 + j];
            s += A[i * 3 + 2] * B[2 * 3 + j];
            C[i * 3 + j] = s;
        }
}
// closed-form inverse, expression tree of Opm::Detail::Inverter<3> (linalg/MatrixBlock.hpp:722-747)
__device__ __forceinline__ void blk_invert(const double* m, double* inv) {
    const double t4 = m[0] * m[4], t6 = m[0] * m[5], t8 = m[1] * m[3];
    const double t10 = m[2] * m[3], t12 = m[1] * m[6], t14 = m[2] * m[6];
    const double det = (t4 * m[8] - t6 * m[7] - t8 * m[8] + t10 * m[7] + t12 * m[5] - t14 * m[4]);
    const double t17 = 1.0 / det;
    inv[0] = (m[4] * m[8] - m[5] * m[7]) * t17;
    inv[1] = -(m[1] * m[8] - m[2] * m[7]) * t17;
    inv[2] = (m[1] * m[5] - m[2] * m[4]) * t17;
    inv[3] = -(m[3] * m[8] - m[5] * m[6]) * t17;
    inv[4] = (m[0] * m[8] - t14) * t17;
    inv[5] = -(t6 - t10) * t17;
    inv[6] = (m[3] * m[7] - m[4] * m[6]) * t17;
    inv[7] = -(m[0] * m[7] - t12) * t17;
    inv[8] = (t4 - t8) * t17;
}
// y -= A x / y += A x per block, see blk_mmv / blk_umv
template <bool SUB>
__device__ __forceinline__ void blk_apply(const double* A, const double* xx, double* acc) {
    if (SUB) blk_mmv(A, xx[0], xx[1], xx[2], acc); else blk_umv(A, xx[0], xx[1], xx[2], acc);
}
template <bool SUB>
__device__ __forceinline__ void blk_apply_lds(const double* A, const double* xx, double* acc) {
    if (SUB) blk_mmv_lds(A, xx[0], xx[1], xx[2], acc); else blk_umv_lds(A, xx[0], xx[1], xx[2], acc);
}
}  // namespace opmhip
