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
