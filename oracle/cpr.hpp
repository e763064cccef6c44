// ORACLE — TEST INFRASTRUCTURE ONLY (see linalg.hpp).
// CPU restatement of the CPR (constrained pressure residual) preconditioner of the hot path, the checker of
// opm-autodiff_amd/csrc/cpr.hip and cpr_setup.cpp.
//
// What follows the reference line by line (in tree):
//   two-level structure        opm/simulators/linalg/twolevelmethodcpr.hh:476-498  (pre-smoothing 0 steps, coarse correction,
//                              residual update, ONE post-smoothing step of the fine smoother; OwningTwoLevelPreconditioner.hpp)
//   quasi-IMPES weights        opm/simulators/linalg/getQuasiImpesWeights.hpp:46-85  (w_i = D_ii^-T e_p / max|.|, p = 1)
//   pressure system            opm/simulators/linalg/PressureTransferPolicy.hpp:92-160 (A_p[i][j] = sum_k A_ij[k][p] w_i[k];
//                              r_p[i] = sum_k r_i[k] w_i[k]; fine correction goes into the pressure component only)
//   fine smoother              ParOverILU0, relaxation 1.0 (setupPropertyTree.cpp:107-108)
//   coarse solver              ONE application of an aggregation AMG (loopsolver, maxiter 1, :110-114), prolongation damping
//                              1.6 (:132), one pre- and one post-smoothing step (:119-120)
// What is NOT the reference's algorithm and cannot be (dune-istl is not in the reference tree):
//   the aggregation and the AMG smoother.  Dune::Amg builds its aggregates with a strength-of-connection front algorithm and
//   smooths with ILU0; here aggregates come from two passes of pairwise matching per level (each node with its strongest
//   still-free neighbour), the smoother is damped Jacobi and the coarsest level (<= COARSE_DIRECT unknowns) is solved by
//   dense LU - an AMG that maps onto the GPU without a level schedule per level.  PARITY WITH Dune::Amg IS THEREFORE
//   UNPINNED; pinned is what the reference's own test can pin: CPR-BiCGStab on tests/matr33.txt reproduces the exact
//   solution of tests/test_flexiblesolver.cpp:93-116 (tests/test_oracle_cpr.py).
// The 3x3 solve for the weights uses the closed-form inverse of linalg/MatrixBlock.hpp:722-747 (Dune's FieldMatrix::solve
// is an LU with pivoting: same number up to rounding).
#pragma once
#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#include "linalg.hpp"

namespace orc {

struct Csr {
    int n = 0;
    std::vector<int> rowptr, col;
    std::vector<double> val;
};

constexpr int CPR_PRESSURE_INDEX = 1;   // pressureVarIndex of BlackOilIndices (ISTLSolverEbos.hpp: pressureIndex)
constexpr int CPR_COARSE_DIRECT = 128;  // coarsest level: dense LU up to this many unknowns
constexpr int CPR_MAX_LEVELS = 15;      // maxlevel (setupPropertyTree.cpp:124)
constexpr int CPR_MAX_W = 96;           // longest row of a level the product builds (its ELL images): coarsening stops before

struct AmgLevel {
    Csr A;                         // level matrix (values refreshed by update_values)
    std::vector<double> dinv;      // 1 / diagonal
    std::vector<int> diag;         // position of the diagonal entry of each row
    std::vector<int> agg;          // node -> aggregate (empty on the coarsest level)
    int nc = 0;
    std::vector<int> mptr, midx;   // members of each aggregate, ascending
    std::vector<int> gptr, gidx;   // Galerkin: coarse entry e = sum of the fine entries gidx[gptr[e] .. gptr[e+1]), ascending
    // ILU0 smoothing (CprAmg::iluLevels): scalar ILU0 factors in A's pattern (strict lower = L, diagonal = 1 / U_ii, strict upper
    // = U) for the elimination order `ord` (pos = its inverse; empty: the stored order)
    std::vector<double> ilu;
    std::vector<int> ord, pos;
};

// the reference's kind of aggregation (DuneLikeAmg::aggregate below) on a level of THIS hierarchy: experiment of round 5 (missing item 3 of
// the round-4 review) - what does the aggregation alone buy, with the product's smoothers, transfers and cycle?
void dune_like_aggregate(const Csr& A, std::vector<int>& agg, int& na);
struct CprAmg {
    std::vector<AmgLevel> lv;
    std::vector<double> lu;        // dense LU (no pivoting) of the coarsest level, row-major
    bool coarse_direct = true;
    double omega = 2.0 / 3.0;      // Jacobi damping
    double damp = 1.6;             // prolongation damping (setupPropertyTree.cpp:132)
    double beta = 0.25;            // a neighbour is a candidate if -a_ij >= beta * max_k(-a_ik)
    std::vector<int> natOf, atNat; // level 0 of a reordered system: natural id of every index / index of every natural id (empty: as stored)
    int maxLevels = CPR_MAX_LEVELS;   // levels of the hierarchy at most (the coarsest one is solved directly or by 1 + 4 Jacobi sweeps)
    int nu = 1;                    // smoothing sweeps before and after the coarse correction (the product runs V(1,1); more: experiments)
    int coarseSweeps = 4;          // Jacobi sweeps (after the first, from x = 0) that stand in for the coarse solve where coarsening stalled
    bool joinAtStall = false;      // experiment switch (orc_cpr_set_sweeps with a negative argument)
    int wFrom = 1 << 30;           // experiment: levels >= wFrom visit their coarse level twice (W-cycle below that level); the product runs V-cycles
    bool join = false;             // leftover nodes join a neighbour's aggregate (uniform coarsening, but measured WORSE: see DESIGN.md)
    // smoother: levels l < iluLevels (that are not the coarsest) smooth with a scalar ILU0, relaxation 1 - the reference's smoother
    // (PreconditionerFactory.hpp:126-151) - instead of damped Jacobi.  Elimination order of such a level: the stored order
    // (level 0: whatever ordering the block ILU0 uses - on the device a line colouring) or, iluColour, a greedy multi-colouring
    // of the level's graph, colour by colour (what a device sweep of an irregular coarse level would need)
    int iluLevels = 0;
    int iluColourFrom = 1 << 30;   // levels >= iluColourFrom eliminate in greedy multi-colour order
    bool iluAlways0 = false;       // level 0 is factored even where it is the hierarchy's only level (a subdomain whose level 0 itself joins the other subdomains')
    // decomposed runs (orc_cpr_solve_blocks with gather_rows): the hierarchy of a subdomain ends at its first level of at most stopRows
    // rows, and that level is not solved here (external): its right-hand side joins those of the other subdomains (vcycle_down), the
    // joined system is cycled on, and the subdomain's slice of the result comes back (vcycle_up)
    int stopRows = CPR_COARSE_DIRECT;
    bool external = false;

    // one pass of pairwise matching, nodes visited in index order: node i takes its strongest (most negative coupling)
    // still-free neighbour, lowest index on ties
    // strength of a coupling: -a_ij (M-matrix-like rows), or |a_ij| when anySign (coarse levels that lost their sign pattern)
    // natOf / atNat (level 0 of a REORDERED system only, else NULL): natural id of every index and its inverse - the nodes are
    // then visited in NATURAL order and ties go to the lowest natural id, so that the aggregates are those of the natural-order
    // matrix whatever ordering the ILU0 wants (matching in a colour-by-colour ordering pairs cells across the grid and stalls)
    static void pairwise(const Csr& A, double beta, bool anySign, bool join_, std::vector<int>& agg, int& na,
                         const int* natOf = nullptr, const int* atNat = nullptr) {
        const int n = A.n;
        agg.assign(n, -1);
        na = 0;
        for (int v = 0; v < n; ++v) {
            const int i = atNat ? atNat[v] : v;
            if (agg[i] >= 0) continue;
            double mx = 0.0;
            for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k)
                if (A.col[k] != i) mx = std::max(mx, anySign ? std::fabs(A.val[k]) : -A.val[k]);
            int best = -1;
            double bv = 0.0;
            for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) {
                const int j = A.col[k];
                if (j == i || agg[j] >= 0) continue;
                const double s = anySign ? std::fabs(A.val[k]) : -A.val[k];
                if (s >= beta * mx && (s > bv || (natOf && best >= 0 && s == bv && natOf[j] < natOf[best]))) { best = j; bv = s; }
            }
            if (best >= 0) {
                agg[i] = agg[best] = na++;
                continue;
            }
            // no free neighbour left: rather than staying a singleton (singletons pile up on the coarse levels and stall the
            // coarsening) the node joins the aggregate of its strongest coupled neighbour
            int join = -1;
            double jv = 0.0;
            for (int k = A.rowptr[i]; join_ && k < A.rowptr[i + 1]; ++k) {
                const int j = A.col[k];
                if (j == i || agg[j] < 0) continue;
                const double s = anySign ? std::fabs(A.val[k]) : -A.val[k];
                if (s > jv) { join = agg[j]; jv = s; }
            }
            agg[i] = join >= 0 ? join : na++;
        }
    }
    // Galerkin product for a piecewise-constant prolongation: pattern, gather lists (fine entries of every coarse entry in
    // ascending fine-entry order) and values
    static void galerkin(const Csr& A, const std::vector<int>& agg, int nc, Csr& C, std::vector<int>& gptr, std::vector<int>& gidx) {
        std::vector<std::map<int, std::vector<int>>> rows(nc);
        for (int i = 0; i < A.n; ++i)
            for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) rows[agg[i]][agg[A.col[k]]].push_back(k);
        C.n = nc;
        C.rowptr.assign(nc + 1, 0);
        C.col.clear();
        gptr.assign(1, 0);
        gidx.clear();
        for (int I = 0; I < nc; ++I) {
            for (auto& e : rows[I]) {
                C.col.push_back(e.first);
                std::sort(e.second.begin(), e.second.end());
                gidx.insert(gidx.end(), e.second.begin(), e.second.end());
                gptr.push_back((int)gidx.size());
            }
            C.rowptr[I + 1] = (int)C.col.size();
        }
        C.val.assign(C.col.size(), 0.0);
        for (size_t e = 0; e < C.col.size(); ++e) {
            double s = 0.0;
            for (int q = gptr[e]; q < gptr[e + 1]; ++q) s += A.val[gidx[q]];
            C.val[e] = s;
        }
    }
    static void finish_level(AmgLevel& L) {
        const int n = L.A.n;
        L.diag.assign(n, -1);
        for (int i = 0; i < n; ++i)
            for (int k = L.A.rowptr[i]; k < L.A.rowptr[i + 1]; ++k)
                if (L.A.col[k] == i) L.diag[i] = k;
    }
    bool duneAgg = false;   // experiment: aggregates of 4-6 within distance 2 (DuneLikeAmg::aggregate) instead of two pairwise passes
    // hierarchy from the values of the first pressure matrix: two pairwise passes per level (aggregates of up to four)
    void setup_structure(const Csr& A0) {
        lv.clear();
        Csr A = A0;
        while (true) {
            AmgLevel L;
            L.A = A;
            finish_level(L);
            const bool last = A.n <= stopRows || (int)lv.size() + 1 >= maxLevels;
            if (!last) {
                std::vector<int> a1, a2, g1p, g1i;
                int n1 = 0, n2 = 0;
                Csr A1;
                if (duneAgg) {
                    std::vector<int> ad;
                    dune_like_aggregate(A, ad, n2);
                    a1.resize(A.n); std::iota(a1.begin(), a1.end(), 0); a2 = ad; n1 = A.n;
                } else
                // small coarse levels lose their strong couplings and their sign pattern: if the strength threshold leaves too
                // many nodes alone, match with any negative coupling, then with the largest coupling of either sign
                for (int attempt = 0; attempt < 3; ++attempt) {
                    const double b = attempt == 0 ? beta : 0.0;
                    const bool lvl0 = lv.empty() && !natOf.empty();
                    pairwise(A, b, attempt == 2, join, a1, n1, lvl0 ? natOf.data() : nullptr, lvl0 ? atNat.data() : nullptr);
                    galerkin(A, a1, n1, A1, g1p, g1i);
                    pairwise(A1, b, attempt == 2, join, a2, n2);
                    if (n2 <= (int)(0.5 * A.n)) break;
                }
                if (n2 >= (int)(0.8 * A.n) && joinAtStall) {   // experiment: leftover nodes join a neighbour's aggregate on the levels where matching stalls
                    pairwise(A, 0.0, true, true, a1, n1);
                    galerkin(A, a1, n1, A1, g1p, g1i);
                    pairwise(A1, 0.0, true, true, a2, n2);
                }
                if (n2 >= (int)(0.8 * A.n)) {   // coarsening stalls (hardly any coupling left): stop here
                    lv.push_back(L);
                    break;
                }
                L.agg.resize(A.n);
                for (int i = 0; i < A.n; ++i) L.agg[i] = a2[a1[i]];
                L.nc = n2;
                Csr Ac;
                galerkin(A, L.agg, n2, Ac, L.gptr, L.gidx);
                {   // the product keeps its levels as ELL images of at most CPR_MAX_W entries per row: a wider coarse level is not built
                    int Wc = 1;
                    for (int I = 0; I < Ac.n; ++I) Wc = std::max(Wc, Ac.rowptr[I + 1] - Ac.rowptr[I]);
                    if (Wc > CPR_MAX_W) {
                        L.agg.clear(); L.nc = 0; L.gptr.clear(); L.gidx.clear();
                        lv.push_back(L);
                        break;
                    }
                }
                L.mptr.assign(n2 + 1, 0);
                for (int i = 0; i < A.n; ++i) L.mptr[L.agg[i] + 1]++;
                for (int I = 0; I < n2; ++I) L.mptr[I + 1] += L.mptr[I];
                L.midx.resize(A.n);
                std::vector<int> w(L.mptr.begin(), L.mptr.end() - 1);
                for (int i = 0; i < A.n; ++i) L.midx[w[L.agg[i]]++] = i;
                lv.push_back(L);
                A = Ac;
                continue;
            }
            lv.push_back(L);
            break;
        }
        coarse_direct = !external && lv.back().A.n <= CPR_COARSE_DIRECT;
        update_values(A0.val);
    }
    // new level-0 values (same pattern): Galerkin values down the hierarchy, inverse diagonals, coarsest LU
    void update_values(const std::vector<double>& a0) {
        lv[0].A.val = a0;
        for (size_t l = 0; l < lv.size(); ++l) {
            AmgLevel& L = lv[l];
            L.dinv.resize(L.A.n);
            for (int i = 0; i < L.A.n; ++i) L.dinv[i] = 1.0 / L.A.val[L.diag[i]];
            if ((int)l < iluLevels && (l + 1 < lv.size() || (l == 0 && iluAlways0))) ilu_factor(L, (int)l >= iluColourFrom);
            else L.ilu.clear();
            if (l + 1 < lv.size()) {
                Csr& C = lv[l + 1].A;
                for (size_t e = 0; e < C.col.size(); ++e) {
                    double s = 0.0;
                    for (int q = L.gptr[e]; q < L.gptr[e + 1]; ++q) s += L.A.val[L.gidx[q]];
                    C.val[e] = s;
                }
            }
        }
        if (coarse_direct) {   // dense LU without pivoting, Doolittle, in place
            const Csr& C = lv.back().A;
            const int n = C.n;
            lu.assign((size_t)n * n, 0.0);
            for (int i = 0; i < n; ++i)
                for (int k = C.rowptr[i]; k < C.rowptr[i + 1]; ++k) lu[(size_t)i * n + C.col[k]] = C.val[k];
            for (int k = 0; k < n; ++k) {
                const double piv = 1.0 / lu[(size_t)k * n + k];
                for (int i = k + 1; i < n; ++i) {
                    const double f = lu[(size_t)i * n + k] * piv;
                    lu[(size_t)i * n + k] = f;
                    for (int j = k + 1; j < n; ++j) lu[(size_t)i * n + j] -= f * lu[(size_t)k * n + j];
                }
                lu[(size_t)k * n + k] = piv;   // the diagonal keeps 1 / u_kk (as the block ILU0 keeps D^-1): the substitution multiplies
            }
        }
    }
    // scalar ILU0 of a level in the elimination order L.ord (IKJ form: row i against the finished rows j in ascending position)
    static void ilu_factor(AmgLevel& L, bool colour) {
        const Csr& A = L.A;
        const int n = A.n;
        if ((int)L.ord.size() != n) {
            L.ord.resize(n);
            L.pos.resize(n);
            if (!colour) for (int i = 0; i < n; ++i) L.ord[i] = i;
            else {   // greedy colouring in index order, then colour-major, index order inside a colour
                std::vector<int> col(n, -1);
                int nc = 0;
                std::vector<char> used;
                for (int i = 0; i < n; ++i) {
                    used.assign(nc + 1, 0);
                    for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k)
                        if (col[A.col[k]] >= 0) used[col[A.col[k]]] = 1;
                    int c = 0;
                    while (used[c]) ++c;
                    col[i] = c;
                    nc = std::max(nc, c + 1);
                }
                int p = 0;
                for (int c = 0; c < nc; ++c)
                    for (int i = 0; i < n; ++i)
                        if (col[i] == c) L.ord[p++] = i;
            }
            for (int p = 0; p < n; ++p) L.pos[L.ord[p]] = p;
        }
        std::vector<double>& f = L.ilu;
        f = A.val;
        std::vector<std::pair<int, int>> low;
        for (int p = 0; p < n; ++p) {
            const int i = L.ord[p];
            low.clear();
            for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k)
                if (L.pos[A.col[k]] < p) low.emplace_back(L.pos[A.col[k]], k);
            std::sort(low.begin(), low.end());
            for (auto& e : low) {
                const int k = e.second, j = A.col[k];
                f[k] = f[k] * f[L.diag[j]];
                for (int q = A.rowptr[j]; q < A.rowptr[j + 1]; ++q) {
                    const int c = A.col[q];
                    if (L.pos[c] <= e.first) continue;                 // U part of row j only
                    const int* b = A.col.data() + A.rowptr[i];
                    const int* en = A.col.data() + A.rowptr[i + 1];
                    const int* t = std::lower_bound(b, en, c);
                    if (t != en && *t == c) f[t - A.col.data()] -= f[k] * f[q];
                }
            }
            f[L.diag[i]] = 1.0 / f[L.diag[i]];
        }
    }
    // v = M^-1 d of level l's smoother: damped Jacobi, or (U^-1 L^-1) of the level's ILU0 in its elimination order
    void smooth(const AmgLevel& L, const double* d, double* v) const {
        const int n = L.A.n;
        if (L.ilu.empty()) {
            for (int i = 0; i < n; ++i) v[i] = omega * L.dinv[i] * d[i];
            return;
        }
        const Csr& A = L.A;
        for (int p = 0; p < n; ++p) {
            const int i = L.ord[p];
            double s = d[i];
            for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k)
                if (L.pos[A.col[k]] < p) s -= L.ilu[k] * v[A.col[k]];
            v[i] = s;
        }
        for (int p = n - 1; p >= 0; --p) {
            const int i = L.ord[p];
            double s = v[i];
            for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k)
                if (L.pos[A.col[k]] > p) s -= L.ilu[k] * v[A.col[k]];
            v[i] = s * L.ilu[L.diag[i]];
        }
    }
    static void residual(const Csr& A, const double* b, const double* x, double* r) {
        for (int i = 0; i < A.n; ++i) {
            double s = b[i];
            for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) s -= A.val[k] * x[A.col[k]];
            r[i] = s;
        }
    }
    // The cycle in two halves around a coarsest level that somebody else solves (external): down - smoothing, residuals and
    // restrictions of the levels above it, the coarsest level's right-hand side comes back in st.back().b; up - with the coarsest
    // level's solution in st.back().x the way back, x = the finest level's result.  Statement for statement vcycle's (V(1,1), no W-cycle).
    struct LevelState { std::vector<double> b, x, r; };
    void vcycle_down(const double* b0, std::vector<LevelState>& st, size_t last) const {   // last: the level somebody else solves
        st.assign(last + 1, LevelState());
        st[0].b.assign(b0, b0 + lv[0].A.n);
        for (size_t l = 0; l < last; ++l) {
            const AmgLevel& L = lv[l];
            const int n = L.A.n;
            LevelState& S = st[l];
            S.x.assign(n, 0.0); S.r.assign(n, 0.0);
            if (L.ilu.empty()) for (int i = 0; i < n; ++i) S.x[i] = omega * L.dinv[i] * S.b[i];
            else smooth(L, S.b.data(), S.x.data());
            residual(L.A, S.b.data(), S.x.data(), S.r.data());
            st[l + 1].b.assign(L.nc, 0.0);
            for (int I = 0; I < L.nc; ++I) {
                double s = 0.0;
                for (int q = L.mptr[I]; q < L.mptr[I + 1]; ++q) s += S.r[L.midx[q]];
                st[l + 1].b[I] = s;
            }
        }
        st.back().x.assign(lv[last].A.n, 0.0);
    }
    void vcycle_up(std::vector<LevelState>& st, double* x0) const {
        for (size_t l = st.size() - 1; l-- > 0;) {
            const AmgLevel& L = lv[l];
            const int n = L.A.n;
            LevelState& S = st[l];
            const std::vector<double>& xc = st[l + 1].x;
            for (int i = 0; i < n; ++i) S.x[i] += damp * xc[L.agg[i]];
            residual(L.A, S.b.data(), S.x.data(), S.r.data());
            if (L.ilu.empty()) for (int i = 0; i < n; ++i) S.x[i] += omega * L.dinv[i] * S.r[i];
            else { std::vector<double> t(n); smooth(L, S.r.data(), t.data()); for (int i = 0; i < n; ++i) S.x[i] += t[i]; }
        }
        std::copy(st[0].x.begin(), st[0].x.end(), x0);
    }
    // one V(1,1) cycle from x = 0
    void vcycle(const double* b, double* x, size_t l = 0) const {
        const AmgLevel& L = lv[l];
        const int n = L.A.n;
        if (l + 1 == lv.size()) {
            if (coarse_direct) {
                for (int i = 0; i < n; ++i) {
                    double s = b[i];
                    for (int j = 0; j < i; ++j) s -= lu[(size_t)i * n + j] * x[j];
                    x[i] = s;
                }
                // backward substitution COLUMN by column: once x_j is final every row above it takes u_ij x_j off - a row's terms go in the
                // order j = n - 1 ... i + 1, then the division.  (Round 5: the row-oriented form - j ascending - made the device walk the
                // rows one after the other, 0.13 ms per application on a 100-row level; this order lets the rows above a column work at once.
                // Both are backward substitutions of the same factors; the AMG is this design's own, no reference number pins the order.)
                for (int j = n - 1; j >= 0; --j) {
                    x[j] = x[j] * lu[(size_t)j * n + j];   // (the diagonal holds 1 / u_jj)
                    for (int i = 0; i < j; ++i) x[i] -= lu[(size_t)i * n + j] * x[j];
                }
            } else {   // could not coarsen further: a few Jacobi sweeps stand in for the coarse solve
                std::vector<double> r(n);
                for (int i = 0; i < n; ++i) x[i] = omega * L.dinv[i] * b[i];
                for (int sweep = 0; sweep < coarseSweeps; ++sweep) {
                    residual(L.A, b, x, r.data());
                    for (int i = 0; i < n; ++i) x[i] += omega * L.dinv[i] * r[i];
                }
            }
            return;
        }
        std::vector<double> r(n), rc(L.nc), xc(L.nc), t;
        if (L.ilu.empty()) for (int i = 0; i < n; ++i) x[i] = omega * L.dinv[i] * b[i];        // pre-smoothing from x = 0
        else { t.resize(n); smooth(L, b, x); }
        residual(L.A, b, x, r.data());
        for (int sweep = 1; sweep < nu; ++sweep) {                           // nu > 1: further Jacobi sweeps (V(nu, nu))
            for (int i = 0; i < n; ++i) x[i] += omega * L.dinv[i] * r[i];
            residual(L.A, b, x, r.data());
        }
        for (int I = 0; I < L.nc; ++I) {                                    // restriction: sum over the aggregate
            double s = 0.0;
            for (int q = L.mptr[I]; q < L.mptr[I + 1]; ++q) s += r[L.midx[q]];
            rc[I] = s;
        }
        vcycle(rc.data(), xc.data(), l + 1);
        if ((int)l >= wFrom && l + 2 < lv.size()) {                         // experiment (W-cycle): a second cycle on the coarse residual
            std::vector<double> rc2(L.nc), xc2(L.nc);
            residual(lv[l + 1].A, rc.data(), xc.data(), rc2.data());
            vcycle(rc2.data(), xc2.data(), l + 1);
            for (int I = 0; I < L.nc; ++I) xc[I] += xc2[I];
        }
        for (int i = 0; i < n; ++i) x[i] += damp * xc[L.agg[i]];            // damped piecewise-constant prolongation
        residual(L.A, b, x, r.data());
        if (L.ilu.empty()) for (int i = 0; i < n; ++i) x[i] += omega * L.dinv[i] * r[i];        // post-smoothing
        else { smooth(L, r.data(), t.data()); for (int i = 0; i < n; ++i) x[i] += t[i]; }
        for (int sweep = 1; sweep < nu; ++sweep) {
            residual(L.A, b, x, r.data());
            for (int i = 0; i < n; ++i) x[i] += omega * L.dinv[i] * r[i];
        }
    }
};

// ---- the reference's pressure AMG, restated for comparison ----------------------------------------------------------------
// Dune::Amg as opm-simulators configures it (linalg/PreconditionerFactory.hpp:126-151, setupPropertyTree.cpp:116-137):
// AggregationCriterion<SymmetricDependency<Matrix, FirstDiagonal>>, alpha 1/3, beta 1e-5, maxDistance 2, aggregates of 4 to 6
// vertices, maxConnectivity 15, coarsenTarget 1200 unknowns, at most 15 levels, minimal coarsening rate 1.2, piecewise-constant
// prolongation damped by 1.6, ILU0 (relaxation 1) as pre- and post-smoother (1 + 1 steps), V-cycle, direct solve on the
// coarsest level.  dune-istl is NOT in the reference tree: this is a restatement of its published algorithm
// (dune-istl/paamg/aggregates.hh: Aggregator::build / growAggregate / the rounding step / mergeNeighbour; dependency.hh:
// SymmetricDependency; amg.hh: mgc) from the sources as I know them - UNVERIFIED, and where the published code breaks ties
// through internal bookkeeping (connectivity counters over neighbouring aggregates, front ordering) this restatement breaks
// them on the lowest vertex index.  It is ORACLE-ONLY and exists for one purpose: a yardstick for the product's own pressure
// AMG (pairwise matching + Jacobi, CprAmg above) - how many CPR-BiCGStab iterations the reference's kind of hierarchy needs
// on the same Jacobians (tools/cpr_amg_compare.py).
struct DuneLikeAmg {
    struct Level {
        Csr A;
        std::vector<double> ilu;       // scalar ILU0 factors in A's pattern: strict lower = L, diagonal = 1 / U_ii, strict upper = U
        std::vector<int> diag;
        std::vector<int> agg;          // vertex -> aggregate (empty on the coarsest level)
        int nc = 0;
        std::vector<int> gptr, gidx;   // Galerkin gather lists (as in CprAmg)
    };
    std::vector<Level> lv;
    std::vector<double> lu;            // dense LU of the coarsest level
    double alpha = 1.0 / 3.0, beta = 1e-5, damp = 1.6, minCoarsenRate = 1.2;
    int maxDistance = 2, minAgg = 4, maxAgg = 6, coarsenTarget = 1200, maxLevel = 15;
    bool jacobi = false;               // experiment: damped Jacobi (2/3) in place of the ILU0 smoother - which of the two, aggregation or smoother, makes the difference to the product's AMG?

    // SymmetricDependency with the sign-preserving norm FirstDiagonal: only negative off-diagonal pairs count;
    // strength e_ij e_ji / (a_ii a_jj); edge strong if > alpha * row maximum; vertex isolated if its maximum < beta
    void dependency(const Csr& A, std::vector<char>& strong, std::vector<char>& isolated) const {
        const int n = A.n;
        std::vector<double> d(n, 1.0);
        for (int i = 0; i < n; ++i)
            for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k)
                if (A.col[k] == i) d[i] = A.val[k];
        auto entry = [&](int r, int c, double& v) {   // a_rc if present
            const int* b = A.col.data() + A.rowptr[r];
            const int* e = A.col.data() + A.rowptr[r + 1];
            const int* q = std::lower_bound(b, e, c);
            if (q == e || *q != c) return false;
            v = A.val[q - A.col.data()];
            return true;
        };
        strong.assign(A.col.size(), 0);
        isolated.assign(n, 0);
        for (int i = 0; i < n; ++i) {
            double maxValue = -std::numeric_limits<double>::max();
            for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) {
                const int j = A.col[k];
                const double eij = A.val[k];
                double eji;
                if (j == i || !(eij < 0.0) || !entry(j, i, eji) || !(eji < 0.0)) continue;
                maxValue = std::max(maxValue, eij / d[i] * eji / d[j]);
            }
            isolated[i] = maxValue < beta;
            for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) {
                const int j = A.col[k];
                const double eij = A.val[k];
                double eji;
                if (j == i || !(eij < 0.0) || !entry(j, i, eji)) continue;
                if (eji / d[j] * eij / d[i] > alpha * maxValue) strong[k] = 1;
            }
        }
        // depends / influences are set on both directions of an edge
        for (int i = 0; i < n; ++i)
            for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k)
                if (strong[k]) {
                    const int j = A.col[k];
                    const int* b = A.col.data() + A.rowptr[j];
                    const int* q = std::lower_bound(b, A.col.data() + A.rowptr[j + 1], i);
                    strong[q - A.col.data()] = 1;
                }
    }
    // Aggregator::build: seeds in index order; growAggregate up to minAgg vertices within maxDistance; the rounding step up to
    // maxAgg; a one-vertex aggregate joins a neighbouring aggregate (mergeNeighbour); isolated vertices stay alone
    void aggregate(const Csr& A, std::vector<int>& agg, int& na) const {
        const int n = A.n;
        std::vector<char> strong, isolated;
        dependency(A, strong, isolated);
        agg.assign(n, -1);
        na = 0;
        std::vector<int> members, front, distOf(n, -1);
        auto strong_into = [&](int v, int id) {   // twoWayConnections
            int c = 0;
            for (int k = A.rowptr[v]; k < A.rowptr[v + 1]; ++k) c += (strong[k] && agg[A.col[k]] == id);
            return c;
        };
        auto nb_counts = [&](int v, int id, int& inAgg, int& freeNb, int& all) {
            inAgg = freeNb = all = 0;
            for (int k = A.rowptr[v]; k < A.rowptr[v + 1]; ++k) {
                const int j = A.col[k];
                if (j == v) continue;
                ++all;
                inAgg += agg[j] == id;
                freeNb += agg[j] < 0;
            }
        };
        auto rebuild_front = [&](int id) {   // unaggregated neighbours (any edge) of the members, ascending
            front.clear();
            for (int m : members)
                for (int k = A.rowptr[m]; k < A.rowptr[m + 1]; ++k)
                    if (agg[A.col[k]] < 0) front.push_back(A.col[k]);
            std::sort(front.begin(), front.end());
            front.erase(std::unique(front.begin(), front.end()), front.end());
            (void)id;
        };
        auto distance_from = [&](int seed, int id, int extra) {   // largest graph distance from the seed inside the aggregate (+ extra vertex)
            std::vector<int> q{seed};
            std::vector<int> touched{seed};
            distOf[seed] = 0;
            int far = 0;
            for (size_t h = 0; h < q.size(); ++h) {
                const int v = q[h];
                for (int k = A.rowptr[v]; k < A.rowptr[v + 1]; ++k) {
                    const int j = A.col[k];
                    if (distOf[j] >= 0 || (agg[j] != id && j != extra)) continue;
                    distOf[j] = distOf[v] + 1;
                    far = std::max(far, distOf[j]);
                    q.push_back(j); touched.push_back(j);
                }
            }
            const int de = extra >= 0 ? distOf[extra] : far;
            for (int v : touched) distOf[v] = -1;
            return extra >= 0 ? (de < 0 ? 1 << 20 : de) : far;
        };
        for (int seed = 0; seed < n; ++seed) {
            if (agg[seed] >= 0) continue;
            const int id = na++;
            members.assign(1, seed);
            agg[seed] = id;
            if (!isolated[seed]) {
                // growAggregate
                int dist = 0;
                while ((int)members.size() < minAgg && dist < maxDistance) {
                    rebuild_front(id);
                    int bestTwo = 0, bestFrontNb = -1;
                    double bestCon = -1.0;
                    std::vector<int> cand;
                    for (int v : front) {
                        if (isolated[v]) continue;
                        const int two = strong_into(v, id);
                        if (two == 0) continue;
                        int inAgg, freeNb, all;
                        nb_counts(v, id, inAgg, freeNb, all);
                        const double con = all > 0 ? (double)inAgg / all : 0.0;
                        int frontNb = 0;   // noFrontNeighbours
                        for (int k = A.rowptr[v]; k < A.rowptr[v + 1]; ++k) frontNb += std::binary_search(front.begin(), front.end(), A.col[k]) && A.col[k] != v;
                        if (two > bestTwo || (two == bestTwo && (con > bestCon || (con == bestCon && frontNb > bestFrontNb)))) {
                            bestTwo = two; bestCon = con; bestFrontNb = frontNb;
                            cand.assign(1, v);
                        } else if (two == bestTwo && con == bestCon && frontNb == bestFrontNb) cand.push_back(v);
                    }
                    if (cand.empty()) break;
                    if ((int)cand.size() > maxAgg - (int)members.size()) cand.resize(maxAgg - (int)members.size());
                    for (int v : cand) { agg[v] = id; members.push_back(v); }
                    dist = distance_from(seed, id, -1);
                }
                // the rounding step: a front vertex with a strong connection that has more neighbours inside than free ones
                while ((int)members.size() < maxAgg) {
                    rebuild_front(id);
                    int pick = -1;
                    for (int v : front) {
                        if (isolated[v] || strong_into(v, id) == 0) continue;
                        int inAgg, freeNb, all;
                        nb_counts(v, id, inAgg, freeNb, all);
                        if (freeNb >= inAgg) continue;
                        if (distance_from(seed, id, v) > maxDistance) continue;
                        pick = v;
                        break;
                    }
                    if (pick < 0) break;
                    agg[pick] = id;
                    members.push_back(pick);
                }
                // mergeNeighbour: a lone non-isolated vertex joins the aggregate of its first aggregated, non-isolated neighbour
                if (members.size() == 1) {
                    int target = -1;
                    for (int k = A.rowptr[seed]; k < A.rowptr[seed + 1] && target < 0; ++k) {
                        const int j = A.col[k];
                        if (j != seed && agg[j] >= 0 && agg[j] != id && !isolated[j]) target = agg[j];
                    }
                    if (target >= 0) { agg[seed] = target; --na; }
                }
            }
        }
    }
    static void ilu0_scalar(const Csr& A, const std::vector<int>& diag, std::vector<double>& f) {
        f = A.val;
        const int n = A.n;
        for (int i = 0; i < n; ++i) {
            for (int k = A.rowptr[i]; k < diag[i]; ++k) {
                const int j = A.col[k];
                f[k] = f[k] * f[diag[j]];                 // l_ij = a_ij / u_jj (the diagonal holds the inverse)
                int p = k + 1, q = diag[j] + 1;
                while (p < A.rowptr[i + 1] && q < A.rowptr[j + 1]) {
                    if (A.col[p] == A.col[q]) { f[p] -= f[k] * f[q]; ++p; ++q; }
                    else if (A.col[p] < A.col[q]) ++p;
                    else ++q;
                }
            }
            f[diag[i]] = 1.0 / f[diag[i]];
        }
    }
    void smooth(const Level& L, const double* d, double* v) const {
        if (!jacobi) { ilu0_apply(L, d, v); return; }
        for (int i = 0; i < L.A.n; ++i) v[i] = (2.0 / 3.0) * d[i] / L.A.val[L.diag[i]];
    }
    static void ilu0_apply(const Level& L, const double* d, double* v) {
        const Csr& A = L.A;
        const int n = A.n;
        for (int i = 0; i < n; ++i) {
            double s = d[i];
            for (int k = A.rowptr[i]; k < L.diag[i]; ++k) s -= L.ilu[k] * v[A.col[k]];
            v[i] = s;
        }
        for (int i = n - 1; i >= 0; --i) {
            double s = v[i];
            for (int k = L.diag[i] + 1; k < A.rowptr[i + 1]; ++k) s -= L.ilu[k] * v[A.col[k]];
            v[i] = s * L.ilu[L.diag[i]];
        }
    }
    void finish(Level& L) const {
        L.diag.assign(L.A.n, 0);
        for (int i = 0; i < L.A.n; ++i)
            for (int k = L.A.rowptr[i]; k < L.A.rowptr[i + 1]; ++k)
                if (L.A.col[k] == i) L.diag[i] = k;
        ilu0_scalar(L.A, L.diag, L.ilu);
    }
    void setup(const Csr& A0) {
        lv.clear();
        lv.emplace_back();
        lv[0].A = A0;
        while ((int)lv.size() < maxLevel && lv.back().A.n > coarsenTarget) {
            Level& L = lv.back();
            std::vector<int> agg;
            int na = 0;
            aggregate(L.A, agg, na);
            if ((double)L.A.n / std::max(na, 1) < minCoarsenRate) break;   // coarsening stalls
            // aggregate ids are dense again after the merges
            std::vector<int> renum(L.A.n + 1, -1);
            int nn = 0;
            for (int i = 0; i < L.A.n; ++i)
                if (renum[agg[i]] < 0) renum[agg[i]] = nn++;
            for (int i = 0; i < L.A.n; ++i) agg[i] = renum[agg[i]];
            L.agg = agg;
            L.nc = nn;
            Level C;
            CprAmg::galerkin(L.A, L.agg, nn, C.A, L.gptr, L.gidx);
            lv.push_back(std::move(C));
        }
        for (Level& L : lv) finish(L);
        const Csr& C = lv.back().A;
        const int n = C.n;
        lu.assign((size_t)n * n, 0.0);
        for (int i = 0; i < n; ++i)
            for (int k = C.rowptr[i]; k < C.rowptr[i + 1]; ++k) lu[(size_t)i * n + C.col[k]] = C.val[k];
        for (int k = 0; k < n; ++k)
            for (int i = k + 1; i < n; ++i) {
                const double f = lu[(size_t)i * n + k] / lu[(size_t)k * n + k];
                lu[(size_t)i * n + k] = f;
                if (f != 0.0)
                    for (int j = k + 1; j < n; ++j) lu[(size_t)i * n + j] -= f * lu[(size_t)k * n + j];
            }
    }
    // the hierarchy's structure is kept (as the reference's CPR keeps it between updates); values: Galerkin sums + factors
    void update_values(const std::vector<double>& a0) {
        lv[0].A.val = a0;
        for (size_t l = 0; l + 1 < lv.size(); ++l) {
            Level& L = lv[l];
            Csr& C = lv[l + 1].A;
            for (size_t e = 0; e < C.val.size(); ++e) {
                double s = 0.0;
                for (int q = L.gptr[e]; q < L.gptr[e + 1]; ++q) s += L.A.val[L.gidx[q]];
                C.val[e] = s;
            }
        }
        const std::vector<Level> keep;   // (structure untouched)
        for (Level& L : lv) ilu0_scalar(L.A, L.diag, L.ilu);
        const Csr& C = lv.back().A;
        const int n = C.n;
        lu.assign((size_t)n * n, 0.0);
        for (int i = 0; i < n; ++i)
            for (int k = C.rowptr[i]; k < C.rowptr[i + 1]; ++k) lu[(size_t)i * n + C.col[k]] = C.val[k];
        for (int k = 0; k < n; ++k)
            for (int i = k + 1; i < n; ++i) {
                const double f = lu[(size_t)i * n + k] / lu[(size_t)k * n + k];
                lu[(size_t)i * n + k] = f;
                if (f != 0.0)
                    for (int j = k + 1; j < n; ++j) lu[(size_t)i * n + j] -= f * lu[(size_t)k * n + j];
            }
    }
    // AMG::mgc, V-cycle with one pre- and one post-smoothing step: x = update for the defect b (x starts at 0)
    void vcycle(const double* b, double* x, size_t l = 0) const {
        const Level& L = lv[l];
        const int n = L.A.n;
        if (l + 1 == lv.size()) {
            for (int i = 0; i < n; ++i) {
                double s = b[i];
                for (int j = 0; j < i; ++j) s -= lu[(size_t)i * n + j] * x[j];
                x[i] = s;
            }
            for (int i = n - 1; i >= 0; --i) {
                double s = x[i];
                for (int j = i + 1; j < n; ++j) s -= lu[(size_t)i * n + j] * x[j];
                x[i] = s / lu[(size_t)i * n + i];
            }
            return;
        }
        std::vector<double> d(b, b + n), v(n), t(n);
        smooth(L, d.data(), v.data());                                  // pre-smoothing: update += M^-1 d ; d -= A v
        for (int i = 0; i < n; ++i) x[i] = v[i];
        CprAmg::residual(L.A, d.data(), v.data(), t.data());
        d.swap(t);
        std::vector<double> rc(L.nc, 0.0), xc(L.nc, 0.0);
        for (int i = 0; i < n; ++i) rc[L.agg[i]] += d[i];               // restriction: sum over the aggregate
        vcycle(rc.data(), xc.data(), l + 1);
        for (int i = 0; i < n; ++i) v[i] = damp * xc[L.agg[i]];         // damped piecewise-constant prolongation
        for (int i = 0; i < n; ++i) x[i] += v[i];
        CprAmg::residual(L.A, d.data(), v.data(), t.data());
        d.swap(t);
        smooth(L, d.data(), v.data());                                  // post-smoothing
        for (int i = 0; i < n; ++i) x[i] += v[i];
    }
};

// True-IMPES weights of one cell (opm/simulators/linalg/getQuasiImpesWeights.hpp:89-128): block[ii][jj] = d storage_ii /
// d x_jj / (V / dt), the pressure column times 50e5; block^T w = e_p; w /= 1000.  dS: derivatives of the storage term
// (equation x primary variable).  The reference solves with Dune's FieldMatrix::solve - an LU with partial pivoting whose
// code is not in the tree; here: Gaussian elimination with row pivoting on the largest magnitude (first one on ties),
// the same statements on the device, hence the same bits there (UNVERIFIED vs Dune's rounding sequence).
inline void true_impes_weights_cell(const double dS[BS][BS], double storage_scale, double w[BS]) {
    const double pressure_scale = 50e5;
    double M[BS][BS + 1];
    for (int r = 0; r < BS; ++r) {          // M = block^T | e_p
        for (int c = 0; c < BS; ++c) {
            double v = dS[c][r] / storage_scale;         // block[c][r], c = equation, r = variable
            if (r == CPR_PRESSURE_INDEX) v = v * pressure_scale;
            M[r][c] = v;
        }
        M[r][BS] = (r == CPR_PRESSURE_INDEX) ? 1.0 : 0.0;
    }
    for (int k = 0; k < BS; ++k) {
        int piv = k;
        double best = std::fabs(M[k][k]);
        for (int r = k + 1; r < BS; ++r)
            if (std::fabs(M[r][k]) > best) { best = std::fabs(M[r][k]); piv = r; }
        if (piv != k)
            for (int c = 0; c <= BS; ++c) { const double t = M[k][c]; M[k][c] = M[piv][c]; M[piv][c] = t; }
        for (int r = k + 1; r < BS; ++r) {
            const double f = M[r][k] / M[k][k];
            for (int c = k; c <= BS; ++c) M[r][c] = M[r][c] - f * M[k][c];
        }
    }
    for (int r = BS - 1; r >= 0; --r) {
        double s = M[r][BS];
        for (int c = r + 1; c < BS; ++c) s = s - M[r][c] * w[c];
        w[r] = s / M[r][r];
    }
    for (int r = 0; r < BS; ++r) w[r] = w[r] / 1000.0;   // "given normal densities this scales weights to about 1"
}

// the whole preconditioner for one block system
inline void dune_like_aggregate(const Csr& A, std::vector<int>& agg, int& na) {
    DuneLikeAmg D;
    D.aggregate(A, agg, na);
    std::vector<int> renum(A.n + 1, -1);   // aggregate ids dense again after the merges, in order of first appearance
    int nn = 0;
    for (int i = 0; i < A.n; ++i)
        if (renum[agg[i]] < 0) renum[agg[i]] = nn++;
    for (int i = 0; i < A.n; ++i) agg[i] = renum[agg[i]];
    na = nn;
}

struct Cpr {
    const Bcrs* A = nullptr;
    Bcrs LU;
    std::vector<int> dg;
    std::vector<double> w;          // weights, Nb x 3: quasi-IMPES from the matrix, or handed in (true-IMPES: they need the model)
    std::vector<double> w_given;    // non-empty: use these
    CprAmg amg;
    DuneLikeAmg dune;               // the reference's kind of hierarchy (comparison only)
    bool useDune = false;
    bool structured = false;

    static void quasi_impes_weights(const Bcrs& A, std::vector<double>& w) {
        const std::vector<int> dg = diag_index(A);
        w.assign((size_t)A.Nb * BS, 0.0);
        for (int i = 0; i < A.Nb; ++i) {
            const double* D = &A.val[(size_t)dg[i] * BB];
            double Dt[BB], inv[BB];
            for (int r = 0; r < BS; ++r)
                for (int c = 0; c < BS; ++c) Dt[r * BS + c] = D[c * BS + r];
            blk_invert(Dt, inv);
            double bw[BS], mx = 0.0;
            for (int r = 0; r < BS; ++r) { bw[r] = inv[r * BS + CPR_PRESSURE_INDEX]; mx = std::max(mx, std::fabs(bw[r])); }
            for (int r = 0; r < BS; ++r) w[(size_t)i * BS + r] = bw[r] / mx;
        }
    }
    static void pressure_values(const Bcrs& A, const std::vector<double>& w, std::vector<double>& ap) {
        ap.resize(A.nnzb());
        for (int i = 0; i < A.Nb; ++i)
            for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) {
                double s = 0.0;
                for (int r = 0; r < BS; ++r) s += A.val[(size_t)k * BB + r * BS + CPR_PRESSURE_INDEX] * w[(size_t)i * BS + r];
                ap[k] = s;
            }
    }
    // (re)builds everything that depends on the matrix VALUES; the AMG hierarchy's structure is built once, from the first
    // matrix (CprReuseSetup-like: aggregates are kept, Galerkin values are refreshed every solve)
    int update(const Bcrs& Ain) {
        A = &Ain;
        LU = Ain;
        const int rc = bilu0_decompose(LU, Ain.Nb);
        if (rc) return rc;
        dg = diag_index(LU);
        if (w_given.empty()) quasi_impes_weights(Ain, w);
        else w = w_given;
        std::vector<double> ap;
        pressure_values(Ain, w, ap);
        if (!structured) {
            Csr P;
            P.n = Ain.Nb; P.rowptr = Ain.rowptr; P.col = Ain.col; P.val = ap;
            if (useDune) dune.setup(P); else amg.setup_structure(P);
            structured = true;
        } else if (useDune) dune.update_values(ap);
        else amg.update_values(ap);
        return 0;
    }
    // moveToCoarseLevel: r_p[i] = sum_k d_i[k] w_i[k]
    void restrict_fine(const double* d, double* rc) const {
        for (int i = 0; i < A->Nb; ++i) {
            double s = 0.0;
            for (int k = 0; k < BS; ++k) s += d[(size_t)i * BS + k] * w[(size_t)i * BS + k];
            rc[i] = s;
        }
    }
    // v = M^-1 d (TwoLevelMethodCpr::apply with 0 pre- and 1 post-smoothing step)
    void apply(const double* d, double* v) const {
        const int Nb = A->Nb;
        std::vector<double> rc(Nb), xc(Nb);
        restrict_fine(d, rc.data());
        if (useDune) { std::fill(xc.begin(), xc.end(), 0.0); dune.vcycle(rc.data(), xc.data()); }
        else amg.vcycle(rc.data(), xc.data());
        finish(d, xc.data(), v);
    }
    // the rest of apply once the pressure correction xc is there: v = (0, xc, 0) + ILU0(d - A (0, xc, 0))
    void finish(const double* d, const double* xc, double* v) const {
        const int Nb = A->Nb;
        const size_t n = (size_t)Nb * BS;
        std::vector<double> r(n), y(n), z(n);
        for (size_t e = 0; e < n; ++e) v[e] = 0.0;                    // moveToFineLevel: pressure component only
        for (int i = 0; i < Nb; ++i) v[(size_t)i * BS + CPR_PRESSURE_INDEX] = xc[i];
        spmv(*A, v, y.data());                                       // post-smoothing on the updated residual
        for (size_t e = 0; e < n; ++e) r[e] = d[e] - y[e];
        ilu0_apply(LU, dg, Nb, r.data(), z.data(), 1.0, 0);
        for (size_t e = 0; e < n; ++e) v[e] += z[e];
    }
};

}  // namespace orc
