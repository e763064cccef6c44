// Host set-up of the CPR pressure AMG (csrc/cpr_setup.cpp: pairwise matching, Galerkin gather lists, ELL images, ILU0 smoothing schedules,
// colourings) under AddressSanitizer + UBSan + libstdc++'s container assertions (test infrastructure; built and run by
// tests/test_host_logic_sanitized.py with g++, no GPU).  cpr_setup.cpp is linked alone, with no stand-in for any HIP runtime call: that the
// link succeeds is the check that the set-up half of the library - which runs on a host thread of its own beside the solves - makes none.
// Per level of every hierarchy the harness checks what the uploads and kernels of cpr.hip rely on: the aggregates are onto [0, nc), the
// member lists invert them, the four-member records are there exactly when every aggregate has 1-4 members, the Galerkin lists cover every
// entry of the finer level once (as places in its ELL image, each inside the right pair of aggregates), every image decodes back to its CSR
// matrix, and every ILU0 schedule is an elimination order its sweeps may run in parallel.  The hierarchy is compared with the oracle's
// (oracle/cpr.hpp: CprAmg::setup_structure on the same matrix): the same levels, sizes and aggregates, the same coarsest matrix bit for bit.
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../opm-autodiff_amd/csrc/internal.hpp"
#include "../../oracle/cpr.hpp"

using opmhip::CprHostCoarse;
using opmhip::CprHostLevel;
using opmhip::CprIluHost;

static int g_fail = 0;
#define CHECK(cond, ...)                                                 \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                    \
            std::printf("\n");                                           \
            ++g_fail;                                                    \
            return false;                                                \
        }                                                                \
    } while (0)

// a scalar pressure matrix: rows [0, n) owned, columns >= n ghost cells (a decomposed run's local pattern), columns ascending, values
struct Mat {
    int n = 0, nghost = 0;
    std::vector<int> rowptr, col;
    std::vector<double> val;
};
static Mat from_rows(int n, int nghost, std::vector<std::vector<std::pair<int, double>>>& rows) {
    Mat m;
    m.n = n; m.nghost = nghost;
    m.rowptr.push_back(0);
    for (auto& r : rows) {
        std::sort(r.begin(), r.end());
        for (auto& e : r) { m.col.push_back(e.first); m.val.push_back(e.second); }
        m.rowptr.push_back((int)m.col.size());
    }
    return m;
}
// M-matrix-like 7-point grid, natural order: a face of transmissibility t couples its cells by -t, the diagonal is the sum of the row's
// couplings plus an accumulation term.  hetero = false: every face alike (ties everywhere - the matching's tie rule decides); nxo < nx: the
// owned part [0, nxo) of the x range, the next layer behind the cut becomes ghost cells numbered behind the owned ones
static Mat grid7(int nx, int ny, int nz, bool hetero, unsigned seed, int nxo = -1) {
    if (nxo < 0) nxo = nx;
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> U(0.05, 2.0);
    auto id = [&](int i, int j, int k) { return i + nxo * (j + ny * k); };
    const int n = nxo * ny * nz;
    std::vector<std::vector<std::pair<int, double>>> rows(n);
    std::vector<double> diag(n, 0.0);
    int nghost = 0;
    std::vector<int> ghostId((size_t)ny * nz, -1);
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nxo; ++i) {
                const int a = id(i, j, k);
                diag[a] += hetero ? 1e-3 * U(rng) : 1e-3;
                const int nbr[3][3] = {{i + 1, j, k}, {i, j + 1, k}, {i, j, k + 1}};
                const double scale[3] = {1.0, 0.7, 0.1};   // anisotropic: z couplings weaker
                for (int d = 0; d < 3; ++d) {
                    const int bi = nbr[d][0], bj = nbr[d][1], bk = nbr[d][2];
                    if (bi >= nx || bj >= ny || bk >= nz) continue;
                    const double t = scale[d] * (hetero ? U(rng) : 1.0);
                    if (bi >= nxo) {   // behind the cut: the coupling to a ghost cell stays in the owned row only
                        int& g = ghostId[j + (size_t)ny * k];
                        if (g < 0) g = n + nghost++;
                        rows[a].push_back({g, -t});
                        diag[a] += t;
                        continue;
                    }
                    const int b = id(bi, bj, bk);
                    rows[a].push_back({b, -t});
                    rows[b].push_back({a, -t});
                    diag[a] += t;
                    diag[b] += t;
                }
            }
    for (int a = 0; a < n; ++a) rows[a].push_back({a, diag[a]});
    return from_rows(n, nghost, rows);
}
// symmetric M-matrix-like pattern with long rows: every row couples to `deg` partners inside a window of +-span (corner-point grids with
// faults and NNCs, in the extreme) - the coarse levels' rows outgrow CPR_MAX_W
static Mat long_rows(int n, int deg, int span, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<std::set<int>> nb(n);
    for (int i = 0; i < n; ++i)
        for (int t = 0; t < deg / 2; ++t) {
            const int j = i + 1 + (int)(rng() % (unsigned)span);
            if (j < n && (int)nb[i].size() < deg && (int)nb[j].size() < deg) { nb[i].insert(j); nb[j].insert(i); }
        }
    std::uniform_real_distribution<double> U(0.1, 1.0);
    std::vector<std::vector<std::pair<int, double>>> rows(n);
    std::vector<double> diag(n, 1e-3);
    for (int i = 0; i < n; ++i)
        for (int j : nb[i])
            if (j > i) {
                const double t = U(rng);
                rows[i].push_back({j, -t}); rows[j].push_back({i, -t});
                diag[i] += t; diag[j] += t;
            }
    for (int i = 0; i < n; ++i) rows[i].push_back({i, diag[i]});
    return from_rows(n, 0, rows);
}
// the grid in a line-coloured order: colour (i + j) % 2 first, then column by column, each z-line in order - the two-colour chained ordering
// of the block ILU0 (neighbours of one colour meet only along a chain).  order[p] = natural id of row p
static Mat permuted(const Mat& A, const std::vector<int>& order) {
    std::vector<int> at(A.n);
    for (int p = 0; p < A.n; ++p) at[order[p]] = p;
    std::vector<std::vector<std::pair<int, double>>> rows(A.n);
    for (int p = 0; p < A.n; ++p)
        for (int k = A.rowptr[order[p]]; k < A.rowptr[order[p] + 1]; ++k) rows[p].push_back({at[A.col[k]], A.val[k]});
    return from_rows(A.n, 0, rows);
}
static std::vector<int> line_colour_order(int nx, int ny, int nz, std::vector<int>& colourPrefix) {
    std::vector<int> order;
    colourPrefix.assign(1, 0);
    for (int c = 0; c < 2; ++c) {
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i)
                if ((i + j) % 2 == c)
                    for (int k = 0; k < nz; ++k) order.push_back(i + nx * (j + ny * k));
        colourPrefix.push_back((int)order.size());
    }
    return order;
}

// place of slot j of row i in a level's image
static size_t at(const CprHostLevel& L, int j, int i) { return L.rm ? (size_t)i * L.W + j : (size_t)j * L.n + i; }

// the image holds the CSR pattern (rowptr, col; columns >= ncols: ghost cells, stored as the row itself), pos the place of every entry
static bool check_image(const char* what, const CprHostLevel& L, const std::vector<int>& rowptr, const std::vector<int>& col, const std::vector<int>& pos, int ncols) {
    const int n = L.n;
    CHECK((int)rowptr.size() == n + 1 && L.nnz == rowptr[n] && (int)pos.size() == L.nnz, "%s: sizes", what);
    int W = 1;
    for (int i = 0; i < n; ++i) W = std::max(W, rowptr[i + 1] - rowptr[i]);
    CHECK(L.W == W && L.W <= opmhip::CPR_MAX_W, "%s: W %d, longest row %d", what, L.W, W);
    CHECK(L.ecol.size() == (size_t)W * n && (int)L.rlen.size() == n && (int)L.diag.size() == n, "%s: image sizes", what);
    for (int i = 0; i < n; ++i) {
        CHECK(L.rlen[i] == rowptr[i + 1] - rowptr[i], "%s: rlen[%d]", what, i);
        bool hasDiag = false;
        for (int j = 0; j < W; ++j) {
            const int k = rowptr[i] + j;
            const int want = j < L.rlen[i] && col[k] < ncols ? col[k] : i;
            CHECK(L.ecol[at(L, j, i)] == want, "%s: row %d slot %d holds %d, not %d", what, i, j, L.ecol[at(L, j, i)], want);
            if (j < L.rlen[i]) {
                CHECK(pos[k] == (int)at(L, j, i), "%s: pos of entry %d", what, k);
                if (col[k] == i) { CHECK(L.diag[i] == pos[k], "%s: diag of row %d", what, i); hasDiag = true; }
            }
        }
        CHECK(hasDiag, "%s: row %d has no diagonal", what, i);
    }
    return true;
}
// the CSR pattern an image stands for (no ghost columns: coarse levels)
static void image_csr(const CprHostLevel& L, std::vector<int>& rowptr, std::vector<int>& col, std::vector<int>& pos) {
    rowptr.assign(1, 0); col.clear(); pos.clear();
    for (int i = 0; i < L.n; ++i) {
        for (int j = 0; j < L.rlen[i]; ++j) { col.push_back(L.ecol[at(L, j, i)]); pos.push_back((int)at(L, j, i)); }
        rowptr.push_back((int)col.size());
    }
}

// transfer of a level (n rows, pattern rowptr/col, entries at pos of its image L) to the next one (image C)
static bool check_transfer(const char* what, const CprHostLevel& H, int n, const std::vector<int>& rowptr, const std::vector<int>& col,
                           const std::vector<int>& pos, const CprHostLevel& L, const CprHostLevel& C) {
    const int nc = H.nc;
    CHECK(nc > 0 && nc < n && (int)H.agg.size() == n && C.n == nc, "%s: nc %d of %d rows, next level %d", what, nc, n, C.n);
    std::vector<int> members(nc, 0);
    for (int i = 0; i < n; ++i) { CHECK(H.agg[i] >= 0 && H.agg[i] < nc, "%s: agg[%d] = %d", what, i, H.agg[i]); ++members[H.agg[i]]; }
    bool upTo4 = true;
    for (int I = 0; I < nc; ++I) { CHECK(members[I] > 0, "%s: aggregate %d is empty", what, I); upTo4 = upTo4 && members[I] <= 4; }
    // member lists
    CHECK((int)H.mptr.size() == nc + 1 && H.mptr[0] == 0 && H.mptr[nc] == n && (int)H.midx.size() == n, "%s: member list sizes", what);
    for (int I = 0; I < nc; ++I) {
        CHECK(H.mptr[I + 1] - H.mptr[I] == members[I], "%s: members of %d", what, I);
        for (int q = H.mptr[I]; q < H.mptr[I + 1]; ++q) {
            CHECK(H.midx[q] >= 0 && H.midx[q] < n && H.agg[H.midx[q]] == I, "%s: member %d of aggregate %d", what, q, I);
            CHECK(q == H.mptr[I] || H.midx[q] > H.midx[q - 1], "%s: members of %d not ascending", what, I);
        }
    }
    // four-member records
    CHECK(upTo4 == !H.mem4.empty(), "%s: mem4 %s, every aggregate 1-4 members: %d", what, H.mem4.empty() ? "absent" : "present", (int)upTo4);
    if (upTo4) {
        CHECK(H.mem4.size() == (size_t)4 * nc, "%s: mem4 size", what);
        for (int I = 0; I < nc; ++I)
            for (int q = 0; q < 4; ++q) CHECK(H.mem4[(size_t)4 * I + q] == (q < members[I] ? H.midx[H.mptr[I] + q] : -1), "%s: mem4 of %d", what, I);
    }
    // the next level's pattern, its entries' places (cpos), and the Galerkin lists: every fine entry once, as its place in L's image, inside
    // the pair of aggregates of the coarse entry, in ascending entry order
    std::vector<int> crp, ccol, cposImg;
    image_csr(C, crp, ccol, cposImg);
    CHECK(H.cpos == cposImg, "%s: cpos is not the place of the next level's entries", what);
    const int nnzc = crp[nc];
    CHECK((int)H.gptr.size() == nnzc + 1 && H.gptr[0] == 0 && H.gptr[nnzc] == rowptr[n] && (int)H.gidx.size() == rowptr[n], "%s: Galerkin list sizes", what);
    std::vector<int> entryAt(L.ecol.size(), -1), rowOf(rowptr[n]);
    for (int i = 0; i < n; ++i)
        for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) { entryAt[pos[k]] = k; rowOf[k] = i; }
    std::vector<char> seen(rowptr[n], 0);
    for (int I = 0; I < nc; ++I)
        for (int e = crp[I]; e < crp[I + 1]; ++e) {
            CHECK(H.gptr[e + 1] > H.gptr[e], "%s: coarse entry %d gathers nothing", what, e);
            int last = -1;
            for (int q = H.gptr[e]; q < H.gptr[e + 1]; ++q) {
                const int p = H.gidx[q];
                CHECK(p >= 0 && p < (int)entryAt.size() && entryAt[p] >= 0, "%s: gidx[%d] = %d is no entry of the finer level", what, q, p);
                const int k = entryAt[p];
                CHECK(!seen[k] && k > last, "%s: fine entry %d gathered twice or out of order", what, k);
                seen[k] = 1;
                last = k;
                CHECK(H.agg[rowOf[k]] == I && H.agg[col[k]] == ccol[e], "%s: fine entry (%d, %d) in coarse entry (%d, %d)", what, rowOf[k], col[k], I, ccol[e]);
            }
        }
    return true;
}

// an ILU0 schedule: rows of colour cc in rowAt[off[cc] ..) as [step][sequence]; every row once; elimination position = colour-major, index
// order inside a colour.  Lower entries (mask, lorder) point to earlier positions, in ascending position; inside a colour they are the
// row's predecessors in its own sequence (what lets the sequences of a colour run in parallel)
static bool check_ilu(const char* what, const CprHostLevel& L, const CprIluHost& S) {
    const int n = L.n, nc = S.ncol;
    CHECK(S.error.empty(), "%s: %s", what, S.error.c_str());
    CHECK(nc >= 1 && (int)S.nseq.size() == nc && (int)S.nsteps.size() == nc && (int)S.off.size() == nc + 1 && S.off[0] == 0 && (int)S.rowAt.size() == S.off[nc], "%s: schedule sizes", what);
    std::vector<int> colour(n, -1), seq(n, -1), step(n, -1);
    for (int cc = 0; cc < nc; ++cc) {
        CHECK(S.off[cc + 1] - S.off[cc] == S.nseq[cc] * S.nsteps[cc], "%s: colour %d size", what, cc);
        for (int t = 0; t < S.nseq[cc]; ++t)
            for (int st = 0; st < S.nsteps[cc]; ++st) {
                const int i = S.rowAt[S.off[cc] + st * S.nseq[cc] + t];
                if (i < 0) continue;
                CHECK(i < n && colour[i] < 0, "%s: row %d scheduled twice", what, i);
                CHECK(st == 0 || S.rowAt[S.off[cc] + (st - 1) * S.nseq[cc] + t] >= 0, "%s: sequence %d of colour %d has a gap", what, t, cc);
                colour[i] = cc; seq[i] = t; step[i] = st;
            }
    }
    for (int i = 0; i < n; ++i) CHECK(colour[i] >= 0, "%s: row %d not scheduled", what, i);
    std::vector<int> order(n), posn(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return colour[a] < colour[b]; });
    for (int p = 0; p < n; ++p) posn[order[p]] = p;
    CHECK(S.MW == (L.W + 31) / 32 && S.mask.size() == (size_t)2 * S.MW * n && S.lorder.size() == (size_t)S.WL * n, "%s: mask / lorder sizes", what);
    CHECK((int)S.wl.size() == nc && (int)S.wu.size() == nc && (int)S.fast.size() == nc, "%s: per-colour sizes", what);
    auto bit = [&](int part, int j, int i) { return (S.mask[(size_t)(part * S.MW + (j >> 5)) * n + i] >> (j & 31)) & 1u; };
    for (int i = 0; i < n; ++i) {
        std::vector<std::pair<int, int>> low;
        int nu = 0;
        for (int j = 0; j < S.MW * 32; ++j) {
            const int c = j < L.rlen[i] ? L.ecol[at(L, j, i)] : i;
            const bool lo = c != i && posn[c] < posn[i], up = c != i && posn[c] > posn[i];
            CHECK(bit(0, j, i) == (unsigned)lo && bit(1, j, i) == (unsigned)up, "%s: mask of row %d slot %d", what, i, j);
            if (lo) {
                low.push_back({posn[c], j});
                CHECK(colour[c] < colour[i] || (seq[c] == seq[i] && step[c] < step[i]), "%s: lower entry (%d, %d) is not eliminated before its row", what, i, c);
            }
            if (up) {
                ++nu;
                CHECK(colour[c] > colour[i] || (seq[c] == seq[i] && step[c] > step[i]), "%s: upper entry (%d, %d) is not eliminated after its row", what, i, c);
            }
        }
        std::sort(low.begin(), low.end());
        CHECK((int)low.size() <= S.wl[colour[i]] && S.wl[colour[i]] <= S.WL && nu <= S.wu[colour[i]] && S.wu[colour[i]] <= S.WU, "%s: widths of row %d", what, i);
        for (int q = 0; q < S.WL; ++q)
            CHECK(S.lorder[(size_t)q * n + i] == (q < (int)low.size() ? low[q].second : 255), "%s: lorder of row %d", what, i);
        if (S.simple)
            for (int q = 0; q < (int)low.size(); ++q) {   // the place of the transposed entry (c, i)
                const int c = L.ecol[at(L, low[q].second, i)], t = S.tpos[(size_t)q * n + i];
                bool inRow = false;
                for (int u = 0; u < L.rlen[c]; ++u) inRow = inRow || t == (int)at(L, u, c);
                CHECK(inRow && L.ecol[t] == i, "%s: tpos of row %d entry %d", what, i, q);
            }
    }
    return true;
}

struct Case {
    std::string name;
    Mat A;                        // internal order
    std::vector<int> order;       // non-empty: natural id of every row (the matching visits them in natural order)
    std::vector<int> colourPrefix;   // non-empty: level 0's ILU0 colours (rows of colour c: [colourPrefix[c], colourPrefix[c + 1]))
};

static bool run(const Case& cs, int iluLevels, int lprRows, int stopRows, int& lines) {
    const Mat& A = cs.A;
    const int n = A.n;
    char what[256];
    // the pattern, as cpr_build_coarse_host reads it
    opmhip::Pattern P;
    P.Nb = n; P.Nghost = A.nghost; P.Nloc = n + A.nghost;
    P.rowptr = A.rowptr; P.col = A.col;
    if (!cs.order.empty()) {
        P.fromOrder = cs.order;
        P.toOrder.assign(n, -1);
        for (int p = 0; p < n; ++p) P.toOrder[cs.order[p]] = p;
    }
    // level 0's image (owned columns, as the device keeps it) and its value image W0 x Nb
    opmhip::HCsr A0;
    A0.n = n; A0.rowptr = A.rowptr; A0.col = A.col;
    CprHostLevel I0;
    std::vector<int> pos0;
    std::snprintf(what, sizeof what, "%s level 0 image", cs.name.c_str());
    CHECK(opmhip::ell_image(A0, I0, pos0, false, n), "%s: refused", what);
    if (!check_image(what, I0, A.rowptr, A.col, pos0, n)) return false;
    std::vector<double> ell0((size_t)I0.W * n, 0.0);
    for (int k = 0; k < (int)A.col.size(); ++k) ell0[pos0[k]] = A.val[k];
    if (!cs.colourPrefix.empty() && iluLevels > 0) {   // level 0's ILU0 schedule in the stored order, with the block ILU0's colours (cpr_setup_level0)
        const int ncol = (int)cs.colourPrefix.size() - 1;
        std::vector<int> posv(n), colour(n);
        for (int cc = 0; cc < ncol; ++cc)
            for (int p = cs.colourPrefix[cc]; p < cs.colourPrefix[cc + 1]; ++p) colour[p] = cc;
        std::iota(posv.begin(), posv.end(), 0);
        CprIluHost S;
        opmhip::cpr_ilu_schedule(I0, posv, colour, ncol, S);
        std::snprintf(what, sizeof what, "%s level 0 ILU0", cs.name.c_str());
        if (!check_ilu(what, I0, S)) return false;
    }
    CprHostCoarse H;
    opmhip::cpr_build_coarse_host(P, ell0, 0.25, lprRows, iluLevels, stopRows, H);
    std::snprintf(what, sizeof what, "%s ilu %d lpr %d stop %d", cs.name.c_str(), iluLevels, lprRows, stopRows);
    CHECK(H.error.empty(), "%s: %s", what, H.error.c_str());
    // the owned part of level 0: what the hierarchy is built from
    std::vector<int> rp(1, 0), cl, ps;
    orc::Csr O;
    O.n = n;
    O.rowptr.assign(1, 0);
    for (int i = 0; i < n; ++i) {
        for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k)
            if (A.col[k] < n) { cl.push_back(A.col[k]); ps.push_back(pos0[k]); O.col.push_back(A.col[k]); O.val.push_back(A.val[k]); }
        rp.push_back((int)cl.size());
        O.rowptr.push_back((int)O.col.size());
    }
    const int nlev = 1 + (int)H.lv.size();
    std::string sizes = std::to_string(n);
    for (int l = 0; l < nlev; ++l) {
        const CprHostLevel& T = l == 0 ? H.l0 : H.lv[l - 1];   // transfer part
        const CprHostLevel& L = l == 0 ? I0 : H.lv[l - 1];     // image
        char lw[300];
        std::snprintf(lw, sizeof lw, "%s level %d", what, l);
        if (l > 0) {
            sizes += " " + std::to_string(L.n);
            const bool iluLevel = l < iluLevels;
            CHECK(L.rm == (L.n <= lprRows && !iluLevel), "%s: row-major %d", lw, (int)L.rm);
            CHECK((L.ilu.ncol > 0) == iluLevel, "%s: ILU0 schedule %d", lw, L.ilu.ncol);
            if (iluLevel && !check_ilu(lw, L, L.ilu)) return false;
        }
        if (l + 1 == nlev) {
            CHECK(T.agg.empty() && T.gptr.empty() && T.cpos.empty(), "%s: the coarsest level has a transfer", lw);
            CHECK(H.lastA.n == L.n && H.lastPos == ps, "%s: last level's matrix", lw);
            if (l > 0) {   // the last level's matrix is the one its image holds
                std::vector<int> r2, c2, p2;
                image_csr(L, r2, c2, p2);
                CHECK(H.lastA.rowptr == r2 && H.lastA.col == c2, "%s: lastA is not the level's pattern", lw);
            }
            break;
        }
        const CprHostLevel& C = H.lv[l];
        if (!check_transfer(lw, T, L.n, rp, cl, ps, L, C)) return false;
        image_csr(C, rp, cl, ps);
        if (!check_image(lw, C, rp, cl, ps, INT_MAX)) return false;
    }
    // stop rules
    const CprHostLevel& last = nlev == 1 ? I0 : H.lv.back();
    const char* why = last.n <= stopRows ? "rows" : nlev >= opmhip::CPR_MAX_LEVELS ? "levels" : "stall or width";
    // the oracle on the same matrix
    orc::CprAmg R;
    R.stopRows = stopRows;
    if (!cs.order.empty()) { R.natOf = P.fromOrder; R.atNat = P.toOrder; }
    R.setup_structure(O);
    CHECK((int)R.lv.size() == nlev, "%s: %d levels, the oracle %zu", what, nlev, R.lv.size());
    for (int l = 0; l < nlev; ++l) {
        const CprHostLevel& T = l == 0 ? H.l0 : H.lv[l - 1];
        const int nl = l == 0 ? n : H.lv[l - 1].n;
        CHECK(R.lv[l].A.n == nl && R.lv[l].nc == T.nc && R.lv[l].agg == T.agg, "%s level %d: n %d nc %d against the oracle's %d %d, aggregates %s", what, l, nl,
              T.nc, R.lv[l].A.n, R.lv[l].nc, R.lv[l].agg == T.agg ? "equal" : "differ");
    }
    const orc::Csr& RC = R.lv.back().A;
    CHECK(RC.rowptr == H.lastA.rowptr && RC.col == H.lastA.col && RC.val == H.lastA.val, "%s: the coarsest matrix differs from the oracle's", what);
    if (std::string(why) == "stall or width") {   // which of the two: the oracle's matching replayed on the last level
        std::vector<int> a1, a2, g1p, g1i;
        int n1 = 0, n2 = 0;
        orc::Csr A1;
        for (int attempt = 0; attempt < 3; ++attempt) {
            const double b = attempt == 0 ? R.beta : 0.0;
            const bool lvl0 = nlev == 1 && !R.natOf.empty();
            orc::CprAmg::pairwise(RC, b, attempt == 2, false, a1, n1, lvl0 ? R.natOf.data() : nullptr, lvl0 ? R.atNat.data() : nullptr);
            orc::CprAmg::galerkin(RC, a1, n1, A1, g1p, g1i);
            orc::CprAmg::pairwise(A1, b, attempt == 2, false, a2, n2);
            if (n2 <= (int)(0.5 * RC.n)) break;
        }
        why = n2 >= (int)(0.8 * RC.n) ? "stall" : "width";
    }
    std::printf("ok  %-48s levels %2d: %s (last: %s); oracle agrees: levels, n, nc, agg, coarsest matrix\n", what, nlev, sizes.c_str(), why);
    ++lines;
    return true;
}

int main() {
    std::vector<Case> cases;
    for (int s : {1, 2, 3, 5, 8, 13}) cases.push_back({"grid " + std::to_string(s) + "^3", grid7(s, s, s, true, 10u + s), {}, {}});
    cases.push_back({"grid 30x20x10 uniform", grid7(30, 20, 10, false, 1u), {}, {}});
    cases.push_back({"grid 40x40x40", grid7(40, 40, 40, true, 2u), {}, {}});   // first coarse level > 4096 rows: galerkin's threads
    cases.push_back({"grid 17x10x6 ghosts", grid7(17, 10, 6, true, 3u, 12), {}, {}});
    {
        Case c;
        c.name = "grid 24x18x9 line-coloured, uniform";
        const Mat nat = grid7(24, 18, 9, false, 4u);
        c.order = line_colour_order(24, 18, 9, c.colourPrefix);
        c.A = permuted(nat, c.order);
        cases.push_back(c);
        Case h;
        h.name = "grid 24x18x9 line-coloured";
        const Mat nat2 = grid7(24, 18, 9, true, 5u);
        h.order = line_colour_order(24, 18, 9, h.colourPrefix);
        h.A = permuted(nat2, h.order);
        cases.push_back(h);
    }
    cases.push_back({"long rows deg 24", long_rows(6000, 24, 400, 6u), {}, {}});
    cases.push_back({"long rows deg 60", long_rows(3000, 60, 2000, 7u), {}, {}});
    int lines = 0, runs = 0;
    for (const Case& cs : cases)
        for (int ilu : {0, 2})
            for (int lpr : {0, opmhip::CPR_LPR_ROWS})
                for (int stop : {opmhip::CPR_COARSE_DIRECT, 1500}) {
                    ++runs;
                    run(cs, ilu, lpr, stop, lines);
                }
    std::printf("%d of %d set-ups checked\n", lines, runs);
    if (g_fail == 0 && lines == runs) std::printf("all checks passed\n");
    return g_fail == 0 && lines == runs ? 0 : 1;
}
