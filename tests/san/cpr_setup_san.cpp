// Host set-up of the CPR pressure AMG (csrc/cpr_setup.cpp: pairwise matching, Galerkin gather lists, ELL images, ILU0 smoothing schedules,
// colourings) under AddressSanitizer + UBSan + libstdc++'s container assertions (test infrastructure; built and run by
// tests/test_host_logic_sanitized.py with g++, no GPU).  cpr_setup.cpp is linked alone, with no stand-in for any HIP runtime call: that the
// link succeeds is the check that the set-up half of the library - which runs on a host thread of its own beside the solves - makes none.
// Per level of every hierarchy the harness checks what the uploads and kernels of cpr.hip rely on: the aggregates are onto [0, nc), the
// member lists invert them, the four-member records are there exactly when every aggregate has 1-4 members, the Galerkin lists cover every
// entry of the finer level once (as places in its ELL image, each inside the right pair of aggregates), every image decodes back to its CSR
// matrix, and every ILU0 schedule is an elimination order its sweeps may run in parallel.  The hierarchy is compared with the oracle's
// (oracle/cpr.hpp: CprAmg::setup_structure on the same matrix): the same levels, sizes and aggregates, the same coarsest matrix bit for bit.
// The joined level of a decomposed run (cpr_joined_aggregates, cpr_joined_rows, cpr_joined_values, cpr_join_rows) is run on small worlds of
// ranks and compared with the Galerkin product of the whole system's matrix; cpr_join_rows is fed buffers a peer has spoiled (run_world, refuses).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <map>
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
        CprIluHost S;
        opmhip::cpr_level0_ilu_schedule(I0, cs.colourPrefix, (int)cs.colourPrefix.size() - 1, S);
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

// ---- the joined level of a decomposed run: cpr_joined_aggregates, cpr_joined_rows, cpr_joined_values, cpr_join_rows ---------------------
// A world: a whole system's pressure matrix (natural order) and the rank that owns every cell.  Every rank numbers its owned cells in
// ascending natural id (reversedLast: the last rank in descending id - its internal order is then not the natural one) and its ghost cells
// behind them, coarsens its owned part down to stopRows and forms its rows of the joined level; the ghost information is taken straight
// from the owners, which is what the halo exchange of cpr_gather_setup delivers.
// Summation order of a joined entry between two ranks: the product's rule is (owned row in my internal order, owner-side place of the
// column).  The oracle (oracle_capi.cpp: orc_cpr_solve_blocks) sums in ascending (row, column) of the matrix it is handed; the GPU tests
// hand it the whole system numbered rank by rank in each rank's internal order (tests/test_gpu_dd.py: frg), where the two orders are one.
// The restatement below numbers the whole system the same way (place = first place of the owner + internal index) and sums in ascending
// (row place, column place): the product's rule holds, and the reversed world shows that it is the place, not the natural id, that orders.
struct World {
    std::string name;
    Mat A;
    std::vector<int> owner;
    int nr = 0, stopRows = 8;
    bool reversedLast = false;
    int wantLevels = -1;        // 0: level 0 itself is joined; 2: at least two transfers are composed; -1: whatever comes
    bool wantShared = false;    // some joined entry sums several fine couplings
    bool wantNoCoupling = false;
};
static World box_world(const std::string& name, int nx, int ny, int nz, std::vector<int> xcuts, std::vector<int> ycuts, unsigned seed, int stopRows) {
    World w;
    w.name = name;
    w.A = grid7(nx, ny, nz, true, seed);
    w.stopRows = stopRows;
    auto part = [](const std::vector<int>& cuts, int v) { int p = 0; for (int c : cuts) p += v >= c; return p; };
    const int npx = (int)xcuts.size() + 1;
    w.nr = npx * ((int)ycuts.size() + 1);
    w.owner.resize(w.A.n);
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) w.owner[i + nx * (j + ny * k)] = part(xcuts, i) + npx * part(ycuts, j);
    return w;
}
static World two_slabs(const std::string& name, unsigned seed) {
    World w;
    w.name = name;
    const Mat a = grid7(3, 4, 3, true, seed), b = grid7(4, 3, 3, true, seed + 1);
    std::vector<std::vector<std::pair<int, double>>> rows(a.n + b.n);
    for (int i = 0; i < a.n; ++i)
        for (int k = a.rowptr[i]; k < a.rowptr[i + 1]; ++k) rows[i].push_back({a.col[k], a.val[k]});
    for (int i = 0; i < b.n; ++i)
        for (int k = b.rowptr[i]; k < b.rowptr[i + 1]; ++k) rows[a.n + i].push_back({a.n + b.col[k], b.val[k]});
    w.A = from_rows(a.n + b.n, 0, rows);
    w.owner.assign(a.n + b.n, 1);
    std::fill(w.owner.begin(), w.owner.begin() + a.n, 0);
    w.nr = 2;
    w.wantNoCoupling = true;
    return w;
}
struct RankSide {
    Mat M;                       // the local pattern with values
    std::vector<int> cells, ghosts;   // natural id of every owned cell (internal order) and of every ghost cell
    CprHostCoarse H;
    std::vector<int> cagg;
    opmhip::CprJoinedRows Q;
    std::vector<double> vals;
};
// the padded buffers every rank holds after the exchanges of step 5
struct Gathered {
    std::vector<int> bl, bc, nnzs, offs;
    std::vector<double> bv;
    int maxn = 1, maxnnz = 1;
};
static bool run_world(const World& w, Gathered& out, int& lines) {
    const Mat& A = w.A;
    const int N = A.n, nr = w.nr;
    const char* what = w.name.c_str();
    std::vector<RankSide> R(nr);
    std::vector<int> local(N);
    for (int i = 0; i < N; ++i) R[w.owner[i]].cells.push_back(i);
    if (w.reversedLast) std::reverse(R[nr - 1].cells.begin(), R[nr - 1].cells.end());
    for (int r = 0; r < nr; ++r)
        for (int q = 0; q < (int)R[r].cells.size(); ++q) local[R[r].cells[q]] = q;
    int levelsMax = 0, levelsMin = INT_MAX;
    for (int r = 0; r < nr; ++r) {   // every rank's subdomain and hierarchy
        RankSide& S = R[r];
        const int n = (int)S.cells.size();
        CHECK(n > 0, "%s: rank %d owns nothing", what, r);
        std::set<int> gs;
        for (int i : S.cells)
            for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k)
                if (w.owner[A.col[k]] != r) gs.insert(A.col[k]);
        S.ghosts.assign(gs.begin(), gs.end());
        std::vector<std::vector<std::pair<int, double>>> rows(n);
        for (int q = 0; q < n; ++q)
            for (int k = A.rowptr[S.cells[q]]; k < A.rowptr[S.cells[q] + 1]; ++k) {
                const int j = A.col[k];
                const int lc = w.owner[j] == r ? local[j] : n + (int)(std::lower_bound(S.ghosts.begin(), S.ghosts.end(), j) - S.ghosts.begin());
                rows[q].push_back({lc, A.val[k]});
            }
        S.M = from_rows(n, (int)S.ghosts.size(), rows);
        opmhip::Pattern P;
        P.Nb = n; P.Nghost = S.M.nghost; P.Nloc = n + S.M.nghost;
        P.rowptr = S.M.rowptr; P.col = S.M.col;
        opmhip::HCsr A0;
        A0.n = n; A0.rowptr = S.M.rowptr; A0.col = S.M.col;
        CprHostLevel I0;
        std::vector<int> pos0;
        CHECK(opmhip::ell_image(A0, I0, pos0, false, n), "%s: level 0 of rank %d refused", what, r);
        std::vector<double> ell0((size_t)I0.W * n, 0.0);
        for (int k = 0; k < (int)S.M.col.size(); ++k) ell0[pos0[k]] = S.M.val[k];
        opmhip::cpr_build_coarse_host(P, ell0, 0.25, opmhip::CPR_LPR_ROWS, 0, w.stopRows, S.H);
        CHECK(S.H.error.empty(), "%s: rank %d: %s", what, r, S.H.error.c_str());
        const int g = (int)S.H.lv.size(), nlast = S.H.lastA.n;
        levelsMax = std::max(levelsMax, g); levelsMin = std::min(levelsMin, g);
        S.cagg = opmhip::cpr_joined_aggregates(n, S.H);
        CHECK((int)S.cagg.size() == n, "%s: cagg size of rank %d", what, r);
        std::vector<int> members(nlast, 0);
        for (int q = 0; q < n; ++q) {   // the transfers applied one after the other, restated cell by cell
            int a = q;
            for (int l = 0; l < g; ++l) a = (l == 0 ? S.H.l0.agg : S.H.lv[l - 1].agg)[a];
            CHECK(S.cagg[q] == a && a >= 0 && a < nlast, "%s: cagg[%d] of rank %d is %d, not %d", what, q, r, S.cagg[q], a);
            ++members[a];
        }
        for (int I = 0; I < nlast; ++I) CHECK(members[I] > 0, "%s: row %d of rank %d's last level has no cell", what, I, r);
    }
    CHECK(w.wantLevels != 0 || levelsMax == 0, "%s: level 0 was to be the joined one, %d transfers", what, levelsMax);
    CHECK(w.wantLevels != 2 || levelsMin >= 2, "%s: at least two transfers were to be composed, %d", what, levelsMin);
    Gathered& G = out;
    G = Gathered();
    G.offs.assign(nr + 1, 0);
    std::vector<int> foffs(nr + 1, 0);
    for (int r = 0; r < nr; ++r) {
        G.offs[r + 1] = G.offs[r] + R[r].H.lastA.n;
        foffs[r + 1] = foffs[r] + (int)R[r].cells.size();
        G.maxn = std::max(G.maxn, R[r].H.lastA.n);
    }
    const int NG = G.offs[nr];
    auto place = [&](int i) { return foffs[w.owner[i]] + local[i]; };                        // of a cell in the whole system, rank by rank
    auto joined = [&](int i) { return G.offs[w.owner[i]] + R[w.owner[i]].cagg[local[i]]; };   // its row of the joined level
    int nqAll = 0, longest = 0;
    for (int r = 0; r < nr; ++r) {   // every rank's rows of the joined level
        RankSide& S = R[r];
        const Mat& M = S.M;
        const int n = M.n, nlast = S.H.lastA.n;
        std::vector<int> ghostRow(S.ghosts.size());
        std::vector<long long> ghostPlace(S.ghosts.size());
        for (size_t gI = 0; gI < S.ghosts.size(); ++gI) { ghostRow[gI] = joined(S.ghosts[gI]); ghostPlace[gI] = place(S.ghosts[gI]); }
        opmhip::CprJoinedRows& Q = S.Q;
        opmhip::cpr_joined_rows(n, M.rowptr, M.col, S.cagg, ghostRow, ghostPlace, G.offs[r], S.H.lastA, S.H.lastPos, Q);
        const int nq = (int)Q.qrow.size(), nnzloc = (int)Q.cols.size();
        nqAll += nq;
        // the couplings to ghost cells, in entry order
        CHECK(Q.qentry.size() == Q.qrow.size(), "%s: rank %d: qrow / qentry sizes", what, r);
        int q = 0;
        for (int i = 0; i < n; ++i)
            for (int k = M.rowptr[i]; k < M.rowptr[i + 1]; ++k)
                if (M.col[k] >= n) { CHECK(q < nq && Q.qrow[q] == i && Q.qentry[q] == k, "%s: rank %d: ghost coupling %d", what, r, q); ++q; }
        CHECK(q == nq, "%s: rank %d: %d ghost couplings listed, the pattern has %d", what, r, nq, q);
        CHECK((int)Q.rowlen.size() == nlast && (int)Q.src.size() == nnzloc && !Q.xptr.empty() && Q.xptr[0] == 0 && Q.xptr.back() == (int)Q.xidx.size(),
              "%s: rank %d: sizes of its rows", what, r);
        CHECK(std::accumulate(Q.rowlen.begin(), Q.rowlen.end(), 0) == nnzloc, "%s: rank %d: rowlen does not sum to nnzloc", what, r);
        std::vector<int> seen(nq, 0);
        int e = 0, x = 0;
        for (int I = 0; I < nlast; ++I) {
            int k = S.H.lastA.rowptr[I];
            for (int t = 0; t < Q.rowlen[I]; ++t, ++e) {
                CHECK(t == 0 || Q.cols[e] > Q.cols[e - 1], "%s: rank %d row %d: columns do not ascend", what, r, I);
                CHECK(Q.cols[e] >= 0 && Q.cols[e] < NG, "%s: rank %d row %d: column %d", what, r, I, Q.cols[e]);
                if (Q.src[e] >= 0) {   // an entry of my last level: the next one of its row, at its place in the level's image
                    CHECK(k < S.H.lastA.rowptr[I + 1] && Q.src[e] == S.H.lastPos[k] && Q.cols[e] == G.offs[r] + S.H.lastA.col[k], "%s: rank %d row %d: own entry %d", what, r, I, t);
                    ++k;
                    continue;
                }
                CHECK(Q.src[e] == -1 - x && x + 1 < (int)Q.xptr.size() && Q.xptr[x + 1] > Q.xptr[x], "%s: rank %d row %d: cross entry %d", what, r, I, x);
                CHECK(Q.cols[e] < G.offs[r] || Q.cols[e] >= G.offs[r + 1], "%s: rank %d row %d: a cross entry inside my slice", what, r, I);
                longest = std::max(longest, Q.xptr[x + 1] - Q.xptr[x]);
                for (int u = Q.xptr[x]; u < Q.xptr[x + 1]; ++u) {
                    const int qq = Q.xidx[u];
                    CHECK(qq >= 0 && qq < nq && !seen[qq], "%s: rank %d: xidx[%d] = %d twice or out of range", what, r, u, qq);
                    seen[qq] = 1;
                    const int gh = M.col[Q.qentry[qq]] - n;
                    CHECK(S.cagg[Q.qrow[qq]] == I && ghostRow[gh] == Q.cols[e], "%s: rank %d: coupling %d in the wrong joined entry", what, r, qq);
                    if (u > Q.xptr[x]) {
                        const int qp = Q.xidx[u - 1];
                        const long long pp = ghostPlace[M.col[Q.qentry[qp]] - n], pn = ghostPlace[gh];
                        CHECK(Q.qrow[qp] < Q.qrow[qq] || (Q.qrow[qp] == Q.qrow[qq] && pp < pn), "%s: rank %d: couplings of cross entry %d out of order", what, r, x);
                    }
                }
                ++x;
            }
            CHECK(k == S.H.lastA.rowptr[I + 1], "%s: rank %d row %d: own entries missing", what, r, I);
        }
        CHECK(x + 1 == (int)Q.xptr.size(), "%s: rank %d: cross entries", what, r);
        for (int qq = 0; qq < nq; ++qq) CHECK(seen[qq], "%s: rank %d: ghost coupling %d is in no joined entry", what, r, qq);
        // values: the pressure value of a coupling of this scalar system is the entry itself
        std::vector<double> apg(std::max(nq, 1), 0.0);
        for (int qq = 0; qq < nq; ++qq) apg[qq] = M.val[Q.qentry[qq]];
        S.vals = opmhip::cpr_joined_values(Q, apg, S.H.lastA.val);
        CHECK((int)S.vals.size() == nnzloc, "%s: rank %d: values", what, r);
        G.nnzs.push_back(nnzloc);
        G.maxnnz = std::max(G.maxnnz, nnzloc);
    }
    CHECK(!w.wantNoCoupling || nqAll == 0, "%s: %d couplings between the slabs", what, nqAll);
    CHECK(w.wantNoCoupling || nqAll > 0, "%s: no coupling between the ranks", what);
    CHECK(!w.wantShared || longest >= 2, "%s: no joined entry sums more than one coupling", what);
    // step 5's buffers, and the joined matrix from them
    G.bl.assign((size_t)nr * G.maxn, 0); G.bc.assign((size_t)nr * G.maxnnz, 0); G.bv.assign((size_t)nr * G.maxnnz, 0.0);
    for (int r = 0; r < nr; ++r) {
        std::copy(R[r].Q.rowlen.begin(), R[r].Q.rowlen.end(), G.bl.begin() + (size_t)r * G.maxn);
        std::copy(R[r].Q.cols.begin(), R[r].Q.cols.end(), G.bc.begin() + (size_t)r * G.maxnnz);
        std::copy(R[r].vals.begin(), R[r].vals.end(), G.bv.begin() + (size_t)r * G.maxnnz);
    }
    opmhip::CprJoined JR;
    opmhip::cpr_join_rows(G.bl, G.bc, G.bv, G.nnzs, G.offs, G.maxn, G.maxnnz, JR);
    CHECK(JR.error.empty(), "%s: %s", what, JR.error.c_str());
    const opmhip::HCsr& J = JR.J;
    CHECK(J.n == NG && (int)J.rowptr.size() == NG + 1 && (int)JR.unpad.size() == NG && JR.vunpad.size() == J.col.size() && J.val.size() == J.col.size(), "%s: sizes of the joined matrix", what);
    for (int r = 0; r < nr; ++r)   // unpad / vunpad invert the padding
        for (int I = 0, e = 0; I < G.offs[r + 1] - G.offs[r]; ++I) {
            CHECK(JR.unpad[G.offs[r] + I] == r * G.maxn + I, "%s: unpad of row %d of rank %d", what, I, r);
            for (int k = J.rowptr[G.offs[r] + I]; k < J.rowptr[G.offs[r] + I + 1]; ++k, ++e)
                CHECK(JR.vunpad[k] == r * G.maxnnz + e && J.col[k] == R[r].Q.cols[e] && J.val[k] == R[r].vals[e], "%s: vunpad of entry %d of rank %d", what, e, r);
        }
    // the Galerkin product of the whole system's matrix with the composed aggregates, map of maps, rows and columns in ascending place
    struct Sum { double v, abs; int terms; bool cross; };
    std::vector<std::map<int, Sum>> prod(NG);
    std::vector<int> cellAt(N);
    for (int i = 0; i < N; ++i) cellAt[place(i)] = i;
    for (int p = 0; p < N; ++p) {
        const int i = cellAt[p];
        std::vector<std::pair<int, int>> ent;
        for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) ent.push_back({place(A.col[k]), k});
        std::sort(ent.begin(), ent.end());
        for (const auto& en : ent) {
            const int j = A.col[en.second];
            const double a = A.val[en.second];
            auto it = prod[joined(i)].find(joined(j));
            if (it == prod[joined(i)].end()) prod[joined(i)][joined(j)] = Sum{0.0 + a, std::fabs(a), 1, w.owner[i] != w.owner[j]};
            else { it->second.v += a; it->second.abs += std::fabs(a); ++it->second.terms; }
        }
    }
    int nCross = 0;
    for (int I = 0; I < NG; ++I) {
        CHECK(J.rowptr[I + 1] - J.rowptr[I] == (int)prod[I].size(), "%s: row %d of the joined matrix has %d entries, the product %zu", what, I, J.rowptr[I + 1] - J.rowptr[I], prod[I].size());
        int k = J.rowptr[I];
        for (const auto& en : prod[I]) {
            CHECK(J.col[k] == en.first, "%s: row %d of the joined matrix: column %d, the product's %d", what, I, J.col[k], en.first);
            const Sum& s = en.second;
            // between two ranks: the same additions in the same order, bit for bit.  Inside a rank the entry is the last level's, a sum of
            // the partial sums of every level in between: equal up to the rounding of `terms` additions of numbers summing to `abs` in size
            if (s.cross) { CHECK(J.val[k] == s.v, "%s: joined entry (%d, %d): %.17g, the product in the stated order %.17g", what, I, en.first, J.val[k], s.v); ++nCross; }
            else CHECK(std::fabs(J.val[k] - s.v) <= s.terms * 2.220446049250313e-16 * s.abs, "%s: joined entry (%d, %d): %.17g, the product %.17g", what, I, en.first, J.val[k], s.v);
            ++k;
        }
    }
    std::printf("ok  joined level of %-44s ranks %d, transfers %d..%d, rows %d, entries %zu (%d between ranks, longest sum %d), ghost couplings %d: pattern and values are the whole system's Galerkin product\n",
                what, nr, levelsMin, levelsMax, NG, J.col.size(), nCross, longest, nqAll);
    ++lines;
    return true;
}
// cpr_join_rows on buffers a peer has spoiled: refused with the rank named, no index followed out of its slice
static bool refuses(const char* what, const Gathered& G, int rank, int& lines) {
    opmhip::CprJoined JR;
    opmhip::cpr_join_rows(G.bl, G.bc, G.bv, G.nnzs, G.offs, G.maxn, G.maxnnz, JR);
    const std::string want = "cpr: the joined level's rows of rank " + std::to_string(rank) + " are inconsistent";
    CHECK(JR.error == want, "%s: \"%s\", not \"%s\"", what, JR.error.c_str(), want.c_str());
    std::printf("ok  refused: %s (rank %d)\n", what, rank);
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
    // the joined level: the smallest worlds that reach every branch
    std::vector<World> worlds;
    worlds.push_back(box_world("6x4x3 cut in two along x", 6, 4, 3, {3}, {}, 21u, 8));
    worlds.push_back(box_world("8x4x3 cut at x = 5", 8, 4, 3, {5}, {}, 22u, 8));                 // uneven slices: both paddings are real
    worlds.push_back(box_world("8x4x3 cut at x = 3", 8, 4, 3, {3}, {}, 22u, 8));                 // the last rank has the largest slice
    worlds.push_back(box_world("8x8x4 in 2 x 2 ranks", 8, 8, 4, {4}, {4}, 23u, 8));              // two neighbours per rank, shared joined entries
    worlds.back().wantShared = true;
    worlds.push_back(worlds.back());
    worlds.back().name = "8x8x4 in 2 x 2 ranks, last rank reversed";
    worlds.back().reversedLast = true;
    worlds.push_back(two_slabs("two slabs without a coupling", 24u));
    worlds.push_back(box_world("6x4x3, stopRows above the subdomains", 6, 4, 3, {3}, {}, 25u, 1000));
    worlds.back().wantLevels = 0;
    worlds.push_back(box_world("8x8x4 in 2 x 2 ranks, stopRows 4", 8, 8, 4, {4}, {4}, 26u, 4));
    worlds.back().wantLevels = 2;
    int wlines = 0, rlines = 0;
    Gathered uneven, mirrored;
    for (const World& w : worlds) {
        Gathered G;
        run_world(w, G, wlines);
        if (w.name == "8x4x3 cut at x = 5") uneven = G;
        if (w.name == "8x4x3 cut at x = 3") mirrored = G;
    }
    std::printf("%d of %zu joined levels checked\n", wlines, worlds.size());
    const int nrefusals = 6;
    if (uneven.nnzs.size() == 2 && uneven.nnzs[0] != uneven.nnzs[1] && mirrored.nnzs.size() == 2 && mirrored.nnzs[1] == mirrored.maxnnz) {
        const int big = uneven.nnzs[0] > uneven.nnzs[1] ? 0 : 1, small = 1 - big;   // big fills its slice: behind rank 1's lies the end of the buffer
        const int lastRow = mirrored.offs[2] - mirrored.offs[1] - 1;
        Gathered G = uneven;
        G.bc[(size_t)small * G.maxnnz + 1] = G.offs[2];
        refuses("a column >= NG", G, small, rlines);
        G = uneven;
        G.bc[(size_t)big * G.maxnnz] = -1;
        refuses("a negative column", G, big, rlines);
        G = uneven;
        G.bl[(size_t)small * G.maxn] += 1;   // (still inside the padded slice: only nnzs tells)
        refuses("a row length running past nnzs[r]", G, small, rlines);
        G = mirrored;
        G.bl[(size_t)1 * G.maxn + lastRow] += G.maxnnz;   // the last row of the last rank, which fills its slice: followed, it leaves the gathered buffer
        refuses("a row length running past maxnnz", G, 1, rlines);
        G = uneven;
        G.bl[(size_t)big * G.maxn] = -1;
        refuses("a negative row length", G, big, rlines);
        G = uneven;
        G.nnzs[small] = G.maxnnz + 1;
        refuses("more entries than the slice holds", G, small, rlines);
    }
    std::printf("%d of %d spoiled buffers refused\n", rlines, nrefusals);
    const bool all = g_fail == 0 && lines == runs && wlines == (int)worlds.size() && rlines == nrefusals;
    if (all) std::printf("all checks passed\n");
    return all ? 0 : 1;
}
