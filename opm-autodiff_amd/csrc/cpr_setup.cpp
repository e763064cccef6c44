// Host side of the CPR pressure-AMG set-up (cpr_setup.hpp): two passes of pairwise matching per level, Galerkin gather lists, ELL
// images of the levels, ILU0 smoothing schedules and colourings.  Mirrors oracle/cpr.hpp (CprAmg::setup_structure: same matching, same
// lists, same stops), and the index work of the level that joins the ranks of a decomposed run.  No HIP call: cpr.hip uploads what is
// built here.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <map>
#include <numeric>
#include <string>
#include <thread>
#include <utility>

#include "internal.hpp"

namespace opmhip {

namespace {
// natOf / atNat (level 0 only, else NULL): natural id of every internal index and its inverse - the cells are visited in
// NATURAL order, ties to the lowest natural id: the aggregates of the natural-order matrix whatever the ILU ordering is
// (matching colour by colour pairs cells across the grid and stalls after five levels; oracle/cpr.hpp: same statements)
void pairwise(const HCsr& A, double beta, bool anySign, std::vector<int>& agg, int& na, const int* natOf = nullptr, const int* atNat = nullptr) {
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
        agg[i] = na;
        if (best >= 0) agg[best] = na;
        ++na;
    }
}
// Galerkin product for piecewise-constant prolongation: coarse pattern (columns ascending), gather lists (fine entries of a
// coarse entry in ascending order), values.  Row by row over the members of each aggregate: the few (coarse column, fine
// entry) pairs of a coarse row are sorted on the spot - O(nnz log(row)) instead of a stable sort of all nnz keys (round 2: 1.5 s
// of host time for the hierarchy of a 10^6-cell grid, most of it here); same lists, same sums, same order.
void galerkin(const HCsr& A, const std::vector<int>& agg, int nc, HCsr& C, std::vector<int>& gptr, std::vector<int>& gidx) {
    const int nnz = (int)A.col.size();
    std::vector<int> mp(nc + 1, 0), mi(A.n);
    for (int i = 0; i < A.n; ++i) mp[agg[i] + 1]++;
    for (int I = 0; I < nc; ++I) mp[I + 1] += mp[I];
    {
        std::vector<int> w(mp.begin(), mp.end() - 1);
        for (int i = 0; i < A.n; ++i) mi[w[agg[i]]++] = i;   // members ascending
    }
    // the coarse rows are independent: slices of them are built by a few host threads, each into vectors of its own, and
    // joined in order - the same lists and sums whatever the number of threads
    const int T = std::max(1, std::min({(int)std::thread::hardware_concurrency(), 8, nc / 4096 + 1}));
    struct Part { std::vector<int> rowlen, col, glen, gidx; std::vector<double> val; };
    std::vector<Part> parts(T);
    auto work = [&](int t) {
        Part& Q = parts[t];
        const int I0 = (int)((long long)nc * t / T), I1 = (int)((long long)nc * (t + 1) / T);
        std::vector<std::pair<int, int>> pairs;   // (coarse column, fine entry) of the coarse row in hand
        Q.rowlen.reserve(I1 - I0);
        for (int I = I0; I < I1; ++I) {
            pairs.clear();
            for (int q = mp[I]; q < mp[I + 1]; ++q) {
                const int i = mi[q];
                for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) pairs.emplace_back(agg[A.col[k]], k);
            }
            std::sort(pairs.begin(), pairs.end());
            int len = 0;
            for (size_t q = 0; q < pairs.size();) {
                const int cc = pairs[q].first;
                double sum = 0.0;
                size_t e = q;
                while (e < pairs.size() && pairs[e].first == cc) { sum += A.val[pairs[e].second]; Q.gidx.push_back(pairs[e].second); ++e; }
                Q.col.push_back(cc);
                Q.val.push_back(sum);
                Q.glen.push_back((int)(e - q));
                ++len;
                q = e;
            }
            Q.rowlen.push_back(len);
        }
    };
    if (T == 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < T; ++t) th.emplace_back(work, t);
        for (auto& x : th) x.join();
    }
    C.n = nc;
    C.rowptr.assign(nc + 1, 0);
    C.col.clear();
    C.val.clear();
    gptr.assign(1, 0);
    gidx.clear();
    gidx.reserve(nnz);
    int I = 0;
    for (const Part& Q : parts) {
        for (int len : Q.rowlen) { C.rowptr[I + 1] = C.rowptr[I] + len; ++I; }
        C.col.insert(C.col.end(), Q.col.begin(), Q.col.end());
        C.val.insert(C.val.end(), Q.val.begin(), Q.val.end());
        for (int gl : Q.glen) gptr.push_back(gptr.back() + gl);
        gidx.insert(gidx.end(), Q.gidx.begin(), Q.gidx.end());
    }
}
}  // namespace

bool ell_image(const HCsr& A, CprHostLevel& L, std::vector<int>& pos, bool rowMajor, int ncols) {
    const int n = A.n;
    int W = 1;
    for (int i = 0; i < n; ++i) W = std::max(W, A.rowptr[i + 1] - A.rowptr[i]);
    L.n = n; L.nnz = (int)A.col.size(); L.W = W; L.rm = rowMajor;
    if (W > CPR_MAX_W) return false;
    // entry j of row i: [j * n + i] (one thread per row reads coalesced) or, row-major, [i * W + j] (a group of lanes per row does)
    auto at = [&](int j, int i) { return rowMajor ? (size_t)i * W + j : (size_t)j * n + i; };
    L.ecol.assign((size_t)W * n, 0); L.rlen.assign(n, 0); L.diag.assign(n, 0);
    pos.resize(A.col.size());
    for (int i = 0; i < n; ++i) {
        const int kb = A.rowptr[i], len = A.rowptr[i + 1] - kb;
        L.rlen[i] = len;
        for (int j = 0; j < W; ++j) L.ecol[at(j, i)] = (j < len && A.col[kb + j] < ncols) ? A.col[kb + j] : i;   // padding and ghost columns (value 0 for good): the row itself
        for (int j = 0; j < len; ++j) {
            pos[kb + j] = (int)at(j, i);
            if (A.col[kb + j] == i) L.diag[i] = (int)at(j, i);
        }
    }
    return true;
}

void cpr_ilu_schedule(const CprHostLevel& L, const std::vector<int>& pos, const std::vector<int>& colour, int ncol, CprIluHost& S) {
    const int n = L.n, W = L.W;
    auto at = [&](int j, int i) { return L.rm ? (size_t)i * W + j : (size_t)j * n + i; };
    S.ncol = ncol;
    S.MW = (W + 31) / 32;
    S.mask.assign((size_t)2 * S.MW * n, 0u);
    std::vector<std::vector<std::pair<int, int>>> low(n);   // (position, slot) of every lower entry
    int WL = 0;
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < L.rlen[i]; ++j) {
            const int c = L.ecol[at(j, i)];
            if (c == i) continue;   // the diagonal, or a ghost column's slot (value 0 for good)
            if (pos[c] < pos[i]) { S.mask[(size_t)(j >> 5) * n + i] |= 1u << (j & 31); low[i].emplace_back(pos[c], j); }
            else S.mask[(size_t)(S.MW + (j >> 5)) * n + i] |= 1u << (j & 31);
        }
        std::sort(low[i].begin(), low[i].end());
        WL = std::max(WL, (int)low[i].size());
    }
    S.WL = std::max(WL, 1);
    if (W > 254) { S.error = "cpr: ILU0 smoothing of a level with rows of more than 254 entries"; return; }
    S.lorder.assign((size_t)S.WL * n, 255);
    for (int i = 0; i < n; ++i)
        for (size_t q = 0; q < low[i].size(); ++q) S.lorder[q * n + i] = (unsigned char)low[i][q].second;
    // sequences: rows of a colour in ascending position; a row with a lower entry of its own colour continues that row's sequence
    std::vector<int> byPos(n);
    for (int i = 0; i < n; ++i) byPos[pos[i]] = i;
    std::vector<int> seqOf(n, -1), idxIn(n, 0);
    std::vector<std::vector<std::vector<int>>> seqs(ncol);
    for (int p = 0; p < n; ++p) {
        const int i = byPos[p], cc = colour[i];
        int sq = -1;
        for (auto& e : low[i]) {
            const int j = L.ecol[at(e.second, i)];
            if (colour[j] != cc) {
                if (colour[j] > cc) { S.error = "cpr: ILU0 smoothing: the colours are not an elimination order"; return; }
                continue;
            }
            if (sq >= 0 && seqOf[j] != sq) { S.error = "cpr: ILU0 smoothing: a row depends on two sequences of its own colour"; return; }
            sq = seqOf[j];
        }
        if (sq < 0) { sq = (int)seqs[cc].size(); seqs[cc].emplace_back(); }
        seqOf[i] = sq;
        idxIn[i] = (int)seqs[cc][sq].size();
        seqs[cc][sq].push_back(i);
    }
    S.wl.assign(ncol, 0); S.wu.assign(ncol, 0);
    for (int i = 0; i < n; ++i) {
        int nu = 0;
        for (int w = 0; w < S.MW; ++w) nu += __builtin_popcount(S.mask[(size_t)(S.MW + w) * n + i]);
        S.wl[colour[i]] = std::max(S.wl[colour[i]], (int)low[i].size());
        S.wu[colour[i]] = std::max(S.wu[colour[i]], nu);
        S.WU = std::max(S.WU, nu);
    }
    S.WU = std::max(S.WU, 1);
    S.nseq.assign(ncol, 0); S.nsteps.assign(ncol, 0); S.off.assign(ncol + 1, 0); S.fast.assign(ncol, 1);
    for (int cc = 0; cc < ncol; ++cc) {
        int steps = 0;
        for (auto& q : seqs[cc]) steps = std::max(steps, (int)q.size());
        S.nseq[cc] = (int)seqs[cc].size();
        S.nsteps[cc] = steps;
        S.off[cc + 1] = S.off[cc] + steps * S.nseq[cc];
    }
    S.rowAt.assign(S.off[ncol], -1);
    for (int cc = 0; cc < ncol; ++cc)
        for (int t = 0; t < S.nseq[cc]; ++t)
            for (size_t st = 0; st < seqs[cc][t].size(); ++st) S.rowAt[S.off[cc] + st * S.nseq[cc] + t] = seqs[cc][t][st];
    // fast: every coupling inside the colour joins neighbours of a sequence (the sweeps may then hand the value on in a register)
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < L.rlen[i]; ++j) {
            const int c = L.ecol[at(j, i)];
            if (c == i || colour[c] != colour[i]) continue;
            if (seqOf[c] != seqOf[i] || std::abs(idxIn[c] - idxIn[i]) != 1) S.fast[colour[i]] = 0;
        }
    // simple?
    bool simple = !L.rm;
    for (int cc = 0; cc < ncol && simple; ++cc) simple = S.fast[cc] != 0;
    std::vector<int> tpos(simple ? (size_t)S.WL * n : 0, -1);
    for (int i = 0; i < n && simple; ++i) {
        int q = 0, lastPos = -1;
        for (int j = 0; j < L.rlen[i] && simple; ++j) {
            if (!((S.mask[(size_t)(j >> 5) * n + i] >> (j & 31)) & 1u)) continue;
            const int cj = L.ecol[at(j, i)];
            if (pos[cj] < lastPos) simple = false;   // the row's order is not the elimination order
            lastPos = pos[cj];
            // row cj's upper entries that row i holds too: must be (cj, i) alone
            int found = -1;
            for (int t = 0; t < L.rlen[cj] && simple; ++t) {
                if (!((S.mask[(size_t)(S.MW + (t >> 5)) * n + cj] >> (t & 31)) & 1u)) continue;
                const int ct = L.ecol[at(t, cj)];
                if (ct == i) { found = (int)at(t, cj); continue; }
                for (int u = 0; u < L.rlen[i]; ++u)
                    if (L.ecol[at(u, i)] == ct && (int)at(u, i) != L.diag[i] && ct != i) { simple = false; break; }
            }
            if (found < 0) simple = false;   // (an unsymmetric pattern)
            if (simple) tpos[(size_t)q * n + i] = found;
            ++q;
        }
    }
    S.simple = simple;
    if (simple) S.tpos = std::move(tpos);
}
int cpr_greedy_colours(const CprHostLevel& L, std::vector<int>& colour, std::vector<int>& pos) {
    const int n = L.n, W = L.W;
    auto at = [&](int j, int i) { return L.rm ? (size_t)i * W + j : (size_t)j * n + i; };
    colour.assign(n, -1);
    int nc = 0;
    std::vector<char> used;
    for (int i = 0; i < n; ++i) {
        used.assign(nc + 1, 0);
        for (int j = 0; j < L.rlen[i]; ++j) {
            const int c = L.ecol[at(j, i)];
            if (colour[c] >= 0) used[colour[c]] = 1;
        }
        int k = 0;
        while (used[k]) ++k;
        colour[i] = k;
        nc = std::max(nc, k + 1);
    }
    pos.assign(n, 0);
    int p = 0;
    for (int k = 0; k < nc; ++k)
        for (int i = 0; i < n; ++i)
            if (colour[i] == k) pos[i] = p++;
    return nc;
}

void cpr_coarsen_host(HCsr A, std::vector<int> pos, const int* natOf, const int* atNat, double beta, int lprRows, int iluLevels, int stopRows, CprHostCoarse& out) {
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
#define CPR_T(acc, stmt) do { const double t_ = now(); stmt; acc += now() - t_; } while (0)
    out.lv.clear();
    CprHostLevel* cur = &out.l0;   // the level being coarsened (its transfer part is filled here)
    cur->n = A.n;
    int nlev = 1;
    while (true) {
        const bool last = A.n <= stopRows || nlev >= CPR_MAX_LEVELS;
        if (last) break;
        std::vector<int> a1, a2, g1p, g1i;
        int n1 = 0, n2 = 0;
        HCsr A1;
        for (int attempt = 0; attempt < 3; ++attempt) {
            const double b = attempt == 0 ? beta : 0.0;
            const bool lvl0 = nlev == 1;   // the finest level is stored in the ILU ordering: visit it in natural order
            CPR_T(out.tAgg, pairwise(A, b, attempt == 2, a1, n1, lvl0 ? natOf : nullptr, lvl0 ? atNat : nullptr));
            CPR_T(out.tGal, galerkin(A, a1, n1, A1, g1p, g1i));
            CPR_T(out.tAgg, pairwise(A1, b, attempt == 2, a2, n2));
            if (n2 <= (int)(0.5 * A.n)) break;
        }
        if (n2 >= (int)(0.8 * A.n)) break;   // coarsening stalls: this level is the coarsest
        std::vector<int> agg(A.n);
        for (int i = 0; i < A.n; ++i) agg[i] = a2[a1[i]];
        HCsr Ac;
        std::vector<int> gptr, gidx;
        CPR_T(out.tGal, galerkin(A, agg, n2, Ac, gptr, gidx));
        {   // a coarse level whose rows outgrow the ELL image (fault- and NNC-heavy patterns): stop here, this level is the coarsest
            int Wc = 1;
            for (int I = 0; I < Ac.n; ++I) Wc = std::max(Wc, Ac.rowptr[I + 1] - Ac.rowptr[I]);
            if (Wc > CPR_MAX_W) break;
        }
        for (int& g : gidx) g = pos[g];                       // gather lists address the fine level's ELL array
        std::vector<int> mptr(n2 + 1, 0), midx(A.n);
        for (int i = 0; i < A.n; ++i) mptr[agg[i] + 1]++;
        for (int I = 0; I < n2; ++I) mptr[I + 1] += mptr[I];
        {
            std::vector<int> wpos(mptr.begin(), mptr.end() - 1);
            for (int i = 0; i < A.n; ++i) midx[wpos[agg[i]]++] = i;
        }
        cur->nc = n2;
        {   // four-int member records (two pairwise passes: never more than four members) for cpr_restricted
            std::vector<int> mem4((size_t)4 * n2, -1);
            bool fits = true;
            for (int I = 0; I < n2 && fits; ++I) {
                fits = mptr[I + 1] - mptr[I] <= 4 && mptr[I + 1] > mptr[I];
                for (int q = mptr[I]; fits && q < mptr[I + 1]; ++q) mem4[(size_t)4 * I + (q - mptr[I])] = midx[q];
            }
            if (fits) cur->mem4 = std::move(mem4); else cur->mem4.clear();
        }
        cur->agg = std::move(agg); cur->mptr = std::move(mptr); cur->midx = std::move(midx);
        cur->gptr = std::move(gptr); cur->gidx = std::move(gidx);
        out.lv.emplace_back();
        std::vector<int> cposv;
        bool fitsW = true;
        const bool iluLevel = nlev < iluLevels;   // (level index nlev: the one being added)
        CPR_T(out.tImg, fitsW = ell_image(Ac, out.lv.back(), cposv, Ac.n <= lprRows && !iluLevel));
        if (!fitsW) { out.error = "cpr: a row of a pressure-AMG level outgrew the level image"; return; }
        if (iluLevel) {   // ILU0 smoothing: greedy multi-colouring of the level's graph, colour by colour
            std::vector<int> colour, posv;
            const int ncolours = cpr_greedy_colours(out.lv.back(), colour, posv);
            CPR_T(out.tImg, cpr_ilu_schedule(out.lv.back(), posv, colour, ncolours, out.lv.back().ilu));
            if (!out.lv.back().ilu.error.empty()) { out.error = out.lv.back().ilu.error; return; }
        }
        // (out.lv may have reallocated: cur is looked up again)
        CprHostLevel* fine = out.lv.size() == 1 ? &out.l0 : &out.lv[out.lv.size() - 2];
        fine->cpos = cposv;                                   // where the coarse entries go
        cur = &out.lv.back();
        pos = std::move(cposv);
        A = std::move(Ac);
        ++nlev;
    }
    out.lastA = std::move(A);
    out.lastPos = std::move(pos);
#undef CPR_T
}
void cpr_build_coarse_host(const Pattern& P, const std::vector<double>& ell0, double beta, int lprRows, int iluLevels, int stopRows, CprHostCoarse& out) {
    HCsr A;
    A.n = P.Nb; A.rowptr = P.rowptr; A.col = P.col;
    CprHostLevel img0;
    std::vector<int> pos;   // ELL position of every CSR entry of the level being coarsened
    (void)ell_image(A, img0, pos, false, P.Nb);
    if (P.Nghost > 0) {   // the host copy the hierarchy is built from: owned columns only (pos follows the entries that stay)
        HCsr F;
        std::vector<int> fpos;
        F.n = P.Nb; F.rowptr.assign(P.Nb + 1, 0);
        for (int i = 0; i < P.Nb; ++i) {
            for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k)
                if (A.col[k] < P.Nb) { F.col.push_back(A.col[k]); fpos.push_back(pos[k]); }
            F.rowptr[i + 1] = (int)F.col.size();
        }
        A = std::move(F);
        pos = std::move(fpos);
    }
    const int nnz0 = (int)A.col.size();
    A.val.resize(nnz0);
    for (int k = 0; k < nnz0; ++k) A.val[k] = ell0[pos[k]];
    cpr_coarsen_host(std::move(A), std::move(pos), P.fromOrder.data(), P.toOrder.data(), beta, lprRows, iluLevels, stopRows, out);
}
void cpr_level0_ilu_schedule(const CprHostLevel& L0, const std::vector<int>& colourPrefix, int ncol, CprIluHost& S) {
    std::vector<int> posv(L0.n), colour(L0.n);
    for (int cc = 0; cc < ncol; ++cc)
        for (int p = colourPrefix[cc]; p < colourPrefix[cc + 1]; ++p) colour[p] = cc;
    std::iota(posv.begin(), posv.end(), 0);
    cpr_ilu_schedule(L0, posv, colour, ncol, S);
}

// ---- the joined level of a decomposed run (cpr_setup.hpp) -----------------------------------------------------------------------------
std::vector<int> cpr_joined_aggregates(int nb, const CprHostCoarse& H) {
    std::vector<int> cagg(nb);
    std::iota(cagg.begin(), cagg.end(), 0);
    for (size_t l = 0; l < H.lv.size(); ++l) {   // (H.lv.size() levels below level 0: as many transfers)
        const std::vector<int>& a = l == 0 ? H.l0.agg : H.lv[l - 1].agg;
        for (int i = 0; i < nb; ++i) cagg[i] = a[cagg[i]];
    }
    return cagg;
}
void cpr_joined_rows(int nb, const std::vector<int>& rowptr, const std::vector<int>& col, const std::vector<int>& cagg, const std::vector<int>& ghostRow,
                     const std::vector<long long>& ghostPlace, int off, const HCsr& LA, const std::vector<int>& lastPos, CprJoinedRows& out) {
    out = CprJoinedRows();
    const int nloc = LA.n;
    // the fine couplings of every pair (my aggregate, joined row of a ghost cell's aggregate); q: the coupling's number in entry order
    struct Fine { int i; long long gf; int q; };
    std::vector<std::map<int, std::vector<Fine>>> cross(nloc);
    for (int i = 0; i < nb; ++i)
        for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) {
            const int gh = col[k] - nb;
            if (gh < 0) continue;
            const int q = (int)out.qrow.size();
            out.qrow.push_back(i); out.qentry.push_back(k);
            cross[cagg[i]][ghostRow[gh]].push_back(Fine{i, ghostPlace[gh], q});
        }
    out.rowlen.assign(nloc, 0);
    out.xptr.assign(1, 0);
    for (int I = 0; I < nloc; ++I) {
        auto cr = cross[I].begin();
        auto emit_cross = [&](int upto) {   // the entries towards other ranks whose joined column lies below `upto`
            for (; cr != cross[I].end() && cr->first < upto; ++cr) {
                std::vector<Fine>& f = cr->second;
                std::sort(f.begin(), f.end(), [](const Fine& a, const Fine& b) { return a.i != b.i ? a.i < b.i : a.gf < b.gf; });
                for (const Fine& e : f) out.xidx.push_back(e.q);
                out.cols.push_back(cr->first);
                out.src.push_back(-1 - (int)(out.xptr.size() - 1));
                out.xptr.push_back((int)out.xidx.size());
                ++out.rowlen[I];
            }
        };
        for (int k = LA.rowptr[I]; k < LA.rowptr[I + 1]; ++k) {
            emit_cross(off + LA.col[k]);
            out.cols.push_back(off + LA.col[k]); out.src.push_back(lastPos[k]);
            ++out.rowlen[I];
        }
        emit_cross(INT_MAX);
    }
}
std::vector<double> cpr_joined_values(const CprJoinedRows& Q, const std::vector<double>& apg, const std::vector<double>& lastval) {
    std::vector<double> vals(Q.src.size());
    size_t k = 0;   // own entries stand in the last level's entry order
    for (size_t e = 0; e < Q.src.size(); ++e) {
        if (Q.src[e] >= 0) { vals[e] = lastval[k++]; continue; }
        const int x = -1 - Q.src[e];
        double s = 0.0;
        for (int t = Q.xptr[x]; t < Q.xptr[x + 1]; ++t) s += apg[Q.xidx[t]];
        vals[e] = s;
    }
    return vals;
}
void cpr_join_rows(const std::vector<int>& bl, const std::vector<int>& bc, const std::vector<double>& bv, const std::vector<int>& nnzs, const std::vector<int>& offs,
                   int maxn, int maxnnz, CprJoined& out) {
    out = CprJoined();
    const int nr = (int)nnzs.size(), NG = offs[nr];
    HCsr& J = out.J;
    J.n = NG;
    J.rowptr.assign(1, 0);
    for (int r = 0; r < nr; ++r) {
        const size_t l0 = (size_t)r * maxn, e0 = (size_t)r * maxnnz;
        const int rows = offs[r + 1] - offs[r], nnz = nnzs[r];
        bool ok = rows >= 0 && rows <= maxn && nnz >= 0 && nnz <= maxnnz && l0 + maxn <= bl.size() && e0 + maxnnz <= bc.size() && e0 + maxnnz <= bv.size();
        int e = 0;
        for (int I = 0; I < rows && ok; ++I) {
            const int len = bl[l0 + I];
            ok = len >= 0 && len <= nnz - e;   // a row that would leave the rank's entries is not followed
            for (int t = 0; t < len && ok; ++t, ++e) {
                const int cj = bc[e0 + e];
                ok = cj >= 0 && cj < NG;
                J.col.push_back(cj); J.val.push_back(bv[e0 + e]); out.vunpad.push_back(r * maxnnz + e);
            }
            J.rowptr.push_back((int)J.col.size());
            out.unpad.push_back(r * maxn + I);
        }
        if (!ok) { out.error = "cpr: the joined level's rows of rank " + std::to_string(r) + " are inconsistent"; return; }
    }
}

}  // namespace opmhip
