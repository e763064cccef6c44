// Host-side analysis done once per sparsity pattern (the reference's "analyse_matrix",
// bda/BILU0.cpp:51-158): ILU ordering, internal (reordered) block-CSR pattern, L/U split, device tiling.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <numeric>
#include <queue>

#include "internal.hpp"

#ifndef OPMHIP_XCD_GROUP_DEFAULT
#define OPMHIP_XCD_GROUP_DEFAULT 8
#endif

namespace opmhip {
namespace {

void transpose_pattern(const Pattern& P, std::vector<int>& cptr, std::vector<int>& ridx);

// level(i) = 1 + max level over the rows j < i that row i is coupled to (Saad 11.6.3).  Couplings are taken
// from the row AND the column of i, as the reference's findLevelScheduling does with its CSR + CSC pair
// (bda/Reorder.cpp:266-318), so that both the forward and the backward sweep are race free on a
// structurally non-symmetric pattern.  For a symmetric pattern this is the plain row-dependency level.
void levels(const Pattern& P, std::vector<int>& color, int& ncol) {
    std::vector<int> cptr, ridx;
    transpose_pattern(P, cptr, ridx);
    color.assign(P.Nb, 0);
    ncol = 0;
    for (int i = 0; i < P.Nb; ++i) {
        int l = 0;
        for (int k = P.nat_rowptr[i]; k < P.nat_rowptr[i + 1]; ++k) {
            const int j = P.nat_col[k];
            if (j < i) l = std::max(l, color[j] + 1);
        }
        for (int k = cptr[i]; k < cptr[i + 1]; ++k) {
            const int j = ridx[k];
            if (j < i) l = std::max(l, color[j] + 1);
        }
        color[i] = l;
        ncol = std::max(ncol, l + 1);
    }
}

uint32_t mix(uint32_t i) {  // splitmix64 -> 31 bits: deterministic replacement for std::random_device weights
    uint64_t z = (uint64_t)i + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(z & 0x7fffffffu);
}

void transpose_pattern(const Pattern& P, std::vector<int>& cptr, std::vector<int>& ridx) {
    cptr.assign(P.Nb + 1, 0);
    ridx.resize(P.nnzb);
    for (int k = 0; k < P.nnzb; ++k) cptr[P.nat_col[k] + 1]++;
    std::partial_sum(cptr.begin(), cptr.end(), cptr.begin());
    std::vector<int> w(cptr.begin(), cptr.end() - 1);
    for (int i = 0; i < P.Nb; ++i)
        for (int k = P.nat_rowptr[i]; k < P.nat_rowptr[i + 1]; ++k) ridx[w[P.nat_col[k]]++] = i;
}

// Jones-Plassmann rounds (bda/Reorder.cpp:59-172): in round c an uncoloured node takes colour c when none
// of its neighbours (row or column) already has c and it carries the largest weight among its uncoloured
// neighbours.
void color_jp(const Pattern& P, std::vector<int>& color, int& ncol) {
    std::vector<int> cptr, ridx;
    transpose_pattern(P, cptr, ridx);
    color.assign(P.Nb, -1);
    std::vector<uint32_t> w(P.Nb);
    for (int i = 0; i < P.Nb; ++i) w[i] = mix((uint32_t)i);
    int left = P.Nb;
    ncol = 0;
    for (int c = 0; left > 0; ++c) {
        for (int i = 0; i < P.Nb; ++i) {
            if (color[i] != -1) continue;
            bool win = true;
            auto look = [&](const int* idx, int b, int e) {
                for (int k = b; k < e && win; ++k) {
                    const int j = idx[k];
                    if (j == i) continue;
                    const int jc = color[j];
                    if (jc == c) win = false;
                    else if (jc == -1 && (w[i] < w[j] || (w[i] == w[j] && i < j))) win = false;
                }
            };
            look(P.nat_col.data(), P.nat_rowptr[i], P.nat_rowptr[i + 1]);
            look(ridx.data(), cptr[i], cptr[i + 1]);
            if (win) {
                color[i] = c;
                --left;
            }
        }
        ncol = c + 1;
    }
}

void color_greedy(const Pattern& P, std::vector<int>& color, int& ncol) {
    std::vector<int> cptr, ridx;
    transpose_pattern(P, cptr, ridx);
    color.assign(P.Nb, -1);
    ncol = 0;
    std::vector<char> used;
    for (int i = 0; i < P.Nb; ++i) {
        used.assign(ncol + 1, 0);
        for (int k = P.nat_rowptr[i]; k < P.nat_rowptr[i + 1]; ++k)
            if (color[P.nat_col[k]] >= 0) used[color[P.nat_col[k]]] = 1;
        for (int k = cptr[i]; k < cptr[i + 1]; ++k)
            if (color[ridx[k]] >= 0) used[color[ridx[k]]] = 1;
        int c = 0;
        while (used[c]) ++c;
        color[i] = c;
        ncol = std::max(ncol, c + 1);
    }
}

// First-fit colouring of the graph of A^2 in the natural visiting order: no two rows of one colour share a neighbour (row or column
// couplings), so level-1 fill - (i, j) through an earlier k coupled to both - never joins two rows of one colour and the colours stay
// a schedule of the ILU(1) factors.  For ILU0 it is one more (weaker) colouring.
void color_distance2(const Pattern& P, std::vector<int>& color, int& ncol) {
    std::vector<int> cptr, ridx;
    transpose_pattern(P, cptr, ridx);
    color.assign(P.Nb, -1);
    ncol = 0;
    std::vector<int> seen;   // seen[c] == i: colour c is taken near row i
    auto each_neighbour = [&](int i, auto&& f) {
        for (int k = P.nat_rowptr[i]; k < P.nat_rowptr[i + 1]; ++k) f(P.nat_col[k]);
        for (int k = cptr[i]; k < cptr[i + 1]; ++k) f(ridx[k]);
    };
    for (int i = 0; i < P.Nb; ++i) {
        auto mark = [&](int j) { if (j != i && color[j] >= 0) seen[color[j]] = i; };
        seen.resize(ncol + 1, -1);
        each_neighbour(i, [&](int j) {
            mark(j);
            each_neighbour(j, mark);
        });
        int c = 0;
        while (seen[c] == i) ++c;
        color[i] = c;
        ncol = std::max(ncol, c + 1);
    }
}

// Symbolic ILU(n) of the owned pattern (rowptr / col: rows and columns in elimination order, ascending columns, diagonal present),
// the level-of-fill rule of the reference's ILU(n) (milun_decomposition): the entries of A have generation 0; row i walks its entries
// left of the diagonal in ascending column order, fill made earlier in the same row included; an entry (i, k) of generation < n pivots
// row k, whose entries (k, j), j >= k, of generation < n create (i, j) with generation gen(k, j) + 1 where row i has no entry yet (an
// existing entry keeps its generation).  Returns false - nothing more is built - as soon as the factors would hold more than `budget`
// blocks.  frowptr / fcol: the filled pattern, ascending columns; fdiag: the diagonal's place in every row.
bool symbolic_fill(int Nb, const std::vector<int>& rowptr, const std::vector<int>& col, int n, long long budget, std::vector<int>& frowptr,
                   std::vector<int>& fcol, std::vector<int>& fdiag) {
    frowptr.assign(Nb + 1, 0);
    fcol.clear();
    fdiag.assign(Nb, -1);
    std::vector<int> fgen;
    std::vector<int> genAt(Nb, -1);      // generation of (i, j) in the row under construction, -1: no entry
    std::vector<int> cols;
    std::priority_queue<int, std::vector<int>, std::greater<int>> lower;   // entries left of the diagonal still to walk, smallest first
    for (int i = 0; i < Nb; ++i) {
        cols.clear();
        for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) {
            const int j = col[k];
            genAt[j] = 0;
            cols.push_back(j);
            if (j < i) lower.push(j);
        }
        while (!lower.empty()) {
            const int k = lower.top();
            lower.pop();
            if (genAt[k] >= n) continue;
            for (int q = fdiag[k]; q < frowptr[k + 1]; ++q) {
                const int j = fcol[q], g = fgen[q];
                if (g >= n || genAt[j] >= 0) continue;
                genAt[j] = g + 1;
                cols.push_back(j);
                if (j < i) lower.push(j);   // j > k: it comes later in this walk
            }
        }
        std::sort(cols.begin(), cols.end());
        if ((long long)fcol.size() + (long long)cols.size() > budget) {
            for (int j : cols) genAt[j] = -1;
            return false;
        }
        for (int j : cols) {
            if (j == i) fdiag[i] = (int)fcol.size();
            fcol.push_back(j);
            fgen.push_back(genAt[j]);
            genAt[j] = -1;
        }
        frowptr[i + 1] = (int)fcol.size();
    }
    return true;
}

// Sub-tiles (<= TILE_ROWS rows, <= TILE_CAP_BLOCKS blocks) grouped into chain-tiles: the sub-tiles of one chain-tile
// are the successive steps of up to TILE_ROWS chains and must be processed in order by one workgroup; different
// chain-tiles of a colour are independent.  Without chains every sub-tile is its own chain-tile.
void build_tiles(const std::vector<int>& rowptr, const std::vector<int>& colorPrefix, const std::vector<int>& stepPrefix,
                 TileSet& T) {
    // stepPrefix: row boundaries of (chain-tile, step) groups, ascending, containing every colour boundary; a value
    // of -1 marks the start of a new chain-tile (encoded as a parallel flag array to keep this simple)
    T.row0.clear();
    T.colorTile.clear();
    T.ctFirst.clear();
    T.colorCT.clear();
    (void)stepPrefix;
    const int ncol = (int)colorPrefix.size() - 1;
    for (int c = 0; c < ncol; ++c) {
        T.colorTile.push_back((int)T.row0.size());
        T.colorCT.push_back((int)T.ctFirst.size());
        int r = colorPrefix[c];
        const int rend = colorPrefix[c + 1];
        while (r < rend) {
            T.ctFirst.push_back((int)T.row0.size());
            T.row0.push_back(r);
            int e = r + 1;  // a tile always holds at least one row (an over-long row is read from HBM directly)
            while (e < rend && e - r < TILE_ROWS && rowptr[e + 1] - rowptr[r] <= TILE_CAP_BLOCKS) ++e;
            r = e;
        }
    }
    T.colorTile.push_back((int)T.row0.size());
    T.colorCT.push_back((int)T.ctFirst.size());
    T.ctFirst.push_back((int)T.row0.size());
    T.row0.push_back(colorPrefix[ncol]);
}

// Line colouring: chains of up to maxLen rows along each row's farthest neighbour (in the natural CpGrid order
// i + nx*(j + ny*k) that is the vertical neighbour, the strongest coupling of a thin-layered reservoir grid), chains
// coloured greedily so that chains of one colour share no coupling.  Inside a chain rows keep their natural order, so
// the factorisation is an exact ILU0 of the permuted matrix; it keeps most of the natural ordering's strength at
// two colours' worth of launches (tools/ordering_study.py: 12.5 BiCGStab iterations against 26.5 for red-black and
// 9.5 for the natural order on a 72^3 Jacobian).
struct Chains {
    std::vector<int> chainOf, posIn;          // per row
    std::vector<std::vector<int>> rows;       // per chain
};
void build_chains(const Pattern& P, int maxLen, Chains& C) {
    const int Nb = P.Nb;
    std::vector<int> succ(Nb, -1);
    for (int i = 0; i < Nb; ++i) {
        const int last = P.nat_col[P.nat_rowptr[i + 1] - 1];
        if (last > i && P.nat_col[P.nat_rowptr[last]] == i) succ[i] = last;  // mutual: i is the farthest lower neighbour of last
    }
    C.chainOf.assign(Nb, -1);
    C.posIn.assign(Nb, 0);
    C.rows.clear();
    for (int i = 0; i < Nb; ++i) {
        if (C.chainOf[i] >= 0) continue;
        const int id = (int)C.rows.size();
        C.rows.emplace_back();
        int cur = i;
        while (cur >= 0 && C.chainOf[cur] < 0 && (int)C.rows[id].size() < maxLen) {
            C.chainOf[cur] = id;
            C.posIn[cur] = (int)C.rows[id].size();
            C.rows[id].push_back(cur);
            cur = succ[cur];
        }
    }
}
void color_chains(const Pattern& P, const Chains& C, std::vector<int>& chainColor, int& ncol) {
    std::vector<int> cptr, ridx;
    transpose_pattern(P, cptr, ridx);
    const int nc = (int)C.rows.size();
    chainColor.assign(nc, -1);
    ncol = 0;
    std::vector<char> used;
    for (int id = 0; id < nc; ++id) {
        used.assign(ncol + 1, 0);
        for (int i : C.rows[id]) {
            for (int k = P.nat_rowptr[i]; k < P.nat_rowptr[i + 1]; ++k) {
                const int o = C.chainOf[P.nat_col[k]];
                if (o != id && chainColor[o] >= 0) used[chainColor[o]] = 1;
            }
            for (int k = cptr[i]; k < cptr[i + 1]; ++k) {
                const int o = C.chainOf[ridx[k]];
                if (o != id && chainColor[o] >= 0) used[chainColor[o]] = 1;
            }
        }
        int c = 0;
        while (used[c]) ++c;
        chainColor[id] = c;
        ncol = std::max(ncol, c + 1);
    }
}

// The sorted, distinct column offsets (col - row) of rows [r0, r1) of a block-CSR
void tile_offsets(const std::vector<int>& rowptr, const std::vector<int>& col, int r0, int r1, std::vector<int>& offs) {
    offs.clear();
    for (int r = r0; r < r1; ++r)
        for (int k = rowptr[r]; k < rowptr[r + 1]; ++k) offs.push_back(col[k] - r);
    std::sort(offs.begin(), offs.end());
    offs.erase(std::unique(offs.begin(), offs.end()), offs.end());
}
}  // namespace

void reset_stencil(StencilForm& S, int Nb, size_t tables) {
    S.word.assign(Nb, 0xFFFFFFFFu);
    S.koff.assign(Nb, 0);
    S.table.assign(STENCIL_TABLE_SLOTS * tables, 0);
}
bool encode_stencil(const std::vector<int>& rowptr, const std::vector<int>& col, int r0, int r1, int slot, StencilForm& S) {
    std::vector<int> offs;
    tile_offsets(rowptr, col, r0, r1, offs);
    if (offs.size() > STENCIL_MAX_OFFSETS) return false;
    for (size_t q = 0; q < offs.size(); ++q) S.table[(size_t)STENCIL_TABLE_SLOTS * slot + q] = offs[q];
    for (int r = r0; r < r1; ++r) {
        const int len = rowptr[r + 1] - rowptr[r], ko = rowptr[r] - rowptr[r0];
        if (len > STENCIL_ROW_ENTRIES || ko > STENCIL_MAX_KOFF) return false;
        unsigned w = 0xFFFFFFFFu;
        for (int u = 0; u < len; ++u) {
            const int idx = (int)(std::lower_bound(offs.begin(), offs.end(), col[rowptr[r] + u] - r) - offs.begin());
            w = (w & ~(0xFu << (4 * u))) | ((unsigned)idx << (4 * u));
        }
        S.word[r] = w;
        S.koff[r] = (unsigned char)ko;
    }
    return true;
}

namespace {
int upload_stencil(opmhip_ctx* c, StencilForm& S) {
    int rc;
    if ((rc = dev_upload(c, &S.d_word, S.word))) return rc;
    if ((rc = dev_upload(c, &S.d_koff, S.koff))) return rc;
    return dev_upload(c, &S.d_table, S.table);
}

// Launch schedules.  The hardware deals consecutive workgroups of a launch round-robin over the 8 XCDs, each with an L2 of
// its own.  With the identity map (workgroup b = tile b) a line of the gathered vector is wanted by ~7 tiles that land
// on ~5 different XCDs and is fetched from the fabric by each (PMC: the 24 MB input vector of the 100^3 SpMV costs
// 116 MB).  The schedule keeps the streaming shape (all 8 XCDs walk through memory side by side) but hands every XCD
// GROUPS of `G` consecutive chain-tiles of every colour at the same relative position of their colour - the same stretch
// of the grid - so that most neighbours of a tile are gathered through the L2 that already holds them.
// Results do not depend on the schedule (each tile's arithmetic is its own); only the order of the partial sums does.
// deal: list k's items to launch positions k, k + 8, k + 16, ... (position % 8 = the XCD), shorter lists padded with `pad`
template <class T>
void deal(const std::vector<std::vector<T>>& lists, const T& pad, std::vector<T>& out) {
    size_t L = 0;
    for (const auto& l : lists) L = std::max(L, l.size());
    for (size_t j = 0; j < L; ++j)
        for (int k = 0; k < 8; ++k) out.push_back(j < lists[k].size() ? lists[k][j] : pad);
}
// Launch schedule of the rest product (internal.hpp: RestSched).  The tiles follow the SpMV's launch order - position b and b + 8 of it are
// consecutive tiles of one stretch of the grid on one XCD - and consecutive tiles are merged while the rows stay contiguous, the tile holds
// at most 64 rows (one per lane) and TILE_CAP_BLOCKS blocks and its rows share at most 15 column offsets: a row of the rest has 2 - 6 blocks
// where the full row has 7, so a tile of the SpMV's 32 rows would stream 4.6 - 13.8 KB per step of the pipelined kernel instead of 16.
// Off (R.on = false) unless the pattern has the property the product rests on (Pattern::ualias), the ordering is line-coloured (the chain
// sweeps are the ones that emit the row sums) and every tile fits the stencil form.
void build_rest_schedule(Pattern& P, const std::vector<int>& order) {
    RestSched& R = P.rest;
    const TileSet& T = P.tiles;
    R.on = false;
    if (!P.ualias || !P.chained) return;
    struct Rt { int r0, r1; };
    std::vector<int> offs;
    std::vector<Rt> out;   // launch positions of both parts, padding = {0, 0}
    int nInt = 0;
    // Decomposed runs (ghost columns): the INTERIOR tiles take this form; the boundary tiles - rows with ghost columns at arbitrary offsets,
    // which rarely fit a table of 15 - keep the whole product over the matrix itself (launch_spmv), so only part 0 is built
    const int nparts = P.Nghost > 0 ? 1 : 2;
    for (int part = 0; part < nparts; ++part) {
        const int p0 = part == 0 ? 0 : T.nschedInt, p1 = part == 0 ? T.nschedInt : T.nsched;
        std::vector<std::vector<Rt>> lists(8);
        for (int k = 0; k < 8; ++k) {
            Rt cur{0, 0};
            for (int b = p0 + k; b < p1; b += 8) {
                if (order[b] < 0) continue;
                const int r0 = T.row0[order[b]], r1 = T.row0[order[b] + 1];
                if (r1 <= r0) continue;
                if (cur.r1 > cur.r0 && r0 == cur.r1 && r1 - cur.r0 <= 64 && P.rrowptr[r1] - P.rrowptr[cur.r0] <= TILE_CAP_BLOCKS) {
                    tile_offsets(P.rrowptr, P.rcol, cur.r0, r1, offs);
                    if (offs.size() <= STENCIL_MAX_OFFSETS) { cur.r1 = r1; continue; }
                }
                if (cur.r1 > cur.r0) lists[k].push_back(cur);
                cur = Rt{r0, r1};
            }
            if (cur.r1 > cur.r0) lists[k].push_back(cur);
        }
        deal(lists, Rt{0, 0}, out);
        if (part == 0) nInt = (int)out.size();
    }
    R.nsched = (int)out.size();
    R.nschedInt = P.Nghost > 0 ? R.nsched : nInt;
    R.sched.assign((size_t)4 * R.nsched, 0);
    reset_stencil(R, P.Nb, std::max(1, R.nsched));
    for (int b = 0; b < R.nsched; ++b) {
        const int r0 = out[b].r0, r1 = out[b].r1;
        if (r1 <= r0) continue;
        R.sched[4 * b] = r0; R.sched[4 * b + 1] = r1;
        R.sched[4 * b + 2] = P.rrowptr[r0]; R.sched[4 * b + 3] = P.rrowptr[r1];
        if (P.rrowptr[r1] - P.rrowptr[r0] > TILE_CAP_BLOCKS || r1 - r0 > 64) return;   // a single SpMV tile too large for the form: off
        if (!encode_stencil(P.rrowptr, P.rcol, r0, r1, b, R)) return;
    }
    R.on = R.nsched > 0;
}

void build_schedules(Pattern& P, int G) {
    TileSet& T = P.tiles;
    const int ncol = P.numColors;
    const int nt = T.ntiles();
    T.ctSched.clear();
    T.ctSchedOff.assign(ncol + 1, 0);
    std::vector<int> order;  // SpMV: tiles in launch order (-1 = padding)
    const bool grouped = P.chained && G > 0;
    if (!grouped) {
        for (int t = 0; t < nt; ++t) order.push_back(t);
        while (order.size() % 8) order.push_back(-1);
        for (int c = 0; c < ncol; ++c) {
            for (int q = T.colorCT[c]; q < T.colorCT[c + 1]; ++q) T.ctSched.push_back(q);
            while (T.ctSched.size() % 8) T.ctSched.push_back(-1);
            T.ctSchedOff[c + 1] = (int)T.ctSched.size();
        }
    } else {
        int maxct = 0;
        for (int c = 0; c < ncol; ++c) maxct = std::max(maxct, T.colorCT[c + 1] - T.colorCT[c]);
        const int NG = std::max(1, (maxct + G - 1) / G);
        // group of chain-tile q (0-based inside colour c): by relative position, so that the colours line up in space
        auto group_of = [&](int c, int q) { return (int)(((long long)q * NG) / std::max(1, T.colorCT[c + 1] - T.colorCT[c])); };
        std::vector<std::vector<int>> spmvLists(8);
        std::vector<std::vector<std::vector<int>>> byGroup(ncol, std::vector<std::vector<int>>(NG));
        for (int c = 0; c < ncol; ++c)
            for (int q = T.colorCT[c]; q < T.colorCT[c + 1]; ++q) byGroup[c][group_of(c, q - T.colorCT[c])].push_back(q);
        for (int g = 0; g < NG; ++g) {
            size_t m = 0;
            for (int c = 0; c < ncol; ++c) m = std::max(m, byGroup[c][g].size());
            for (size_t i = 0; i < m; ++i)   // colours interleaved chain-tile by chain-tile
                for (int c = 0; c < ncol; ++c)
                    if (i < byGroup[c][g].size())
                        for (int t = T.ctFirst[byGroup[c][g][i]]; t < T.ctFirst[byGroup[c][g][i] + 1]; ++t) spmvLists[g % 8].push_back(t);
        }
        deal(spmvLists, -1, order);
        for (int c = 0; c < ncol; ++c) {
            std::vector<std::vector<int>> lists(8);
            for (int g = 0; g < NG; ++g)
                for (int q : byGroup[c][g]) lists[g % 8].push_back(q);
            deal(lists, -1, T.ctSched);
            T.ctSchedOff[c + 1] = (int)T.ctSched.size();
        }
    }
    // descriptor records of the chain kernels' launch positions (ILU0 only: an ILU(n) context is never chained)
    if (P.fillLevel == 0) {
        int S = 1;
        for (size_t q = 0; q + 1 < T.ctFirst.size(); ++q) S = std::max(S, T.ctFirst[q + 1] - T.ctFirst[q]);
        T.descS1 = S + 1;
        T.descStride = desc_stride(T.descS1);
        T.ctDesc.assign((size_t)T.ctSched.size() * T.descStride, 0);
        for (size_t pos = 0; pos < T.ctSched.size(); ++pos) {
            int* rec = &T.ctDesc[pos * T.descStride];
            const int ct = T.ctSched[pos];
            rec[1] = ct;
            if (ct < 0) continue;
            const int q0 = T.ctFirst[ct], n = T.ctFirst[ct + 1] - q0;
            rec[0] = n;
            rec[2] = q0;   // first tile of the chain-tile: where its steps' stencil tables start
            for (int i = 0; i <= n; ++i) {
                const int r = T.row0[q0 + i];
                rec[DESC_HEAD + i] = r;
                rec[DESC_HEAD + T.descS1 + i] = P.lrowptr[r];
                rec[DESC_HEAD + 2 * T.descS1 + i] = P.urowptr[r];
            }
        }
    }
    // decomposed runs: interior tiles first, boundary tiles (a row with a ghost column) behind them, each part keeping the
    // dealing over the 8 XCD columns (position % 8) it had
    T.nschedInt = (int)order.size();
    if (P.Nghost > 0) {
        auto boundary = [&](int t) {
            for (int k = P.rowptr[T.row0[t]]; k < P.rowptr[T.row0[t + 1]]; ++k)
                if (P.col[k] >= P.Nb) return true;
            return false;
        };
        std::vector<std::vector<int>> in8(8), bd8(8);
        for (size_t b = 0; b < order.size(); ++b)
            if (order[b] >= 0) (boundary(order[b]) ? bd8 : in8)[b % 8].push_back(order[b]);
        std::vector<int> o2;
        deal(in8, -1, o2);
        T.nschedInt = (int)o2.size();
        deal(bd8, -1, o2);
        order.swap(o2);
    }
    T.nsched = (int)order.size();
    T.spmvSched.assign((size_t)4 * T.nsched, 0);
    for (int b = 0; b < T.nsched; ++b)
        if (order[b] >= 0) {
            const int r0 = T.row0[order[b]], r1 = T.row0[order[b] + 1];
            T.spmvSched[4 * b] = r0; T.spmvSched[4 * b + 1] = r1;
            T.spmvSched[4 * b + 2] = P.rowptr[r0]; T.spmvSched[4 * b + 3] = P.rowptr[r1];
        }
    // stencil form of the index streams, one table per launch position, judged per part of the schedule: the interior tiles of a
    // decomposed run are as regular as a single domain's, its boundary tiles (ghost columns at arbitrary offsets) usually are not
    T.stencilPart[0] = T.stencilPart[1] = true;
    reset_stencil(T.st, P.Nb, T.nsched);
    for (int b = 0; b < T.nsched; ++b) {
        if (order[b] < 0) continue;
        bool& on = T.stencilPart[b < T.nschedInt ? 0 : 1];
        if (on) on = encode_stencil(P.rowptr, P.col, T.row0[order[b]], T.row0[order[b] + 1], b, T.st);
    }
    T.stencil = T.stencilPart[0] || T.stencilPart[1];
    build_rest_schedule(P, order);
    // the same for the two factor parts the sweeps stream, one table per tile (chained orderings only: their kernels are the ones that read it)
    P.sweepStencil = P.chained;
    for (int part = 0; part < 2 && P.sweepStencil; ++part) {
        reset_stencil(P.sw[part], P.Nb, nt);
        for (int t = 0; t < nt && P.sweepStencil; ++t)
            P.sweepStencil = encode_stencil(part == 0 ? P.lrowptr : P.urowptr, part == 0 ? P.lcol : P.ucol, T.row0[t], T.row0[t + 1], t, P.sw[part]);
    }
}

// ILU0: L / U split of the internal pattern (what Dune's convertToCRS produces, linalg/ParallelOverlappingILU0.hpp:497-584; here both
// parts keep ascending columns and the sweeps choose their own direction), the elimination steps' targets (lmatch) and whether U is
// upper(A) (ualias)
void build_ilu0_split(Pattern& P) {
    const int Nb = P.Nb;
    P.lrowptr.assign(Nb + 1, 0);
    P.urowptr.assign(Nb + 1, 0);
    P.lcol.clear();
    P.ucol.clear();
    P.fdest.assign(P.nnzb, -1);
    for (int p = 0; p < Nb; ++p) {
        for (int k = P.rowptr[p]; k < P.rowptr[p + 1]; ++k) {
            if (P.col[k] < p) { P.fdest[k] = (int)P.lcol.size(); P.lcol.push_back(P.col[k]); }
            else if (P.col[k] > p && P.col[k] < Nb) { P.fdest[k] = -2 - (int)P.ucol.size(); P.ucol.push_back(P.col[k]); }  // ghost columns are not part of the ILU
        }
        P.lrowptr[p + 1] = (int)P.lcol.size();
        P.urowptr[p + 1] = (int)P.ucol.size();
    }
    P.nl = (int)P.lcol.size();
    P.nu = (int)P.ucol.size();
    // symbolic elimination: which entries of row p the step against row j updates (k_ilu_factor looks them up instead of merging two
    // column lists per L entry - three dependent rounds of loads became one)
    P.lmatch.assign(P.nnzb, -2);
    for (int p = 0; p < Nb; ++p) {
        const int kb = P.rowptr[p], ke = P.rowptr[p + 1];
        for (int k = kb; k < ke; ++k) {
            const int j = P.col[k];
            if (j >= p) break;
            int count = 0, uidx = -1, target = -1;
            int ik = k + 1, jk = P.urowptr[j];
            const int jend = P.urowptr[j + 1];
            while (ik < ke && jk < jend) {
                if (P.col[ik] == P.ucol[jk]) { if (count++ == 0) { uidx = jk; target = ik - kb; } ++ik; ++jk; }
                else if (P.col[ik] < P.ucol[jk]) ++ik;
                else ++jk;
            }
            if (count == 0) P.lmatch[k] = -1;
            else if (count == 1 && target < 64 && uidx < (1 << 25)) P.lmatch[k] = uidx * 64 + target;
        }
    }
    // U == upper(A)?  (Pattern::ualias)  Every match of an elimination step must lie on or left of the diagonal of the row being eliminated.
    P.ualias = true;
    for (int p = 0; p < Nb && P.ualias; ++p) {
        const int kb = P.rowptr[p], ke = P.rowptr[p + 1];
        for (int k = kb; k < ke && P.ualias; ++k) {
            const int j = P.col[k];
            if (j >= p) break;
            int ik = k + 1, jk = P.urowptr[j];
            const int jend = P.urowptr[j + 1];
            while (ik < ke && jk < jend) {
                if (P.col[ik] == P.ucol[jk]) { if (P.col[ik] > p) { P.ualias = false; break; } ++ik; ++jk; }
                else if (P.col[ik] < P.ucol[jk]) ++ik;
                else ++jk;
            }
        }
    }
}

// ILU(n): the filled pattern (rows and columns in the fill's elimination order, ibase: that order -> natural row) renamed into the
// internal order and split into L and U, every matrix entry's place in it, and the sweeps' tiles over the filled rows.  U is not upper(A)
// (fill right of the diagonal): the product after M^-1 streams the whole matrix.
int build_fill_split(opmhip_ctx* c, const std::vector<int>& frp, const std::vector<int>& fcl, const std::vector<int>& ibase) {
    Pattern& P = c->pat;
    const int Nb = P.Nb;
    std::vector<int> bpos(Nb), colorOf(Nb);   // natural row -> elimination-order row; internal row -> colour
    for (int b = 0; b < Nb; ++b) bpos[ibase[b]] = b;
    for (int cc = 0; cc < P.numColors; ++cc)
        for (int p = P.colorPrefix[cc]; p < P.colorPrefix[cc + 1]; ++p) colorOf[p] = cc;
    P.lrowptr.assign(Nb + 1, 0);
    P.urowptr.assign(Nb + 1, 0);
    P.lcol.clear();
    P.ucol.clear();
    std::vector<int> row;
    for (int p = 0; p < Nb; ++p) {
        const int b = bpos[P.fromOrder[p]];
        row.clear();
        for (int q = frp[b]; q < frp[b + 1]; ++q) row.push_back(P.toOrder[ibase[fcl[q]]]);
        std::sort(row.begin(), row.end());
        for (int j : row) {
            if (j != p && colorOf[j] == colorOf[p])
                return fail(c, OPMHIP_ANALYSIS_FAILED, "ILU(%d): the ordering is not a schedule of the filled pattern at row %d", P.fillLevel, p);
            if (j < p) P.lcol.push_back(j);
            else if (j > p) P.ucol.push_back(j);
        }
        P.lrowptr[p + 1] = (int)P.lcol.size();
        P.urowptr[p + 1] = (int)P.ucol.size();
    }
    P.nl = (int)P.lcol.size();
    P.nu = (int)P.ucol.size();
    P.fdest.assign(P.nnzb, -1);
    for (int p = 0; p < Nb; ++p)
        for (int k = P.rowptr[p]; k < P.rowptr[p + 1]; ++k) {
            const int j = P.col[k];
            if (j == p || j >= Nb) continue;   // diagonal; ghost columns are not part of the ILU
            const int* b0 = j < p ? &P.lcol[P.lrowptr[p]] : &P.ucol[P.urowptr[p]];
            const int* b1 = j < p ? &P.lcol[0] + P.lrowptr[p + 1] : &P.ucol[0] + P.urowptr[p + 1];
            const int* f = std::lower_bound(b0, b1, j);
            if (f == b1 || *f != j) return fail(c, OPMHIP_ANALYSIS_FAILED, "ILU(%d): entry (%d, %d) of the matrix is missing from the filled pattern", P.fillLevel, p, j);
            P.fdest[k] = j < p ? (int)(f - &P.lcol[0]) : -2 - (int)(f - &P.ucol[0]);
        }
    P.ualias = false;
    std::vector<int> trp(Nb + 1, 0);   // the tiles bound a row's L and U blocks together: both sweeps read the same tiles
    for (int p = 0; p <= Nb; ++p) trp[p] = P.lrowptr[p] + P.urowptr[p];
    build_tiles(trp, P.colorPrefix, {}, P.ftiles);
    return OPMHIP_SUCCESS;
}

}  // namespace

int build_pattern(opmhip_ctx* c, int Nb, int Nghost, int nnzb, const int* rows, const int* cols) {
    // Nb = owned block rows (the rows of the matrix); columns may also point at Nghost ghost cells numbered
    // Nb .. Nb+Nghost-1 (owner-cells-first ordering, linalg/ISTLSolverEbos.hpp:171-178).  Ghost columns take part in
    // SpMV and assembly only; the ILU0 is the block-Jacobi one of ghost_last_bilu0_decomposition: it never sees them.
    Pattern& P = c->pat;
    if (Nb <= 0 || Nghost < 0 || nnzb <= 0 || !rows || !cols) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_pattern: bad arguments");
    if (rows[0] != 0 || rows[Nb] != nnzb) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_pattern: rows[] inconsistent with nnzb");
    const int Nloc = Nb + Nghost;
    P.Nb = Nb;
    P.Nghost = Nghost;
    P.Nloc = Nloc;
    P.nnzb = nnzb;
    P.maxRowBlocks = 0;
    for (int i = 0; i < Nb; ++i) P.maxRowBlocks = std::max(P.maxRowBlocks, rows[i + 1] - rows[i]);
    P.nat_rowptr.assign(rows, rows + Nb + 1);
    P.nat_col.assign(cols, cols + nnzb);
    for (int i = 0; i < Nb; ++i) {
        bool hasDiag = false;
        for (int k = rows[i]; k < rows[i + 1]; ++k) {
            if (cols[k] < 0 || cols[k] >= Nloc) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_pattern: column out of range in row %d", i);
            if (k > rows[i] && cols[k] <= cols[k - 1]) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_pattern: columns of row %d not ascending", i);
            hasDiag |= (cols[k] == i);
        }
        // "diagonal entry missing" (linalg/ParallelOverlappingILU0.hpp:484-485) -> analysis failure
        if (!hasDiag) return fail(c, OPMHIP_ANALYSIS_FAILED, "set_pattern: row %d has no diagonal block", i);
    }
    std::vector<int> color;
    int ncol = 0;
    Chains CH;
    std::vector<int> chainColor;
    // OPMHIP_REORDER_AUTO: the line colouring where it pays, the greedy colouring elsewhere.  Measured (tools/ordering_by_size.py,
    // tools/config_rates.py): the chain kernels walk a chain-tile's 8-10 steps one after the other, each step a few
    // dependent rounds of loads - on 10^6 rows eight workgroups per CU hide that, on a small system nothing does (44 777-cell corner-point
    // grid: 31 Newton its/s line-coloured, 259 greedy; regular grids: the greedy colouring wins below ~125 000 cells although it needs
    // twice the iterations - with chains of 10; shorter chains move that point down), and on an irregular pattern the sweeps lose their
    // stencil form as well.  Line colouring: at least AUTO_LINE_MIN_ROWS rows, rows of at most 8 blocks, at most 15 distinct column
    // offsets (col - row) in the natural order - a structured grid handed over in its natural order; the chain length grows with the size.
    int kind = c->cfg.reorder;
    int autoChain = 10;
    if (kind == OPMHIP_REORDER_AUTO && c->ilu_fillin > 0 && !use_cpr(c)) {
        // ILU(n), n >= 1: the distance-2 colouring.  Measured (tools/ilun_study.py, profiles/ilun_study.json), ILU(1)
        // Newton its/s distance-2 against level scheduling: 193 / 102 on configs[2], 99 / 25 on configs[4], 34 / 10 at 10^6 cells - the
        // level schedule saves iterations (2 - 5 against 6 - 14 per Newton iteration) but pays 114 - 595 dependent launches per sweep
        kind = OPMHIP_REORDER_DISTANCE2_COLORING;
        if (c->cfg.verbosity > 0) std::fprintf(stderr, "opmhip: reorder auto (ILU(%d)) -> distance2_coloring (%d rows)\n", c->ilu_fillin, Nb);
    } else if (kind == OPMHIP_REORDER_AUTO) {
        // structured grids (tools/chain_by_size.py, Newton its/s): 32^3 greedy 568, chains of 4: 583; 40^3 423 / 487 (chains of 3-4); 50^3
        // 267 / 361 (4); 64^3 165 / 246 (8; 239 with 4, 208 with 10); 80^3 99 / 168 (8; 153 with 10); 100^3: 10 (section 5) - the shorter
        // the chains, the fewer dependent steps a launch walks through, the more iterations
        constexpr int AUTO_LINE_MIN_ROWS = 30000;
        autoChain = Nb < 200000 ? 4 : Nb < 700000 ? 8 : 10;
        bool regular = Nb >= AUTO_LINE_MIN_ROWS;
        std::vector<int> offs;
        for (int i = 0; i < Nb && regular; ++i) {
            if (rows[i + 1] - rows[i] > STENCIL_ROW_ENTRIES) regular = false;
            for (int k = rows[i]; k < rows[i + 1] && regular; ++k) {
                if (cols[k] >= Nb) continue;
                const int o = cols[k] - i;
                if (std::find(offs.begin(), offs.end(), o) == offs.end()) {
                    offs.push_back(o);
                    if (offs.size() > STENCIL_MAX_OFFSETS) regular = false;
                }
            }
        }
        kind = regular ? OPMHIP_REORDER_LINE_COLORING : OPMHIP_REORDER_GRAPH_COLORING_GREEDY;
        if (c->cfg.verbosity > 0) std::fprintf(stderr, "opmhip: reorder auto -> %s (%d rows)\n", regular ? "line_coloring" : "graph_coloring_greedy", Nb);
    }
    bool chained = (kind == OPMHIP_REORDER_LINE_COLORING);
    int maxLen = 1;
    // the ordering is computed on the owned-owned couplings only
    Pattern Q;
    Q.Nb = Nb;
    Q.nat_rowptr.assign(Nb + 1, 0);
    for (int i = 0; i < Nb; ++i) {
        for (int k = rows[i]; k < rows[i + 1]; ++k)
            if (cols[k] < Nb) Q.nat_col.push_back(cols[k]);
        Q.nat_rowptr[i + 1] = (int)Q.nat_col.size();
    }
    Q.nnzb = (int)Q.nat_col.size();
    switch (kind) {
        case OPMHIP_REORDER_LEVEL_SCHEDULING: levels(Q, color, ncol); break;
        case OPMHIP_REORDER_GRAPH_COLORING: color_jp(Q, color, ncol); break;
        case OPMHIP_REORDER_GRAPH_COLORING_GREEDY: color_greedy(Q, color, ncol); break;
        case OPMHIP_REORDER_LINE_COLORING: {
            maxLen = c->cfg.chain_length > 0 ? c->cfg.chain_length : (c->cfg.reorder == OPMHIP_REORDER_AUTO ? autoChain : 8);
            build_chains(Q, maxLen, CH);
            color_chains(Q, CH, chainColor, ncol);
            color.resize(Nb);
            for (int i = 0; i < Nb; ++i) color[i] = chainColor[CH.chainOf[i]];
        } break;
        case OPMHIP_REORDER_DISTANCE2_COLORING: color_distance2(Q, color, ncol); break;
        default: return fail(c, OPMHIP_INVALID_ARGUMENT, "unknown reorder kind %d", c->cfg.reorder);
    }
    // ILU(n), n >= 1 (opmhip_set_ilu_fillin_level): the fill is computed in the ordering's elimination order - the natural order for level
    // scheduling (the reference's ILU(n) runs on the natural order), colour by colour otherwise (line colouring: colour, chain, step; the
    // chains do not survive the fill).  Where the colours are independent sets of the filled pattern too (the distance-2 colouring with
    // n = 1) they stay the schedule; otherwise the rows are renumbered by the levels of the filled pattern - a topological order of its
    // couplings, which leaves the fill and the factors' arithmetic as they are.
    const int fillN = use_cpr(c) ? 0 : c->ilu_fillin;   // the CPR's fine smoother is ILU0 (setupPropertyTree.cpp:109-110)
    P.fillLevel = fillN;
    std::vector<int> frp, fcl, fdg, ibase;   // the filled pattern in the fill's elimination order
    P.fillBase.clear();
    if (fillN > 0) {
        if (Nghost > 0 || c->comm.kind != COMM_NONE)
            return fail(c, OPMHIP_INVALID_ARGUMENT, "ILU(%d) on a decomposed context is not supported (use --ilu-fillin-level=0)", fillN);
        ibase.resize(Nb);
        std::iota(ibase.begin(), ibase.end(), 0);
        if (kind != OPMHIP_REORDER_LEVEL_SCHEDULING) {
            if (chained) std::stable_sort(ibase.begin(), ibase.end(), [&](int a, int b) {
                const int ca = color[a], cb = color[b];
                if (ca != cb) return ca < cb;
                if (CH.chainOf[a] != CH.chainOf[b]) return CH.chainOf[a] < CH.chainOf[b];
                return CH.posIn[a] < CH.posIn[b];
            });
            else std::stable_sort(ibase.begin(), ibase.end(), [&](int a, int b) { return color[a] < color[b]; });
        }
        std::vector<int>& base = P.fillBase;
        base.resize(Nb);
        for (int b = 0; b < Nb; ++b) base[ibase[b]] = b;
        std::vector<int> brp(Nb + 1, 0), bcl;
        bcl.reserve(Q.nnzb);
        for (int b = 0; b < Nb; ++b) {
            const int i = ibase[b];
            const size_t o = bcl.size();
            for (int k = Q.nat_rowptr[i]; k < Q.nat_rowptr[i + 1]; ++k) bcl.push_back(base[Q.nat_col[k]]);
            std::sort(bcl.begin() + o, bcl.end());
            brp[b + 1] = (int)bcl.size();
        }
        const long long budget = (long long)ILUN_BUDGET_FACTOR * nnzb;
        if (!symbolic_fill(Nb, brp, bcl, fillN, budget, frp, fcl, fdg))
            return fail(c, OPMHIP_INVALID_ARGUMENT, "ILU(%d): the filled factors of this %d-row pattern would hold more than %lld blocks (%d x the matrix's %d); refused",
                        fillN, Nb, budget, ILUN_BUDGET_FACTOR, nnzb);
        bool keep = kind != OPMHIP_REORDER_LEVEL_SCHEDULING && !chained;
        for (int b = 0; b < Nb && keep; ++b)
            for (int q = frp[b]; q < frp[b + 1]; ++q)
                if (fcl[q] != b && color[ibase[fcl[q]]] == color[ibase[b]]) { keep = false; break; }
        if (!keep) {   // levels of the filled pattern over its row AND column couplings (as levels() does for the matrix)
            std::vector<int> lev(Nb, 0);
            ncol = 0;
            for (int b = 0; b < Nb; ++b) {
                for (int q = frp[b]; q < fdg[b]; ++q) lev[b] = std::max(lev[b], lev[fcl[q]] + 1);
                for (int q = fdg[b] + 1; q < frp[b + 1]; ++q) lev[fcl[q]] = std::max(lev[fcl[q]], lev[b] + 1);
                color[ibase[b]] = lev[b];
                ncol = std::max(ncol, lev[b] + 1);
            }
            chained = false;
        }
    }
    P.numColors = ncol;
    P.chained = chained;
    P.kindInForce = kind;
    P.chainLen = chained ? maxLen : 0;
    P.colorPrefix.assign(ncol + 1, 0);
    for (int i = 0; i < Nb; ++i) P.colorPrefix[color[i] + 1]++;
    std::partial_sum(P.colorPrefix.begin(), P.colorPrefix.end(), P.colorPrefix.begin());
    P.toOrder.resize(Nloc);
    P.fromOrder.resize(Nloc);
    for (int g = Nb; g < Nloc; ++g) P.toOrder[g] = P.fromOrder[g] = g;  // ghosts stay last, in the given order
    // (chain-tile, step) row groups of the chained ordering: rows [groupRow[g], groupRow[g+1]) ; groupNewCT[g] = 1 if the
    // group opens a new chain-tile
    std::vector<int> groupRow, groupNewCT;
    if (!chained) {
        // rows keep their natural relative order inside a colour (colorsToReordering, bda/Reorder.cpp:212-226)
        std::vector<int> next(P.colorPrefix.begin(), P.colorPrefix.end() - 1);
        for (int i = 0; i < Nb; ++i) {
            const int p = next[color[i]]++;
            P.toOrder[i] = p;
            P.fromOrder[p] = i;
        }
    } else {
        // colour -> chain-tile of TILE_ROWS chains (longest chains first, so that the live chains of a step are a
        // prefix) -> step -> chain
        int p = 0;
        for (int cc = 0; cc < ncol; ++cc) {
            std::vector<int> ids;
            for (int id = 0; id < (int)CH.rows.size(); ++id)
                if (chainColor[id] == cc) ids.push_back(id);
            std::stable_sort(ids.begin(), ids.end(), [&](int a, int b) { return CH.rows[a].size() > CH.rows[b].size(); });
            for (size_t b0 = 0; b0 < ids.size(); b0 += TILE_ROWS) {
                const size_t b1 = std::min(ids.size(), b0 + (size_t)TILE_ROWS);
                const int steps = (int)CH.rows[ids[b0]].size();
                for (int st = 0; st < steps; ++st) {
                    groupRow.push_back(p);
                    groupNewCT.push_back(st == 0 ? 1 : 0);
                    for (size_t b = b0; b < b1; ++b) {
                        if ((int)CH.rows[ids[b]].size() <= st) break;
                        const int i = CH.rows[ids[b]][st];
                        P.toOrder[i] = p;
                        P.fromOrder[p] = i;
                        ++p;
                    }
                }
            }
        }
        groupRow.push_back(p);
        if (p != Nb) return fail(c, OPMHIP_ANALYSIS_FAILED, "line colouring lost rows (%d of %d)", p, Nb);
    }
    // internal pattern: row p = natural row fromOrder[p], columns renamed and re-sorted
    // (reorderBlockedMatrixByPattern, bda/Reorder.cpp:179-207) - done once here for the pattern; values follow
    // on the device through nnzMap.
    P.rowptr.assign(Nb + 1, 0);
    P.col.resize(nnzb);
    P.nnzMap.resize(nnzb);
    P.diag.assign(Nb, -1);
    std::vector<std::pair<int, int>> tmp;
    for (int p = 0; p < Nb; ++p) {
        const int i = P.fromOrder[p];
        tmp.clear();
        for (int k = rows[i]; k < rows[i + 1]; ++k) tmp.emplace_back(P.toOrder[cols[k]], k);
        std::sort(tmp.begin(), tmp.end());
        int o = P.rowptr[p];
        for (auto& t : tmp) {
            P.col[o] = t.first;
            P.nnzMap[o] = t.second;
            if (t.first == p) P.diag[p] = o;
            ++o;
        }
        P.rowptr[p + 1] = o;
    }
    // every lower entry must point into an earlier colour, otherwise the colour-by-colour sweeps are wrong
    {
        std::vector<int> colorOf(Nb);
        for (int cc = 0; cc < ncol; ++cc)
            for (int p = P.colorPrefix[cc]; p < P.colorPrefix[cc + 1]; ++p) colorOf[p] = cc;
        for (int p = 0; p < Nb; ++p)
            for (int k = P.rowptr[p]; k < P.rowptr[p + 1]; ++k)
                if (P.col[k] != p && P.col[k] < Nb && colorOf[P.col[k]] == colorOf[p] &&
                    !(chained && CH.chainOf[P.fromOrder[P.col[k]]] == CH.chainOf[P.fromOrder[p]]))
                        return fail(c, OPMHIP_ANALYSIS_FAILED, "ordering is not a valid schedule at row %d", p);
    }
    if (fillN == 0) build_ilu0_split(P);
    else if (int rc = build_fill_split(c, frp, fcl, ibase)) return rc;
    // the rest of the matrix beside the U part, as a block-CSR of its own (ascending columns: the order of the full row without its U entries)
    P.rrowptr.assign(Nb + 1, 0);
    P.rcol.clear();
    P.rdest.assign(P.nnzb, -1);
    for (int p = 0; p < Nb; ++p) {
        for (int k = P.rowptr[p]; k < P.rowptr[p + 1]; ++k)
            if (P.fdest[k] > -2) { P.rdest[k] = (int)P.rcol.size(); P.rcol.push_back(P.col[k]); }
        P.rrowptr[p + 1] = (int)P.rcol.size();
    }
    P.nr = (int)P.rcol.size();
    P.lightL.assign(ncol, 0);
    P.lightU.assign(ncol, 0);
    if (chained) {
        for (int cc = 0; cc < ncol; ++cc) {
            bool lL = true, lU = true;
            for (int p = P.colorPrefix[cc]; p < P.colorPrefix[cc + 1] && (lL || lU); ++p) {
                const int i = P.fromOrder[p], id = CH.chainOf[i], pos = CH.posIn[i];
                const int nL = P.lrowptr[p + 1] - P.lrowptr[p], nU = P.urowptr[p + 1] - P.urowptr[p];
                if (nL > 1 || (nL == 1 && (pos == 0 || P.lcol[P.lrowptr[p]] != P.toOrder[CH.rows[id][pos - 1]]))) lL = false;
                if (nU > 1 || (nU == 1 && (pos + 1 >= (int)CH.rows[id].size() || P.ucol[P.urowptr[p]] != P.toOrder[CH.rows[id][pos + 1]]))) lU = false;
            }
            P.lightL[cc] = lL;
            P.lightU[cc] = lU;
        }
    }
    if (!chained) {
        build_tiles(P.rowptr, P.colorPrefix, groupRow, P.tiles);
    } else {
        // one sub-tile per (chain-tile, step) group: a group has <= TILE_ROWS rows by construction; over-long groups in
        // blocks are split (still processed in order inside the chain-tile)
        TileSet& T = P.tiles;
        T.row0.clear(); T.colorTile.clear(); T.ctFirst.clear(); T.colorCT.clear();
        int cnext = 0;
        for (size_t g = 0; g + 1 < groupRow.size(); ++g) {
            while (cnext <= ncol - 1 && groupRow[g] == P.colorPrefix[cnext]) {
                T.colorTile.push_back((int)T.row0.size());
                T.colorCT.push_back((int)T.ctFirst.size());
                ++cnext;
            }
            if (groupNewCT[g]) T.ctFirst.push_back((int)T.row0.size());
            int r = groupRow[g];
            const int rend = groupRow[g + 1];
            int pieces = 0;
            while (r < rend) {
                T.row0.push_back(r);
                int e = r + 1;
                while (e < rend && P.rowptr[e + 1] - P.rowptr[r] <= TILE_CAP_BLOCKS) ++e;
                r = e;
                ++pieces;
            }
            // a step cut into several sub-tiles no longer maps chain b to lane b: the lane-private light sweeps
            // (which keep the chain's previous row in registers without looking) are off for that colour
            if (pieces > 1 && cnext >= 1) P.lightL[cnext - 1] = P.lightU[cnext - 1] = 0;
        }
        T.colorTile.push_back((int)T.row0.size());
        T.colorCT.push_back((int)T.ctFirst.size());
        T.ctFirst.push_back((int)T.row0.size());
        T.row0.push_back(Nb);
        for (size_t q = 0; q + 1 < T.ctFirst.size(); ++q)
            if (T.ctFirst[q + 1] - T.ctFirst[q] > CHAIN_MAX_STEPS)
                return fail(c, OPMHIP_ANALYSIS_FAILED, "line colouring: a chain-tile has %d steps (limit %d); lower the chain length", T.ctFirst[q + 1] - T.ctFirst[q], CHAIN_MAX_STEPS);
    }

    build_schedules(P, OPMHIP_XCD_GROUP_DEFAULT);   // chain-tiles per XCD group of the launch schedules (0 = identity map), see DESIGN.md
    int rc;
    if ((rc = dev_upload(c, &P.tiles.d_spmvSched, P.tiles.spmvSched))) return rc;
    for (int part = 0; part < 2 && P.sweepStencil; ++part)
        if ((rc = upload_stencil(c, P.sw[part]))) return rc;
    if (P.tiles.stencil && (rc = upload_stencil(c, P.tiles.st))) return rc;
    if ((rc = dev_upload(c, &P.tiles.d_ctSched, P.tiles.ctSched))) return rc;
    if (fillN == 0 && (rc = dev_upload(c, &P.tiles.d_ctDesc, P.tiles.ctDesc))) return rc;
    if ((rc = dev_upload(c, &P.d_rowptr, P.rowptr))) return rc;
    if ((rc = dev_upload(c, &P.d_col, P.col))) return rc;
    if ((rc = dev_upload(c, &P.d_diag, P.diag))) return rc;
    if ((rc = dev_upload(c, &P.d_nnzMap, P.nnzMap))) return rc;
    if ((rc = dev_upload(c, &P.d_toOrder, P.toOrder))) return rc;
    if ((rc = dev_upload(c, &P.d_fromOrder, P.fromOrder))) return rc;
    if ((rc = dev_upload(c, &P.d_lrowptr, P.lrowptr))) return rc;
    if ((rc = dev_upload(c, &P.d_lcol, P.lcol))) return rc;
    if ((rc = dev_upload(c, &P.d_urowptr, P.urowptr))) return rc;
    if ((rc = dev_upload(c, &P.d_ucol, P.ucol))) return rc;
    if ((rc = dev_upload(c, &P.d_fdest, P.fdest))) return rc;
    if (fillN == 0 && (rc = dev_upload(c, &P.d_lmatch, P.lmatch))) return rc;
    if (fillN > 0 && (rc = dev_upload(c, &P.ftiles.d_row0, P.ftiles.row0))) return rc;
    if (P.rest.on) {
        if ((rc = dev_upload(c, &P.d_rdest, P.rdest))) return rc;
        if ((rc = dev_upload(c, &P.d_rrowptr, P.rrowptr))) return rc;
        if ((rc = dev_upload(c, &P.rest.d_sched, P.rest.sched))) return rc;
        if ((rc = upload_stencil(c, P.rest))) return rc;
    }
    if ((rc = dev_upload(c, &P.tiles.d_row0, P.tiles.row0))) return rc;
    if ((rc = dev_upload(c, &P.tiles.d_ctFirst, P.tiles.ctFirst))) return rc;
    return OPMHIP_SUCCESS;
}

}  // namespace opmhip
