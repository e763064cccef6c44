// Host set-up of the assembly (asm_setup.hpp).  No HIP call: capi_asm.cpp uploads what is built here.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <map>

#include "asm_setup.hpp"
#include "fluid_tables.hpp"
#include "internal.hpp"

namespace opmhip {

namespace {
// the text as fail() will cut it
int refuse(std::string& msg, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return code;
}
}  // namespace

int asm_static_check(const Pattern& P, int num_pvt, int num_sat, const double* trans, const double* area, const double* thpres, const double* poro,
                     const double* volume, const int* pvtnum, const int* satnum, std::string& msg) {
    std::vector<int> tr(P.nnzb, -1);
    for (int i = 0; i < P.Nb; ++i)
        for (int k = P.nat_rowptr[i]; k < P.nat_rowptr[i + 1]; ++k) {
            const int j = P.nat_col[k];
            if (j >= P.Nb) { tr[k] = k; continue; }  // ghost column: its row lives on the neighbouring subdomain
            const int* b = P.nat_col.data() + P.nat_rowptr[j];
            const int* e = P.nat_col.data() + P.nat_rowptr[j + 1];   // (not &nat_col[...]: one past the end for the last row)
            const int* q = std::lower_bound(b, e, i);
            if (q == e || *q != i) return refuse(msg, OPMHIP_INVALID_ARGUMENT, "set_static: pattern is not structurally symmetric at (%d,%d)", i, j);
            tr[k] = (int)(q - P.nat_col.data());
        }
    for (int k = 0; k < P.nnzb; ++k)
        if (trans[k] != trans[tr[k]] || area[k] != area[tr[k]] || (thpres && thpres[k] != thpres[tr[k]]))
            return refuse(msg, OPMHIP_INVALID_ARGUMENT, "set_static: trans/area/thpres differ between entry %d and its transpose", k);
    for (int i = 0; i < P.Nloc; ++i) {
        if (!(volume[i] > 0.0) || !(poro[i] >= 0.0)) return refuse(msg, OPMHIP_INVALID_ARGUMENT, "set_static: cell %d has non-positive volume or negative porosity", i);
        if (pvtnum && (pvtnum[i] < 0 || pvtnum[i] >= num_pvt)) return refuse(msg, OPMHIP_INVALID_ARGUMENT, "set_static: pvtnum[%d] out of range", i);
        if (satnum && (satnum[i] < 0 || satnum[i] >= num_sat)) return refuse(msg, OPMHIP_INVALID_ARGUMENT, "set_static: satnum[%d] out of range", i);
    }
    return OPMHIP_SUCCESS;
}

int asm_plan(const Pattern& P, int threads, int max_rows, AsmPlan& out, std::string& msg) {
    AsmPlan A;
    // assembly tiles: whole rows, at most `threads` entries
    std::vector<int>& row0 = A.row0;
    int r = 0;
    while (r < P.Nb) {
        row0.push_back(r);
        int e = r;
        while (e < P.Nb && P.rowptr[e + 1] - P.rowptr[r] <= threads && e - r < max_rows) ++e;
        if (e == r) return refuse(msg, OPMHIP_ANALYSIS_FAILED, "set_static: row %d has more than %d blocks", r, threads);
        r = e;
    }
    row0.push_back(P.Nb);
    A.ntiles = (int)row0.size() - 1;
    // Schedule: the ILU ordering stores the colours one after the other, so a cell and its neighbours of another
    // colour sit at the same RELATIVE position of two far-apart regions.  Tiles are therefore launched by their
    // relative position inside their colour, colours interleaved: the intensive quantities a tile gathers from
    // the other colours were, or will shortly be, touched by the tiles running next to it and stay in L2.
    // One record per tile (first row, end row, first entry, end entry): the kernel's first load.
    std::vector<int>& sched = A.sched;
    {
        std::vector<int> colorOfTile(A.ntiles), first(P.numColors + 1, A.ntiles), cnt(P.numColors, 0);
        int cc = 0;
        for (int t = 0; t < A.ntiles; ++t) {
            while (cc + 1 < P.numColors && row0[t] >= P.colorPrefix[cc + 1]) ++cc;
            colorOfTile[t] = cc;
            first[cc] = std::min(first[cc], t);
            cnt[cc]++;
        }
        std::vector<int> order(A.ntiles);
        for (int t = 0; t < A.ntiles; ++t) order[t] = t;
        auto frac = [&](int t) { const int q = colorOfTile[t]; return (double)(t - first[q]) / (double)cnt[q]; };
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return frac(x) < frac(y); });
        // Workgroup b of the launch runs on XCD b % 8; every XCD gets one contiguous eighth of this order, so that the
        // neighbour records several nearby tiles gather are found in that XCD's own L2.  The permutation is folded
        // into the schedule (record b = what workgroup b, b + gridDim, ... work on); the last records may be empty.
        const int chunk = (A.ntiles + 7) / 8;
        A.nsched = 8 * chunk;
        sched.assign((size_t)4 * A.nsched, 0);
        for (int b = 0; b < A.nsched; ++b) {
            const int pos = (b & 7) * chunk + (b >> 3);
            if (pos >= A.ntiles) continue;
            const int t = order[pos];
            sched[(size_t)4 * b] = row0[t];
            sched[(size_t)4 * b + 1] = row0[t + 1];
            sched[(size_t)4 * b + 2] = P.rowptr[row0[t]];
            sched[(size_t)4 * b + 3] = P.rowptr[row0[t + 1]];
        }
    }
    // Per workgroup and lane = per entry (I,J) of the workgroup's tile: the column and an entry word - everything a
    // lane needs to know about its entry, addressed by the workgroup index alone (no dependent load):
    //   bits 0-5  row of the entry inside its tile
    //   bit  6    upwind tie-break of a face with equal pressures and volumes: "the DOF which exhibits the smaller
    //             global index" (ebos/eclfluxmodule.hh:303-314) - set if the global id of I (the index of the natural
    //             order; the global id in decomposed runs) is below that of J, never the position in the ILU ordering
    //   bits 8-15 the row's entries in ascending natural-column order (ascending GLOBAL neighbour id in decomposed
    //             runs): in-row position of the entry that comes i-th, stored with the row's i-th entry - the order
    //             in which the natural-order CPU path sums the face fluxes of a cell
    //   bit  16, bits 17-23 (split assembly, ILU0 patterns without ghost columns): the block belongs to the U stream (1) or to the
    //             rest stream (0), and its place there counted from the first block of the tile's rows in that stream - a tile is a
    //             run of whole rows, so it owns one contiguous run of either stream
    {
        const int T = threads;
        std::vector<int>& desc = A.desc;
        desc.assign((size_t)2 * T * A.nsched, 0);
        std::vector<int> byNat;
        const bool places = P.fillLevel == 0 && P.Nghost == 0 && (int)P.rdest.size() == P.nnzb && (int)P.fdest.size() == P.nnzb;
        A.split_ok = places;
        for (int b = 0; b < A.nsched; ++b) {
            const int tr0 = sched[(size_t)4 * b], tr1 = sched[(size_t)4 * b + 1], tk0 = sched[(size_t)4 * b + 2];
            for (int p = tr0; p < tr1; ++p) {
                const int kb = P.rowptr[p], ke = P.rowptr[p + 1];
                byNat.resize(ke - kb);
                for (int k = kb; k < ke; ++k) byNat[k - kb] = k;
                if (P.gids.empty())
                    std::sort(byNat.begin(), byNat.end(), [&](int x, int y) { return P.nnzMap[x] < P.nnzMap[y]; });
                else  // natural local id of a column = fromOrder[internal col]
                    std::sort(byNat.begin(), byNat.end(),
                              [&](int x, int y) { return P.gids[P.fromOrder[P.col[x]]] < P.gids[P.fromOrder[P.col[y]]]; });
                const int in = P.fromOrder[p];
                const long long gi = P.gids.empty() ? (long long)in : P.gids[in];
                for (int k = kb; k < ke; ++k) {
                    const int jn = P.fromOrder[P.col[k]];
                    const long long gj = P.gids.empty() ? (long long)jn : P.gids[jn];
                    const size_t o = (size_t)2 * ((size_t)b * T + (k - tk0));
                    desc[o] = P.col[k];
                    desc[o + 1] = (p - tr0) | (gi < gj ? 64 : 0) | ((byNat[k - kb] - kb) << 8);
                    if (places) {
                        const bool upper = P.rdest[k] < 0;
                        const int rel = upper ? (-2 - P.fdest[k]) - P.urowptr[tr0] : P.rdest[k] - P.rrowptr[tr0];
                        if (rel < 0 || rel >= T || (upper && P.fdest[k] > -2)) A.split_ok = false;   // (cannot happen on such a pattern: the assembly then keeps writing the matrix itself)
                        else desc[o + 1] |= (upper ? 1 << 16 : 0) | (rel << 17);
                    }
                }
            }
        }
    }
    out = std::move(A);
    return OPMHIP_SUCCESS;
}

int water_compaction_tables(int num_tables, const int* num_pressure, const int* num_sw, const double* pressure, const double* sw, const double* pv_mult,
                            const double* trans_mult, WaterCompactionTables& out, std::string& msg) {
    std::vector<int> desc;
    std::vector<double> data;
    size_t op = 0, os = 0, ov = 0;
    for (int t = 0; t < num_tables; ++t) {
        const int np = num_pressure[t], ns = num_sw[t];
        if (np < 2 || ns < 2) return refuse(msg, OPMHIP_INVALID_ARGUMENT, "set_water_compaction: table %d needs at least two pressure and two saturation nodes", t);
        for (int i = 1; i < np; ++i) if (!(pressure[op + i] > pressure[op + i - 1])) return refuse(msg, OPMHIP_INVALID_ARGUMENT, "set_water_compaction: pressure nodes of table %d not ascending", t);
        for (int j = 1; j < ns; ++j) if (!(sw[os + j] > sw[os + j - 1])) return refuse(msg, OPMHIP_INVALID_ARGUMENT, "set_water_compaction: saturation nodes of table %d not ascending", t);
        const int atP = (int)data.size();
        data.insert(data.end(), pressure + op, pressure + op + np);
        const int atS = (int)data.size();
        data.insert(data.end(), sw + os, sw + os + ns);
        const int atV = (int)data.size();
        data.insert(data.end(), pv_mult + ov, pv_mult + ov + (size_t)np * ns);
        int atT = -1;
        if (trans_mult) { atT = (int)data.size(); data.insert(data.end(), trans_mult + ov, trans_mult + ov + (size_t)np * ns); }
        const int d[6] = {np, ns, atP, atS, atV, atT};
        desc.insert(desc.end(), d, d + 6);
        op += np; os += ns; ov += (size_t)np * ns;
    }
    out.desc = std::move(desc);
    out.data = std::move(data);
    return OPMHIP_SUCCESS;
}

int cell_end_points(const EndPointsCheck& K, size_t at, int cell, int region, size_t pos, std::string& msg) {
    const double* u = &K.sat_eps[(size_t)region * EPS_COUNT];
    double s[EPS_COUNT];
    for (int f = 0; f < EPS_COUNT; ++f) {
        s[f] = K.src && K.src[f] ? K.src[f][at] : u[f];
        if (!std::isfinite(s[f])) return refuse(msg, OPMHIP_INVALID_ARGUMENT, "%s: %send point %d of cell %d is not finite", K.call, K.kind, f, cell);
    }
    const std::string why = end_points_refusal(s, u, (K.cfg & 1) != 0, (K.cfg >> 2) & 3, (K.cfg >> 4) & 3, (K.cfg >> 6) & 3);
    if (!why.empty()) return refuse(msg, OPMHIP_INVALID_ARGUMENT, "%s: the %send points of cell %d (saturation region %d) %s", K.call, K.kind, cell, region, why.c_str());
    if (K.v)
        for (int f = 0; f < EPS_COUNT; ++f) K.v[(size_t)f * K.N + pos] = s[f];
    return OPMHIP_SUCCESS;
}

int source_cells(int n, const int* cells, const double* source, const double* dsource, int Nloc, const int* toOrder, SourceCells& out, std::string& msg) {
    SourceCells S;
    std::map<int, int> slot;
    for (int i = 0; i < n; ++i) {
        if (cells[i] < 0 || cells[i] >= Nloc) return refuse(msg, OPMHIP_INVALID_ARGUMENT, "set_source_cells: cell %d of %d", cells[i], Nloc);
        auto it = slot.find(cells[i]);
        int sidx;
        if (it == slot.end()) {
            sidx = (int)S.pos.size();
            slot.emplace(cells[i], sidx);
            S.pos.push_back(toOrder[cells[i]]);
            S.val.insert(S.val.end(), 3, 0.0);
            S.dval.insert(S.dval.end(), 9, 0.0);
        } else sidx = it->second;
        for (int q = 0; q < 3; ++q) {
            if (!std::isfinite(source[(size_t)i * 3 + q])) return refuse(msg, OPMHIP_INVALID_ARGUMENT, "set_source_cells: source of cell %d is not finite", cells[i]);
            S.val[(size_t)sidx * 3 + q] += source[(size_t)i * 3 + q];
        }
        if (dsource)
            for (int q = 0; q < 9; ++q) S.dval[(size_t)sidx * 9 + q] += dsource[(size_t)i * 9 + q];
    }
    out = std::move(S);
    return OPMHIP_SUCCESS;
}

}  // namespace opmhip
