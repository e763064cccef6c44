// Host set-up of the device-resident multisegment wells (ms_wells_setup.hpp).  No HIP call: capi_ms_wells.cpp uploads what is
// built here.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <utility>

#include "ms_wells_setup.hpp"

namespace opmhip {

namespace {
// the text as fail() will cut it
int refuse(std::string& msg, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return OPMHIP_INVALID_ARGUMENT;
}
// the dense cap's text: under DENSE from the list check, under AUTO also from the layout, for a well that neither form takes
int over_M(std::string& msg, int w, int Mb) {
    return refuse(msg, "set_ms_wells: well %d has %d segments, M = %lld > OPMHIP_MS_WELLS_MAX_M = %d: above the size cap of the device form (use the callback form)",
                  w, Mb, 4 * (long long)Mb, OPMHIP_MS_WELLS_MAX_M);
}
}  // namespace

int ms_wells_tree_analyse(int well, int Mb, const int* colptr, const int* rows, MsTreeWell& out, std::string& msg) {
    const int M = 4 * Mb, nnz = colptr[M];
    // the block graph: every off-diagonal block once, as (lower, higher) segment
    std::vector<std::pair<int, int>> edges;
    for (int c = 0; c < M; ++c)
        for (int k = colptr[c]; k < colptr[c + 1]; ++k) {
            const int i = rows[k] / 4, j = c / 4;
            if (i != j) edges.emplace_back(std::min(i, j), std::max(i, j));
        }
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    std::vector<int> aptr((size_t)Mb + 1, 0), adj(2 * edges.size());
    for (const auto& e : edges) { aptr[(size_t)e.first + 1]++; aptr[(size_t)e.second + 1]++; }
    for (int i = 0; i < Mb; ++i) aptr[(size_t)i + 1] += aptr[i];
    {
        // edges are sorted by (lower, higher): a segment's lower neighbours arrive before its higher ones, each group ascending
        std::vector<int> fill(aptr.begin(), aptr.end() - 1);
        for (const auto& e : edges) adj[(size_t)fill[e.second]++] = e.first;
        for (const auto& e : edges) adj[(size_t)fill[e.first]++] = e.second;
        for (int i = 0; i < Mb; ++i) std::sort(adj.begin() + aptr[i], adj.begin() + aptr[(size_t)i + 1]);
    }
    // breadth first from the lowest segment number not yet reached: parents, levels; a neighbour already reached that is not the
    // parent closes a cycle
    MsTreeWell t;
    t.Mb = Mb;
    t.parent.assign(Mb, -1);
    t.level.assign(Mb, -1);
    std::vector<int> queue;
    queue.reserve(Mb);
    for (int root = 0; root < Mb; ++root) {
        if (t.level[root] >= 0) continue;
        t.level[root] = 0;
        size_t head = queue.size();
        queue.push_back(root);
        for (; head < queue.size(); ++head) {
            const int u = queue[head];
            for (int k = aptr[u]; k < aptr[(size_t)u + 1]; ++k) {
                const int v = adj[k];
                if (v == t.parent[u]) continue;
                if (t.level[v] >= 0)
                    return refuse(msg, "set_ms_wells: well %d: the block pattern of D is not a tree (the blocks between segments %d and %d close a cycle); "
                                       "the tree form takes wells whose segments form a tree or a forest only",
                                  well, std::min(u, v), std::max(u, v));
                t.parent[v] = u;
                t.level[v] = t.level[u] + 1;
                queue.push_back(v);
            }
        }
    }
    t.child_ptr.assign((size_t)Mb + 1, 0);
    for (int i = 0; i < Mb; ++i) {
        t.depth = std::max(t.depth, t.level[i] + 1);
        if (t.parent[i] >= 0) t.child_ptr[(size_t)t.parent[i] + 1]++;
    }
    for (int i = 0; i < Mb; ++i) t.child_ptr[(size_t)i + 1] += t.child_ptr[i];
    t.child.assign((size_t)t.child_ptr[Mb], 0);
    t.level_ptr.assign((size_t)t.depth + 1, 0);
    for (int i = 0; i < Mb; ++i) t.level_ptr[(size_t)t.level[i] + 1]++;
    for (int l = 0; l < t.depth; ++l) {
        t.width = std::max(t.width, t.level_ptr[(size_t)l + 1]);
        t.level_ptr[(size_t)l + 1] += t.level_ptr[l];
    }
    t.level_seg.assign(Mb, 0);
    {
        std::vector<int> cfill(t.child_ptr.begin(), t.child_ptr.end() - 1), lfill(t.level_ptr.begin(), t.level_ptr.end() - 1);
        for (int i = 0; i < Mb; ++i) {   // ascending i: both lists come out ascending
            if (t.parent[i] >= 0) t.child[(size_t)cfill[t.parent[i]]++] = i;
            t.level_seg[(size_t)lfill[t.level[i]]++] = i;
        }
    }
    t.dest.assign((size_t)nnz, 0);
    for (int c = 0; c < M; ++c)
        for (int k = colptr[c]; k < colptr[c + 1]; ++k) {
            const int i = rows[k] / 4, j = c / 4, place = 4 * (rows[k] % 4) + c % 4;
            if (i == j) t.dest[k] = j * MS_TREE_SEG + MS_TREE_DIAG + place;
            else if (t.parent[j] == i) t.dest[k] = j * MS_TREE_SEG + MS_TREE_UP + place;     // row in the parent of j
            else t.dest[k] = i * MS_TREE_SEG + MS_TREE_DOWN + place;                         // row in the child i of j
        }
    out = std::move(t);
    return OPMHIP_SUCCESS;
}

int ms_wells_list_check(const opmhip_ms_wells& ms, int form, int Nb, MsWellsList& out, std::string& msg) {
    const int nw = ms.num_ms_wells;
    if (ms.Mb_pointers[0] != 0 || ms.block_pointers[0] != 0 || ms.Dnnz_pointers[0] != 0)
        return refuse(msg, "set_ms_wells: inconsistent pointers (Mb_pointers, block_pointers and Dnnz_pointers start at 0)");
    MsWellsList L;
    L.all.resize(nw);
    L.wform.assign(nw, 0);
    for (int w = 0; w < nw; ++w) {
        const int Mb = ms.Mb_pointers[w + 1] - ms.Mb_pointers[w], nblk = ms.block_pointers[w + 1] - ms.block_pointers[w];
        const int nnz = ms.Dnnz_pointers[w + 1] - ms.Dnnz_pointers[w];
        if (Mb < 1 || nblk < 0 || nnz < 0) return refuse(msg, "set_ms_wells: inconsistent pointers (well %d: %d segments, %d blocks, %d entries of D)", w, Mb, nblk, nnz);
        const bool overM = 4 * (long long)Mb > OPMHIP_MS_WELLS_MAX_M;
        if (overM && form == OPMHIP_MS_WELLS_DENSE) return over_M(msg, w, Mb);
        L.wform[w] = form == OPMHIP_MS_WELLS_TREE || (form == OPMHIP_MS_WELLS_AUTO && overM);
        if (L.wform[w] && Mb > OPMHIP_MS_WELLS_TREE_MAX_SEGMENTS)
            return refuse(msg, "set_ms_wells: well %d has %d segments > OPMHIP_MS_WELLS_TREE_MAX_SEGMENTS = %d: above the size cap of the tree form (use the callback form)",
                          w, Mb, OPMHIP_MS_WELLS_TREE_MAX_SEGMENTS);
        MsWellDesc& d = L.all[w];
        d.Mb = Mb; d.nblk = nblk;
        d.seg0 = ms.Mb_pointers[w] + w; d.blk0 = ms.block_pointers[w];
        d.dcol0 = 4 * ms.Mb_pointers[w] + w; d.dnz0 = ms.Dnnz_pointers[w];
        d.inv0 = 0;
        d.well = w;
        if (!L.wform[w]) {
            d.inv0 = (int)L.invDoubles;
            L.invDoubles += (size_t)16 * Mb * Mb;
            if (L.invDoubles * sizeof(double) > (size_t)OPMHIP_MS_WELLS_MAX_KIB * 1024)
                return refuse(msg, "set_ms_wells: the dense D^-1 of the list exceed OPMHIP_MS_WELLS_MAX_KIB = %d KiB at well %d: above the size cap of the device form (use the callback form)",
                              OPMHIP_MS_WELLS_MAX_KIB, w);
        }
        L.maxM = std::max(L.maxM, 4 * Mb);
        const int* br = ms.Brows + d.seg0;
        bool ok = br[0] == 0 && br[Mb] == nblk;
        for (int r = 0; r < Mb && ok; ++r) ok = br[r] <= br[r + 1];
        const int* cp = ms.Dcol_pointers + d.dcol0;
        ok = ok && cp[0] == 0 && cp[4 * Mb] == nnz;
        for (int q = 0; q < 4 * Mb && ok; ++q) ok = cp[q] <= cp[q + 1];
        if (!ok) return refuse(msg, "set_ms_wells: inconsistent pointers (Brows or Dcol_pointers of well %d)", w);
        for (int k = 0; k < nnz; ++k) {
            if (ms.Drows[d.dnz0 + k] < 0 || ms.Drows[d.dnz0 + k] >= 4 * Mb)
                return refuse(msg, "set_ms_wells: well %d, entry %d of D: row %d outside [0, %d)", w, k, ms.Drows[d.dnz0 + k], 4 * Mb);
            if (!std::isfinite(ms.Dvals[d.dnz0 + k])) return refuse(msg, "set_ms_wells: well %d, entry %d of D is not finite", w, k);
        }
    }
    L.nseg = (size_t)ms.Mb_pointers[nw]; L.nblk = (size_t)ms.block_pointers[nw]; L.nnz = (size_t)ms.Dnnz_pointers[nw];
    for (size_t k = 0; k < L.nblk; ++k)
        if (ms.Bcols[k] < 0 || ms.Bcols[k] >= Nb) return refuse(msg, "set_ms_wells: block %zu: cell %d out of range [0, %d)", k, ms.Bcols[k], Nb);
    out = std::move(L);
    return OPMHIP_SUCCESS;
}

int ms_wells_list_layout(const opmhip_ms_wells& ms, int form, int Nb, const int* toOrder, const MsWellsList& list, MsWellsLayout& out, std::string& msg) {
    const int nw = ms.num_ms_wells;
    MsWellsLayout Y;
    // the tree wells: the segment tree and the entries' places, the index lists one after the other
    for (int w = 0; w < nw; ++w) {
        const MsWellDesc& d = list.all[w];
        if (!list.wform[w]) { Y.desc.push_back(d); continue; }
        MsTreeWell t;
        if (ms_wells_tree_analyse(w, d.Mb, ms.Dcol_pointers + d.dcol0, ms.Drows + d.dnz0, t, msg)) {
            if (form == OPMHIP_MS_WELLS_AUTO) return over_M(msg, w, d.Mb);   // (neither form takes it)
            return OPMHIP_INVALID_ARGUMENT;
        }
        MsTreeDesc td{};
        td.Mb = d.Mb; td.nblk = d.nblk; td.seg0 = d.seg0; td.blk0 = d.blk0; td.dcol0 = d.dcol0; td.dnz0 = d.dnz0; td.well = w;
        td.depth = t.depth; td.width = t.width;
        auto put = [&](const std::vector<int>& v) { const int at = (int)Y.tint.size(); Y.tint.insert(Y.tint.end(), v.begin(), v.end()); return at; };
        if (Y.tint.size() + 4 * (size_t)d.Mb + 2 + t.dest.size() > (size_t)INT_MAX || (Y.facDoubles + (size_t)MS_TREE_SEG * d.Mb) > (size_t)INT_MAX)
            return refuse(msg, "set_ms_wells: the tree wells' index lists exceed 2^31 entries at well %d: above the size cap of the tree form", w);
        td.par0 = put(t.parent); td.cptr0 = put(t.child_ptr); td.child0 = put(t.child); td.lptr0 = put(t.level_ptr); td.lseg0 = put(t.level_seg);
        td.dest0 = put(t.dest);
        td.fac0 = (int)Y.facDoubles;
        Y.facDoubles += (size_t)MS_TREE_SEG * d.Mb;
        Y.treeSeg = std::max(Y.treeSeg, d.Mb);
        Y.treeDepth = std::max(Y.treeDepth, t.depth);
        Y.tdesc.push_back(td);
    }
    Y.cell.resize(list.nblk);
    Y.blkrow.resize(list.nblk);
    std::vector<char> seen((size_t)Nb, 0);
    for (int w = 0; w < nw; ++w) {
        const int* br = ms.Brows + list.all[w].seg0;
        for (int r = 0; r < list.all[w].Mb; ++r)
            for (int k = br[r]; k < br[r + 1]; ++k) Y.blkrow[(size_t)list.all[w].blk0 + k] = r;
    }
    for (size_t k = 0; k < list.nblk; ++k) {
        Y.cell[k] = toOrder[ms.Bcols[k]];
        if (seen[(size_t)ms.Bcols[k]]) Y.shared = true;
        seen[(size_t)ms.Bcols[k]] = 1;
    }
    out = std::move(Y);
    return OPMHIP_SUCCESS;
}

}   // namespace opmhip
