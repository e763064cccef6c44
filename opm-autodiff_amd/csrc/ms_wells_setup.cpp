// Host set-up of the tree form of the device-resident multisegment wells (ms_wells_setup.hpp).  No HIP call: capi.cpp uploads what is
// built here.
#include <algorithm>
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

}   // namespace opmhip
