// The host set-up of the multisegment wells' tree form (csrc/ms_wells_setup.cpp: ms_wells_tree_analyse) under AddressSanitizer + UBSan +
// libstdc++'s container assertions (test infrastructure; built and run by tests/test_ms_wells_tree_sanitized.py with g++, no GPU).  The
// unit is linked alone, with no stand-in for any HIP runtime call: that the link succeeds is the check that the unit makes none.
// A chain, a star whose hub is not the lowest segment, a forest of two components, a single segment, a cycle, two entries in one place
// and an empty column: parents, levels, child lists, level lists and the entry map against values written here.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../opm-autodiff_amd/csrc/ms_wells_setup.hpp"

using namespace opmhip;

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
typedef std::vector<int> V;

struct Csc {
    V colptr, rows;
};
// the scalar CSC arrays from each column's rows
static Csc from_columns(const std::vector<V>& cols) {
    Csc m;
    m.colptr.push_back(0);
    for (const V& c : cols) {
        m.rows.insert(m.rows.end(), c.begin(), c.end());
        m.colptr.push_back((int)m.rows.size());
    }
    return m;
}
// full 4 x 4 blocks (i, j), every diagonal block included; a column's rows ascending
static std::vector<V> block_columns(int Mb, const std::vector<std::pair<int, int>>& offdiag) {
    std::vector<V> cols(4 * Mb);
    for (int j = 0; j < Mb; ++j)
        for (int i = 0; i < Mb; ++i) {
            bool has = i == j;
            for (const auto& b : offdiag) has = has || (b.first == i && b.second == j);
            if (!has) continue;
            for (int cc = 0; cc < 4; ++cc)
                for (int r = 0; r < 4; ++r) cols[4 * j + cc].push_back(4 * i + r);
        }
    return cols;
}
static int place(int seg, int block, int r, int c) { return seg * MS_TREE_SEG + block + 4 * r + c; }
// every entry's place lies inside the well's blocks, and two entries share a place only if they share row and column
static bool map_is_sound(const Csc& m, int Mb, const MsTreeWell& t) {
    CHECK(t.dest.size() == m.rows.size(), "%zu", t.dest.size());
    std::vector<int> row_at((size_t)MS_TREE_SEG * Mb, -1), col_at((size_t)MS_TREE_SEG * Mb, -1);
    for (int c = 0; c < 4 * Mb; ++c)
        for (int k = m.colptr[c]; k < m.colptr[c + 1]; ++k) {
            const int d = t.dest[k];
            CHECK(d >= 0 && d < MS_TREE_SEG * Mb, "entry %d: place %d", k, d);
            CHECK(row_at[d] < 0 || (row_at[d] == m.rows[k] && col_at[d] == c), "entry %d shares place %d with entry (%d, %d)", k, d, row_at[d], col_at[d]);
            row_at[d] = m.rows[k];
            col_at[d] = c;
        }
    return true;
}

static bool chain() {
    const Csc m = from_columns(block_columns(4, {{0, 1}, {1, 0}, {1, 2}, {2, 1}, {2, 3}, {3, 2}}));
    MsTreeWell t;
    std::string msg;
    CHECK(ms_wells_tree_analyse(0, 4, m.colptr.data(), m.rows.data(), t, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(t.Mb == 4 && t.depth == 4 && t.width == 1, "%d %d %d", t.Mb, t.depth, t.width);
    CHECK(t.parent == (V{-1, 0, 1, 2}) && t.level == (V{0, 1, 2, 3}), "parents / levels");
    CHECK(t.child_ptr == (V{0, 1, 2, 3, 3}) && t.child == (V{1, 2, 3}), "children");
    CHECK(t.level_ptr == (V{0, 1, 2, 3, 4}) && t.level_seg == (V{0, 1, 2, 3}), "levels' segments");
    // column 0 (segment 0): its diagonal block, then block (1, 0) - rows in the child 1: the DOWN block of 1
    CHECK(t.dest[0] == place(0, MS_TREE_DIAG, 0, 0) && t.dest[3] == place(0, MS_TREE_DIAG, 3, 0), "%d %d", t.dest[0], t.dest[3]);
    CHECK(t.dest[4] == place(1, MS_TREE_DOWN, 0, 0) && t.dest[7] == place(1, MS_TREE_DOWN, 3, 0), "%d %d", t.dest[4], t.dest[7]);
    // column 5 (segment 1, second column): block (0, 1) - rows in the parent: the UP block of 1; the diagonal; block (2, 1): DOWN of 2
    const int k = m.colptr[5];
    CHECK(t.dest[k] == place(1, MS_TREE_UP, 0, 1) && t.dest[k + 2] == place(1, MS_TREE_UP, 2, 1), "%d %d", t.dest[k], t.dest[k + 2]);
    CHECK(t.dest[k + 4] == place(1, MS_TREE_DIAG, 0, 1) && t.dest[k + 7] == place(1, MS_TREE_DIAG, 3, 1), "%d %d", t.dest[k + 4], t.dest[k + 7]);
    CHECK(t.dest[k + 8] == place(2, MS_TREE_DOWN, 0, 1) && t.dest[k + 11] == place(2, MS_TREE_DOWN, 3, 1), "%d %d", t.dest[k + 8], t.dest[k + 11]);
    // the last column: block (2, 3): UP of 3, and the diagonal of 3
    const int e = m.colptr[15];
    CHECK(m.colptr[16] - e == 8 && t.dest[e + 1] == place(3, MS_TREE_UP, 1, 3) && t.dest[e + 7] == place(3, MS_TREE_DIAG, 3, 3), "%d %d", t.dest[e + 1], t.dest[e + 7]);
    if (!map_is_sound(m, 4, t)) return false;
    std::printf("ok  chain\n");
    return true;
}

static bool star() {
    // the hub is segment 2; the root is the lowest number, 0, so the hub hangs on 0 and carries 1, 3 and 4
    const Csc m = from_columns(block_columns(5, {{0, 2}, {2, 0}, {1, 2}, {2, 1}, {3, 2}, {2, 3}, {4, 2}, {2, 4}}));
    MsTreeWell t;
    std::string msg;
    CHECK(ms_wells_tree_analyse(0, 5, m.colptr.data(), m.rows.data(), t, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(t.depth == 3 && t.width == 3, "%d %d", t.depth, t.width);
    CHECK(t.parent == (V{-1, 2, 0, 2, 2}) && t.level == (V{0, 2, 1, 2, 2}), "parents / levels");
    CHECK(t.child_ptr == (V{0, 1, 1, 4, 4, 4}) && t.child == (V{2, 1, 3, 4}), "children");
    CHECK(t.level_ptr == (V{0, 1, 2, 5}) && t.level_seg == (V{0, 2, 1, 3, 4}), "levels' segments");
    // column 4 (segment 1): block (1, 1), then block (2, 1) - rows in the PARENT 2 of 1: the UP block of 1
    const int k = m.colptr[4];
    CHECK(t.dest[k] == place(1, MS_TREE_DIAG, 0, 0) && t.dest[k + 4] == place(1, MS_TREE_UP, 0, 0) && t.dest[k + 6] == place(1, MS_TREE_UP, 2, 0), "%d %d", t.dest[k], t.dest[k + 4]);
    // column 8 (segment 2): blocks (0, 2): UP of 2; (1, 2): DOWN of 1; (2, 2); (3, 2): DOWN of 3; (4, 2): DOWN of 4
    const int h = m.colptr[8];
    CHECK(m.colptr[9] - h == 20, "%d", m.colptr[9] - h);
    CHECK(t.dest[h] == place(2, MS_TREE_UP, 0, 0) && t.dest[h + 4] == place(1, MS_TREE_DOWN, 0, 0) && t.dest[h + 8] == place(2, MS_TREE_DIAG, 0, 0) &&
              t.dest[h + 13] == place(3, MS_TREE_DOWN, 1, 0) && t.dest[h + 19] == place(4, MS_TREE_DOWN, 3, 0), "hub column");
    if (!map_is_sound(m, 5, t)) return false;
    std::printf("ok  star\n");
    return true;
}

static bool forest() {
    const Csc m = from_columns(block_columns(4, {{0, 2}, {2, 0}, {1, 3}, {3, 1}}));
    MsTreeWell t;
    std::string msg;
    CHECK(ms_wells_tree_analyse(0, 4, m.colptr.data(), m.rows.data(), t, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(t.depth == 2 && t.width == 2, "%d %d", t.depth, t.width);
    CHECK(t.parent == (V{-1, -1, 0, 1}) && t.level == (V{0, 0, 1, 1}), "parents / levels");
    CHECK(t.child_ptr == (V{0, 1, 2, 2, 2}) && t.child == (V{2, 3}), "children");
    CHECK(t.level_ptr == (V{0, 2, 4}) && t.level_seg == (V{0, 1, 2, 3}), "levels' segments");
    const int k = m.colptr[12];   // segment 3: block (1, 3): UP of 3, then its diagonal
    CHECK(t.dest[k + 1] == place(3, MS_TREE_UP, 1, 0) && t.dest[k + 5] == place(3, MS_TREE_DIAG, 1, 0), "%d %d", t.dest[k + 1], t.dest[k + 5]);
    if (!map_is_sound(m, 4, t)) return false;
    std::printf("ok  forest\n");
    return true;
}

static bool single() {
    const Csc m = from_columns(block_columns(1, {}));
    MsTreeWell t;
    std::string msg;
    CHECK(ms_wells_tree_analyse(0, 1, m.colptr.data(), m.rows.data(), t, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(t.depth == 1 && t.width == 1 && t.parent == (V{-1}) && t.level == (V{0}) && t.child_ptr == (V{0, 0}) && t.child.empty(), "tree");
    CHECK(t.level_ptr == (V{0, 1}) && t.level_seg == (V{0}), "levels' segments");
    CHECK(t.dest == (V{0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15}), "column-major entries to the row-major block");
    std::printf("ok  single segment\n");
    return true;
}

static bool cycle() {
    // 0 - 1, 1 - 2 and a one-sided block (0, 2): an edge all the same
    const Csc m = from_columns(block_columns(3, {{0, 1}, {1, 0}, {1, 2}, {2, 1}, {0, 2}}));
    MsTreeWell t;
    t.Mb = 77;
    t.parent = {5};
    std::string msg;
    CHECK(ms_wells_tree_analyse(7, 3, m.colptr.data(), m.rows.data(), t, msg) == OPMHIP_INVALID_ARGUMENT, "accepted");
    CHECK(msg.find("well 7") != std::string::npos && msg.find("tree") != std::string::npos && msg.find("segments 1 and 2") != std::string::npos, "%s", msg.c_str());
    CHECK(t.Mb == 77 && t.parent == (V{5}) && t.dest.empty() && t.level.empty(), "the output was touched");
    std::printf("ok  refused: %s\n", msg.c_str());
    return true;
}

static bool duplicate_and_empty_column() {
    // two segments; column 0 names row 1 twice and row 5 (block (1, 0)) twice, not adjacent; column 6 is empty; block (0, 1) is absent
    std::vector<V> cols = {{0, 1, 5, 1, 5}, {1}, {2}, {3, 7}, {4}, {5}, {}, {7, 4}};
    const Csc m = from_columns(cols);
    MsTreeWell t;
    std::string msg;
    CHECK(ms_wells_tree_analyse(0, 2, m.colptr.data(), m.rows.data(), t, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(t.parent == (V{-1, 0}) && t.level == (V{0, 1}) && t.child_ptr == (V{0, 1, 1}) && t.child == (V{1}), "tree");
    CHECK(t.level_ptr == (V{0, 1, 2}) && t.level_seg == (V{0, 1}) && t.depth == 2 && t.width == 1, "levels");
    CHECK(t.dest == (V{place(0, MS_TREE_DIAG, 0, 0), place(0, MS_TREE_DIAG, 1, 0), place(1, MS_TREE_DOWN, 1, 0), place(0, MS_TREE_DIAG, 1, 0), place(1, MS_TREE_DOWN, 1, 0),
                       place(0, MS_TREE_DIAG, 1, 1), place(0, MS_TREE_DIAG, 2, 2), place(0, MS_TREE_DIAG, 3, 3), place(1, MS_TREE_DOWN, 3, 3),
                       place(1, MS_TREE_DIAG, 0, 0), place(1, MS_TREE_DIAG, 1, 1), place(1, MS_TREE_DIAG, 3, 3), place(1, MS_TREE_DIAG, 0, 3)}), "entry map");
    CHECK(m.colptr[6] == m.colptr[7], "column 6 is empty");
    if (!map_is_sound(m, 2, t)) return false;
    std::printf("ok  duplicate entries and an empty column\n");
    return true;
}

int main() {
    chain();
    star();
    forest();
    single();
    cycle();
    duplicate_and_empty_column();
    if (g_fail) {
        std::printf("%d checks FAILED\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
