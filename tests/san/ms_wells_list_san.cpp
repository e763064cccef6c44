// The host set-up of the device-resident multisegment wells (csrc/ms_wells_setup.cpp: ms_wells_list_check, ms_wells_list_layout) under
// AddressSanitizer + UBSan + libstdc++'s container assertions (test infrastructure; built and run by
// tests/test_ms_wells_list_sanitized.py with g++, no GPU).  The unit is linked alone, with no stand-in for any HIP runtime call: that the
// link succeeds is the check that the unit makes none.
// Every refusal of the list check, one defect each, in the order the code tests them, with the words the GPU tests look for; a list with
// two defects; the descriptors, forms, totals and the layout of small lists against values written here.
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>
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
typedef std::vector<std::pair<int, int>> Pairs;

// the rows of every scalar column of D: full 4 x 4 blocks (i, j), every diagonal block included; a column's rows ascending
static std::vector<V> block_columns(int Mb, const Pairs& offdiag) {
    std::vector<std::vector<char>> has(Mb, std::vector<char>(Mb, 0));
    for (int i = 0; i < Mb; ++i) has[i][i] = 1;
    for (const auto& b : offdiag) has[b.first][b.second] = 1;
    std::vector<V> cols(4 * Mb);
    for (int j = 0; j < Mb; ++j)
        for (int i = 0; i < Mb; ++i) {
            if (!has[i][j]) continue;
            for (int cc = 0; cc < 4; ++cc)
                for (int r = 0; r < 4; ++r) cols[4 * j + cc].push_back(4 * i + r);
        }
    return cols;
}
static Pairs chain_blocks(int Mb) {
    Pairs p;
    for (int i = 0; i + 1 < Mb; ++i) { p.emplace_back(i, i + 1); p.emplace_back(i + 1, i); }
    return p;
}
// the caller's arrays of opmhip_ms_wells, well after well
struct List {
    V Mbp{0}, Brows, blkp{0}, Bcols, Dcolp, Drows, Dnzp{0};
    std::vector<double> Bvals, Cvals, Dvals;
    // segCells: per segment the cells of its blocks
    void add(const std::vector<V>& segCells, const Pairs& offdiag = {}) {
        const int Mb = (int)segCells.size();
        Mbp.push_back(Mbp.back() + Mb);
        int nb = 0;
        Brows.push_back(0);
        for (const V& s : segCells) {
            Bcols.insert(Bcols.end(), s.begin(), s.end());
            nb += (int)s.size();
            Brows.push_back(nb);
        }
        blkp.push_back(blkp.back() + nb);
        Bvals.resize(12 * Bcols.size(), 1.0);
        Cvals.resize(12 * Bcols.size(), 1.0);
        int n = 0;
        Dcolp.push_back(0);
        for (const V& c : block_columns(Mb, offdiag)) {
            Drows.insert(Drows.end(), c.begin(), c.end());
            n += (int)c.size();
            Dcolp.push_back(n);
        }
        Dnzp.push_back(Dnzp.back() + n);
        Dvals.resize(Drows.size(), 1.0);
    }
    // a well of Mb segments with one block, in its first segment
    void add_long(int Mb, int cell, const Pairs& offdiag = {}) {
        std::vector<V> segs(Mb);
        segs[0] = {cell};
        add(segs, offdiag);
    }
    opmhip_ms_wells view() const {
        opmhip_ms_wells m{};
        m.num_ms_wells = (int)Mbp.size() - 1;
        m.dim = 3; m.dim_wells = 4;
        m.Mb_pointers = Mbp.data(); m.Brows = Brows.data(); m.block_pointers = blkp.data(); m.Bcols = Bcols.data();
        m.Bvals = Bvals.data(); m.Cvals = Cvals.data(); m.Dcol_pointers = Dcolp.data(); m.Drows = Drows.data(); m.Dvals = Dvals.data();
        m.Dnnz_pointers = Dnzp.data();
        return m;
    }
};
// two sound wells in 6 cells: 2 segments with blocks in cells 0 | 1, 2 and 3 segments with blocks in cells 3 | - | 4
static List base() {
    List l;
    l.add({{0}, {1, 2}});
    l.add({{3}, {}, {4}});
    return l;
}
static bool same_desc(const MsWellDesc& d, int Mb, int nblk, int seg0, int blk0, int dcol0, int dnz0, int inv0, int well) {
    return d.Mb == Mb && d.nblk == nblk && d.seg0 == seg0 && d.blk0 == blk0 && d.dcol0 == dcol0 && d.dnz0 == dnz0 && d.inv0 == inv0 && d.well == well;
}

// the list check refuses with every word of `words` in its text and leaves `out` alone
static bool refused(const char* name, const List& l, int form, int Nb, std::initializer_list<const char*> words) {
    const opmhip_ms_wells m = l.view();
    MsWellsList out;
    out.maxM = 77;
    std::string msg;
    CHECK(ms_wells_list_check(m, form, Nb, out, msg) == OPMHIP_INVALID_ARGUMENT, "%s: accepted", name);
    for (const char* w : words) CHECK(msg.find(w) != std::string::npos, "%s: no '%s' in: %s", name, w, msg.c_str());
    CHECK(out.maxM == 77 && out.all.empty() && out.wform.empty(), "%s: the output was touched", name);
    std::printf("ok  refused: %s: %s\n", name, msg.c_str());
    return true;
}

static bool refusals() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    bool ok = true;
    { CHECK(base().Mbp == (V{0, 2, 5}) && base().Dnzp == (V{0, 32, 80}) && base().blkp == (V{0, 3, 5}), "the base list"); }
    { List l = base(); l.Mbp[0] = 1; ok = refused("pointers not from 0", l, OPMHIP_MS_WELLS_DENSE, 6, {"inconsistent pointers", "start at 0"}) && ok; }
    { List l = base(); l.Mbp[2] = 2; ok = refused("Mb < 1", l, OPMHIP_MS_WELLS_DENSE, 6, {"inconsistent pointers", "well 1", "0 segments"}) && ok; }
    {   // 4 Mb one segment above the dense cap
        List l;
        l.add({{0}});
        l.add_long(OPMHIP_MS_WELLS_MAX_M / 4 + 1, 1);
        ok = refused("dense cap under DENSE", l, OPMHIP_MS_WELLS_DENSE, 6, {"well 1", "65 segments", "M = 260", "OPMHIP_MS_WELLS_MAX_M", "cap"}) && ok;
    }
    {
        List l;
        l.add_long(OPMHIP_MS_WELLS_TREE_MAX_SEGMENTS + 1, 0);
        ok = refused("tree cap under TREE", l, OPMHIP_MS_WELLS_TREE, 6, {"well 0", "1025 segments", "OPMHIP_MS_WELLS_TREE_MAX_SEGMENTS", "cap", "tree"}) && ok;
    }
    {   // the largest dense well takes 512 KiB: the 65th is the first that can cross the list's cap (well 64, the second of the last pair)
        List l;
        const int n = OPMHIP_MS_WELLS_MAX_KIB / 512 + 1;
        for (int w = 0; w < n; ++w) l.add_long(OPMHIP_MS_WELLS_MAX_M / 4, w % 6);
        ok = refused("KiB cap", l, OPMHIP_MS_WELLS_DENSE, 6, {"OPMHIP_MS_WELLS_MAX_KIB", "at well 64", "cap"}) && ok;
        MsWellsList out;   // one well fewer: exactly at the cap, taken
        std::string msg;
        l = List();
        for (int w = 0; w < n - 1; ++w) l.add_long(OPMHIP_MS_WELLS_MAX_M / 4, w % 6);
        const opmhip_ms_wells m = l.view();
        CHECK(ms_wells_list_check(m, OPMHIP_MS_WELLS_DENSE, 6, out, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
        CHECK(out.invDoubles * sizeof(double) == (size_t)OPMHIP_MS_WELLS_MAX_KIB * 1024 && out.all[63].inv0 == 63 * 65536, "%zu", out.invDoubles);
    }
    { List l = base(); l.Brows[1] = 4; ok = refused("Brows not ascending", l, OPMHIP_MS_WELLS_DENSE, 6, {"inconsistent pointers", "Brows", "well 0"}) && ok; }
    { List l = base(); l.Brows[6] = 1; ok = refused("Brows not ending at nblk", l, OPMHIP_MS_WELLS_DENSE, 6, {"inconsistent pointers", "Brows", "well 1"}) && ok; }
    { List l = base(); l.Dcolp[1] = 9; ok = refused("Dcol_pointers not ascending", l, OPMHIP_MS_WELLS_DENSE, 6, {"inconsistent pointers", "Dcol_pointers", "well 0"}) && ok; }
    { List l = base(); l.Dcolp[9 + 12] = 47; ok = refused("Dcol_pointers not ending at nnz", l, OPMHIP_MS_WELLS_DENSE, 6, {"inconsistent pointers", "Dcol_pointers", "well 1"}) && ok; }
    { List l = base(); l.Drows[32 + 5] = 12; ok = refused("Drows at 4 Mb", l, OPMHIP_MS_WELLS_DENSE, 6, {"well 1", "entry 5", "row 12 outside [0, 12)"}) && ok; }
    { List l = base(); l.Drows[7] = -1; ok = refused("Drows at -1", l, OPMHIP_MS_WELLS_DENSE, 6, {"well 0", "entry 7", "row -1 outside [0, 8)"}) && ok; }
    { List l = base(); l.Dvals[3] = nan; ok = refused("NaN in Dvals", l, OPMHIP_MS_WELLS_DENSE, 6, {"well 0", "entry 3", "not finite"}) && ok; }
    { List l = base(); l.Dvals[32] = -inf; ok = refused("Inf in Dvals", l, OPMHIP_MS_WELLS_TREE, 6, {"well 1", "entry 0", "not finite"}) && ok; }
    { List l = base(); l.Bcols[4] = 6; ok = refused("Bcols at Nb", l, OPMHIP_MS_WELLS_DENSE, 6, {"block 4", "cell 6", "out of range [0, 6)"}) && ok; }
    { List l = base(); l.Bcols[0] = -1; ok = refused("Bcols at -1", l, OPMHIP_MS_WELLS_AUTO, 6, {"block 0", "cell -1", "out of range"}) && ok; }
    return ok;
}

static bool two_defects() {
    // the first block's cell is out of range and a row of the second well's D is: the wells are looked at before the cells
    List l = base();
    l.Bcols[0] = 6;
    l.Drows[32] = -1;
    if (!refused("two defects, D's row first", l, OPMHIP_MS_WELLS_DENSE, 6, {"well 1", "entry 0", "outside"})) return false;
    // a NaN in the first well and a second well without segments: the wells in list order
    l = base();
    l.Dvals[31] = std::numeric_limits<double>::quiet_NaN();
    l.Mbp[2] = 2;
    return refused("two defects, the first well first", l, OPMHIP_MS_WELLS_DENSE, 6, {"well 0", "entry 31", "not finite"});
}

static bool one_well_one_segment() {
    List l;
    l.add({{3}});
    const opmhip_ms_wells m = l.view();
    const V to = {0, 1, 2, 3, 4};
    MsWellsList L;
    MsWellsLayout Y;
    std::string msg;
    CHECK(ms_wells_list_check(m, OPMHIP_MS_WELLS_DENSE, 5, L, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(L.all.size() == 1 && same_desc(L.all[0], 1, 1, 0, 0, 0, 0, 0, 0) && L.wform == (V{0}), "descriptor");
    CHECK(L.invDoubles == 16 && L.maxM == 4 && L.nseg == 1 && L.nblk == 1 && L.nnz == 16, "%zu %d %zu %zu %zu", L.invDoubles, L.maxM, L.nseg, L.nblk, L.nnz);
    CHECK(ms_wells_list_layout(m, OPMHIP_MS_WELLS_DENSE, 5, to.data(), L, Y, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(Y.desc.size() == 1 && same_desc(Y.desc[0], 1, 1, 0, 0, 0, 0, 0, 0) && Y.tdesc.empty() && Y.tint.empty() && Y.facDoubles == 0, "dense layout");
    CHECK(Y.treeSeg == 0 && Y.treeDepth == 0 && Y.cell == (V{3}) && Y.blkrow == (V{0}) && !Y.shared, "blocks");
    std::printf("ok  one well of one segment\n");
    return true;
}

static bool two_dense_wells() {
    // 3 segments, the second without a block, and 2 segments
    List l;
    l.add({{1}, {}, {4, 2}});
    l.add({{0}, {5}});
    const opmhip_ms_wells m = l.view();
    const V to = {0, 1, 2, 3, 4, 5};
    MsWellsList L;
    MsWellsLayout Y;
    std::string msg;
    CHECK(ms_wells_list_check(m, OPMHIP_MS_WELLS_DENSE, 6, L, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(same_desc(L.all[0], 3, 3, 0, 0, 0, 0, 0, 0), "first well");
    // seg0: 3 segments + 1 pointer of the first well; dcol0: 12 columns + 1; dnz0: 3 blocks of 16; inv0: 12 x 12
    CHECK(same_desc(L.all[1], 2, 2, 4, 3, 13, 48, 144, 1), "second well: %d %d %d %d %d", L.all[1].seg0, L.all[1].blk0, L.all[1].dcol0, L.all[1].dnz0, L.all[1].inv0);
    CHECK(L.wform == (V{0, 0}) && L.invDoubles == 144 + 64 && L.maxM == 12 && L.nseg == 5 && L.nblk == 5 && L.nnz == 80, "totals");
    CHECK(ms_wells_list_layout(m, OPMHIP_MS_WELLS_DENSE, 6, to.data(), L, Y, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(Y.desc.size() == 2 && same_desc(Y.desc[1], 2, 2, 4, 3, 13, 48, 144, 1) && Y.tdesc.empty(), "dense layout");
    CHECK(Y.blkrow == (V{0, 2, 2, 0, 1}) && Y.cell == (V{1, 4, 2, 0, 5}) && !Y.shared, "blocks");
    // the same list under TREE: every well in the tree form, no dense D^-1
    CHECK(ms_wells_list_check(m, OPMHIP_MS_WELLS_TREE, 6, L, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(L.wform == (V{1, 1}) && L.invDoubles == 0 && L.all[1].inv0 == 0 && L.all[1].dnz0 == 48, "under TREE");
    std::printf("ok  two dense wells\n");
    return true;
}

static bool mixed_under_auto() {
    // at the dense cap: dense; one and two segments above it: tree (chains)
    const int cap = OPMHIP_MS_WELLS_MAX_M / 4;
    List l;
    l.add_long(cap, 0, chain_blocks(cap));
    l.add_long(cap + 1, 1, chain_blocks(cap + 1));
    l.add_long(cap + 2, 2, chain_blocks(cap + 2));
    const opmhip_ms_wells m = l.view();
    const V to = {0, 1, 2, 3};
    MsWellsList L;
    MsWellsLayout Y;
    std::string msg;
    CHECK(ms_wells_list_check(m, OPMHIP_MS_WELLS_AUTO, 4, L, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(L.wform == (V{0, 1, 1}) && L.invDoubles == 65536 && L.maxM == 4 * (cap + 2) && L.all[1].inv0 == 0 && L.all[2].inv0 == 0, "forms");
    CHECK(ms_wells_list_layout(m, OPMHIP_MS_WELLS_AUTO, 4, to.data(), L, Y, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(Y.desc.size() == 1 && Y.desc[0].well == 0 && Y.tdesc.size() == 2 && Y.tdesc[0].well == 1 && Y.tdesc[1].well == 2, "which goes where");
    // a chain of n segments: n diagonal and 2 (n - 1) other blocks of 16 entries; its lists: parent n | child_ptr n + 1 | child n - 1 |
    // level_ptr n + 1 | level_seg n | dest
    const int n1 = cap + 1, nnz1 = 16 * (3 * n1 - 2), n2 = cap + 2, nnz2 = 16 * (3 * n2 - 2);
    const MsTreeDesc &a = Y.tdesc[0], &b = Y.tdesc[1];
    CHECK(a.Mb == n1 && a.nblk == 1 && a.seg0 == cap + 1 && a.blk0 == 1 && a.dcol0 == 4 * cap + 1 && a.dnz0 == 16 * (3 * cap - 2), "first tree well: %d %d %d", a.seg0, a.dcol0, a.dnz0);
    CHECK(a.depth == n1 && a.width == 1 && a.par0 == 0 && a.cptr0 == n1 && a.child0 == 2 * n1 + 1 && a.lptr0 == 3 * n1 && a.lseg0 == 4 * n1 + 1 && a.dest0 == 5 * n1 + 1 && a.fac0 == 0,
          "first tree well's lists: %d %d %d %d %d %d", a.par0, a.cptr0, a.child0, a.lptr0, a.lseg0, a.dest0);
    const int at = 5 * n1 + 1 + nnz1;
    CHECK(b.Mb == n2 && b.par0 == at && b.cptr0 == at + n2 && b.dest0 == at + 5 * n2 + 1 && b.fac0 == MS_TREE_SEG * n1, "second tree well's lists: %d %d %d", b.par0, b.dest0, b.fac0);
    CHECK((int)Y.tint.size() == at + 5 * n2 + 1 + nnz2 && Y.facDoubles == (size_t)MS_TREE_SEG * (n1 + n2) && Y.treeSeg == n2 && Y.treeDepth == n2, "totals");
    CHECK(Y.tint[a.par0] == -1 && Y.tint[a.par0 + 1] == 0 && Y.tint[b.par0] == -1 && Y.tint[b.par0 + n2 - 1] == n2 - 2, "parents in the lists");
    CHECK(Y.cell == (V{0, 1, 2}) && Y.blkrow == (V{0, 0, 0}) && !Y.shared, "blocks");
    std::printf("ok  a mixed list under AUTO\n");
    return true;
}

static bool permuted_order_and_shared_cells() {
    List l;
    l.add({{3}, {0, 2}});
    opmhip_ms_wells m = l.view();
    const V to = {2, 0, 3, 1};
    MsWellsList L;
    MsWellsLayout Y;
    std::string msg;
    CHECK(ms_wells_list_check(m, OPMHIP_MS_WELLS_DENSE, 4, L, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(ms_wells_list_layout(m, OPMHIP_MS_WELLS_DENSE, 4, to.data(), L, Y, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(Y.cell == (V{1, 2, 3}) && Y.blkrow == (V{0, 1, 1}) && !Y.shared, "cells in the internal order");
    // a second well with a block in cell 0 as well
    l.add({{1, 0}});
    m = l.view();
    CHECK(ms_wells_list_check(m, OPMHIP_MS_WELLS_DENSE, 4, L, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(ms_wells_list_layout(m, OPMHIP_MS_WELLS_DENSE, 4, to.data(), L, Y, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(Y.cell == (V{1, 2, 3, 0, 2}) && Y.blkrow == (V{0, 1, 1, 0, 0}) && Y.shared, "two blocks in one cell");
    std::printf("ok  a permuted order and shared cells\n");
    return true;
}

static bool no_tree_above_the_dense_cap() {
    // one segment above the dense cap, and the blocks 0 - 1, 1 - 2, 0 - 2 close a cycle
    const int n = OPMHIP_MS_WELLS_MAX_M / 4 + 1;
    Pairs p = chain_blocks(n);
    p.emplace_back(0, 2);
    List l;
    l.add({{0}});
    l.add_long(n, 1, p);
    const opmhip_ms_wells m = l.view();
    const V to = {0, 1};
    MsWellsList L;
    MsWellsLayout Y;
    Y.treeSeg = 77;
    std::string msg;
    CHECK(ms_wells_list_check(m, OPMHIP_MS_WELLS_AUTO, 2, L, msg) == OPMHIP_SUCCESS && L.wform == (V{0, 1}), "%s", msg.c_str());
    CHECK(ms_wells_list_layout(m, OPMHIP_MS_WELLS_AUTO, 2, to.data(), L, Y, msg) == OPMHIP_INVALID_ARGUMENT, "accepted under AUTO");
    CHECK(msg.find("well 1") != std::string::npos && msg.find("OPMHIP_MS_WELLS_MAX_M") != std::string::npos && msg.find("cap") != std::string::npos &&
              msg.find("cycle") == std::string::npos, "%s", msg.c_str());
    CHECK(Y.treeSeg == 77 && Y.desc.empty() && Y.cell.empty(), "the output was touched");
    std::printf("ok  refused: neither form under AUTO: %s\n", msg.c_str());
    CHECK(ms_wells_list_check(m, OPMHIP_MS_WELLS_TREE, 2, L, msg) == OPMHIP_SUCCESS && L.wform == (V{1, 1}), "%s", msg.c_str());
    CHECK(ms_wells_list_layout(m, OPMHIP_MS_WELLS_TREE, 2, to.data(), L, Y, msg) == OPMHIP_INVALID_ARGUMENT, "accepted under TREE");
    CHECK(msg.find("well 1") != std::string::npos && msg.find("cycle") != std::string::npos && msg.find("tree") != std::string::npos && msg.find("segments 1 and 2") != std::string::npos,
          "%s", msg.c_str());
    CHECK(Y.treeSeg == 77 && Y.desc.empty(), "the output was touched");
    std::printf("ok  refused: no tree under TREE: %s\n", msg.c_str());
    return true;
}

int main() {
    refusals();
    two_defects();
    one_well_one_segment();
    two_dense_wells();
    mixed_under_auto();
    permuted_order_and_shared_cells();
    no_tree_above_the_dense_cap();
    if (g_fail) {
        std::printf("%d checks FAILED\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
