// Host set-up of the assembly (csrc/asm_setup.cpp: the static-data check, k_assemble's tiles, launch schedule and entry words, the
// water-compaction tables, the per-cell end points, the source-cell list) under AddressSanitizer + UBSan + libstdc++'s container
// assertions (test infrastructure; built and run by tests/test_asm_setup_sanitized.py with g++, no GPU).  The patterns come from
// csrc/reorder.cpp's own analysis, so that the colours, the L / U / rest places and the row pointers of the streams are the real ones; the
// HIP runtime calls reorder.cpp makes for its uploads are served from the host heap, as in host_logic_san.cpp.  The tile edges run on
// hand-made patterns whose row lengths are chosen freely.  Every property is restated here from the description in asm_setup.hpp, not
// taken from the code under test.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../opm-autodiff_amd/csrc/asm_setup.hpp"
#include "../../opm-autodiff_amd/csrc/fluid_tables.hpp"
#include "../../opm-autodiff_amd/csrc/internal.hpp"

extern "C" hipError_t hipMalloc(void** p, size_t n) {
    *p = std::malloc(n);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
extern "C" hipError_t hipFree(void* p) {
    std::free(p);
    return hipSuccess;
}
extern "C" hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) {
    std::memcpy(d, s, n);
    return hipSuccess;
}
extern "C" hipError_t hipMemset(void* d, int v, size_t n) {
    std::memset(d, v, n);
    return hipSuccess;
}
extern "C" hipError_t hipDeviceSynchronize() { return hipSuccess; }
extern "C" const char* hipGetErrorString(hipError_t) { return "host stand-in"; }

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

// the shipped tile: ASM_THREADS lanes = entries, ASM_MAX_ROWS = ASM_THREADS / 7 + 4 rows (csrc/assemble.hip); and a small one
static const int SIZES[2][2] = {{64, 13}, {8, 3}};

struct Graph {
    int Nb = 0, Nghost = 0;
    std::vector<int> rowptr, col;
};
// 7-point grid in its natural order; nxo < nx: the owned part [0, nxo) of the x range, the first layer behind the cut as ghost cells
static Graph cartesian(int nx, int ny, int nz, int nxo = -1) {
    if (nxo < 0) nxo = nx;
    auto id = [&](int i, int j, int k) { return i + nxo * (j + ny * k); };
    Graph g;
    g.Nb = nxo * ny * nz;
    std::vector<int> ghostId((size_t)ny * nz, -1);
    g.rowptr.push_back(0);
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nxo; ++i) {
                std::vector<int> r;
                if (k > 0) r.push_back(id(i, j, k - 1));
                if (j > 0) r.push_back(id(i, j - 1, k));
                if (i > 0) r.push_back(id(i - 1, j, k));
                r.push_back(id(i, j, k));
                if (i + 1 < nxo) r.push_back(id(i + 1, j, k));
                else if (i + 1 < nx) {
                    int& gidx = ghostId[j + (size_t)ny * k];
                    if (gidx < 0) gidx = g.Nb + g.Nghost++;
                    r.push_back(gidx);
                }
                if (j + 1 < ny) r.push_back(id(i, j + 1, k));
                if (k + 1 < nz) r.push_back(id(i, j, k + 1));
                std::sort(r.begin(), r.end());
                g.col.insert(g.col.end(), r.begin(), r.end());
                g.rowptr.push_back((int)g.col.size());
            }
    return g;
}
static Graph diagonal(int n) {   // cells without neighbours: one colour
    Graph g;
    g.Nb = n;
    g.rowptr.push_back(0);
    for (int i = 0; i < n; ++i) { g.col.push_back(i); g.rowptr.push_back(i + 1); }
    return g;
}

// a context whose pattern reorder.cpp has analysed
struct Built {
    opmhip_ctx c;
    bool ok = false;
    Built(const Graph& g, int fill = 0, bool reversed_gids = false) {
        std::memset(&c.cfg, 0, sizeof c.cfg);
        c.cfg.abi_version = OPMHIP_ABI_VERSION;
        c.cfg.reorder = OPMHIP_REORDER_AUTO;
        c.ilu_fillin = fill;
        ok = build_pattern(&c, g.Nb, g.Nghost, (int)g.col.size(), g.rowptr.data(), g.col.data()) == OPMHIP_SUCCESS;
        if (ok && reversed_gids)
            for (int i = 0; i < c.pat.Nloc; ++i) c.pat.gids.push_back(1000 - 3LL * i);
    }
    ~Built() { for (void* p : c.allocs) std::free(p); }
    Built(const Built&) = delete;
    Built& operator=(const Built&) = delete;
};

// ---- the plan ------------------------------------------------------------------------------------------------------------------------
static bool check_plan(const char* name, const Pattern& P, int T, int cap, bool expect_places, bool say = true) {
    AsmPlan A;
    std::string msg;
    const int rc = asm_plan(P, T, cap, A, msg);
    CHECK(rc == OPMHIP_SUCCESS && msg.empty(), "%s: asm_plan -> %d (%s)", name, rc, msg.c_str());
    const int Nb = P.Nb;
    // tiles: whole rows, every row in exactly one, at most T entries and cap rows, none ends early
    CHECK(A.ntiles == (int)A.row0.size() - 1 && A.ntiles >= 1 && A.row0.front() == 0 && A.row0.back() == Nb, "%s: tile ends", name);
    for (int t = 0; t < A.ntiles; ++t) {
        const int r0 = A.row0[t], r1 = A.row0[t + 1];
        CHECK(r1 > r0 && r1 - r0 <= cap && P.rowptr[r1] - P.rowptr[r0] <= T, "%s: tile %d: rows %d..%d, %d entries", name, t, r0, r1, P.rowptr[r1] - P.rowptr[r0]);
        CHECK(r1 == Nb || r1 - r0 == cap || P.rowptr[r1 + 1] - P.rowptr[r0] > T, "%s: tile %d ends although row %d fits", name, t, r1);
    }
    // schedule: 8 eighths of `chunk` records; record b holds position (b & 7) * chunk + (b >> 3) of the order; positions past the
    // tiles are empty, all zero
    const int chunk = (A.ntiles + 7) / 8;
    CHECK(A.nsched == 8 * chunk && (int)A.sched.size() == 4 * A.nsched && (int)A.desc.size() == 2 * T * A.nsched, "%s: schedule sizes", name);
    std::vector<int> tileOfRow(Nb), order(A.ntiles, -1), recOfTile(A.ntiles, -1);
    for (int t = 0; t < A.ntiles; ++t)
        for (int r = A.row0[t]; r < A.row0[t + 1]; ++r) tileOfRow[r] = t;
    int empty = 0;
    for (int b = 0; b < A.nsched; ++b) {
        const int* s = &A.sched[(size_t)4 * b];
        const int pos = (b & 7) * chunk + (b >> 3);
        if (pos >= A.ntiles) {
            CHECK(s[0] == 0 && s[1] == 0 && s[2] == 0 && s[3] == 0, "%s: record %d (position %d, no tile) is not empty", name, b, pos);
            ++empty;
            continue;
        }
        CHECK(s[0] >= 0 && s[0] < Nb, "%s: record %d starts at row %d", name, b, s[0]);
        const int t = tileOfRow[s[0]];
        CHECK(s[0] == A.row0[t] && s[1] == A.row0[t + 1] && s[2] == P.rowptr[s[0]] && s[3] == P.rowptr[s[1]], "%s: record %d is not tile %d", name, b, t);
        CHECK(recOfTile[t] < 0, "%s: tile %d in two records", name, t);
        recOfTile[t] = b;
        order[pos] = t;
    }
    CHECK(empty == A.nsched - A.ntiles, "%s: %d empty records", name, empty);
    // the order: by relative position inside the colour (a tile's colour: that of its first row), ties by tile number
    std::vector<int> colourOf(A.ntiles), first(P.numColors, A.ntiles), cnt(P.numColors, 0);
    for (int t = 0; t < A.ntiles; ++t) {
        int q = 0;
        for (int cc = 0; cc < P.numColors; ++cc)
            if (P.colorPrefix[cc] <= A.row0[t]) q = cc;
        colourOf[t] = q;
        first[q] = std::min(first[q], t);
        cnt[q]++;
    }
    auto frac = [&](int t) { return (double)(t - first[colourOf[t]]) / (double)cnt[colourOf[t]]; };
    for (int pos = 1; pos < A.ntiles; ++pos) {
        const int a = order[pos - 1], b = order[pos];
        CHECK(frac(a) < frac(b) || (frac(a) == frac(b) && a < b), "%s: positions %d, %d hold tiles %d (%.6f), %d (%.6f)", name, pos - 1, pos, a, frac(a), b, frac(b));
    }
    // entry words
    const bool places = P.fillLevel == 0 && P.Nghost == 0 && (int)P.rdest.size() == P.nnzb && (int)P.fdest.size() == P.nnzb;
    CHECK(places == expect_places && A.split_ok == places, "%s: places %d, expected %d, split_ok %d", name, (int)places, (int)expect_places, (int)A.split_ok);
    auto gid = [&](int nat) { return P.gids.empty() ? (long long)nat : P.gids[nat]; };
    std::vector<char> lane((size_t)T * A.nsched, 0);
    for (int t = 0; t < A.ntiles; ++t) {
        const int b = recOfTile[t], r0 = A.row0[t], r1 = A.row0[t + 1], k0 = P.rowptr[r0];
        std::vector<char> restSeen, upSeen;
        for (int p = r0; p < r1; ++p) {
            const int kb = P.rowptr[p], ke = P.rowptr[p + 1], len = ke - kb;
            std::vector<int> nth(len);
            std::vector<char> seen(len, 0);
            for (int k = kb; k < ke; ++k) {
                const size_t l = (size_t)b * T + (k - k0);
                lane[l] = 1;
                const int col = A.desc[2 * l], w = A.desc[2 * l + 1];
                CHECK(col == P.col[k], "%s: entry %d: column %d, not %d", name, k, col, P.col[k]);
                CHECK((w & 63) == p - r0 && !(w & 128), "%s: entry %d: row in tile %d, not %d", name, k, w & 63, p - r0);
                CHECK(((w >> 6) & 1) == (gid(P.fromOrder[p]) < gid(P.fromOrder[P.col[k]]) ? 1 : 0), "%s: entry %d: tie-break bit", name, k);
                const int v = (w >> 8) & 255;
                CHECK(v < len && !seen[v], "%s: row %d: summation order names position %d twice or outside", name, p, v);
                seen[v] = 1;
                nth[k - kb] = v;
                if (!places) { CHECK((w >> 16) == 0, "%s: entry %d carries a place", name, k); continue; }
                const bool upper = (w >> 16) & 1;
                const int rel = (w >> 17) & 127;
                CHECK((w >> 24) == 0, "%s: entry %d: bits above the place", name, k);
                CHECK(upper == (P.rdest[k] < 0), "%s: entry %d: stream", name, k);
                const int want = upper ? (-2 - P.fdest[k]) - P.urowptr[r0] : P.rdest[k] - P.rrowptr[r0];
                CHECK(rel == want, "%s: entry %d: place %d, not %d", name, k, rel, want);
                std::vector<char>& S = upper ? upSeen : restSeen;
                if ((int)S.size() <= rel) S.resize(rel + 1, 0);
                CHECK(!S[rel], "%s: tile %d: place %d of stream %d twice", name, t, rel, (int)upper);
                S[rel] = 1;
            }
            for (int i = 1; i < len; ++i)
                CHECK(gid(P.fromOrder[P.col[kb + nth[i - 1]]]) < gid(P.fromOrder[P.col[kb + nth[i]]]), "%s: row %d: summation order not ascending at %d", name, p, i);
        }
        if (places) {   // a run 0 .. m - 1 without gaps in either stream, m = the tile's rows' blocks there
            CHECK(std::count(restSeen.begin(), restSeen.end(), 0) == 0 && (int)restSeen.size() == P.rrowptr[r1] - P.rrowptr[r0], "%s: tile %d: rest places", name, t);
            CHECK(std::count(upSeen.begin(), upSeen.end(), 0) == 0 && (int)upSeen.size() == P.urowptr[r1] - P.urowptr[r0], "%s: tile %d: U places", name, t);
        }
    }
    for (size_t l = 0; l < lane.size(); ++l)
        CHECK(lane[l] || (A.desc[2 * l] == 0 && A.desc[2 * l + 1] == 0), "%s: lane %zu has no entry but a word", name, l);
    if (!say) return true;
    std::printf("ok  plan: %s (T %d, cap %d)\n", name, T, cap);
    std::printf("    %d rows, %d colours, %d tiles, %d records, places %d\n", Nb, P.numColors, A.ntiles, A.nsched, (int)places);
    return true;
}

// the first line of cells whose plan has `want` tiles
static bool check_line_with_tiles(const char* name, int want, int T, int cap) {
    for (int n = 1; n <= 400; ++n) {
        Built B(cartesian(n, 1, 1));
        CHECK(B.ok, "%s: build_pattern of %d cells", name, n);
        AsmPlan A;
        std::string msg;
        CHECK(asm_plan(B.c.pat, T, cap, A, msg) == OPMHIP_SUCCESS, "%s: %s", name, msg.c_str());
        if (A.ntiles == want) return check_plan(name, B.c.pat, T, cap, true);
    }
    CHECK(false, "%s: no line of up to 400 cells has %d tiles", name, want);
    return false;
}

static bool check_plans(int T, int cap) {
    bool ok = true;
    { Built B(cartesian(1, 1, 1)); CHECK(B.ok, "1 cell"); ok &= check_plan("1 cell", B.c.pat, T, cap, true); }
    ok &= check_line_with_tiles("7 tiles", 7, T, cap);
    ok &= check_line_with_tiles("9 tiles", 9, T, cap);
    { Built B(cartesian(3, 3, 3)); CHECK(B.ok, "3x3x3"); ok &= check_plan("grid 3x3x3", B.c.pat, T, cap, true); }
    { Built B(cartesian(5, 4, 3)); CHECK(B.ok, "5x4x3"); ok &= check_plan("grid 5x4x3", B.c.pat, T, cap, true); }
    {
        Built B(diagonal(2 * cap + 1));
        CHECK(B.ok && B.c.pat.numColors == 1, "one colour: %d colours", B.c.pat.numColors);
        ok &= check_plan("one colour", B.c.pat, T, cap, true);
    }
    {
        Built B(cartesian(3, 3, 3), 1);
        CHECK(B.ok && B.c.pat.fillLevel == 1, "ILU(1): fill level %d", B.c.pat.fillLevel);
        ok &= check_plan("ILU(1) on grid 3x3x3", B.c.pat, T, cap, false);
    }
    {
        Built B(cartesian(6, 3, 3, 3), 0, true);
        CHECK(B.ok && B.c.pat.Nghost == 9 && (int)B.c.pat.gids.size() == B.c.pat.Nloc, "subdomain: %d ghosts", B.c.pat.Nghost);
        ok &= check_plan("subdomain 3(+ghosts)x3x3, gids reversed", B.c.pat, T, cap, false);
    }
    return ok;
}

// ---- tile edges: hand-made patterns, rows of any length ---------------------------------------------------------------------------------
static Pattern rows_of(const std::vector<int>& len) {
    Pattern P;
    P.Nb = (int)len.size();
    P.Nloc = std::max(P.Nb, *std::max_element(len.begin(), len.end()));
    P.Nghost = P.Nloc - P.Nb;
    P.numColors = 1;
    P.colorPrefix = {0, P.Nb};
    P.rowptr.push_back(0);
    for (int l : len) {
        for (int j = 0; j < l; ++j) P.col.push_back(j);
        P.rowptr.push_back((int)P.col.size());
    }
    P.nnzb = (int)P.col.size();
    for (int i = 0; i < P.Nloc; ++i) { P.fromOrder.push_back(i); P.toOrder.push_back(i); }
    for (int k = 0; k < P.nnzb; ++k) P.nnzMap.push_back(k);
    return P;
}
static bool check_tile_edges(int T, int cap) {
    struct Case { std::vector<int> len, row0; };
    const int h = T / 2;
    const std::vector<Case> cases = {
        {{h, T - h, 1}, {0, 2, 3}},             // exactly T
        {{h, T - h + 1, 1}, {0, 1, 3}},         // T + 1: the second row opens a tile
        {{h, T - h - 1, 1, 1}, {0, 3, 4}},      // T - 1: one more block fits, a second does not
        {{T}, {0, 1}},
        {std::vector<int>(cap, 1), {0, cap}},
        {std::vector<int>(cap + 1, 1), {0, cap, cap + 1}},
        {std::vector<int>(2 * cap, 1), {0, cap, 2 * cap}},
    };
    for (size_t i = 0; i < cases.size(); ++i) {
        const Pattern P = rows_of(cases[i].len);
        AsmPlan A;
        std::string msg;
        CHECK(asm_plan(P, T, cap, A, msg) == OPMHIP_SUCCESS, "edge case %zu: %s", i, msg.c_str());
        CHECK(A.row0 == cases[i].row0, "edge case %zu (T %d, cap %d): %d tiles", i, T, cap, A.ntiles);
        const std::string name = "edge case " + std::to_string(i);
        if (!check_plan(name.c_str(), P, T, cap, false, false)) return false;
    }
    {   // a row longer than a tile: refused, the outputs as they were
        const Pattern P = rows_of({1, 2, T + 1, 1});
        AsmPlan A;
        A.row0 = {7}; A.sched = {8}; A.desc = {9}; A.ntiles = 5; A.nsched = 6; A.split_ok = true;
        std::string msg;
        const int rc = asm_plan(P, T, cap, A, msg);
        char want[128];
        std::snprintf(want, sizeof want, "set_static: row 2 has more than %d blocks", T);
        CHECK(rc == OPMHIP_ANALYSIS_FAILED && msg == want, "long row: %d '%s'", rc, msg.c_str());
        CHECK(A.row0 == std::vector<int>{7} && A.sched == std::vector<int>{8} && A.desc == std::vector<int>{9} && A.ntiles == 5 && A.nsched == 6 && A.split_ok,
              "long row: outputs touched");
    }
    std::printf("ok  tile edges: rows summing to T, T + 1, T - 1; single-entry runs of cap, cap + 1, 2 cap; a row of T + 1 blocks refused (T %d, cap %d)\n", T, cap);
    return true;
}

// ---- static data -----------------------------------------------------------------------------------------------------------------------
static bool refused(int rc, const std::string& msg, int code, const char* text) {
    CHECK(rc == code && msg == text, "-> %d '%s', expected %d '%s'", rc, msg.c_str(), code, text);
    return true;
}
static bool check_static() {
    const Graph g = cartesian(6, 3, 3, 3);   // with ghost columns
    Built B(g);
    CHECK(B.ok, "static: build_pattern");
    const Pattern& P = B.c.pat;
    const int nnz = P.nnzb, N = P.Nloc;
    std::vector<double> trans(nnz), area(nnz), thpres(nnz), poro(N, 0.2), vol(N, 10.0);
    std::vector<int> pvt(N, 1), sat(N, 2);
    for (int i = 0; i < P.Nb; ++i)
        for (int k = g.rowptr[i]; k < g.rowptr[i + 1]; ++k) {
            const int j = g.col[k], a = std::min(i, j), b = std::max(i, j);
            // a ghost column has no transpose here: any value goes
            trans[k] = j >= P.Nb ? 1000.0 + k : 1.0 + a + 100.0 * b;
            area[k] = j >= P.Nb ? 2000.0 + k : 2.0 + a * b;
            thpres[k] = j >= P.Nb ? 3000.0 + k : 0.5 * (a + b);
        }
    std::string msg;
    auto run = [&](const double* th, const int* pv, const int* sa) { msg.clear(); return asm_static_check(P, 2, 3, trans.data(), area.data(), th, poro.data(), vol.data(), pv, sa, msg); };
    CHECK(run(thpres.data(), pvt.data(), sat.data()) == OPMHIP_SUCCESS && msg.empty(), "static: accepted input refused: %s", msg.c_str());
    CHECK(run(nullptr, nullptr, nullptr) == OPMHIP_SUCCESS && msg.empty(), "static: NULL optional arrays refused: %s", msg.c_str());
    poro[3] = 0.0;   // a porosity of zero is allowed
    CHECK(run(thpres.data(), nullptr, sat.data()) == OPMHIP_SUCCESS, "static: porosity 0 refused: %s", msg.c_str());
    // an entry k whose transpose lies behind it
    int k = -1;
    for (int q = g.rowptr[1]; q < g.rowptr[2]; ++q) if (g.col[q] > 1 && g.col[q] < P.Nb) { k = q; break; }
    CHECK(k >= 0, "static: no entry");
    char text[160];
    std::snprintf(text, sizeof text, "set_static: trans/area/thpres differ between entry %d and its transpose", k);
    for (int which = 0; which < 3; ++which) {
        std::vector<double>& v = which == 0 ? trans : which == 1 ? area : thpres;
        const double keep = v[k];
        v[k] += 1.0;
        if (!refused(run(thpres.data(), pvt.data(), sat.data()), msg, OPMHIP_INVALID_ARGUMENT, text)) return false;
        if (which == 2) CHECK(run(nullptr, pvt.data(), sat.data()) == OPMHIP_SUCCESS, "static: thpres looked at although NULL");
        vol[0] = 0.0;   // two faults: the connection data come first
        if (!refused(run(thpres.data(), pvt.data(), sat.data()), msg, OPMHIP_INVALID_ARGUMENT, text)) return false;
        vol[0] = 10.0;
        v[k] = keep;
    }
    vol[4] = 0.0;
    if (!refused(run(nullptr, pvt.data(), sat.data()), msg, OPMHIP_INVALID_ARGUMENT, "set_static: cell 4 has non-positive volume or negative porosity")) return false;
    pvt[2] = 2;   // two faults: the cell with the smaller number
    if (!refused(run(nullptr, pvt.data(), sat.data()), msg, OPMHIP_INVALID_ARGUMENT, "set_static: pvtnum[2] out of range")) return false;
    pvt[2] = 1; pvt[4] = -1;   // in one cell: the volume first
    if (!refused(run(nullptr, pvt.data(), sat.data()), msg, OPMHIP_INVALID_ARGUMENT, "set_static: cell 4 has non-positive volume or negative porosity")) return false;
    vol[4] = std::numeric_limits<double>::quiet_NaN();
    if (!refused(run(nullptr, nullptr, nullptr), msg, OPMHIP_INVALID_ARGUMENT, "set_static: cell 4 has non-positive volume or negative porosity")) return false;
    vol[4] = 10.0; poro[N - 1] = -0.1;   // a ghost cell's data are checked too
    std::snprintf(text, sizeof text, "set_static: cell %d has non-positive volume or negative porosity", N - 1);
    if (!refused(run(nullptr, nullptr, nullptr), msg, OPMHIP_INVALID_ARGUMENT, text)) return false;
    poro[N - 1] = 0.2;
    if (!refused(run(nullptr, pvt.data(), sat.data()), msg, OPMHIP_INVALID_ARGUMENT, "set_static: pvtnum[4] out of range")) return false;
    pvt[4] = 0; sat[7] = 3;
    if (!refused(run(nullptr, pvt.data(), sat.data()), msg, OPMHIP_INVALID_ARGUMENT, "set_static: satnum[7] out of range")) return false;
    sat[7] = -1;
    if (!refused(run(nullptr, pvt.data(), sat.data()), msg, OPMHIP_INVALID_ARGUMENT, "set_static: satnum[7] out of range")) return false;
    CHECK(run(nullptr, pvt.data(), nullptr) == OPMHIP_SUCCESS, "static: satnum looked at although NULL");
    {   // a pattern that lacks a transpose: named before any value is looked at
        Pattern Q;
        Q.Nb = Q.Nloc = 3; Q.nnzb = 6;
        Q.nat_rowptr = {0, 2, 4, 6};
        Q.nat_col = {0, 2, 0, 1, 1, 2};   // (0,2) without (2,0); (1,0) without (0,1)
        const double one[6] = {1, 1, 1, 1, 1, 1}, bad[6] = {1, 2, 3, 4, 5, 6};
        const int rc = asm_static_check(Q, 1, 1, bad, one, nullptr, one, one, nullptr, nullptr, msg);
        if (!refused(rc, msg, OPMHIP_INVALID_ARGUMENT, "set_static: pattern is not structurally symmetric at (0,2)")) return false;
        Q.nat_col = {0, 1, 0, 1, 0, 2};   // the search runs off the end of row 0
        const int rc2 = asm_static_check(Q, 1, 1, one, one, nullptr, one, one, nullptr, nullptr, msg);
        if (!refused(rc2, msg, OPMHIP_INVALID_ARGUMENT, "set_static: pattern is not structurally symmetric at (2,0)")) return false;
    }
    std::printf("ok  static data: accepted with ghost columns and with NULL thpres / pvtnum / satnum; every refusal, the earlier fault of two\n");
    return true;
}

// ---- water compaction ------------------------------------------------------------------------------------------------------------------
static bool check_water_compaction() {
    WaterCompactionTables W;
    std::string msg;
    W.desc = {1}; W.data = {2.0};
    CHECK(water_compaction_tables(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, W, msg) == OPMHIP_SUCCESS && W.desc.empty() && W.data.empty(), "0 tables");
    const int np[2] = {2, 3}, ns[2] = {2, 2};
    const double p[5] = {1e5, 2e5, 1e5, 3e5, 9e5}, sw[4] = {0.1, 0.9, 0.2, 0.8};
    const double pv[10] = {1, 2, 3, 4, 11, 12, 13, 14, 15, 16}, tm[10] = {21, 22, 23, 24, 31, 32, 33, 34, 35, 36};
    CHECK(water_compaction_tables(1, np, ns, p, sw, pv, nullptr, W, msg) == OPMHIP_SUCCESS, "one table: %s", msg.c_str());
    CHECK((W.desc == std::vector<int>{2, 2, 0, 2, 4, -1}) && (W.data == std::vector<double>{1e5, 2e5, 0.1, 0.9, 1, 2, 3, 4}), "one table without trans_mult");
    CHECK(water_compaction_tables(2, np, ns, p, sw, pv, nullptr, W, msg) == OPMHIP_SUCCESS, "two tables: %s", msg.c_str());
    CHECK((W.desc == std::vector<int>{2, 2, 0, 2, 4, -1, 3, 2, 8, 11, 13, -1}) &&
              (W.data == std::vector<double>{1e5, 2e5, 0.1, 0.9, 1, 2, 3, 4, 1e5, 3e5, 9e5, 0.2, 0.8, 11, 12, 13, 14, 15, 16}),
          "two tables without trans_mult");
    CHECK(water_compaction_tables(2, np, ns, p, sw, pv, tm, W, msg) == OPMHIP_SUCCESS, "two tables: %s", msg.c_str());
    CHECK((W.desc == std::vector<int>{2, 2, 0, 2, 4, 8, 3, 2, 12, 15, 17, 23}) &&
              (W.data == std::vector<double>{1e5, 2e5, 0.1, 0.9, 1, 2, 3, 4, 21, 22, 23, 24, 1e5, 3e5, 9e5, 0.2, 0.8, 11, 12, 13, 14, 15, 16, 31, 32, 33, 34, 35, 36}),
          "two tables with trans_mult");
    const WaterCompactionTables keep = W;
    auto same = [&] { return W.desc == keep.desc && W.data == keep.data; };
    const double pEq[5] = {1e5, 2e5, 1e5, 3e5, 3e5}, swEq[4] = {0.1, 0.9, 0.8, 0.8}, swNaN[4] = {0.1, std::nan(""), 0.2, 0.8};
    if (!refused(water_compaction_tables(2, np, ns, pEq, sw, pv, tm, W, msg), msg, OPMHIP_INVALID_ARGUMENT, "set_water_compaction: pressure nodes of table 1 not ascending")) return false;
    CHECK(same(), "refused: outputs touched");
    if (!refused(water_compaction_tables(2, np, ns, p, swEq, pv, tm, W, msg), msg, OPMHIP_INVALID_ARGUMENT, "set_water_compaction: saturation nodes of table 1 not ascending")) return false;
    if (!refused(water_compaction_tables(2, np, ns, p, swNaN, pv, tm, W, msg), msg, OPMHIP_INVALID_ARGUMENT, "set_water_compaction: saturation nodes of table 0 not ascending")) return false;
    if (!refused(water_compaction_tables(2, np, ns, pEq, swEq, pv, tm, W, msg), msg, OPMHIP_INVALID_ARGUMENT, "set_water_compaction: pressure nodes of table 1 not ascending")) return false;
    const int np1[2] = {2, 1};
    if (!refused(water_compaction_tables(2, np1, ns, p, sw, pv, tm, W, msg), msg, OPMHIP_INVALID_ARGUMENT, "set_water_compaction: table 1 needs at least two pressure and two saturation nodes")) return false;
    CHECK(same(), "refused: outputs touched");
    std::printf("ok  water compaction: 0, 1 and 2 tables, with and without trans_mult, the second table's offsets, nodes not ascending\n");
    return true;
}

// ---- end points ------------------------------------------------------------------------------------------------------------------------
static bool check_end_points() {
    // two saturation regions' own points
    std::vector<double> u(2 * EPS_COUNT);
    for (int r = 0; r < 2; ++r) {
        double* e = &u[(size_t)r * EPS_COUNT];
        e[EPS_SWL] = 0.1 + 0.01 * r; e[EPS_SWCR] = 0.15; e[EPS_SWU] = 1.0; e[EPS_SOWCR] = 0.2; e[EPS_SGL] = 0.0; e[EPS_SGCR] = 0.05; e[EPS_SGU] = 0.85; e[EPS_SOGCR] = 0.1;
        e[EPS_MAXPCOW] = 3e4; e[EPS_MAXPCGO] = 1e4; e[EPS_MAXKRW] = 0.9; e[EPS_MAXKROW] = 1.0; e[EPS_MAXKRG] = 0.8; e[EPS_MAXKROG] = 1.0;
        e[EPS_KRWR] = 0.4; e[EPS_KRORW] = 0.5; e[EPS_KRGR] = r == 0 ? 0.3 : 0.0; e[EPS_KRORG] = 0.6;
    }
    const int N = 4, fromOrder[N] = {2, 0, 3, 1}, region[N] = {0, 1, 1, 0};   // region: by natural cell
    std::vector<double> swl = {0.11, 0.12, 0.13, 0.14}, krw = {0.5, 0.6, 0.7, 0.8};
    const double* src[EPS_COUNT] = {};
    src[EPS_SWL] = swl.data();
    src[EPS_MAXKRW] = krw.data();
    opmhip_endpoint_scaling opt;
    std::memset(&opt, 0, sizeof opt);
    opt.sat_scaling = 1; opt.krw = 1;
    std::vector<double> v((size_t)EPS_COUNT * N, -1.0);
    EndPointsCheck K{"set_endpoint_scaling", "", src, u.data(), eps_config(opt), v.data(), (size_t)N};
    std::string msg;
    for (int pos = 0; pos < N; ++pos) {
        const int i = fromOrder[pos];
        CHECK(cell_end_points(K, i, i, region[i], pos, msg) == OPMHIP_SUCCESS, "end points of cell %d: %s", i, msg.c_str());
    }
    for (int f = 0; f < EPS_COUNT; ++f)
        for (int pos = 0; pos < N; ++pos) {
            const int i = fromOrder[pos];
            const double want = f == EPS_SWL ? swl[i] : f == EPS_MAXKRW ? krw[i] : u[(size_t)region[i] * EPS_COUNT + f];   // a NULL field: the region's own
            CHECK(v[(size_t)f * N + pos] == want, "end point %d at position %d: %g, not %g", f, pos, v[(size_t)f * N + pos], want);
        }
    // without any source and without a destination: the regions' own points, checked only
    EndPointsCheck None{"set_hysteresis", "imbibition ", nullptr, u.data(), eps_config(opt), nullptr, (size_t)N};
    CHECK(cell_end_points(None, 0, 0, 1, 0, msg) == OPMHIP_SUCCESS, "own points refused: %s", msg.c_str());
    // refusals leave v alone
    const std::vector<double> keep = v;
    krw[3] = std::numeric_limits<double>::infinity();
    if (!refused(cell_end_points(K, 3, 3, 0, 2, msg), msg, OPMHIP_INVALID_ARGUMENT, "set_endpoint_scaling: end point 10 of cell 3 is not finite")) return false;
    swl[3] = std::nan("");   // two in one cell: the field with the smaller number
    if (!refused(cell_end_points(K, 3, 3, 0, 2, msg), msg, OPMHIP_INVALID_ARGUMENT, "set_endpoint_scaling: end point 0 of cell 3 is not finite")) return false;
    K.call = "set_hysteresis"; K.kind = "imbibition ";
    if (!refused(cell_end_points(K, 3, 3, 0, 2, msg), msg, OPMHIP_INVALID_ARGUMENT, "set_hysteresis: imbibition end point 0 of cell 3 is not finite")) return false;
    swl[1] = 1.0;   // SWL == SWU: no interval
    if (!refused(cell_end_points(K, 1, 1, 1, 3, msg), msg, OPMHIP_INVALID_ARGUMENT,
                 "set_hysteresis: the imbibition end points of cell 1 (saturation region 1) leave a curve no saturation interval"))
        return false;
    K.call = "set_endpoint_scaling"; K.kind = "";
    opt.sat_scaling = 0; opt.krw = 0; opt.krg = 2;   // region 1 has no krg at the critical oil saturation
    K.cfg = eps_config(opt);
    if (!refused(cell_end_points(K, 1, 1, 1, 3, msg), msg, OPMHIP_INVALID_ARGUMENT,
                 "set_endpoint_scaling: the end points of cell 1 (saturation region 1) scale krg vertically (mode 2) by a table value of 0 at the displacing phase's critical saturation"))
        return false;
    CHECK(cell_end_points(K, 0, 0, 0, 1, msg) == OPMHIP_SUCCESS, "region 0 under krg mode 2: %s", msg.c_str());   // cell 0 again, in its place
    CHECK(v == keep, "refused: v touched");
    std::printf("ok  end points: a non-finite point names field and cell, a NULL field is the region's own, the refusal's text, the field-major internal-order layout\n");
    return true;
}

static bool check_eps_config() {
    int n = 0;
    for (int ss = 0; ss < 2; ++ss) for (int tp = 0; tp < 2; ++tp) for (int kw = 0; kw < 3; ++kw) for (int ko = 0; ko < 3; ++ko) for (int kg = 0; kg < 3; ++kg)
        for (int pw = 0; pw < 2; ++pw) for (int pg = 0; pg < 2; ++pg) {
            opmhip_endpoint_scaling s;
            std::memset(&s, 0, sizeof s);
            s.sat_scaling = 7 * ss; s.three_point_kr = -tp; s.krw = kw; s.kro = ko; s.krg = kg; s.pcw = 3 * pw; s.pcg = pg;   // any non-zero value is "on"
            const opmhip_endpoint_scaling* e = &s;
            const int want = (e->sat_scaling ? 1 : 0) | (e->three_point_kr ? 2 : 0) | (e->krw << 2) | (e->kro << 4) | (e->krg << 6) | (e->pcw ? 256 : 0) | (e->pcg ? 512 : 0);
            CHECK(eps_config(s) == want && want == ss + 2 * tp + 4 * kw + 16 * ko + 64 * kg + 256 * pw + 512 * pg, "eps_config(%d %d %d %d %d %d %d) = %d", ss, tp, kw, ko, kg, pw, pg, eps_config(s));
            ++n;
        }
    CHECK(n == 2 * 2 * 3 * 3 * 3 * 2 * 2, "%d combinations", n);
    std::printf("ok  eps_config: %d option combinations\n", n);
    return true;
}

// ---- source cells ----------------------------------------------------------------------------------------------------------------------
static bool check_source_cells() {
    const int Nloc = 6, toOrder[Nloc] = {4, 2, 5, 0, 1, 3};
    SourceCells S;
    std::string msg;
    S.pos = {1}; S.val = {1.0}; S.dval = {1.0};
    CHECK(source_cells(0, nullptr, nullptr, nullptr, Nloc, toOrder, S, msg) == OPMHIP_SUCCESS && S.pos.empty() && S.val.empty() && S.dval.empty(), "n = 0");
    // cell 3 three times, with values whose sum depends on the order: (2^53 + 1) - 2^53 = 0, 2^53 + (1 - 2^53) = 1
    const double big = 9007199254740992.0;
    const int cells[5] = {3, 5, 3, 0, 3};
    double src[15], dsrc[45];
    for (int i = 0; i < 15; ++i) src[i] = 0.1 * (i + 1);
    for (int i = 0; i < 45; ++i) dsrc[i] = 1.0 / (i + 3);
    src[0] = big; src[6] = 1.0; src[12] = -big;
    dsrc[8] = big; dsrc[18 + 8] = 1.0; dsrc[36 + 8] = -big;
    CHECK(source_cells(5, cells, src, dsrc, Nloc, toOrder, S, msg) == OPMHIP_SUCCESS, "source cells: %s", msg.c_str());
    CHECK((S.pos == std::vector<int>{0, 3, 4}) && S.val.size() == 9 && S.dval.size() == 27, "first mention: %zu cells", S.pos.size());
    for (int q = 0; q < 3; ++q) {
        CHECK(S.val[q] == ((0.0 + src[q]) + src[6 + q]) + src[12 + q], "sum of cell 3, component %d", q);
        CHECK(S.val[3 + q] == 0.0 + src[3 + q] && S.val[6 + q] == 0.0 + src[9 + q], "single items, component %d", q);
    }
    CHECK(S.val[0] == 0.0 && (src[0] + (src[6] + src[12])) == 1.0, "the order of the sum does not show");
    for (int q = 0; q < 9; ++q) {
        CHECK(S.dval[q] == ((0.0 + dsrc[q]) + dsrc[18 + q]) + dsrc[36 + q], "derivative sum of cell 3, entry %d", q);
        CHECK(S.dval[9 + q] == 0.0 + dsrc[9 + q] && S.dval[18 + q] == 0.0 + dsrc[27 + q], "single items' derivatives, entry %d", q);
    }
    CHECK(S.dval[8] == 0.0, "the order of the derivatives' sum does not show");
    CHECK(source_cells(5, cells, src, nullptr, Nloc, toOrder, S, msg) == OPMHIP_SUCCESS && S.dval == std::vector<double>(27, 0.0) && S.pos.size() == 3, "dsource NULL");
    // refusals by item: a NaN at item 2 comes before a bad cell at item 5, a bad cell at item 1 before the NaN; the outputs stay
    const SourceCells keep = S;
    int c7[7] = {3, 5, 3, 0, 3, 6, 1};
    double s7[21];
    for (int i = 0; i < 21; ++i) s7[i] = 1.0;
    s7[2 * 3 + 1] = std::nan("");
    if (!refused(source_cells(7, c7, s7, nullptr, Nloc, toOrder, S, msg), msg, OPMHIP_INVALID_ARGUMENT, "set_source_cells: source of cell 3 is not finite")) return false;
    c7[1] = -1;
    if (!refused(source_cells(7, c7, s7, nullptr, Nloc, toOrder, S, msg), msg, OPMHIP_INVALID_ARGUMENT, "set_source_cells: cell -1 of 6")) return false;
    c7[1] = 5; s7[2 * 3 + 1] = 1.0;
    if (!refused(source_cells(7, c7, s7, nullptr, Nloc, toOrder, S, msg), msg, OPMHIP_INVALID_ARGUMENT, "set_source_cells: cell 6 of 6")) return false;
    c7[5] = 2; s7[5 * 3] = std::numeric_limits<double>::infinity();   // in one item: the cell is looked at first, then its values
    if (!refused(source_cells(7, c7, s7, nullptr, Nloc, toOrder, S, msg), msg, OPMHIP_INVALID_ARGUMENT, "set_source_cells: source of cell 2 is not finite")) return false;
    CHECK(S.pos == keep.pos && S.val == keep.val && S.dval == keep.dval, "refused: outputs touched");
    std::printf("ok  source cells: n = 0, order of first mention, left-to-right sums bit for bit, dsource NULL, refusals in item order\n");
    return true;
}

int main() {
    for (const auto& s : SIZES) {
        check_plans(s[0], s[1]);
        check_tile_edges(s[0], s[1]);
    }
    check_static();
    check_water_compaction();
    check_end_points();
    check_eps_config();
    check_source_cells();
    std::printf(g_fail ? "%d check(s) FAILED\n" : "all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
}
