// Symbolic ILU(n) of libopmhip (csrc/reorder.cpp: symbolic_fill, build_fill_split, the distance-2 colouring) under AddressSanitizer +
// UBSan + libstdc++'s container assertions (test infrastructure; built and run by tests/test_ilun_pattern.py with g++, no GPU).
// Input (argv[1]): cases, each "Nb nnzb kind n" then the rows' pointers and the columns of the natural pattern.  For every case the
// harness runs build_pattern with the fill level set and checks what must hold whatever the rule's details: the matrix's pattern lies
// inside the filled one, every matrix entry has its place in L, U or on the diagonal, every filled-L dependency points into an earlier
// level and every filled-U one into a later level, the sweeps' tiles cut every level into pieces a wavefront can take.  It writes
// (argv[2]) the return code and, on success, the level count, the elimination order the fill was computed in, the internal order, the
// rows per level and the filled L / U patterns, for the test to compare with its own restatement of the fill rule.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../opm-autodiff_amd/csrc/internal.hpp"

// ---- the HIP runtime entry points reorder.cpp links against, on the host heap --------------------------------------------------
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

static int g_fail = 0;
#define CHECK(cond, ...)                                                 \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                    \
            std::printf("\n");                                           \
            ++g_fail;                                                    \
            return;                                                      \
        }                                                                \
    } while (0)

static void put(FILE* f, const std::vector<int>& v) {
    std::fprintf(f, "%zu", v.size());
    for (int x : v) std::fprintf(f, " %d", x);
    std::fprintf(f, "\n");
}

static void run_case(int no, int Nb, int kind, int n, const std::vector<int>& rowptr, const std::vector<int>& col, FILE* out) {
    using namespace opmhip;
    opmhip_ctx c;
    std::memset(&c.cfg, 0, sizeof c.cfg);
    c.cfg.abi_version = OPMHIP_ABI_VERSION;
    c.cfg.reorder = kind;
    c.ilu_fillin = n;
    const int rc = build_pattern(&c, Nb, 0, (int)col.size(), rowptr.data(), col.data());
    struct Guard { opmhip_ctx& c; ~Guard() { for (void* p : c.allocs) std::free(p); c.allocs.clear(); } } guard{c};
    std::fprintf(out, "case %d rc %d\n", no, rc);
    if (rc != OPMHIP_SUCCESS) {
        std::printf("ok  case %d kind %d n %d: refused (%d): %s\n", no, kind, n, rc, c.err.c_str());
        return;
    }
    const Pattern& P = c.pat;
    const bool fill = n > 0;
    CHECK(P.fillLevel == n, "case %d: fill level %d", no, P.fillLevel);
    const std::vector<int> &lrp = P.lrowptr, &lcl = P.lcol, &urp = P.urowptr, &ucl = P.ucol;
    std::vector<int> levelOf(Nb);
    for (int l = 0; l < P.numColors; ++l)
        for (int p = P.colorPrefix[l]; p < P.colorPrefix[l + 1]; ++p) levelOf[p] = l;
    CHECK(P.colorPrefix[P.numColors] == Nb, "case %d", no);
    for (int p = 0; p < Nb; ++p) {
        CHECK(P.fromOrder[P.toOrder[p]] == p, "case %d: permutations not inverse at %d", no, p);
        for (int q = lrp[p]; q < lrp[p + 1]; ++q) {
            CHECK(lcl[q] < p && (q == lrp[p] || lcl[q] > lcl[q - 1]), "case %d: L row %d not ascending / not lower", no, p);
            CHECK(levelOf[lcl[q]] < levelOf[p], "case %d: L dependency (%d, %d) inside level %d", no, p, lcl[q], levelOf[p]);
        }
        for (int q = urp[p]; q < urp[p + 1]; ++q) {
            CHECK(ucl[q] > p && ucl[q] < Nb && (q == urp[p] || ucl[q] > ucl[q - 1]), "case %d: U row %d not ascending / not upper", no, p);
            CHECK(levelOf[ucl[q]] > levelOf[p], "case %d: U dependency (%d, %d) inside level %d", no, p, ucl[q], levelOf[p]);
        }
        // every matrix entry has its place: the diagonal, or the L / U entry of its column
        for (int k = P.rowptr[p]; k < P.rowptr[p + 1]; ++k) {
            const int j = P.col[k];
            const int d = P.fdest[k];
            if (j == p) CHECK(d == -1, "case %d: diagonal has a place %d", no, d);
            else if (j < p) CHECK(d >= lrp[p] && d < lrp[p + 1] && lcl[d] == j, "case %d: entry (%d, %d) -> %d", no, p, j, d);
            else CHECK(d <= -2 && -2 - d >= urp[p] && -2 - d < urp[p + 1] && ucl[-2 - d] == j, "case %d: entry (%d, %d) -> %d", no, p, j, d);
        }
    }
    if (fill) {
        CHECK((long long)P.nl + P.nu + Nb <= (long long)ILUN_BUDGET_FACTOR * (long long)col.size(), "case %d: over the budget", no);
        const TileSet& T = P.ftiles;
        CHECK(T.row0.front() == 0 && T.row0.back() == Nb && (int)T.colorTile.size() == P.numColors + 1, "case %d: tiles", no);
        for (int l = 0; l < P.numColors; ++l) CHECK(T.row0[T.colorTile[l]] == P.colorPrefix[l], "case %d: level %d's tiles", no, l);
        for (int t = 0; t + 1 < (int)T.row0.size(); ++t) {
            const int r0 = T.row0[t], r1 = T.row0[t + 1];
            CHECK(r1 > r0 && r1 - r0 <= TILE_ROWS, "case %d: tile %d", no, t);
            CHECK(r1 - r0 == 1 || (lrp[r1] - lrp[r0]) + (urp[r1] - urp[r0]) <= TILE_CAP_BLOCKS, "case %d: tile %d over the cap", no, t);
        }
        CHECK(P.fillBase.size() == (size_t)Nb && !P.ualias && !P.chained, "case %d", no);
    }
    std::fprintf(out, "levels %d kind %d\n", P.numColors, P.kindInForce);
    put(out, fill ? P.fillBase : std::vector<int>());
    put(out, P.toOrder);
    put(out, P.colorPrefix);
    put(out, lrp);
    put(out, lcl);
    put(out, urp);
    put(out, ucl);
    std::printf("ok  case %d kind %d n %d: %d rows, %d levels, L %zu U %zu blocks\n", no, kind, n, Nb, P.numColors, lcl.size(), ucl.size());
}

int main(int argc, char** argv) {
    if (argc != 3) { std::printf("usage: ilun_san cases.txt out.txt\n"); return 2; }
    FILE* in = std::fopen(argv[1], "r");
    FILE* out = std::fopen(argv[2], "w");
    if (!in || !out) { std::printf("FAILED cannot open files\n"); return 2; }
    int Nb, nnzb, kind, n, no = 0;
    while (std::fscanf(in, "%d %d %d %d", &Nb, &nnzb, &kind, &n) == 4) {
        std::vector<int> rowptr(Nb + 1), col(nnzb);
        for (int& x : rowptr) if (std::fscanf(in, "%d", &x) != 1) return 2;
        for (int& x : col) if (std::fscanf(in, "%d", &x) != 1) return 2;
        run_case(no++, Nb, kind, n, rowptr, col, out);
    }
    std::fclose(in);
    std::fclose(out);
    if (g_fail) { std::printf("FAILED %d checks\n", g_fail); return 1; }
    std::printf("all checks passed (%d cases)\n", no);
    return 0;
}
