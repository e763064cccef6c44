// The schedule behind opmhip_set_std_wells_matrix_add (csrc/source_lists.cpp: std_wells_matrix_add_schedule, std_wells_matrix_add_check)
// under AddressSanitizer + UBSan + libstdc++'s container assertions (test infrastructure; built and run by
// tests/test_std_wells_matrix_add_sanitized.py with g++, no GPU).  source_lists.cpp is linked alone, with no stand-in for any HIP runtime
// call: that the link succeeds is the check that the unit makes none.  The schedule is compared with a quadratic restatement: for every
// block of the pattern, the list of every (well, a, b) that lands on it, found by walking all wells and all pairs for that block.
#include <cstdio>
#include <string>
#include <vector>

#include "../../opm-autodiff_amd/csrc/source_lists.hpp"

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

// a pattern over n cells in a permuted internal order: the 1-D chain i - 1, i, i + 1 in natural numbers plus the cliques handed in
struct Pat {
    int n;
    std::vector<int> toOrder, fromOrder, rowptr, col;
    Pat(int n_, const std::vector<std::vector<int>>& cliques) : n(n_), toOrder(n_), fromOrder(n_) {
        for (int i = 0; i < n; ++i) toOrder[i] = (i * 7 + 3) % n;   // n is coprime to 7
        for (int i = 0; i < n; ++i) fromOrder[toOrder[i]] = i;
        std::vector<std::vector<char>> on(n, std::vector<char>(n, 0));
        for (int i = 0; i < n; ++i)
            for (int j = i - 1; j <= i + 1; ++j)
                if (j >= 0 && j < n) on[toOrder[i]][toOrder[j]] = 1;
        for (const auto& q : cliques)
            for (int a : q)
                for (int b : q) on[toOrder[a]][toOrder[b]] = 1;
        rowptr.push_back(0);
        for (int r = 0; r < n; ++r) {
            for (int k = 0; k < n; ++k)
                if (on[r][k]) col.push_back(k);
            rowptr.push_back((int)col.size());
        }
    }
};

struct Wells {
    std::vector<int> vp{0}, cell, pos;   // natural cells; their internal positions
    Wells(const Pat& P, const std::vector<std::vector<int>>& wells) {
        for (const auto& w : wells) {
            for (int c : w) { cell.push_back(c); pos.push_back(P.toOrder[c]); }
            vp.push_back((int)cell.size());
        }
    }
    int nw() const { return (int)vp.size() - 1; }
};

// for every entry of the pattern, by walking all wells and all their pairs: what lands there, in well order, then a * np + b
static bool restated(const char* what, const Pat& P, const Wells& W, const StdWellsMatrixAdd& H, int want_targets, int want_pairs) {
    std::vector<int> target, tptr{0}, contrib;
    for (int r = 0; r < P.n; ++r)
        for (int e = P.rowptr[r]; e < P.rowptr[r + 1]; ++e) {
            const size_t before = contrib.size();
            for (int w = 0; w < W.nw(); ++w) {
                const int pb = W.vp[w], np = W.vp[w + 1] - pb;
                for (int q = 0; q < np * np; ++q)
                    if (W.pos[pb + q / np] == r && W.pos[pb + q % np] == P.col[e]) { contrib.push_back(w); contrib.push_back(q / np); contrib.push_back(q % np); }
            }
            if (contrib.size() != before) { target.push_back(e); tptr.push_back((int)contrib.size() / 3); }
        }
    CHECK(H.target == target, "%s: the distinct blocks (%zu against %zu)", what, H.target.size(), target.size());
    CHECK(H.tptr == tptr, "%s: the ranges", what);
    CHECK(H.contrib == contrib, "%s: the contributions", what);
    int total = 0;
    for (int w = 0; w < W.nw(); ++w) total += (W.vp[w + 1] - W.vp[w]) * (W.vp[w + 1] - W.vp[w]);
    CHECK(H.pairs == total && H.pairs == want_pairs && (int)H.target.size() == want_targets, "%s: %d pairs on %zu blocks, expected %d on %d", what, H.pairs,
          H.target.size(), want_pairs, want_targets);
    for (size_t t = 0; t + 1 < H.target.size(); ++t) CHECK(H.target[t] < H.target[t + 1], "%s: targets not ascending / not distinct", what);
    std::printf("ok  %s\n", what);
    return true;
}

static bool accepted(const char* what, const std::vector<std::vector<int>>& wells, int want_targets, int want_pairs) {
    const Pat P(11, wells);
    const Wells W(P, wells);
    StdWellsMatrixAdd H;
    std::string msg;
    const int rc = std_wells_matrix_add_schedule(W.nw(), W.vp.data(), W.pos.data(), P.fromOrder.data(), P.rowptr.data(), P.col.data(), H, msg);
    CHECK(rc == OPMHIP_SUCCESS, "%s: %d '%s'", what, rc, msg.c_str());
    return restated(what, P, W, H, want_targets, want_pairs);
}

static bool missing_block() {
    // the pattern holds the clique of well 0 only; well 1 = cells 2, 9: (2, 9) is not there
    const std::vector<std::vector<int>> wells{{0, 5, 8}, {2, 9}};
    const Pat P(11, {wells[0]});
    const Wells W(P, wells);
    StdWellsMatrixAdd H;
    H.target = {-1}; H.tptr = {-2, -3}; H.contrib = {-4}; H.pairs = -5;
    std::string msg;
    const int rc = std_wells_matrix_add_schedule(W.nw(), W.vp.data(), W.pos.data(), P.fromOrder.data(), P.rowptr.data(), P.col.data(), H, msg);
    CHECK(rc == OPMHIP_INVALID_ARGUMENT, "missing block: code %d", rc);
    CHECK(msg.find("set_std_wells_matrix_add") != std::string::npos && msg.find("block (2, 9) of well 1") != std::string::npos && msg.find("not in the pattern") != std::string::npos,
          "missing block: text '%s'", msg.c_str());
    CHECK(H.target == std::vector<int>{-1} && H.tptr == std::vector<int>({-2, -3}) && H.contrib == std::vector<int>{-4} && H.pairs == -5, "missing block: the outputs changed");
    std::printf("ok  refused: missing block\n");
    return true;
}

static bool switch_values() {
    std::string msg;
    CHECK(std_wells_matrix_add_check(0, msg) == OPMHIP_SUCCESS && std_wells_matrix_add_check(1, msg) == OPMHIP_SUCCESS, "0 and 1");
    for (int on : {2, -1}) {
        msg.clear();
        CHECK(std_wells_matrix_add_check(on, msg) == OPMHIP_INVALID_ARGUMENT && msg.find("set_std_wells_matrix_add: on = ") != std::string::npos, "on = %d: '%s'", on, msg.c_str());
        std::printf("ok  refused: on = %d\n", on);
    }
    return true;
}

int main() {
    accepted("a one-perforation well", {{4}}, 1, 1);
    accepted("one well of three", {{0, 5, 8}}, 9, 9);
    // two wells share cell 5: block (5, 5) takes one contribution of each, in well order
    accepted("a shared cell", {{0, 5, 8}, {5, 2, 9, 10}}, 9 + 16 - 1, 25);
    // cell 3 twice: 2 distinct cells -> 4 blocks, 9 pairs; (3, 3) takes four of them in the order of a * np + b
    accepted("a repeated cell", {{3, 7, 3}}, 4, 9);
    accepted("all of them in one list", {{0, 5, 8}, {5, 2, 9, 10}, {3, 7, 3}, {4}, {8, 3}}, 9 + 15 + 4 + 1 + 2, 9 + 16 + 9 + 1 + 4);
    accepted("no well", {}, 0, 0);
    missing_block();
    switch_values();
    if (g_fail) { std::printf("%d checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
