// Host set-up of the passive tracers (csrc/tracers_setup.cpp: the phase batches and every refusal, the level sets of an ordering's lower
// triangle, the rows' faces in natural column order, the connections grouped by distinct cell) under AddressSanitizer + UBSan + libstdc++'s
// container assertions (test infrastructure; built and run by tests/test_tracers_setup_sanitized.py with g++, no GPU).  tracers_setup.cpp
// is linked with source_lists.cpp alone, with no stand-in for any HIP runtime call: that the link succeeds is the check that the set-up
// makes none.  The level sets are computed on a 4 x 3 x 2 seven-point pattern in the natural order, a two-coloured order and a
// line-coloured order (chains of four cells along x, the lines in two colours) and held against a restatement by relaxation and against
// the counts these orders must give.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../opm-autodiff_amd/csrc/tracers_setup.hpp"

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
static void report(bool ok, const char* what) {
    if (ok) std::printf("ok  %s\n", what);
}

constexpr int NX = 4, NY = 3, NZ = 2, NB = NX * NY * NZ;
struct Csr {
    std::vector<int> rowptr, col, nnzMap;
};
// the seven-point pattern in the order `fromOrder` (internal row p = natural cell fromOrder[p]), columns ascending; nnzMap: natural entry
static Csr pattern(const std::vector<int>& fromOrder) {
    std::vector<int> to(NB);
    for (int p = 0; p < NB; ++p) to[fromOrder[p]] = p;
    auto nbrs = [](int c) {
        const int i = c % NX, j = (c / NX) % NY, k = c / (NX * NY);
        std::vector<int> v{c};
        if (i > 0) v.push_back(c - 1);
        if (i < NX - 1) v.push_back(c + 1);
        if (j > 0) v.push_back(c - NX);
        if (j < NY - 1) v.push_back(c + NX);
        if (k > 0) v.push_back(c - NX * NY);
        if (k < NZ - 1) v.push_back(c + NX * NY);
        std::sort(v.begin(), v.end());
        return v;
    };
    std::vector<int> natptr{0};
    for (int c = 0; c < NB; ++c) natptr.push_back(natptr.back() + (int)nbrs(c).size());
    Csr P;
    P.rowptr.push_back(0);
    for (int p = 0; p < NB; ++p) {
        const int c = fromOrder[p];
        const std::vector<int> v = nbrs(c);
        std::vector<std::pair<int, int>> e;   // (internal column, natural entry)
        for (size_t q = 0; q < v.size(); ++q) e.push_back({to[v[q]], natptr[c] + (int)q});
        std::sort(e.begin(), e.end());
        for (auto& x : e) { P.col.push_back(x.first); P.nnzMap.push_back(x.second); }
        P.rowptr.push_back((int)P.col.size());
    }
    return P;
}
static std::vector<int> order_by(const std::vector<int>& key) {
    std::vector<int> fr(NB);
    for (int c = 0; c < NB; ++c) fr[c] = c;
    std::stable_sort(fr.begin(), fr.end(), [&](int a, int b) { return key[a] < key[b]; });
    return fr;
}

static bool check_levels(const char* what, const std::vector<int>& fromOrder, int expect_levels) {
    const Csr P = pattern(fromOrder);
    TracerLevels L;
    tracer_levels(NB, P.rowptr.data(), P.col.data(), L);
    const int nlev = (int)L.ptr.size() - 1;
    CHECK(nlev == expect_levels, "%s: %d levels, expected %d", what, nlev, expect_levels);
    CHECK(L.ptr[0] == 0 && L.ptr[nlev] == NB && (int)L.rows.size() == NB, "%s: ranges", what);
    std::vector<int> lev(NB, -1);
    for (int l = 0; l < nlev; ++l) {
        CHECK(L.ptr[l + 1] > L.ptr[l], "%s: level %d is empty", what, l);
        for (int q = L.ptr[l]; q < L.ptr[l + 1]; ++q) {
            CHECK(L.rows[q] >= 0 && L.rows[q] < NB && lev[L.rows[q]] == -1, "%s: row twice", what);
            CHECK(q == L.ptr[l] || L.rows[q - 1] < L.rows[q], "%s: rows of a level not ascending", what);
            lev[L.rows[q]] = l;
        }
    }
    // the restatement: relax level(i) = 1 + max level(j), j < i a column of row i, until nothing changes
    std::vector<int> r(NB, 0);
    for (bool changed = true; changed;) {
        changed = false;
        for (int i = NB - 1; i >= 0; --i)
            for (int k = P.rowptr[i]; k < P.rowptr[i + 1]; ++k)
                if (P.col[k] < i && r[i] < r[P.col[k]] + 1) { r[i] = r[P.col[k]] + 1; changed = true; }
    }
    for (int i = 0; i < NB; ++i) CHECK(lev[i] == r[i], "%s: row %d has level %d, the restatement %d", what, i, lev[i], r[i]);
    // what the backward sweep relies on: every upper column lies in a later level
    for (int i = 0; i < NB; ++i)
        for (int k = P.rowptr[i]; k < P.rowptr[i + 1]; ++k)
            if (P.col[k] > i) CHECK(lev[P.col[k]] > lev[i], "%s: upper column %d of row %d is not in a later level", what, P.col[k], i);
    // the rows' faces in natural column order
    std::vector<int> ford;
    tracer_face_order(NB, P.rowptr.data(), P.nnzMap.data(), ford);
    CHECK((int)ford.size() == P.rowptr[NB], "%s: ford size", what);
    for (int p = 0; p < NB; ++p) {
        std::vector<char> seen(P.rowptr[p + 1] - P.rowptr[p], 0);
        for (int q = P.rowptr[p]; q < P.rowptr[p + 1]; ++q) {
            CHECK(ford[q] >= P.rowptr[p] && ford[q] < P.rowptr[p + 1] && !seen[ford[q] - P.rowptr[p]], "%s: ford is not a permutation of row %d", what, p);
            seen[ford[q] - P.rowptr[p]] = 1;
            CHECK(q == P.rowptr[p] || fromOrder[P.col[ford[q - 1]]] < fromOrder[P.col[ford[q]]], "%s: row %d not in ascending natural column", what, p);
        }
    }
    return true;
}

static bool refusals() {
    const double Inf = std::numeric_limits<double>::infinity(), NaN = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> c((size_t)3 * NB, 0.5);
    std::string msg;
    TracerBatches B;
    B.phase = {7};
    auto untouched = [&]() { return B.phase.size() == 1 && B.phase[0] == 7 && B.slot.empty(); };
    const int water_oil[3] = {0, 1, 0}, gas[3] = {0, 2, 0}, bad[3] = {0, 3, 0};
    CHECK(tracer_batches(3, gas, c.data(), NB, false, 1, 0, B, msg) == OPMHIP_INVALID_ARGUMENT && msg.find("gas tracer") != std::string::npos && untouched(), "gas: %s", msg.c_str());
    CHECK(tracer_batches(3, bad, c.data(), NB, false, 1, 0, B, msg) == OPMHIP_INVALID_ARGUMENT && msg.find("phase 3") != std::string::npos && untouched(), "phase: %s", msg.c_str());
    CHECK(tracer_batches(3, water_oil, c.data(), NB, true, 1, 0, B, msg) == OPMHIP_INVALID_ARGUMENT && msg.find("PVTG") != std::string::npos && untouched(), "pvtg: %s", msg.c_str());
    CHECK(tracer_batches(3, water_oil, c.data(), NB, false, 2, 0, B, msg) == OPMHIP_INVALID_ARGUMENT && msg.find("decomposed") != std::string::npos && untouched(), "ranks: %s", msg.c_str());
    CHECK(tracer_batches(3, water_oil, c.data(), NB, false, 1, 5, B, msg) == OPMHIP_INVALID_ARGUMENT && msg.find("decomposed") != std::string::npos && untouched(), "ghosts: %s", msg.c_str());
    CHECK(tracer_batches(3, nullptr, c.data(), NB, false, 1, 0, B, msg) == OPMHIP_INVALID_ARGUMENT && untouched(), "null phase");
    CHECK(tracer_batches(3, water_oil, nullptr, NB, false, 1, 0, B, msg) == OPMHIP_INVALID_ARGUMENT && untouched(), "null concentration");
    CHECK(tracer_batches(-1, water_oil, c.data(), NB, false, 1, 0, B, msg) == OPMHIP_INVALID_ARGUMENT && untouched(), "negative count");
    for (double v : {NaN, Inf, -Inf}) {
        c[(size_t)2 * NB + 5] = v;
        CHECK(tracer_batches(3, water_oil, c.data(), NB, false, 1, 0, B, msg) == OPMHIP_INVALID_ARGUMENT && msg.find("tracer 2 in cell 5 is not finite") != std::string::npos && untouched(),
              "not finite: %s", msg.c_str());
    }
    c[(size_t)2 * NB + 5] = 0.5;
    std::vector<int> many(OPMHIP_TRACERS_MAX_PER_PHASE + 1, 0);
    std::vector<double> cm((size_t)many.size() * NB, 0.0);
    CHECK(tracer_batches((int)many.size(), many.data(), cm.data(), NB, false, 1, 0, B, msg) == OPMHIP_INVALID_ARGUMENT && msg.find("more than 32") != std::string::npos && untouched(), "cap: %s", msg.c_str());
    report(true, "refused: gas, phase, PVTG, ranks, ghosts, null arrays, count, non-finite, cap");
    // accepted: the batches in the caller's order
    CHECK(tracer_batches(3, water_oil, c.data(), NB, false, 1, 0, B, msg) == OPMHIP_SUCCESS, "accepted: %s", msg.c_str());
    CHECK(B.members[0] == (std::vector<int>{0, 2}) && B.members[1] == (std::vector<int>{1}) && B.members[2].empty(), "members");
    CHECK(B.slot == (std::vector<int>{0, 0, 1}) && B.phase == (std::vector<int>{0, 1, 0}), "slots");
    many.pop_back();
    CHECK(tracer_batches((int)many.size(), many.data(), cm.data(), NB, false, 1, 0, B, msg) == OPMHIP_SUCCESS && (int)B.members[0].size() == OPMHIP_TRACERS_MAX_PER_PHASE, "the cap itself is taken");
    CHECK(tracer_batches(0, water_oil, c.data(), NB, false, 1, 0, B, msg) == OPMHIP_SUCCESS && B.phase.empty(), "no tracers");
    report(true, "accepted: batches, the cap itself, none");
    // the solver's constants
    CHECK(tracer_solver_check(1e-2, 100, msg) == OPMHIP_SUCCESS && tracer_solver_check(1e-300, 1, msg) == OPMHIP_SUCCESS, "solver accepted");
    for (double t : {0.0, -1.0, NaN, Inf}) CHECK(tracer_solver_check(t, 100, msg) == OPMHIP_INVALID_ARGUMENT && msg.find("tolerance") != std::string::npos, "tolerance %g", t);
    CHECK(tracer_solver_check(1e-2, 0, msg) == OPMHIP_INVALID_ARGUMENT && msg.find("maxit = 0") != std::string::npos, "maxit");
    report(true, "refused: solver constants");
    return true;
}

static bool connections() {
    std::vector<int> toOrder(NB);
    for (int c = 0; c < NB; ++c) toOrder[c] = NB - 1 - c;
    const int cell[4] = {3, 20, 3, 7};
    std::vector<double> rate(12, 1e-3), inj(8, 0.5);
    std::string msg;
    TracerConnLists L;
    CHECK(tracer_connections(4, cell, rate.data(), inj.data(), 2, NB, toOrder.data(), L, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(L.cpos == (std::vector<int>{NB - 4, NB - 21, NB - 8}) && L.cptr == (std::vector<int>{0, 2, 3, 4}) && L.cconn == (std::vector<int>{0, 2, 1, 3}), "grouping");
    CHECK(L.pos == (std::vector<int>{NB - 4, NB - 21, NB - 4, NB - 8}), "positions");
    report(true, "connections: a cell named twice keeps its connections in list order");
    TracerConnLists U;
    U.cptr = {42};
    auto untouched = [&]() { return U.cptr.size() == 1 && U.cptr[0] == 42 && U.pos.empty(); };
    const int out_of_range[4] = {3, NB, 3, 7}, negative[4] = {3, -1, 3, 7};
    CHECK(tracer_connections(4, out_of_range, rate.data(), inj.data(), 2, NB, toOrder.data(), U, msg) == OPMHIP_INVALID_ARGUMENT && msg.find("outside") != std::string::npos && untouched(), "cell: %s", msg.c_str());
    CHECK(tracer_connections(4, negative, rate.data(), inj.data(), 2, NB, toOrder.data(), U, msg) == OPMHIP_INVALID_ARGUMENT && untouched(), "negative cell");
    CHECK(tracer_connections(4, nullptr, rate.data(), inj.data(), 2, NB, toOrder.data(), U, msg) == OPMHIP_INVALID_ARGUMENT && untouched(), "null cells");
    CHECK(tracer_connections(4, cell, nullptr, inj.data(), 2, NB, toOrder.data(), U, msg) == OPMHIP_INVALID_ARGUMENT && untouched(), "null rates");
    CHECK(tracer_connections(4, cell, rate.data(), nullptr, 2, NB, toOrder.data(), U, msg) == OPMHIP_INVALID_ARGUMENT && untouched(), "null injected");
    CHECK(tracer_connections(-4, cell, rate.data(), inj.data(), 2, NB, toOrder.data(), U, msg) == OPMHIP_INVALID_ARGUMENT && untouched(), "negative n");
    rate[7] = std::numeric_limits<double>::infinity();
    CHECK(tracer_connections(4, cell, rate.data(), inj.data(), 2, NB, toOrder.data(), U, msg) == OPMHIP_INVALID_ARGUMENT && msg.find("connection 2 is not finite") != std::string::npos && untouched(), "rate: %s", msg.c_str());
    rate[7] = 0.0;
    inj[5] = std::numeric_limits<double>::quiet_NaN();
    CHECK(tracer_connections(4, cell, rate.data(), inj.data(), 2, NB, toOrder.data(), U, msg) == OPMHIP_INVALID_ARGUMENT && msg.find("tracer 1 at connection 1 is not finite") != std::string::npos && untouched(),
          "injected: %s", msg.c_str());
    report(true, "refused: connections");
    return true;
}

int main() {
    std::vector<int> key(NB);
    for (int c = 0; c < NB; ++c) key[c] = 0;
    report(check_levels("natural", order_by(key), NX + NY + NZ - 2), "levels: natural order");
    for (int c = 0; c < NB; ++c) key[c] = (c % NX + (c / NX) % NY + c / (NX * NY)) % 2;
    report(check_levels("coloured", order_by(key), 2), "levels: two colours");
    // line colouring: the lines along x (chains of NX = 4 cells) in two colours by (j + k) % 2; a colour's rows chain by chain.  The first
    // colour's chains give the levels 0 .. 3; a cell of the second colour waits for its predecessor and for its neighbours of the first
    // colour at the same place of their chains: levels 1 .. 4
    for (int c = 0; c < NB; ++c) key[c] = ((c / NX) % NY + c / (NX * NY)) % 2;
    report(check_levels("line-coloured", order_by(key), NX + 1), "levels: line colouring");
    // a single row
    {
        const int rp[2] = {0, 1}, col[1] = {0};
        TracerLevels L;
        tracer_levels(1, rp, col, L);
        const bool ok = L.ptr == std::vector<int>{0, 1} && L.rows == std::vector<int>{0};
        if (!ok) { std::printf("FAILED single row\n"); ++g_fail; }
        report(ok, "levels: a single row");
        tracer_levels(0, rp, col, L);
        const bool none = L.ptr == std::vector<int>{0} && L.rows.empty();
        if (!none) { std::printf("FAILED no rows\n"); ++g_fail; }
        report(none, "levels: no rows");
    }
    refusals();
    connections();
    if (g_fail == 0) std::printf("all checks passed\n");
    return g_fail == 0 ? 0 : 1;
}
