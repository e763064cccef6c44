// Host set-up of the resident standard wells and analytic aquifers (csrc/source_lists.cpp: every check of the two lists, the packing of
// the arrays the kernels read, the grouping by distinct cell, the aquifers' table look-ups, step scalars and sums) under AddressSanitizer +
// UBSan + libstdc++'s container assertions (test infrastructure; built and run by tests/test_host_logic_sanitized.py with g++, no GPU).
// source_lists.cpp is linked alone, with no stand-in for any HIP runtime call: that the link succeeds is the check that the unit makes none.
// group_by_cell is compared with a quadratic restatement written here and held to the invariants the kernels rely on; every refusal is
// provoked once and must come back with the code and, character for character, the text the C API has always given - the format strings
// below are pasted from the library's source as it stood before the unit existed - and with the outputs untouched.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <limits>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../opm-autodiff_amd/csrc/internal.hpp"
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
static void report(bool ok, const char* what) {
    if (ok) std::printf("ok  %s\n", what);
}
static std::string text(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}
static const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();

static std::vector<int> permutation(int n, unsigned seed) {
    std::vector<int> p(n);
    std::iota(p.begin(), p.end(), 0);
    std::mt19937 rng(seed);
    for (int i = n - 1; i > 0; --i) std::swap(p[i], p[rng() % (i + 1)]);
    return p;
}

// ---- group_by_cell ----------------------------------------------------------------------------------------------------------------
static bool check_group(const std::vector<int>& cell, int Nb, const std::vector<int>& toOrder, const std::vector<int>& pos, const std::vector<int>& cpos,
                        const std::vector<int>& cptr, const std::vector<int>& items) {
    const int n = (int)cell.size();
    // the restatement: the distinct cells in the order of first mention, each with every item that names it, found by looking at all items
    std::vector<int> dcell, rpos, rptr{0}, ritems;
    for (int i = 0; i < n; ++i) {
        bool seen = false;
        for (int j = 0; j < i; ++j) seen = seen || cell[j] == cell[i];
        if (seen) continue;
        dcell.push_back(cell[i]);
        rpos.push_back(toOrder[cell[i]]);
        for (int j = 0; j < n; ++j)
            if (cell[j] == cell[i]) ritems.push_back(j);
        rptr.push_back((int)ritems.size());
    }
    CHECK((int)pos.size() == n && (int)items.size() == n, "sizes %zu %zu of %d", pos.size(), items.size(), n);
    CHECK(cpos == rpos && cptr == rptr && items == ritems, "differs from the restatement (%zu distinct cells)", rpos.size());
    // the invariants
    CHECK(cptr.size() == cpos.size() + 1 && cptr.front() == 0 && cptr.back() == n, "cptr ends");
    std::vector<int> hit(n, 0);
    for (size_t t = 0; t < cpos.size(); ++t) {
        CHECK(cptr[t + 1] > cptr[t], "cptr does not ascend at %zu", t);
        for (int k = cptr[t]; k < cptr[t + 1]; ++k) {
            CHECK(items[k] >= 0 && items[k] < n, "item %d", items[k]);
            CHECK(k == cptr[t] || items[k] > items[k - 1], "items of cell %zu do not ascend", t);
            CHECK(pos[items[k]] == cpos[t], "pos[item] != cpos[cell]");
            hit[items[k]]++;
        }
    }
    for (int i = 0; i < n; ++i) {
        CHECK(hit[i] == 1, "item %d appears %d times", i, hit[i]);
        CHECK(pos[i] == toOrder[cell[i]], "pos[%d]", i);
    }
    (void)Nb;
    return true;
}
static bool run_group(const char* what, const std::vector<int>& cell, int Nb, unsigned seed) {
    const std::vector<int> toOrder = permutation(Nb, seed);
    std::vector<int> pos{7, 7}, cpos{7}, cptr{7}, items{7, 7, 7};   // whatever they held goes
    group_by_cell(cell.data(), (int)cell.size(), Nb, toOrder.data(), pos, cpos, cptr, items);
    const bool ok = check_group(cell, Nb, toOrder, pos, cpos, cptr, items);
    report(ok, what);
    return ok;
}
// wells of the given lengths down the columns of an nx x ny x nz grid (cell = (k * ny + j) * nx + i), well w in column w % (nx * ny):
// more wells than columns share their cells
static std::vector<int> column_wells(int nx, int ny, int nz, const std::vector<int>& len, std::vector<int>* ptr = nullptr) {
    std::vector<int> cell;
    if (ptr) ptr->assign(1, 0);
    for (size_t w = 0; w < len.size(); ++w) {
        const int col = (int)w % (nx * ny);
        for (int k = 0; k < len[w] && k < nz; ++k) cell.push_back(k * nx * ny + col);
        if (ptr) ptr->push_back((int)cell.size());
    }
    return cell;
}
static void group_cases() {
    run_group("group_by_cell: the empty list", {}, 5, 1);
    run_group("group_by_cell: one item", {3}, 5, 2);
    run_group("group_by_cell: one item, one cell", {0}, 1, 2);
    run_group("group_by_cell: all items in one cell", std::vector<int>(9, 4), 6, 3);
    {
        std::vector<int> c(40);
        std::iota(c.begin(), c.end(), 0);
        run_group("group_by_cell: all items distinct, ascending", c, 40, 4);
        run_group("group_by_cell: all items distinct, permuted", permutation(40, 5), 40, 6);
    }
    run_group("group_by_cell: cells 0 and Nb - 1", {599, 0, 599, 0, 0}, 600, 7);
    run_group("group_by_cell: wells of 150 / 64 / 65 / 1 perforations", column_wells(2, 2, 150, {150, 64, 65, 1}), 600, 8);
    run_group("group_by_cell: wells of 150 / 64 / 65 / 1 perforations, two wells sharing a cell", column_wells(2, 2, 150, {150, 64, 65, 1, 1}), 600, 9);
    run_group("group_by_cell: wells of 1 / 64 / 65 / 150 perforations, five more on the same columns", column_wells(2, 2, 150, {1, 64, 65, 150, 150, 3, 70, 2, 64}), 600, 10);
    std::mt19937 rng(11);
    for (int t = 0; t < 20; ++t) {
        const int Nb = 1 + (int)(rng() % 50), n = (int)(rng() % 120);
        std::vector<int> c(n);
        for (int& v : c) v = (int)(rng() % Nb);
        run_group(text("group_by_cell: random %d items over %d cells", n, Nb).c_str(), c, Nb, 100 + t);
    }
}

// ---- standard wells ---------------------------------------------------------------------------------------------------------------
struct WellsInput {
    std::vector<int> ptr, cell, producer, inj_phase, rate_component, control;
    std::vector<double> tw, dz, rate_target, bhp_limit, x;
    opmhip_std_wells view() const {
        return opmhip_std_wells{(int)producer.size(), ptr.data(), cell.data(), tw.data(), dz.data(), producer.data(), inj_phase.data(), rate_component.data(),
                                rate_target.data(), bhp_limit.data(), control.data(), x.empty() ? nullptr : x.data()};
    }
};
static WellsInput wells_input(int nx, int ny, int nz, const std::vector<int>& len, bool with_x) {
    WellsInput in;
    in.cell = column_wells(nx, ny, nz, len, &in.ptr);
    const int nw = (int)len.size(), np = (int)in.cell.size();
    for (int w = 0; w < nw; ++w) {
        in.producer.push_back(w % 2);
        in.inj_phase.push_back(w % 2 ? 7 : w % 3);   // a producer's is not looked at
        in.rate_component.push_back((w + 1) % 3);
        in.control.push_back((w / 2) % 2);
        in.rate_target.push_back(100.0 + w);
        in.bhp_limit.push_back(2e7 - 1e5 * w);
        if (with_x)
            for (int i = 0; i < 4; ++i) in.x.push_back(10.0 * w + i + 0.5);
    }
    for (int p = 0; p < np; ++p) { in.tw.push_back(1e-12 * (p + 1)); in.dz.push_back(0.25 * p - 3.0); }
    return in;
}
static const StdWellsLists SENTINEL_W{{-1}, {-2}, {-3}, {-4}, {-5}, {-6.0}, {-7.0}};
static bool same(const StdWellsLists& a, const StdWellsLists& b) {
    return a.pos == b.pos && a.cpos == b.cpos && a.cptr == b.cptr && a.cperf == b.cperf && a.wi == b.wi && a.wd == b.wd && a.pack == b.pack;
}
static bool wells_accepted(const char* what, const WellsInput& in, int Nb, unsigned seed) {
    const std::vector<int> toOrder = permutation(Nb, seed);
    const opmhip_std_wells sw = in.view();
    StdWellsLists H = SENTINEL_W;
    std::string msg = "untouched";
    const int rc = std_wells_lists(&sw, Nb, toOrder.data(), H, msg);
    CHECK(rc == OPMHIP_SUCCESS && msg == "untouched", "%s: rc %d, '%s'", what, rc, msg.c_str());
    CHECK(check_group(in.cell, Nb, toOrder, H.pos, H.cpos, H.cptr, H.cperf), "%s: grouping", what);
    const size_t nw = in.producer.size();
    CHECK(H.wi.size() == 3 * nw && H.wd.size() == 2 * nw && H.pack.size() == (size_t)SW_PACK * nw, "%s: sizes", what);
    for (size_t w = 0; w < nw; ++w) {
        CHECK(H.wi[3 * w] == in.producer[w] && H.wi[3 * w + 1] == (in.producer[w] ? 0 : in.inj_phase[w]) && H.wi[3 * w + 2] == in.rate_component[w], "%s: wi of well %zu", what, w);
        CHECK(H.wd[2 * w] == in.rate_target[w] && H.wd[2 * w + 1] == in.bhp_limit[w], "%s: wd of well %zu", what, w);
        for (int i = 0; i < 4; ++i) CHECK(H.pack[4 * w + i] == (in.x.empty() ? 0.0 : in.x[4 * w + i]), "%s: x of well %zu", what, w);
        CHECK(H.pack[4 * nw + w] == in.control[w], "%s: control of well %zu", what, w);   // the layout as the kernels have always read it:
        for (int i = 0; i < 4; ++i) CHECK(H.pack[5 * nw + 4 * w + i] == 0.0, "%s: r_w of well %zu", what, w);   // x | control | r_w | flag
        CHECK(H.pack[9 * nw + w] == 0.0, "%s: flag of well %zu", what, w);
    }
    return true;
}
static bool wells_refused(const char* what, const WellsInput& in, const opmhip_std_wells& sw, int Nb, const std::string& expected) {
    const std::vector<int> toOrder = permutation(Nb, 3);
    StdWellsLists H = SENTINEL_W;
    std::string msg;
    const int rc = std_wells_lists(&sw, Nb, toOrder.data(), H, msg);
    CHECK(rc == OPMHIP_INVALID_ARGUMENT, "%s: rc %d", what, rc);
    CHECK(msg == expected, "%s: '%s' instead of '%s'", what, msg.c_str(), expected.c_str());
    CHECK(same(H, SENTINEL_W), "%s: outputs touched", what);
    (void)in;
    return true;
}
static void wells_cases() {
    const int Nb = 600;
    report(wells_accepted("accepted", wells_input(2, 2, 150, {150, 64, 65, 1}, true), Nb, 21), "std_wells_lists: wells of 150 / 64 / 65 / 1 perforations, x given");
    report(wells_accepted("accepted", wells_input(2, 2, 150, {150, 64, 65, 1, 1, 150}, false), Nb, 22), "std_wells_lists: two wells sharing a cell, two sharing a column, x absent");
    report(wells_accepted("accepted", wells_input(1, 1, 1, {1}, false), 1, 23), "std_wells_lists: one well, one perforation, one cell");
    const WellsInput base = wells_input(2, 2, 150, {3, 2, 4}, true);   // wells 0 and 2 inject, well 1 produces
#define WELLS_REFUSED(what, edit, ...)                                                  \
    do {                                                                                \
        WellsInput in = base;                                                           \
        opmhip_std_wells sw;                                                            \
        bool viewed = false;                                                            \
        edit;                                                                           \
        if (!viewed) sw = in.view();                                                    \
        report(wells_refused(what, in, sw, Nb, text(__VA_ARGS__)), "refused: " what);   \
    } while (0)
#define VIEW (sw = in.view(), viewed = true)
    WELLS_REFUSED("set_std_wells: num_wells < 0", (VIEW, sw.num_wells = -2), "set_std_wells: num_wells = %d", -2);
    WELLS_REFUSED("set_std_wells: a null array", (VIEW, sw.bhp_limit = nullptr), "set_std_wells: null array (only x is optional)");
    WELLS_REFUSED("set_std_wells: control == NULL", (VIEW, sw.control = nullptr), "set_std_wells: null array (only x is optional)");
    WELLS_REFUSED("set_std_wells: perf_pointers[0] != 0", in.ptr[0] = 1, "set_std_wells: inconsistent pointers (perf_pointers[0] = %d, not 0)", 1);
    WELLS_REFUSED("set_std_wells: a well without perforation", in.ptr[2] = in.ptr[1], "set_std_wells: inconsistent pointers (well %d has no perforation)", 1);
    WELLS_REFUSED("set_std_wells: producer flag", in.producer[2] = 2, "set_std_wells: producer[%d] = %d (1 producer, 0 injector)", 2, 2);
    WELLS_REFUSED("set_std_wells: injected phase", in.inj_phase[0] = 3, "set_std_wells: unknown phase: inj_phase[%d] = %d (0 water, 1 oil, 2 gas)", 0, 3);
    WELLS_REFUSED("set_std_wells: rate component", in.rate_component[1] = -1, "set_std_wells: unknown component: rate_component[%d] = %d (0 oil, 1 water, 2 gas)", 1, -1);
    WELLS_REFUSED("set_std_wells: control", in.control[2] = 5, "set_std_wells: control[%d] = %d (0 rate, 1 bhp)", 2, 5);
    WELLS_REFUSED("set_std_wells: rate target not finite", in.rate_target[1] = NaN, "set_std_wells: rate target / bhp limit of well %d is not finite", 1);
    WELLS_REFUSED("set_std_wells: bhp limit not finite", in.bhp_limit[0] = Inf, "set_std_wells: rate target / bhp limit of well %d is not finite", 0);
    WELLS_REFUSED("set_std_wells: cell == Nb", in.cell[4] = Nb, "set_std_wells: perforation %d names cell %d, outside [0, %d)", 4, Nb, Nb);
    WELLS_REFUSED("set_std_wells: cell < 0", in.cell[0] = -1, "set_std_wells: perforation %d names cell %d, outside [0, %d)", 0, -1, Nb);
    WELLS_REFUSED("set_std_wells: tw not finite", in.tw[8] = Inf, "set_std_wells: tw / dz of perforation %d is not finite", 8);
    WELLS_REFUSED("set_std_wells: dz not finite", in.dz[2] = NaN, "set_std_wells: tw / dz of perforation %d is not finite", 2);
    // the first fault in perforation order is the one named, whatever its kind
    WELLS_REFUSED("set_std_wells: two faults, the earlier perforation is named", (in.cell[1] = -4, in.tw[0] = NaN), "set_std_wells: tw / dz of perforation %d is not finite", 0);
#undef WELLS_REFUSED
#undef VIEW
}

static bool setter_refused(const char* what, int rc, const std::string& msg, const std::string& expected) {
    CHECK(rc == OPMHIP_INVALID_ARGUMENT, "%s: rc %d", what, rc);
    CHECK(msg == expected, "%s: '%s' instead of '%s'", what, msg.c_str(), expected.c_str());
    return true;
}
static void wells_setter_cases() {
    const size_t nw = 3, np = 5;
    const std::vector<int> wi{0, 2, 1, 1, 0, 0, 1, 0, 2};   // injector, producer, producer
    std::string msg;
    auto fresh = [&]() -> std::string& { msg = "untouched"; return msg; };
    {   // set_std_wells_state
        std::vector<double> x(4 * nw, 1.0), target(nw, 5.0);
        std::vector<int> control{0, 1, 0};
        bool ok = std_wells_check_state(nw, x.data(), control.data(), target.data(), fresh()) == OPMHIP_SUCCESS && msg == "untouched";
        ok = ok && std_wells_check_state(nw, nullptr, nullptr, nullptr, fresh()) == OPMHIP_SUCCESS && msg == "untouched";
        if (!ok) { std::printf("FAILED std_wells_check_state: a good state is refused: %s\n", msg.c_str()); ++g_fail; }
        report(ok, "std_wells_check_state: accepted, with every array and with none");
        control[2] = 2;
        report(setter_refused("state", std_wells_check_state(nw, x.data(), control.data(), target.data(), fresh()), msg, text("set_std_wells_state: control[%zu] = %d (0 rate, 1 bhp)", (size_t)2, 2)),
               "refused: set_std_wells_state: control");
        control[2] = 0; target[1] = Inf;
        report(setter_refused("state", std_wells_check_state(nw, x.data(), control.data(), target.data(), fresh()), msg, text("set_std_wells_state: rate_target[%zu] is not finite", (size_t)1)),
               "refused: set_std_wells_state: rate target");
        target[1] = 1.0; x[11] = NaN;
        report(setter_refused("state", std_wells_check_state(nw, x.data(), control.data(), target.data(), fresh()), msg, text("set_std_wells_state: x[%zu] is not finite", (size_t)11)),
               "refused: set_std_wells_state: x");
    }
    {   // set_std_wells_crossflow
        std::vector<int> allow{0, 1, 0};
        bool any = false;
        bool ok = std_wells_check_crossflow(nw, allow.data(), wi.data(), any, fresh()) == OPMHIP_SUCCESS && any && msg == "untouched";
        any = true;
        ok = ok && std_wells_check_crossflow(nw, nullptr, wi.data(), any, fresh()) == OPMHIP_SUCCESS && !any;
        any = true; allow[1] = 0;
        ok = ok && std_wells_check_crossflow(nw, allow.data(), wi.data(), any, fresh()) == OPMHIP_SUCCESS && !any;
        if (!ok) { std::printf("FAILED std_wells_check_crossflow: accepted cases\n"); ++g_fail; }
        report(ok, "std_wells_check_crossflow: a producer's switch, no array, all off");
        allow[2] = 3; any = false;
        report(setter_refused("crossflow", std_wells_check_crossflow(nw, allow.data(), wi.data(), any, fresh()), msg, text("set_std_wells_crossflow: allow[%zu] = %d (0 off, 1 on)", (size_t)2, 3)) && !any,
               "refused: set_std_wells_crossflow: allow");
        allow = {1, 1, 0}; any = false;
        report(setter_refused("crossflow", std_wells_check_crossflow(nw, allow.data(), wi.data(), any, fresh()), msg,
                              text("set_std_wells_crossflow: well %zu is an injector - crossflow is modelled for producers only (the injected composition is fixed)", (size_t)0)) && !any,
               "refused: set_std_wells_crossflow: an injector");
    }
    {   // set_std_wells_head_model
        std::vector<double> depth(np, 2000.0), ref(nw, 1990.0);
        std::vector<int> phase{9, 2, 0}, pref{-1};   // the injector's is not looked at
        opmhip_std_wells_wellbore wb{depth.data(), ref.data(), phase.data()};
        bool ok = std_wells_head_model(&wb, nw, np, wi.data(), pref, fresh()) == OPMHIP_SUCCESS && pref == std::vector<int>{1, 2, 0} && msg == "untouched";
        if (!ok) { std::printf("FAILED std_wells_head_model: accepted case\n"); ++g_fail; }
        report(ok, "std_wells_head_model: pref = the producers' preferred phase, oil for an injector");
        const std::vector<int> before{-1};
        pref = before; wb.ref_depth = nullptr;
        report(setter_refused("head model", std_wells_head_model(&wb, nw, np, wi.data(), pref, fresh()), msg, text("set_std_wells_head_model: null array")) && pref == before,
               "refused: set_std_wells_head_model: a null array");
        wb.ref_depth = ref.data(); depth[4] = NaN;
        report(setter_refused("head model", std_wells_head_model(&wb, nw, np, wi.data(), pref, fresh()), msg, text("set_std_wells_head_model: perf_depth[%zu] is not finite", (size_t)4)) && pref == before,
               "refused: set_std_wells_head_model: perforation depth");
        depth[4] = 1.0; ref[0] = -Inf;
        report(setter_refused("head model", std_wells_head_model(&wb, nw, np, wi.data(), pref, fresh()), msg, text("set_std_wells_head_model: ref_depth[%zu] is not finite", (size_t)0)) && pref == before,
               "refused: set_std_wells_head_model: reference depth");
        ref[0] = 1.0; phase[2] = 3;
        report(setter_refused("head model", std_wells_head_model(&wb, nw, np, wi.data(), pref, fresh()), msg,
                              text("set_std_wells_head_model: unknown phase: preferred_phase[%zu] = %d (0 water, 1 oil, 2 gas)", (size_t)2, 3)) && pref == before,
               "refused: set_std_wells_head_model: preferred phase of a producer");
    }
    {   // set_std_wells_perf_state
        std::vector<double> pp(np, 2e7), pr(3 * np, 0.5);
        bool ok = std_wells_check_perf_state(np, pp.data(), pr.data(), false, fresh()) == OPMHIP_SUCCESS && std_wells_check_perf_state(np, pp.data(), nullptr, false, msg) == OPMHIP_SUCCESS &&
                  std_wells_check_perf_state(np, nullptr, pr.data(), true, msg) == OPMHIP_SUCCESS && msg == "untouched";
        if (!ok) { std::printf("FAILED std_wells_check_perf_state: accepted cases\n"); ++g_fail; }
        report(ok, "std_wells_check_perf_state: both, the pressures alone, the rates alone once pressures exist");
        pp[3] = NaN;
        report(setter_refused("perf state", std_wells_check_perf_state(np, pp.data(), pr.data(), false, fresh()), msg, text("set_std_wells_perf_state: perf_pressure[%zu] is not finite", (size_t)3)),
               "refused: set_std_wells_perf_state: pressure");
        pp[3] = 1.0; pr[14] = Inf;
        report(setter_refused("perf state", std_wells_check_perf_state(np, pp.data(), pr.data(), false, fresh()), msg, text("set_std_wells_perf_state: perf_rates[%zu] is not finite", (size_t)14)),
               "refused: set_std_wells_perf_state: rates");
        pr[14] = 1.0;
        report(setter_refused("perf state", std_wells_check_perf_state(np, nullptr, pr.data(), false, fresh()), msg,
                              text("set_std_wells_perf_state: rates alone before the perforation pressures exist (they are taken from the cells at the first begin_iteration(0))")),
               "refused: set_std_wells_perf_state: rates alone before the pressures exist");
    }
}

// ---- analytic aquifers ------------------------------------------------------------------------------------------------------------
struct AqInput {
    std::vector<int> type, id, ptr, cell, has_p, tabptr, has_restart;
    std::vector<double> alpha, Tc, rhow, datum, pa0, beta, td, pd, PI, ct, V0, rW, rp;
    opmhip_aquifers view() const {
        return opmhip_aquifers{(int)type.size(), type.data(), id.data(), ptr.data(), cell.data(), alpha.data(), Tc.data(), rhow.data(), datum.data(), pa0.data(),
                               has_p.empty() ? nullptr : has_p.data(), beta.data(), tabptr.data(), td.data(), pd.data(), PI.data(), ct.data(), V0.data(),
                               has_restart.empty() ? nullptr : has_restart.data(), rW.data(), rp.data()};
    }
};
// types: 0 Carter-Tracy (tables of 2, 3, 4 ... nodes), 1 Fetkovich; conns[a]: the cells of aquifer a
static AqInput aq_input(const std::vector<int>& types, const std::vector<std::vector<int>>& conns) {
    AqInput in;
    in.ptr.push_back(0);
    in.tabptr.push_back(0);
    for (size_t a = 0; a < types.size(); ++a) {
        in.type.push_back(types[a]);
        in.id.push_back(10 + (int)a);
        for (int c : conns[a]) { in.cell.push_back(c); in.alpha.push_back(1.0 / (1 + in.alpha.size())); }
        in.ptr.push_back((int)in.cell.size());
        in.Tc.push_back(1e6 * (a + 1));
        in.rhow.push_back(1000.0 + a);
        in.datum.push_back(2000.0 + 10 * a);
        in.pa0.push_back(2e7 + 1e5 * a);
        in.beta.push_back(3.0 + a);
        in.PI.push_back(1e-9 * (a + 1));
        in.ct.push_back(1e-9);
        in.V0.push_back(1e9 * (a + 1));
        in.rW.push_back(77.0 + a);
        in.rp.push_back(1.9e7 + a);
        if (types[a] == 0)
            for (int i = 0, n = 2 + (int)(in.tabptr.size() - 1); i < n; ++i) { in.td.push_back(0.5 * i * i + 0.01 * i); in.pd.push_back(std::sqrt(1.0 + i)); }
        in.tabptr.push_back((int)in.td.size());
    }
    return in;
}
static AquiferLists aq_sentinel() {
    AquiferLists L;
    L.nc = -9; L.par = {-1.0}; L.td = {-2.0}; L.pd = {-3.0}; L.tabptr = {-4}; L.need_eq = {-5}; L.of = {-6}; L.pos = {-7}; L.cpos = {-8}; L.cptr = {-9}; L.cconn = {-10};
    return L;
}
static bool same(const AquiferLists& a, const AquiferLists& b) {
    return a.nc == b.nc && a.par == b.par && a.td == b.td && a.pd == b.pd && a.tabptr == b.tabptr && a.need_eq == b.need_eq && a.of == b.of && a.pos == b.pos &&
           a.cpos == b.cpos && a.cptr == b.cptr && a.cconn == b.cconn;
}
static bool aq_accepted(const char* what, const AqInput& in, int Nb, unsigned seed, AquiferLists* keep = nullptr) {
    const std::vector<int> toOrder = permutation(Nb, seed);
    const opmhip_aquifers aq = in.view();
    AquiferLists H = aq_sentinel();
    std::string msg = "untouched";
    const int rc = aquifer_lists(&aq, Nb, toOrder.data(), H, msg);
    CHECK(rc == OPMHIP_SUCCESS && msg == "untouched", "%s: rc %d, '%s'", what, rc, msg.c_str());
    const int na = (int)in.type.size(), nc = (int)in.cell.size();
    CHECK(H.nc == nc && (int)H.of.size() == nc && (int)H.par.size() == na * AQ_PAR && (int)H.tabptr.size() == na + 1, "%s: sizes", what);
    CHECK(check_group(in.cell, Nb, toOrder, H.pos, H.cpos, H.cptr, H.cconn), "%s: grouping", what);
    std::vector<int> need;
    for (int a = 0; a < na; ++a) {
        for (int i = in.ptr[a]; i < in.ptr[a + 1]; ++i) CHECK(H.of[i] == a, "%s: of[%d]", what, i);
        const double* p = &H.par[(size_t)a * AQ_PAR];
        const bool has_p = in.has_p.empty() || in.has_p[a];
        if (!has_p) need.push_back(a);
        CHECK(p[AQ_TYPE] == in.type[a] && p[AQ_TC] == in.Tc[a] && p[AQ_RHOW] == in.rhow[a] && p[AQ_DATUM] == in.datum[a] && p[AQ_PA0] == (has_p ? in.pa0[a] : 0.0), "%s: par of %d", what, a);
        const int n = in.tabptr[a + 1] - in.tabptr[a];
        if (in.type[a] == 0) {
            CHECK(p[AQ_BETA] == in.beta[a] && p[AQ_PI] == 0.0 && p[AQ_CV] == 0.0 && H.tabptr[a + 1] - H.tabptr[a] == n, "%s: Carter-Tracy par of %d", what, a);
            for (int i = 0; i < n; ++i) CHECK(H.td[H.tabptr[a] + i] == in.td[in.tabptr[a] + i] && H.pd[H.tabptr[a] + i] == in.pd[in.tabptr[a] + i], "%s: table of %d", what, a);
        } else CHECK(p[AQ_BETA] == 0.0 && p[AQ_PI] == in.PI[a] && p[AQ_CV] == in.ct[a] * in.V0[a] && H.tabptr[a + 1] == H.tabptr[a], "%s: Fetkovich par of %d", what, a);
    }
    CHECK(H.need_eq == need && H.tabptr.back() == (int)H.td.size() && H.td.size() == H.pd.size(), "%s: need_eq / tables", what);
    if (keep) *keep = H;
    return true;
}
static bool aq_refused(const char* what, const opmhip_aquifers& aq, int Nb, const std::string& expected) {
    const std::vector<int> toOrder = permutation(Nb, 5);
    AquiferLists H = aq_sentinel();
    std::string msg;
    const int rc = aquifer_lists(&aq, Nb, toOrder.data(), H, msg);
    CHECK(rc == OPMHIP_INVALID_ARGUMENT, "%s: rc %d", what, rc);
    CHECK(msg == expected, "%s: '%s' instead of '%s'", what, msg.c_str(), expected.c_str());
    CHECK(same(H, aq_sentinel()), "%s: outputs touched", what);
    return true;
}
static void aquifer_cases() {
    const int Nb = 30;
    report(aq_accepted("accepted", aq_input({0, 0, 1, 1}, {{3, 4, 5}, {}, {5, 6, 29, 0}, {4}}), Nb, 31),
           "aquifer_lists: Carter-Tracy plus Fetkovich, an aquifer with no connection, cells shared between aquifers, cells 0 and Nb - 1");
    {
        AqInput in = aq_input({0, 1}, {{}, {}});
        opmhip_aquifers aq = in.view();
        aq.cell = nullptr; aq.alpha = nullptr;   // nothing to name
        AquiferLists H = aq_sentinel();
        std::string msg;
        const std::vector<int> toOrder = permutation(Nb, 32);
        const bool ok = aquifer_lists(&aq, Nb, toOrder.data(), H, msg) == OPMHIP_SUCCESS && H.nc == 0 && H.pos.empty() && H.cpos.empty() && H.cptr == std::vector<int>{0} && H.cconn.empty();
        if (!ok) { std::printf("FAILED aquifer_lists: nc == 0: %s\n", msg.c_str()); ++g_fail; }
        report(ok, "aquifer_lists: nc == 0, cell and alpha absent");
    }
    {
        AqInput in = aq_input({0, 1, 1}, {{1, 2}, {2, 3}, {7}});
        in.has_p = {0, 1, 0};
        in.has_restart = {0, 1, 0};
        AquiferLists H;
        bool ok = aq_accepted("accepted", in, Nb, 33, &H);
        if (ok) {
            const opmhip_aquifers aq = in.view();
            H.par[0 * AQ_PAR + AQ_PA0] = 1.5e7; H.par[2 * AQ_PAR + AQ_PA0] = 1.7e7;   // as the equilibration leaves them
            std::vector<double> state{-1.0};
            aquifer_initial_state(&aq, H.par, state);
            ok = state == std::vector<double>{0.0, 0.0, in.rW[1], in.rp[1], 0.0, 1.7e7};
            if (!ok) { std::printf("FAILED aquifer_initial_state\n"); ++g_fail; }
        }
        report(ok, "aquifer_lists / aquifer_initial_state: initial pressures absent, restart data for a Fetkovich aquifer");
    }
    const AqInput base = aq_input({0, 0, 1}, {{3, 4}, {4, 8, 9}, {9, 10}});
#define AQ_REFUSED(what, edit, ...)                                               \
    do {                                                                          \
        AqInput in = base;                                                        \
        opmhip_aquifers aq;                                                       \
        bool viewed = false;                                                      \
        edit;                                                                     \
        if (!viewed) aq = in.view();                                              \
        report(aq_refused(what, aq, Nb, text(__VA_ARGS__)), "refused: " what);    \
    } while (0)
#define VIEW (aq = in.view(), viewed = true)
    AQ_REFUSED("set_aquifers: num_aquifers < 0", (VIEW, aq.num_aquifers = -1), "set_aquifers: num_aquifers = %d", -1);
    AQ_REFUSED("set_aquifers: a mandatory array absent", (VIEW, aq.id = nullptr),
               "set_aquifers: null array (type, id, conn_pointers, time_constant, water_density, datum_depth are mandatory)");
    AQ_REFUSED("set_aquifers: conn_pointers[0] != 0", in.ptr[0] = 2, "set_aquifers: conn_pointers[0] = %d, not 0", 2);
    AQ_REFUSED("set_aquifers: conn_pointers descend", in.ptr[2] = 1, "set_aquifers: conn_pointers descend at aquifer %d", 1);
    AQ_REFUSED("set_aquifers: type", in.type[1] = 2, "set_aquifers: type[%d] = %d (0 Carter-Tracy, 1 Fetkovich)", 1, 2);
    AQ_REFUSED("set_aquifers: Fetkovich before Carter-Tracy", in.type[0] = 1,
               "set_aquifers: Carter-Tracy aquifer %d behind a Fetkovich one (Carter-Tracy first: the order of addToSource)", 1);
    AQ_REFUSED("set_aquifers: cell absent", (VIEW, aq.cell = nullptr), "set_aquifers: null array (cell / alpha)");
    AQ_REFUSED("set_aquifers: a Carter-Tracy array absent", (VIEW, aq.pd = nullptr), "set_aquifers: null array (a Carter-Tracy aquifer needs influx_constant, table_pointers, td, pd)");
    AQ_REFUSED("set_aquifers: a Fetkovich array absent", (VIEW, aq.total_compr = nullptr), "set_aquifers: null array (a Fetkovich aquifer needs prod_index, total_compr, initial_watvolume)");
    AQ_REFUSED("set_aquifers: has_restart without W_flux", (in.has_restart = {0, 0, 1}, VIEW, aq.restart_W_flux = nullptr),
               "set_aquifers: null array (has_restart without restart_W_flux / restart_pressure)");
    AQ_REFUSED("set_aquifers: has_restart without the Fetkovich pressure", (in.has_restart = {0, 0, 0}, VIEW, aq.restart_pressure = nullptr),
               "set_aquifers: null array (has_restart without restart_W_flux / restart_pressure)");
    AQ_REFUSED("set_aquifers: Tc == 0", in.Tc[1] = 0.0, "set_aquifers: aquifer %d has time constant Tc = %g, must be positive", 1, 0.0);
    AQ_REFUSED("set_aquifers: Tc NaN", in.Tc[2] = NaN, "set_aquifers: aquifer %d has time constant Tc = %g, must be positive", 2, NaN);
    AQ_REFUSED("set_aquifers: initial_pressure absent", (VIEW, aq.initial_pressure = nullptr), "set_aquifers: null array (initial_pressure)");
    AQ_REFUSED("set_aquifers: restart data for a Carter-Tracy aquifer", (in.has_restart = {0, 1, 1}),
               "set_aquifers: restart data for Carter-Tracy aquifer %d - restart-based initialisation is not supported for Carter-Tracy aquifers (as in the reference)", 1);
    AQ_REFUSED("set_aquifers: a table of one node", (in.tabptr[1] = 1), "set_aquifers: the influence table of aquifer %d has fewer than two nodes", 0);
    AQ_REFUSED("set_aquifers: a table that starts before 0", (in.tabptr[0] = -1), "set_aquifers: the influence table of aquifer %d has fewer than two nodes", 0);
    AQ_REFUSED("set_aquifers: a table not ascending", in.td[4] = in.td[3], "set_aquifers: the influence table of aquifer %d is not ascending at node %d", 1, 2);
    AQ_REFUSED("set_aquifers: Fetkovich compressible volume", in.V0[2] = -1e9, "set_aquifers: Fetkovich aquifer %d has total_compr * initial_watvolume = %g, must be positive", 2, 1e-9 * -1e9);
    AQ_REFUSED("set_aquifers: cell == Nb", in.cell[3] = Nb, "set_aquifers: connection %d of aquifer %d names cell %d, outside [0, %d)", 1, 1, Nb, Nb);
    AQ_REFUSED("set_aquifers: cell < 0", in.cell[0] = -1, "set_aquifers: connection %d of aquifer %d names cell %d, outside [0, %d)", 0, 0, -1, Nb);
    AQ_REFUSED("set_aquifers: a cell twice in one aquifer", in.cell[4] = 4, "set_aquifers: cell %d is repeated within aquifer %d (one connection per cell)", 4, 1);
#undef AQ_REFUSED
#undef VIEW
}

static bool table_cases_body() {
    // a two-node table: one interval, which every query extrapolates or interpolates on
    const double x2[2] = {1.0, 3.0}, y2[2] = {10.0, 14.0};
    for (double q : {-5.0, 1.0, 2.0, 3.0, 40.0}) {
        CHECK(table_interval(x2, 2, q) == 0, "two nodes, query %g", q);
        CHECK(table_slope(x2, y2, 2, q) == 2.0 && table_value(x2, y2, 2, q) == 2.0 * (q - 1.0) + 10.0, "two nodes, query %g", q);
    }
    const double x[5] = {0.0, 1.0, 2.5, 4.0, 8.0}, y[5] = {0.0, 2.0, 3.0, 3.5, 3.75};
    const struct { double q; int j; } at[] = {{-1.0, 0}, {0.0, 0}, {0.5, 0}, {1.0, 1}, {2.4, 1}, {2.5, 2}, {4.0, 3}, {7.9, 3}, {8.0, 3}, {100.0, 3}};   // below, on nodes, above
    for (const auto& t : at) {
        CHECK(table_interval(x, 5, t.q) == t.j, "query %g: interval %d, not %d", t.q, table_interval(x, 5, t.q), t.j);
        const double slope = (y[t.j + 1] - y[t.j]) / (x[t.j + 1] - x[t.j]);
        CHECK(table_slope(x, y, 5, t.q) == slope && table_value(x, y, 5, t.q) == slope * (t.q - x[t.j]) + y[t.j], "query %g", t.q);
    }
    for (int j = 0; j < 5; ++j) CHECK(table_value(x, y, 5, x[j]) == y[j] || j == 4, "node %d", j);   // the last node is reached from the left: one rounding
    CHECK(std::fabs(table_value(x, y, 5, x[4]) - y[4]) <= 1e-15 * y[4], "the last node");
    return true;
}
static bool step_cases_body() {
    AqInput in = aq_input({0, 1, 1, 1}, {{1}, {2}, {3}, {4}});
    in.Tc = {2e6, 1e30, 1e-3, 5e5};   // dt / Tc tiny, large, ordinary
    const std::vector<int> toOrder = permutation(10, 41);
    const opmhip_aquifers aq = in.view();
    AquiferLists H;
    std::string msg;
    CHECK(aquifer_lists(&aq, 10, toOrder.data(), H, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    const double time = 3e6, dt = 86400.0;
    std::vector<double> step(4 * AQ_STEP, -1.0);
    aquifer_step_scalars(4, H.par, H.tabptr, H.td, H.pd, time, dt, step.data());
    const double tdd = (dt + time) / 2e6;
    CHECK(step[AQ_TD] == time / 2e6 && step[AQ_PITD] == table_value(H.td.data(), H.pd.data(), 2, tdd) && step[AQ_PITDPRIME] == table_slope(H.td.data(), H.pd.data(), 2, tdd) && step[AQ_COEF] == 0.0,
          "Carter-Tracy scalars");
    for (int a = 1; a < 4; ++a) {
        const double* s = &step[(size_t)a * AQ_STEP];
        const double r = dt / in.Tc[a];
        CHECK(s[AQ_TD] == 0.0 && s[AQ_PITD] == 0.0 && s[AQ_PITDPRIME] == 0.0 && s[AQ_COEF] == (1 - std::exp(-r)) / r, "Fetkovich scalars of %d", a);
        CHECK(std::isfinite(s[AQ_COEF]) && s[AQ_COEF] >= 0.0 && s[AQ_COEF] <= 1.0, "Fetkovich coefficient of %d = %g", a, s[AQ_COEF]);
    }
    CHECK(step[2 * AQ_STEP + AQ_COEF] == 1.0 / (dt / 1e-3), "dt / Tc large: exp underflows to 0, coef = Tc / dt");
    return true;
}
static bool sums_cases_body() {
    // the equilibrium pressure of one aquifer against a restatement; the record's fields by the numbers the kernels write them at
    const int IQS = 68, n = 3, i0 = 2;
    const std::vector<double> alpha{9.0, 9.0, 0.25, 0.5, 0.125, 9.0};
    const std::vector<int> order{4, 2, 3}, p{6, 1, 3};
    std::vector<double> rec((size_t)n * IQS, -1.0), depth{0, 2010.0, 0, 2020.0, 0, 0, 2005.0};
    for (int i = 0; i < n; ++i) { rec[(size_t)i * IQS + 12] = 2e7 + 1e5 * i; rec[(size_t)i * IQS + 48] = 1000.0 + i; }   // p_w: field 3, rho_w: field 12, 4 doubles each
    const double datum = 2000.0;
    double sa = 0.0, sp = 0.0;
    for (int i = i0; i < i0 + n; ++i) sa += alpha[i];
    for (int i = 0; i < n; ++i) sp += alpha[order[i]] * ((2e7 + 1e5 * i) - (1000.0 + i) * (9.80665 * (depth[p[i]] - datum)));
    CHECK(aquifer_equilibrium_pressure(alpha.data(), i0, n, order.data(), rec.data(), IQS, depth.data(), p.data(), datum) == sp / sa, "equilibrium pressure");
    // opmhip_get_aquifers' sums
    const std::vector<double> par{0.0, 1, 1, 1, 2.5e7, 0, 0, 0, /**/ 1.0, 1, 1, 1, 2.6e7, 0, 0, 1.0, /**/ 1.0, 1, 1, 1, 2.7e7, 0, 0, 1.0};
    const std::vector<int> ptr{0, 2, 2, 5};
    const std::vector<double> state{5.0, 6.0, 7.0, 8.0, 9.0, 10.0};
    std::vector<double> q4(20, 100.0);
    for (int i = 0; i < 5; ++i) q4[4 * i] = 1.0 + 0.1 * i;
    std::vector<double> W(3, -1), P(3, -1), F(3, -1), I(3, -1);
    aquifer_report(3, par, ptr, state.data(), q4.data(), W.data(), P.data(), F.data(), I.data());
    CHECK((W == std::vector<double>{5.0, 7.0, 9.0}) && (P == std::vector<double>{2.5e7, 8.0, 10.0}) && (I == std::vector<double>{2.5e7, 2.6e7, 2.7e7}), "report");
    CHECK(F[0] == 1.0 + 1.1 && F[1] == 0.0 && F[2] == (1.2 + 1.3) + 1.4, "flux sums, an aquifer with no connection");
    aquifer_report(3, par, ptr, state.data(), nullptr, nullptr, nullptr, nullptr, nullptr);   // every output may be absent
    return true;
}

int main() {
    group_cases();
    wells_cases();
    wells_setter_cases();
    aquifer_cases();
    report(table_cases_body(), "tables: two nodes; queries below the first node, on nodes, above the last");
    report(step_cases_body(), "aquifer_step_scalars: Carter-Tracy; Fetkovich at dt / Tc tiny, large and ordinary");
    report(sums_cases_body(), "aquifer_equilibrium_pressure against a restatement; aquifer_report");
    if (g_fail) {
        std::printf("%d checks FAILED\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
