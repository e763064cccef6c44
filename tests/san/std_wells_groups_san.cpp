// The checks and the packing behind opmhip_set_std_wells_groups, opmhip_set_std_wells_guide_rates, opmhip_set_std_wells_group_targets and the
// control value 8 of opmhip_set_std_wells_state (csrc/source_lists.cpp: std_wells_groups, std_wells_groups_check_guide_rates,
// std_wells_group_targets, std_wells_groups_check_controls) under AddressSanitizer + UBSan + libstdc++'s container assertions (test
// infrastructure; built and run by tests/test_std_wells_groups_sanitized.py with g++, no GPU).  source_lists.cpp is linked alone, with no
// stand-in for any HIP runtime call: that the link succeeds is the check that the unit makes none.  Every refusal is provoked once and must
// come back with OPMHIP_INVALID_ARGUMENT, a text that names the reason, and the outputs untouched.
#include <cstdio>
#include <cstring>
#include <limits>
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
static const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();

// five wells (wi: producer, injected phase, rate component): producers 0, 1, 3, 4, a water injector 2; two groups, their wells interleaved
static const std::vector<int> WI{1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 2, 1, 0, 0};
struct Grp {
    std::vector<int> of{1, 0, 0, 1, -1}, mode{0, 4}, available{1, 1, 1, 0, 1}, control{0, 0, 0, 1, 0};
    std::vector<double> oil{2.0, Inf}, water{Inf, Inf}, gas{Inf, 3.0}, liquid{Inf, 4.0}, resv{5.0, Inf}, guide;
    opmhip_std_wells_groups t{};
    Grp() : guide(25, 1.5) { guide[7] = 0.0; }
    const opmhip_std_wells_groups* link() {
        t.num_groups = 2; t.well_group = of.data(); t.oil_target = oil.data(); t.water_target = water.data(); t.gas_target = gas.data();
        t.liquid_target = liquid.data(); t.resv_target = resv.data(); t.mode = mode.data(); t.guide_rate = guide.data(); t.available = available.data();
        t.nupcol = 3;
        return &t;
    }
};
static StdWellsGroupsLists sentinel() {
    StdWellsGroupsLists H;
    H.num_groups = 7; H.nupcol = 9;
    H.ptr = {0, 1}; H.idx = {3}; H.target = {-1.0}; H.mode = {5}; H.any = true;
    return H;
}
static bool untouched(const StdWellsGroupsLists& H) {
    return H.num_groups == 7 && H.nupcol == 9 && H.ptr == std::vector<int>{0, 1} && H.idx == std::vector<int>{3} && H.target == std::vector<double>{-1.0} &&
           H.mode == std::vector<int>{5} && H.any && !H.any_resv && H.of.empty() && H.guide.empty() && H.resv.empty() && H.available.empty();
}

static bool packing() {
    Grp g;
    StdWellsGroupsLists H;
    std::string msg;
    CHECK(std_wells_groups(g.link(), 5, WI.data(), g.control.data(), H, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    // group 0: wells 1 (producer) and 2 (injector: ignored); group 1: wells 0 and 3
    CHECK(H.ptr == std::vector<int>({0, 1, 3}) && H.idx == std::vector<int>({1, 0, 3}), "the groups' producers, ascending");
    const std::vector<double> want{2.0, Inf, Inf, Inf, 5.0, Inf, Inf, 3.0, 4.0, Inf};
    CHECK(H.target == want && H.mode == std::vector<int>({0, 4}) && H.num_groups == 2 && H.nupcol == 3 && H.any && H.any_resv, "targets and modes");
    CHECK(H.resv == std::vector<int>({0, 1, 0, 0, 0}) && H.of == g.of && H.available == g.available && H.guide == g.guide, "per-well arrays");
    // NULL arrays: none of that kind, all modes NONE, all available; NULL / no groups: off
    g.link();
    g.t.resv_target = nullptr; g.t.mode = nullptr; g.t.available = nullptr;
    CHECK(std_wells_groups(&g.t, 5, WI.data(), g.control.data(), H, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(!H.any_resv && H.mode == std::vector<int>({0, 0}) && H.available == std::vector<int>(5, 1) && H.target[4] == Inf && H.resv == std::vector<int>(5, 0), "NULL arrays");
    CHECK(std_wells_groups(nullptr, 5, WI.data(), g.control.data(), H, msg) == OPMHIP_SUCCESS && !H.any && H.num_groups == 0 && H.idx.empty(), "switched off");
    g.link();
    g.t.num_groups = 0;
    CHECK(std_wells_groups(&g.t, 5, WI.data(), g.control.data(), H, msg) == OPMHIP_SUCCESS && !H.any, "no groups");
    // a well under control 8 that stays an available producer in a group
    Grp k;
    k.control = {8, 8, 1, 0, 0};
    CHECK(std_wells_groups(k.link(), 5, WI.data(), k.control.data(), H, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    // a group without a producer
    Grp e;
    e.of = {1, -1, 0, 1, -1};
    e.resv = {Inf, Inf};
    CHECK(std_wells_groups(e.link(), 5, WI.data(), e.control.data(), H, msg) == OPMHIP_SUCCESS && H.ptr == std::vector<int>({0, 0, 2}), "%s", msg.c_str());
    std::printf("ok  packing\n");
    return true;
}

static bool refused(const char* what, const char* text, void (*change)(Grp&)) {
    Grp g;
    g.link();
    change(g);
    StdWellsGroupsLists H = sentinel();
    std::string msg;
    const int rc = std_wells_groups(&g.t, 5, WI.data(), g.control.data(), H, msg);
    CHECK(rc == OPMHIP_INVALID_ARGUMENT, "%s: code %d", what, rc);
    CHECK(msg.find("set_std_wells_groups") == 0 && msg.find(text) != std::string::npos, "%s: text '%s'", what, msg.c_str());
    CHECK(untouched(H), "%s: the outputs changed", what);
    std::printf("ok  refused: %s\n", what);
    return true;
}

static bool events() {
    Grp g;
    StdWellsGroupsLists cur, H;
    std::string msg;
    CHECK(std_wells_groups(g.link(), 5, WI.data(), g.control.data(), cur, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    // new targets: a NULL array stays; the RESV flags follow
    const std::vector<double> liquid{6.0, 7.0}, resv{Inf, 8.0};
    const double* arr[5] = {nullptr, nullptr, nullptr, liquid.data(), resv.data()};
    const std::vector<int> mode{4, 5};
    CHECK(std_wells_group_targets(cur, 5, arr, mode.data(), H, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(H.target[3] == 6.0 && H.target[8] == 7.0 && H.target[4] == Inf && H.target[9] == 8.0 && H.target[0] == 2.0 && H.mode == mode, "the new targets");
    CHECK(H.resv == std::vector<int>({1, 0, 0, 1, 0}) && H.any_resv && H.idx == cur.idx && H.guide == cur.guide, "the RESV flags");
    const double* none[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    CHECK(std_wells_group_targets(cur, 5, none, nullptr, H, msg) == OPMHIP_SUCCESS && H.target == cur.target && H.mode == cur.mode, "nothing handed in");
    auto refuse_targets = [&](const char* what, std::vector<double> v, int kind, std::vector<int> m, const char* text) {
        const double* a[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        if (kind >= 0) a[kind] = v.data();
        StdWellsGroupsLists out = sentinel();
        msg.clear();
        const int rc = std_wells_group_targets(cur, 5, a, m.empty() ? nullptr : m.data(), out, msg);
        if (rc != OPMHIP_INVALID_ARGUMENT || msg.find("set_std_wells_group_targets") != 0 || msg.find(text) == std::string::npos || !untouched(out)) {
            std::printf("FAILED %s: %d '%s'\n", what, rc, msg.c_str());
            ++g_fail;
            return;
        }
        std::printf("ok  refused: targets, %s\n", what);
    };
    refuse_targets("a mode without its target", {}, -1, {2, 4}, "has no such target");
    refuse_targets("taking away the target of the mode in force", {1.0, Inf}, 3, {}, "has no such target");
    refuse_targets("NaN", {NaN, 1.0}, 0, {}, "not > 0");
    refuse_targets("zero", {1.0, 0.0}, 1, {}, "not > 0");
    refuse_targets("-infinity", {-Inf, 1.0}, 4, {}, "not > 0");
    refuse_targets("a mode out of range", {}, -1, {0, 6}, "mode[1] = 6");
    // guide rates
    std::vector<double> gr(25, 2.0);
    CHECK(std_wells_groups_check_guide_rates(5, gr.data(), msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    struct { int at; double v; } badg[] = {{3, -1.0}, {24, NaN}, {10, Inf}};
    for (auto& b : badg) {
        std::vector<double> v = gr;
        v[b.at] = b.v;
        msg.clear();
        const int rc = std_wells_groups_check_guide_rates(5, v.data(), msg);
        CHECK(rc == OPMHIP_INVALID_ARGUMENT && msg.find("set_std_wells_guide_rates") == 0 && msg.find("negative or not finite") != std::string::npos, "guide %d: '%s'", b.at, msg.c_str());
        std::printf("ok  refused: guide rate %d\n", b.at);
    }
    msg.clear();
    CHECK(std_wells_groups_check_guide_rates(5, nullptr, msg) == OPMHIP_INVALID_ARGUMENT && msg.find("null array") != std::string::npos, "'%s'", msg.c_str());
    std::printf("ok  refused: guide rates NULL\n");
    std::printf("ok  events\n");
    return true;
}

static bool controls() {
    Grp g;
    StdWellsGroupsLists H;
    std::string msg;
    CHECK(std_wells_groups(g.link(), 5, WI.data(), g.control.data(), H, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    auto check = [&](std::vector<int> c, bool groups) {
        msg.clear();
        return std_wells_groups_check_controls(5, c.data(), WI.data(), groups ? H.of.data() : nullptr, groups ? H.available.data() : nullptr, msg);
    };
    CHECK(check({8, 8, 1, 0, 7}, true) == OPMHIP_SUCCESS && check({0, 1, 2, 3, 4}, false) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(std_wells_groups_check_controls(5, nullptr, WI.data(), nullptr, nullptr, msg) == OPMHIP_SUCCESS, "no controls handed in");
    struct { std::vector<int> c; bool groups; const char* text; } bad[] = {
        {{8, 0, 0, 0, 0}, false, "without groups in force"}, {{0, 0, 8, 0, 0}, true, "for an injector"}, {{0, 0, 0, 0, 8}, true, "without a group"},
        {{0, 0, 0, 8, 0}, true, "not available"}};
    for (auto& b : bad) {
        const int rc = check(b.c, b.groups);
        CHECK(rc == OPMHIP_INVALID_ARGUMENT && msg.find("set_std_wells_state") == 0 && msg.find("= 8") != std::string::npos && msg.find(b.text) != std::string::npos, "%s: %d '%s'",
              b.text, rc, msg.c_str());
        std::printf("ok  refused: control, %s\n", b.text);
    }
    std::printf("ok  controls\n");
    return true;
}

int main() {
    packing();
    refused("num_groups < 0", "num_groups = -1", [](Grp& g) { g.t.num_groups = -1; });
    refused("well_group NULL", "null array", [](Grp& g) { g.t.well_group = nullptr; });
    refused("guide_rate NULL", "null array", [](Grp& g) { g.t.guide_rate = nullptr; });
    refused("a group index too large", "outside [-1, 2)", [](Grp& g) { g.of[4] = 2; });
    refused("a group index below -1", "outside [-1, 2)", [](Grp& g) { g.of[0] = -2; });
    refused("a NaN target", "not > 0", [](Grp& g) { g.liquid[0] = NaN; });
    refused("a -infinity target", "not > 0", [](Grp& g) { g.resv[1] = -Inf; });
    refused("a zero target", "not > 0", [](Grp& g) { g.gas[0] = 0.0; });
    refused("a negative target", "not > 0", [](Grp& g) { g.oil[0] = -2.0; });
    refused("a mode whose target the group lacks", "has no such target", [](Grp& g) { g.mode[0] = 2; });
    refused("a mode out of range", "mode[1] = 6", [](Grp& g) { g.mode[1] = 6; });
    refused("a negative mode", "mode[0] = -1", [](Grp& g) { g.mode[0] = -1; });
    refused("a negative guide rate", "negative or not finite", [](Grp& g) { g.guide[12] = -0.5; });
    refused("an infinite guide rate", "negative or not finite", [](Grp& g) { g.guide[0] = Inf; });
    refused("a NaN guide rate", "negative or not finite", [](Grp& g) { g.guide[24] = NaN; });
    refused("available out of range", "(0 / 1)", [](Grp& g) { g.available[1] = 2; });
    refused("nupcol < 0", "nupcol = -1", [](Grp& g) { g.t.nupcol = -1; });
    refused("control 8 for an injector", "under control 8", [](Grp& g) { g.control[2] = 8; });
    refused("control 8 for a well without a group", "under control 8", [](Grp& g) { g.control[4] = 8; });
    refused("control 8 for an unavailable well", "under control 8", [](Grp& g) { g.control[3] = 8; });
    // removing the groups while a well is under control 8
    {
        std::vector<int> c{0, 8, 0, 0, 0};
        StdWellsGroupsLists H = sentinel();
        std::string msg;
        const int rc = std_wells_groups(nullptr, 5, WI.data(), c.data(), H, msg);
        if (rc == OPMHIP_INVALID_ARGUMENT && msg.find("cannot be removed") != std::string::npos && untouched(H)) std::printf("ok  refused: removed while in force\n");
        else { std::printf("FAILED removed while in force: %d '%s'\n", rc, msg.c_str()); ++g_fail; }
    }
    events();
    controls();
    if (g_fail) { std::printf("%d checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
