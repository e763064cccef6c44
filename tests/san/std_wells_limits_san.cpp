// The checks and the packing behind opmhip_set_std_wells_limits and the control values 3 .. 7 of opmhip_set_std_wells_state
// (csrc/source_lists.cpp: std_wells_limits, std_wells_limits_check_controls) under AddressSanitizer + UBSan + libstdc++'s container
// assertions (test infrastructure; built and run by tests/test_std_wells_limits_sanitized.py with g++, no GPU).  source_lists.cpp is
// linked alone, with no stand-in for any HIP runtime call: that the link succeeds is the check that the unit makes none.  Every refusal is
// provoked once and must come back with OPMHIP_INVALID_ARGUMENT, a text that names the reason, and the outputs untouched.
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

// three wells: a producer on an oil target, a producer on a gas target, a water injector (wi: producer, injected phase, rate component)
static const std::vector<int> WI{1, 0, 0, 1, 0, 2, 0, 0, 1};
struct Lim {
    std::vector<double> oil{Inf, 2.0, Inf}, water{3.0, Inf, Inf}, gas{4.0, Inf, Inf}, liquid{5.0, 6.0, Inf}, resv{Inf, 7.0, 8.0};
    std::vector<int> use{1, 1, 1}, control{0, 0, 0};
    opmhip_std_wells_limits t{};
    const opmhip_std_wells_limits* link() {
        t.oil_rate = oil.data(); t.water_rate = water.data(); t.gas_rate = gas.data(); t.liquid_rate = liquid.data(); t.resv_rate = resv.data();
        t.use_list_target = use.data();
        return &t;
    }
};
static StdWellsLimitsLists sentinel() {
    StdWellsLimitsLists H;
    H.lim = {-1.0, -2.0};
    H.use = {7};
    H.any = true;
    return H;
}
static bool untouched(const StdWellsLimitsLists& H) { return H.lim == std::vector<double>{-1.0, -2.0} && H.use == std::vector<int>{7} && H.any && !H.any_resv; }

static bool packing() {
    Lim l;
    StdWellsLimitsLists H;
    std::string msg;
    CHECK(std_wells_limits(l.link(), 3, WI.data(), l.control.data(), H, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    const std::vector<double> want{Inf, 3.0, 4.0, 5.0, Inf, 2.0, Inf, Inf, 6.0, 7.0, Inf, Inf, Inf, Inf, 8.0};
    CHECK(H.lim == want && H.use == std::vector<int>({1, 1, 1}) && H.any && H.any_resv, "the packed limits");
    // NULL arrays: none of that kind; NULL use_list_target: all 1; the struct itself NULL: off
    l.link();
    l.t.resv_rate = nullptr; l.t.use_list_target = nullptr; l.t.oil_rate = nullptr;
    CHECK(std_wells_limits(&l.t, 3, WI.data(), l.control.data(), H, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(H.lim[4] == Inf && H.lim[9] == Inf && H.lim[14] == Inf && H.lim[5] == Inf && H.lim[3] == 5.0 && H.any && !H.any_resv && H.use[2] == 1, "NULL arrays");
    CHECK(std_wells_limits(nullptr, 3, WI.data(), l.control.data(), H, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(!H.any && !H.any_resv && H.lim == std::vector<double>(15, Inf) && H.use == std::vector<int>(3, 1), "switched off");
    // use_list_target = 0 alone counts as a limit set (the own target leaves the checks), for a well that is not under control 0
    Lim u;
    u.oil = {9.0, Inf, Inf}; u.use = {0, 1, 1}; u.control = {1, 0, 0};
    CHECK(std_wells_limits(u.link(), 3, WI.data(), u.control.data(), H, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(H.lim[0] == 9.0 && H.use[0] == 0 && H.any, "the own target's component may carry a limit once the own target is out");
    // a well under control of a limit keeps it
    Lim k;
    k.control = {6, 7, 7};
    CHECK(std_wells_limits(k.link(), 3, WI.data(), k.control.data(), H, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    std::printf("ok  packing\n");
    return true;
}

static bool refused(const char* what, const char* text, void (*change)(Lim&)) {
    Lim l;
    change(l);
    StdWellsLimitsLists H = sentinel();
    std::string msg;
    const int rc = std_wells_limits(l.link(), 3, WI.data(), l.control.data(), H, msg);
    CHECK(rc == OPMHIP_INVALID_ARGUMENT, "%s: code %d", what, rc);
    CHECK(msg.find("set_std_wells_limits") != std::string::npos && msg.find(text) != std::string::npos, "%s: text '%s'", what, msg.c_str());
    CHECK(untouched(H), "%s: the outputs changed", what);
    std::printf("ok  refused: %s\n", what);
    return true;
}

static bool controls() {
    Lim l;
    StdWellsLimitsLists H;
    std::string msg;
    l.use = {1, 0, 1}; l.control = {0, 1, 0};
    CHECK(std_wells_limits(l.link(), 3, WI.data(), l.control.data(), H, msg) == OPMHIP_SUCCESS, "%s", msg.c_str());
    const std::vector<int> thp{0, -1, -1};
    auto check = [&](std::vector<int> c, const int* table) { msg.clear(); return std_wells_limits_check_controls(3, c.data(), table, H.lim.data(), H.use.data(), msg); };
    CHECK(check({4, 3, 7}, nullptr) == OPMHIP_SUCCESS && check({5, 6, 0}, nullptr) == OPMHIP_SUCCESS && check({2, 7, 1}, thp.data()) == OPMHIP_SUCCESS, "%s", msg.c_str());
    CHECK(std_wells_limits_check_controls(3, nullptr, nullptr, H.lim.data(), H.use.data(), msg) == OPMHIP_SUCCESS, "no controls handed in");
    struct { std::vector<int> c; const int* table; const char* text; } bad[] = {
        {{8, 1, 0}, nullptr, "control[0] = 8"}, {{-1, 1, 0}, nullptr, "control[0] = -1"}, {{3, 1, 0}, nullptr, "without that limit"},
        {{0, 1, 6}, nullptr, "without that limit"}, {{0, 0, 0}, nullptr, "use_list_target = 0"}, {{2, 1, 0}, nullptr, "without a THP limit"},
        {{0, 2, 0}, thp.data(), "without a THP limit"}};
    for (auto& b : bad) {
        const int rc = check(b.c, b.table);
        CHECK(rc == OPMHIP_INVALID_ARGUMENT && msg.find("set_std_wells_state") != std::string::npos && msg.find(b.text) != std::string::npos, "%s: %d '%s'", b.text, rc,
              msg.c_str());
        std::printf("ok  refused: control, %s\n", b.text);
    }
    std::printf("ok  controls\n");
    return true;
}

int main() {
    packing();
    refused("NaN", "not > 0", [](Lim& l) { l.liquid[0] = NaN; });
    refused("-infinity", "not > 0", [](Lim& l) { l.resv[1] = -Inf; });
    refused("zero", "not > 0", [](Lim& l) { l.gas[0] = 0.0; });
    refused("negative", "not > 0", [](Lim& l) { l.water[0] = -3.0; });
    refused("the own target's component, producer 0", "already names", [](Lim& l) { l.oil[0] = 1.0; });
    refused("the own target's component, producer 1", "already names", [](Lim& l) { l.gas[1] = 1.0; });
    refused("a producer's limit on an injector", "is an injector", [](Lim& l) { l.liquid[2] = 1.0; });
    refused("a component limit on an injector", "is an injector", [](Lim& l) { l.water[2] = 1.0; });
    refused("use_list_target out of range", "(0 / 1)", [](Lim& l) { l.use[1] = 2; });
    refused("use_list_target = 0 under control 0", "under control 0", [](Lim& l) { l.use[0] = 0; });
    refused("use_list_target = 0 for an injector under control 0", "under control 0", [](Lim& l) { l.use[2] = 0; });
    refused("taking away the limit in force (LRAT)", "cannot be taken away", [](Lim& l) { l.control[0] = 6; l.liquid[0] = Inf; });
    refused("taking away the limit in force (RESV, injector)", "cannot be taken away", [](Lim& l) { l.control[2] = 7; l.resv[2] = Inf; });
    refused("a control whose limit was never there", "cannot be taken away", [](Lim& l) { l.control[1] = 4; });
    controls();
    // the struct NULL while a well is under a limit's control: switching off takes the limit away
    {
        std::vector<int> c{0, 6, 0};
        StdWellsLimitsLists H = sentinel();
        std::string msg;
        const int rc = std_wells_limits(nullptr, 3, WI.data(), c.data(), H, msg);
        if (rc == OPMHIP_INVALID_ARGUMENT && msg.find("cannot be taken away") != std::string::npos && untouched(H)) std::printf("ok  refused: off while in force\n");
        else { std::printf("FAILED off while in force: %d '%s'\n", rc, msg.c_str()); ++g_fail; }
    }
    if (g_fail) { std::printf("%d checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
