// end_points_refusal (csrc/fluid_tables.cpp): the one check opmhip_set_endpoint_scaling and opmhip_set_hysteresis put a cell's scaled
// end points through before anything is uploaded, on accepted and on refused inputs, under AddressSanitizer + UBSan + libstdc++'s
// container assertions (test infrastructure; built and run by tests/test_host_logic_sanitized.py with g++, no GPU).
// fluid_tables.cpp is linked alone: that the link succeeds is the check that the unit makes no HIP call.
// Three saturation regions: 0 with every curve mobile, 1 whose krw is zero up to 1 - SOWCR - SGL (KRWR = 0), 2 with an immobile gas
// phase (the maximum of krg and KRGR both 0).  One line per case: "ok  <name>" or "FAILED <name>: <text>".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../opm-autodiff_amd/csrc/fluid_tables.hpp"

using namespace opmhip;

namespace {
int failures = 0;
void expect(const char* name, const std::string& got, const char* want) {   // want: a part of the refusal's text, "" = accepted
    const bool ok = want[0] ? got.find(want) != std::string::npos : got.empty();
    if (ok) std::printf("ok  %s%s%s\n", name, got.empty() ? "" : ": ", got.c_str());
    else { std::printf("FAILED %s: got \"%s\", wanted \"%s\"\n", name, got.c_str(), want); ++failures; }
}
}  // namespace

int main() {
    const double bar = 1e5;
    const double pvtw[5] = {250 * bar, 1.03, 4.5e-10, 0.35e-3, 1e-10}, density[3] = {850.0, 1030.0, 0.9};
    const int pvdg_ptr[2] = {0, 2};
    const double pvdg[6] = {50 * bar, 0.02, 1.4e-5, 400 * bar, 0.004, 2.6e-5};
    const int node_ptr[2] = {0, 2}, row_ptr[3] = {0, 1, 3};
    const double pvto_rs[2] = {10.0, 150.0};
    const double pvto[9] = {60 * bar, 1.1, 1.2e-3, 280 * bar, 1.5, 0.5e-3, 450 * bar, 1.45, 0.6e-3};
    // SWOF (Sw, krw, krow, pcow) and SGOF (Sg, krg, krog, pcog) of the three regions, five rows each
    const double swof[3][20] = {
        {0.1, 0.0, 0.9, 4e4, 0.2, 0.0, 0.7, 3e4, 0.5, 0.2, 0.2, 1e4, 0.8, 0.5, 0.0, 5e3, 1.0, 0.8, 0.0, 0.0},
        {0.1, 0.0, 0.9, 4e4, 0.2, 0.0, 0.7, 3e4, 0.5, 0.0, 0.2, 1e4, 0.8, 0.0, 0.0, 5e3, 1.0, 0.8, 0.0, 0.0},     // krw = 0 up to Sw = 0.8 = 1 - SOWCR
        {0.1, 0.0, 0.9, 4e4, 0.2, 0.0, 0.7, 3e4, 0.5, 0.2, 0.2, 1e4, 0.8, 0.5, 0.0, 5e3, 1.0, 0.8, 0.0, 0.0}};
    const double sgof[3][20] = {
        {0.0, 0.0, 0.9, 0.0, 0.05, 0.0, 0.8, 1e3, 0.4, 0.3, 0.2, 5e3, 0.7, 0.6, 0.0, 8e3, 0.9, 0.9, 0.0, 1e4},
        {0.0, 0.0, 0.9, 0.0, 0.05, 0.0, 0.8, 1e3, 0.4, 0.3, 0.2, 5e3, 0.7, 0.6, 0.0, 8e3, 0.9, 0.9, 0.0, 1e4},
        {0.0, 0.0, 0.9, 0.0, 0.05, 0.0, 0.8, 1e3, 0.4, 0.0, 0.2, 5e3, 0.7, 0.0, 0.0, 8e3, 0.9, 0.0, 0.0, 1e4}};   // the gas never moves
    std::vector<double> W, G;
    for (int r = 0; r < 3; ++r) { W.insert(W.end(), swof[r], swof[r] + 20); G.insert(G.end(), sgof[r], sgof[r] + 20); }
    const int sat_ptr[4] = {0, 5, 10, 15};
    opmhip_fluid fl;
    std::memset(&fl, 0, sizeof(fl));
    fl.num_pvt = 1; fl.num_sat = 3;
    fl.pvtw = pvtw; fl.density = density; fl.pvdg_ptr = pvdg_ptr; fl.pvdg = pvdg;
    fl.pvto_node_ptr = node_ptr; fl.pvto_rs = pvto_rs; fl.pvto_row_ptr = row_ptr; fl.pvto = pvto;
    fl.swof_ptr = sat_ptr; fl.swof = W.data(); fl.sgof_ptr = sat_ptr; fl.sgof = G.data();
    fl.rock_pref = 1e5; fl.pc_scaling = 1;
    FluidTables T;
    const std::string err = build_fluid_tables(&fl, T);
    if (!err.empty()) { std::printf("FAILED build_fluid_tables: %s\n", err.c_str()); return 1; }
    double u[3][EPS_COUNT];
    for (int r = 0; r < 3; ++r) sat_end_points(T, r, u[r]);
    // the tables are what the cases below are cut for
    expect("region 0: every denominator positive", (u[0][EPS_KRWR] > 0 && u[0][EPS_KRORW] > 0 && u[0][EPS_KRGR] > 0 && u[0][EPS_KRORG] > 0 && u[0][EPS_MAXKRG] > 0) ? "" : "a denominator is 0", "");
    expect("region 1: KRWR = 0 under a positive maximum", (u[1][EPS_KRWR] == 0.0 && u[1][EPS_MAXKRW] > 0) ? "" : "KRWR is not 0", "");
    expect("region 2: the maximum of krg and KRGR are 0", (u[2][EPS_MAXKRG] == 0.0 && u[2][EPS_KRGR] == 0.0) ? "" : "krg is not 0", "");

    // ---- accepted ----
    for (int r = 0; r < 2; ++r) expect("accepted: the table's own points, no vertical scaling", end_points_refusal(u[r], u[r], true, 0, 0, 0), "");
    expect("accepted: region 2's own points without saturation scaling", end_points_refusal(u[2], u[2], false, 0, 0, 0), "");
    for (int m = 0; m < 3; ++m) expect("accepted: region 0, one mode for every curve", end_points_refusal(u[0], u[0], true, m, m, m), "");
    double s[EPS_COUNT];
    auto fresh = [&](int r) { std::memcpy(s, u[r], sizeof(s)); };
    fresh(0); s[EPS_SWL] = 0.12; s[EPS_SWCR] = 0.12; s[EPS_SWU] = 0.95; s[EPS_SOWCR] = 0.05; s[EPS_SGU] = 0.8;
    expect("accepted: SWCR == SWL, 1 - SOWCR - SGL == SWU", end_points_refusal(s, u[0], true, 2, 2, 2), "");
    expect("accepted: region 1 with krw in mode 1 (divides by the maximum, 0.8)", end_points_refusal(u[1], u[1], true, 1, 0, 2), "");
    expect("refused: region 1, kro in mode 2 (SWCR = 0.8, where krow is 0: KRORW = 0)", end_points_refusal(u[1], u[1], true, 1, 2, 2), "scale krow vertically (mode 2)");
    expect("accepted: region 2 with krg and kro unscaled", end_points_refusal(u[2], u[2], false, 2, 0, 0), "");
    fresh(0); s[EPS_SWL] = 0.9; s[EPS_SWU] = 0.5;
    expect("accepted: an empty interval without saturation scaling", end_points_refusal(s, u[0], false, 2, 2, 2), "");

    // ---- refused: no saturation interval ----
    const char* NO = "no saturation interval";
    fresh(0); s[EPS_SWU] = s[EPS_SWL];
    expect("refused: SWL == SWU", end_points_refusal(s, u[0], true, 0, 0, 0), NO);
    fresh(0); s[EPS_SGU] = s[EPS_SGL];
    expect("refused: SGL == SGU", end_points_refusal(s, u[0], true, 0, 0, 0), NO);
    fresh(0); s[EPS_SWCR] = s[EPS_SWU];
    expect("refused: SWCR == SWU", end_points_refusal(s, u[0], true, 0, 0, 0), NO);
    fresh(0); s[EPS_SGCR] = s[EPS_SGU];
    expect("refused: SGCR == SGU", end_points_refusal(s, u[0], true, 0, 0, 0), NO);
    fresh(0); s[EPS_SOWCR] = 1.0 - s[EPS_SWL] - s[EPS_SGL];
    expect("refused: SWL + SGL == 1 - SOWCR", end_points_refusal(s, u[0], true, 0, 0, 0), NO);
    fresh(0); s[EPS_SOGCR] = 1.0 - s[EPS_SWL] - s[EPS_SGL];
    expect("refused: SOGCR == 1 - SWL - SGL", end_points_refusal(s, u[0], true, 0, 0, 0), NO);
    fresh(0); s[EPS_SWL] = 0.9; s[EPS_SWU] = 0.5;
    expect("refused: SWL > SWU", end_points_refusal(s, u[0], true, 2, 2, 2), NO);

    expect("refused: region 2's own points under saturation scaling (an immobile gas has SGCR == SGU)", end_points_refusal(u[2], u[2], true, 0, 0, 0), NO);

    // ---- refused: a table denominator of 0 ----
    expect("refused: region 1, krw in mode 2", end_points_refusal(u[1], u[1], true, 2, 0, 0), "scale krw vertically (mode 2)");
    expect("refused: region 1, krw in mode 2, without saturation scaling", end_points_refusal(u[1], u[1], false, 2, 0, 0), "scale krw vertically (mode 2)");
    expect("refused: region 2, krg in mode 1", end_points_refusal(u[2], u[2], false, 0, 0, 1), "scale krg vertically (mode 1)");
    expect("refused: region 2, krg in mode 2", end_points_refusal(u[2], u[2], false, 0, 0, 2), "scale krg vertically (mode 2)");
    double z[EPS_COUNT];
    std::memcpy(z, u[0], sizeof(z)); z[EPS_MAXKROW] = 0.0;
    expect("refused: a maximum of krow of 0, kro in mode 1", end_points_refusal(u[0], z, true, 0, 1, 0), "scale krow vertically (mode 1)");
    std::memcpy(z, u[0], sizeof(z)); z[EPS_KRORG] = 0.0;
    expect("refused: KRORG of 0, kro in mode 2", end_points_refusal(u[0], z, true, 0, 2, 0), "scale krog vertically (mode 2)");
    std::memcpy(z, u[0], sizeof(z)); z[EPS_KRORG] = 0.0;
    expect("accepted: KRORG of 0, kro in mode 1", end_points_refusal(u[0], z, true, 0, 1, 0), "");

    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
