// Host set-up of the fluid-in-place report (csrc/fip_setup.cpp: the checks with their codes and texts, the region lists, the chunk
// descriptors of every level, the pressure averages) under AddressSanitizer + UBSan + libstdc++'s container assertions (test
// infrastructure; built and run by tests/test_fip_setup_sanitized.py with g++, no GPU).  fip_setup.cpp is linked alone, with no stand-in
// for any HIP runtime call: that the link succeeds is the check that the set-up makes none.  A plan is checked twice: its index ranges
// (every read inside what an earlier level wrote, every slot written once) and its meaning - the descriptors are walked on the host the
// way k_fip_reduce walks them, lane by lane, and the region's value is held against a restatement of the stated order that knows nothing
// of descriptors.
#include <cmath>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "../../opm-autodiff_amd/csrc/fip_setup.hpp"

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

// one chunk as one wavefront forms it: x(i) = item i of the chunk or 0.0 beyond its count
template <class X>
static double chunk_sum(int count, X x) {
    double v[64];
    for (int l = 0; l < 64; ++l) {
        double a = 0.0;
        for (int k = 0; k < 4; ++k) {
            const int i = l + 64 * k;
            a = a + (i < count ? x(i) : 0.0);
        }
        v[l] = a;
    }
    for (int o = 32; o > 0; o >>= 1)
        for (int l = 0; l < o; ++l) v[l] = v[l] + v[l + o];
    return v[0];
}
// the stated order on a plain list
static double reduce256(std::vector<double> x) {
    for (;;) {
        std::vector<double> res;
        for (size_t c0 = 0; c0 < x.size(); c0 += 256) {
            const int count = (int)std::min<size_t>(256, x.size() - c0);
            res.push_back(chunk_sum(count, [&](int i) { return x[c0 + i]; }));
        }
        x = res;
        if (x.size() == 1) return x[0];
    }
}
// a plan's index ranges, then the descriptors walked over `value` (per INTERNAL cell) -> per region its sum (0.0 for a missing id)
static bool walk(const FipPlan& P, int Nb, const std::vector<double>& value, std::vector<double>& out) {
    CHECK((int)P.items.size() == P.ncells && (int)P.desc.size() == 3 * P.npart && (int)P.result.size() == P.max_id, "sizes");
    CHECK(!P.level_ptr.empty() && P.level_ptr[0] == 0 && P.level_ptr.back() == P.npart, "level_ptr");
    for (int it : P.items) CHECK(it >= 0 && it < Nb, "item %d", it);
    std::vector<double> part(P.npart, 0.0);
    std::vector<char> written(P.npart, 0);
    for (int level = 0; level < P.levels(); ++level) {
        CHECK(P.chunks(level) > 0, "an empty level %d", level);
        for (int ch = P.level_ptr[level]; ch < P.level_ptr[level + 1]; ++ch) {
            const int first = P.desc[3 * ch], count = P.desc[3 * ch + 1], dest = P.desc[3 * ch + 2];
            CHECK(count >= 1 && count <= FIP_CHUNK && first >= 0, "chunk %d: first %d count %d", ch, first, count);
            CHECK(dest >= 0 && dest < P.npart && !written[dest], "chunk %d: destination %d", ch, dest);
            if (level == 0) {
                CHECK(first + count <= P.ncells, "chunk %d reads items %d .. %d of %d", ch, first, first + count, P.ncells);
                part[dest] = chunk_sum(count, [&](int i) { return value[P.items[first + i]]; });
            } else {
                for (int i = 0; i < count; ++i)
                    CHECK(first + i < P.level_ptr[level] && first + i >= P.level_ptr[level - 1] && written[first + i], "chunk %d reads slot %d", ch, first + i);
                part[dest] = chunk_sum(count, [&](int i) { return part[first + i]; });
            }
        }
        for (int ch = P.level_ptr[level]; ch < P.level_ptr[level + 1]; ++ch) written[P.desc[3 * ch + 2]] = 1;
    }
    out.assign(P.max_id, 0.0);
    for (int r = 0; r < P.max_id; ++r) {
        CHECK(P.result[r] >= -1 && P.result[r] < P.npart, "result %d", P.result[r]);
        if (P.result[r] >= 0) out[r] = part[P.result[r]];
    }
    return true;
}

static const int LENGTHS[] = {1, 63, 64, 65, 255, 256, 257, 511, 513, 65537};

// region 2 holds n cells, scattered between cells of region 1, of no region (0, -4) and in front of an unused id 3 and a region 4 of one cell
static bool one_length(int n) {
    const int Nb = 2 * n + 7;
    std::vector<int> region(Nb), to(Nb);
    int left = n;
    for (int i = 0; i < Nb; ++i) {
        if (i % 2 == 1 && left > 0) { region[i] = 2; --left; }
        else region[i] = (i % 6 == 0) ? 0 : (i % 6 == 2) ? -4 : 1;
    }
    region[Nb - 1] = 4;
    CHECK(left == 0, "n = %d", n);
    for (int i = 0; i < Nb; ++i) to[i] = (int)(((long long)i * 7919 + 13) % Nb);   // a permutation: Nb is odd and no multiple of 7919
    {
        std::vector<char> seen(Nb, 0);
        for (int t : to) { CHECK(t >= 0 && t < Nb && !seen[t], "not a permutation"); seen[t] = 1; }
    }
    std::vector<double> nat(Nb), internal(Nb);
    for (int i = 0; i < Nb; ++i) {
        nat[i] = std::ldexp((double)((i * 2654435761u) % 1000003u) - 5e5, (i % 40) - 20);   // magnitudes apart: another order, other bits
        internal[to[i]] = nat[i];
    }
    const int* sets[1] = {region.data()};
    std::vector<int> max_id;
    std::string msg;
    CHECK(fip_regions_check(1, sets, Nb, 1, 0, max_id, msg) == OPMHIP_SUCCESS && max_id.size() == 1 && max_id[0] == 4, "%s", msg.c_str());
    FipPlan P;
    fip_plan(Nb, to.data(), region.data(), max_id[0], P);
    int in_regions = 0;
    for (int r : region) in_regions += r >= 1;
    CHECK(P.max_id == 4 && P.ncells == in_regions, "cells %d of %d", P.ncells, in_regions);
    std::vector<double> got;
    if (!walk(P, Nb, internal, got)) return false;
    int levels = 0;   // of the longest list: m -> ceil(m / 256) -> ... -> 1
    for (int r = 1; r <= 4; ++r) {
        std::vector<double> x;
        for (int i = 0; i < Nb; ++i)
            if (region[i] == r) x.push_back(nat[i]);
        if (x.empty()) {
            CHECK(r == 3 && P.result[r - 1] == -1 && got[r - 1] == 0.0, "unused id %d", r);
            continue;
        }
        const double want = reduce256(x);
        CHECK(got[r - 1] == want, "n = %d region %d: %.17g, not %.17g", n, r, got[r - 1], want);
        int lv = 0;
        for (size_t m = x.size();;) { ++lv; m = (m + 255) / 256; if (m == 1) break; }
        levels = std::max(levels, lv);
    }
    CHECK(P.levels() == levels, "n = %d: %d levels, not %d", n, P.levels(), levels);
    if (n == 65537) CHECK(P.levels() == 3, "65 537 items need three levels, not %d", P.levels());
    return true;
}

static bool lengths() {
    for (int n : LENGTHS)
        if (!one_length(n)) return false;
    return true;
}

static bool empty_plans() {
    // no cell in any region; no cells at all
    std::vector<int> region{0, -1, 0}, to{2, 0, 1};
    FipPlan P;
    fip_plan(3, to.data(), region.data(), 0, P);
    CHECK(P.max_id == 0 && P.ncells == 0 && P.npart == 0 && P.levels() == 0 && P.result.empty() && P.desc.empty(), "no regions");
    fip_plan(0, nullptr, nullptr, 0, P);
    CHECK(P.max_id == 0 && P.ncells == 0 && P.levels() == 0, "no cells");
    // every cell its own region: one level of single-item chunks
    std::vector<int> own{3, 1, 2};
    fip_plan(3, to.data(), own.data(), 3, P);
    CHECK(P.levels() == 1 && P.npart == 3 && P.items == (std::vector<int>{0, 1, 2}), "own regions");
    std::vector<double> got;
    if (!walk(P, 3, {10.0, 20.0, 30.0}, got)) return false;   // internal values: cell 0 -> position 2, cell 1 -> 0, cell 2 -> 1
    CHECK(got == (std::vector<double>{10.0, 20.0, 30.0}), "own regions' sums");
    return true;
}

static bool refusals() {
    std::vector<int> a{1, 2, 0, 5}, b{1, 1, 1, 1}, big{1, 2, 3, 4};
    std::vector<int> max_id{77};
    std::string msg;
    const int* two[2] = {a.data(), b.data()};
    auto refused = [&](int rc, const char* word) {
        const bool ok = rc == OPMHIP_INVALID_ARGUMENT && msg.find(word) != std::string::npos && msg.find("set_fip_regions") == 0 && max_id == std::vector<int>{77};
        msg.clear();
        return ok;
    };
    CHECK(refused(fip_regions_check(-1, two, 4, 1, 0, max_id, msg), "num_sets = -1"), "negative count");
    CHECK(refused(fip_regions_check(OPMHIP_FIP_MAX_SETS + 1, two, 4, 1, 0, max_id, msg), "num_sets = 17"), "17 sets");
    CHECK(refused(fip_regions_check(2, nullptr, 4, 1, 0, max_id, msg), "region == NULL"), "null list");
    const int* hole[2] = {a.data(), nullptr};
    CHECK(refused(fip_regions_check(2, hole, 4, 1, 0, max_id, msg), "region[1] == NULL"), "null array");
    CHECK(refused(fip_regions_check(2, two, 4, 1, 0, max_id, msg), "the id 5, above the 4 cells"), "id above Nb");
    CHECK(refused(fip_regions_check(2, two, 4, 2, 0, max_id, msg), "decomposed"), "ranks");
    CHECK(refused(fip_regions_check(2, two, 4, 1, 3, max_id, msg), "decomposed"), "ghosts");
    // accepted: the largest id equal to Nb, 16 sets, none
    const int* ok1[1] = {big.data()};
    CHECK(fip_regions_check(1, ok1, 4, 1, 0, max_id, msg) == OPMHIP_SUCCESS && max_id == std::vector<int>{4}, "id == Nb");
    std::vector<const int*> many(OPMHIP_FIP_MAX_SETS, b.data());
    CHECK(fip_regions_check(OPMHIP_FIP_MAX_SETS, many.data(), 4, 1, 0, max_id, msg) == OPMHIP_SUCCESS && (int)max_id.size() == OPMHIP_FIP_MAX_SETS, "16 sets");
    CHECK(fip_regions_check(0, nullptr, 4, 1, 0, max_id, msg) == OPMHIP_SUCCESS && max_id.empty() && msg.empty(), "no sets");
    // the calls
    CHECK(fip_call_check("fluid_in_place", false, 2, 0, msg) == OPMHIP_NOT_READY && msg == "fluid_in_place before set_state", "%s", msg.c_str());
    CHECK(fip_call_check("fluid_in_place", true, 0, 0, msg) == OPMHIP_NOT_READY && msg == "fluid_in_place before set_fip_regions", "%s", msg.c_str());
    CHECK(fip_call_check("fluid_in_place", true, 2, 2, msg) == OPMHIP_INVALID_ARGUMENT && msg == "fluid_in_place: set 2 of 2", "%s", msg.c_str());
    CHECK(fip_call_check("fluid_in_place", true, 2, -1, msg) == OPMHIP_INVALID_ARGUMENT && msg == "fluid_in_place: set -1 of 2", "%s", msg.c_str());
    CHECK(fip_call_check("fluid_in_place", true, 2, 1, msg) == OPMHIP_SUCCESS, "a set in range");
    return true;
}

static bool pressures() {
    CHECK(fip_pressure_average(12.0, 4.0, 10.0, 5.0, true) == 3.0 && fip_pressure_average(12.0, 4.0, 10.0, 5.0, false) == 2.0, "both weights");
    CHECK(fip_pressure_average(12.0, 1e-10, 10.0, 5.0, true) == 2.0, "HydroCarbonPV = 1e-10 is not > 1e-10");
    CHECK(fip_pressure_average(12.0, 1.0000001e-10, 10.0, 5.0, true) == 12.0 / 1.0000001e-10, "just above");
    CHECK(std::isnan(fip_pressure_average(0.0, 0.0, 0.0, 0.0, true)) && std::isnan(fip_pressure_average(0.0, 0.0, 0.0, 0.0, false)), "0.0 / 0.0");
    return true;
}

int main() {
    report(lengths(), "plans: 1, 63, 64, 65, 255, 256, 257, 511, 513 and 65 537 cells in a region");
    report(empty_plans(), "plans: no regions, no cells, every cell its own region");
    report(refusals(), "refused: count, null arrays, id above Nb, ranks, ghosts; accepted: id == Nb, 16 sets, none; the calls' checks");
    report(pressures(), "pressure averages: both weights, the 1e-10 threshold, no pore volume");
    if (g_fail == 0) std::printf("all checks passed\n");
    return g_fail == 0 ? 0 : 1;
}
