// Host set-up of the fluid-in-place report: see fip_setup.hpp.  No HIP call, no context.
#include "fip_setup.hpp"

#include <algorithm>
#include <cstdio>

namespace opmhip {

namespace {

std::string text(const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
    char buf[256];
    std::snprintf(buf, sizeof buf, fmt, a, b, c);
    return buf;
}

}  // namespace

int fip_regions_check(int num_sets, const int* const* region, int Nb, int nranks, int nghost, std::vector<int>& max_id, std::string& msg) {
    if (num_sets < 0 || num_sets > OPMHIP_FIP_MAX_SETS) {
        msg = text("set_fip_regions: num_sets = %lld, not in 0 .. %lld", num_sets, OPMHIP_FIP_MAX_SETS);
        return OPMHIP_INVALID_ARGUMENT;
    }
    if (nranks > 1 || nghost > 0) {
        msg = "set_fip_regions: a decomposed context (the sums over the ranks are not formed)";
        return OPMHIP_INVALID_ARGUMENT;
    }
    if (num_sets > 0 && !region) {
        msg = "set_fip_regions: region == NULL";
        return OPMHIP_INVALID_ARGUMENT;
    }
    for (int s = 0; s < num_sets; ++s)
        if (!region[s]) {
            msg = text("set_fip_regions: region[%lld] == NULL", s);
            return OPMHIP_INVALID_ARGUMENT;
        }
    std::vector<int> mx(num_sets, 0);
    for (int s = 0; s < num_sets; ++s) {
        for (int i = 0; i < Nb; ++i) mx[s] = std::max(mx[s], region[s][i]);
        // regionMax is the length of every array the report carries: an id beyond the cell count can only be a damaged array
        if (mx[s] > Nb) {
            msg = text("set_fip_regions: set %lld has the id %lld, above the %lld cells", s, mx[s], Nb);
            return OPMHIP_INVALID_ARGUMENT;
        }
    }
    max_id = mx;
    return OPMHIP_SUCCESS;
}

void fip_plan(int Nb, const int* toOrder, const int* region, int max_id, FipPlan& out) {
    FipPlan P;
    P.max_id = max_id;
    // counting sort by id, stable over the natural cell index; ids <= 0 belong to no region (regionSum, :724-727)
    std::vector<int> start(max_id + 1, 0);
    for (int i = 0; i < Nb; ++i)
        if (region[i] >= 1) ++start[region[i]];
    std::vector<int> first(max_id, 0), count(max_id, 0);
    int n = 0;
    for (int r = 1; r <= max_id; ++r) {
        first[r - 1] = n;
        count[r - 1] = start[r];
        start[r] = n;
        n += count[r - 1];
    }
    P.ncells = n;
    P.items.resize(n);
    for (int i = 0; i < Nb; ++i)
        if (region[i] >= 1) P.items[start[region[i]]++] = toOrder[i];
    // level 0 over the lists, then over the chunk results for as long as some region has more than one; a chunk's destination is its
    // own number, so that a region's results of one level lie side by side for the next
    P.level_ptr.push_back(0);
    int nchunks = 0;
    for (int level = 0;; ++level) {
        bool any = false;
        for (int r = 0; r < max_id; ++r) {
            if (level == 0 ? count[r] < 1 : count[r] < 2) continue;
            any = true;
            const int nch = (count[r] + FIP_CHUNK - 1) / FIP_CHUNK, f0 = first[r], cnt = count[r];
            first[r] = nchunks;
            for (int j = 0; j < nch; ++j) {
                P.desc.push_back(f0 + j * FIP_CHUNK);
                P.desc.push_back(std::min(FIP_CHUNK, cnt - j * FIP_CHUNK));
                P.desc.push_back(nchunks++);
            }
            count[r] = nch;
        }
        if (!any) break;
        P.level_ptr.push_back(nchunks);
    }
    P.npart = nchunks;
    P.result.assign(max_id, -1);
    for (int r = 0; r < max_id; ++r)
        if (count[r] == 1) P.result[r] = first[r];
    out = std::move(P);
}

double fip_pressure_average(double pressurePvHydrocarbon, double pvHydrocarbon, double pressurePv, double pv, bool hydrocarbon) {
    if (hydrocarbon && (pvHydrocarbon > 1e-10))
        return pressurePvHydrocarbon / pvHydrocarbon;

    return pressurePv / pv;
}

int fip_call_check(const char* who, bool state_set, int num_sets, int set, std::string& msg) {
    if (!state_set) {
        msg = std::string(who) + " before set_state";
        return OPMHIP_NOT_READY;
    }
    if (num_sets == 0) {
        msg = std::string(who) + " before set_fip_regions";
        return OPMHIP_NOT_READY;
    }
    if (set < 0 || set >= num_sets) {
        msg = std::string(who) + text(": set %lld of %lld", set, num_sets);
        return OPMHIP_INVALID_ARGUMENT;
    }
    return OPMHIP_SUCCESS;
}

}  // namespace opmhip
