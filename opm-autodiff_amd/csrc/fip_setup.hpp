// Host set-up of the fluid-in-place report (opmhip_set_fip_regions, opmhip_fluid_in_place): the checks of what the caller hands over, the
// region lists, the chunk descriptors of every level of the reduction and the pressure averages.  Pure host work on its arguments, no
// context and no HIP call, so that it is built and checked without a device (tests/san/fip_setup_san.cpp).  capi_fip.cpp allocates,
// uploads and launches.
// A refusal is a code other than OPMHIP_SUCCESS with its text in `msg`, for the caller's fail(); the outputs are then untouched.
//
// The stated order of a region's sums, `reduce256` (fip.py restates it in NumPy; DESIGN.md "fluids in place"):
//   1. the region's list - its cells by ascending natural index - is cut into chunks of FIP_CHUNK = 256 consecutive items; the last
//      chunk may be ragged, a missing item counts as 0.0;
//   2. in a chunk, lane l of one wavefront forms (((0.0 + x[l]) + x[l + 64]) + x[l + 128]) + x[l + 192];
//   3. the 64 lanes are combined by the shuffle-down tree v[l] += v[l + o], o = 32, 16, ..., 1;
//   4. the chunk results of a region, in ascending order, are a new list: the same rule again, until one value is left.
// The order depends on the region array and the natural cell numbering alone - not on the ordering of the context, the grid of a
// launch or the call.
#pragma once
#include <string>
#include <vector>

#include "../../include/opmhip.h"

namespace opmhip {

constexpr int FIP_CHUNK = 256;   // items of a chunk: four per lane of a wavefront

// opmhip_set_fip_regions' arguments (num_sets != 0 is not asked: 0 releases).  max_id[s]: the largest id of set s, 0 where no cell has an id >= 1
int fip_regions_check(int num_sets, const int* const* region, int Nb, int nranks, int nghost, std::vector<int>& max_id, std::string& msg);

// One region set's plan.  items: the cells with an id >= 1 by (region id, natural cell index), as INTERNAL cell ids (toOrder).
// A level is one launch: chunks [level_ptr[v], level_ptr[v + 1]) of desc, three ints each - first item, count, destination.  Level 0 reads
// `items` (first / count index that list), every later level the partial sums (first / count index the slots the level before wrote);
// a destination is a slot of the partial sums, npart in all.  result[r - 1]: the slot that holds region r's sums after the last level, or
// -1 for an id no cell carries (zeros).
struct FipPlan {
    int max_id = 0, ncells = 0, npart = 0;
    std::vector<int> items, desc, level_ptr, result;
    int levels() const { return (int)level_ptr.size() - 1; }
    int chunks(int level) const { return level_ptr[level + 1] - level_ptr[level]; }
};
void fip_plan(int Nb, const int* toOrder, const int* region, int max_id, FipPlan& out);

// pressureAverage_ (ebos/eclgenericoutputblackoilmodule.cc:1240-1250), literally; a region without pore volume gives its 0.0 / 0.0
double fip_pressure_average(double pressurePvHydrocarbon, double pvHydrocarbon, double pressurePv, double pv, bool hydrocarbon);

// opmhip_fluid_in_place's `set` argument and its state: OPMHIP_NOT_READY / OPMHIP_INVALID_ARGUMENT with the text, or OPMHIP_SUCCESS
int fip_call_check(const char* who, bool state_set, int num_sets, int set, std::string& msg);

}  // namespace opmhip
