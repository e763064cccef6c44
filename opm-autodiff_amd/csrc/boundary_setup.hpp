// Host set-up of the open boundaries (opmhip_set_boundary_conditions): every check of what the caller hands over, the packing of the
// arrays the kernels read, the grouping of the faces by distinct cell and the exterior records' slots.  Pure host work on its
// arguments, no context and no HIP call, so that it is built and checked without a device (tests/san/boundary_setup_san.cpp).
// capi_boundary.cpp allocates, uploads and launches.
// A refusal is a code other than OPMHIP_SUCCESS with its text in `msg`, for the caller's fail(); the outputs are then untouched.
#pragma once
#include <string>
#include <vector>

#include "../../include/opmhip.h"

namespace opmhip {

// what of the context decides a refusal
struct BoundaryContext {
    int Nb = 0, nranks = 1;
    bool hysteresis = false, water_compaction = false;
};
struct BoundaryLists {
    int nf = 0;                                // faces
    std::vector<int> type;                     // per face
    std::vector<double> geo, rate;             // per face: area, transmissibility, face depth; the three rates (0 for a FREE face)
    std::vector<int> pos, cpos, cptr, cconn;   // group_by_cell (source_lists.hpp) of the faces
    std::vector<int> slot, fcell;              // per distinct cell: its exterior record or -1; per record: its distinct cell
};
int boundary_lists(const opmhip_boundary_conditions* bc, const BoundaryContext& ctx, const int* toOrder, BoundaryLists& out, std::string& msg);   // bc->num_faces != 0

}  // namespace opmhip
