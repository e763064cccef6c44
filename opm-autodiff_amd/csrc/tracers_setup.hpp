// Host set-up of the passive tracers (opmhip_set_tracers, opmhip_set_tracer_solver, opmhip_set_tracer_connections): every check of what
// the caller hands over, the phase batches, the level sets of the ordering's lower triangle, the rows' faces in natural column order, the
// connections grouped by distinct cell.  Pure host work on its arguments, no context and no HIP call, so that it is built and checked
// without a device (tests/san/tracers_san.cpp).  capi_tracers.cpp allocates, uploads and launches.
// A refusal is a code other than OPMHIP_SUCCESS with its text in `msg`, for the caller's fail(); the outputs are then untouched.
#pragma once
#include <string>
#include <vector>

#include "../../include/opmhip.h"

namespace opmhip {

// prepareTracerBatches (ebos/ecltracermodel.hh:441-479): per phase (0 water, 1 oil, 2 gas) its tracers in the caller's order
struct TracerBatches {
    std::vector<int> phase, slot;      // per tracer: its phase, its place in the phase's batch
    std::vector<int> members[3];       // per phase: the tracers' numbers in the caller's list
};
// has_pvtg: the context's fluid has PVTG; nranks / nghost: the context's ranks and ghost cells
int tracer_batches(int num_tracers, const int* phase, const double* concentration, int Nb, bool has_pvtg, int nranks, int nghost, TracerBatches& out,
                   std::string& msg);
int tracer_solver_check(double tolerance, int maxit, std::string& msg);

// Level sets of the lower triangle of a structurally symmetric CSR pattern (columns ascending in every row): level(i) = 1 + the largest
// level among the columns j < i of row i, 0 without any.  rows: the rows level by level, ascending inside a level; ptr[l] .. ptr[l + 1]
// the rows of level l.  The rows of one level do not depend on each other in the forward sweep and the factorisation; the levels in
// DESCENDING order are a schedule of the backward sweep (a column j > i of row i has i in its own lower part, so level(j) > level(i)).
struct TracerLevels {
    std::vector<int> ptr, rows;
};
void tracer_levels(int Nb, const int* rowptr, const int* col, TracerLevels& out);

// ford[rowptr[p] .. rowptr[p + 1]): the entries of row p (diagonal included) by ascending natural entry number nnzMap[k] - ascending
// natural column, the order in which k_assemble sums a row's faces
void tracer_face_order(int Nb, const int* rowptr, const int* nnzMap, std::vector<int>& ford);

// opmhip_set_tracer_connections: n != 0.  group_by_cell (source_lists.hpp) of the connections
struct TracerConnLists {
    std::vector<int> pos, cpos, cptr, cconn;
};
int tracer_connections(int n, const int* cell, const double* rate, const double* injected, int num_tracers, int Nb, const int* toOrder,
                       TracerConnLists& out, std::string& msg);

}  // namespace opmhip
