// Host set-up of the two resident source lists - standard wells (opmhip_set_std_wells and its setters) and analytic aquifers
// (opmhip_set_aquifers, opmhip_aquifers_begin_time_step, opmhip_get_aquifers): every check of what the caller hands over, the packing
// of the arrays the kernels read, the grouping by distinct cell.  Pure host work on its arguments, no context and no HIP call, so that
// it is built and checked without a device (tests/san/source_lists_san.cpp).  capi_std_wells.cpp (wells) and capi_aquifers.cpp (aquifers) allocate, upload and launch.
// A refusal is a code other than OPMHIP_SUCCESS with its text in `msg`, for the caller's fail(); the outputs are then untouched.
#pragma once
#include <string>
#include <vector>

#include "../../include/opmhip.h"

namespace opmhip {

// Items (perforations, connections) by distinct cell.  cell: the natural cell of every item, each inside [0, Nb).  pos: the cell's
// internal position per item; cpos: the distinct cells' positions in the order of first mention; the items of distinct cell t are
// items[cptr[t] .. cptr[t + 1]), in ascending item number.
void group_by_cell(const int* cell, int n, int Nb, const int* toOrder, std::vector<int>& pos, std::vector<int>& cpos, std::vector<int>& cptr,
                   std::vector<int>& items);

// ---- standard wells ----
struct StdWellsLists {
    std::vector<int> pos, cpos, cptr, cperf;   // group_by_cell of the perforations
    std::vector<int> wi;                       // per well: producer, injected phase, rate component
    std::vector<double> wd, pack;              // per well: rate target, bhp limit; StdWellsDev's d_pack
};
int std_wells_lists(const opmhip_std_wells* sw, int Nb, const int* toOrder, StdWellsLists& out, std::string& msg);   // sw->num_wells != 0
int std_wells_check_state(size_t nw, const double* x, const int* control, const double* rate_target, std::string& msg);
// wi: the list's; any: some well has the switch
int std_wells_check_crossflow(size_t nw, const int* allow, const int* wi, bool& any, std::string& msg);
// opmhip_set_std_wells_vaporised_oil.  has_pvtg: the context's fluid has PVTG, so that its records hold Rv
int std_wells_check_vaporised_oil(int on, bool has_pvtg, std::string& msg);
// opmhip_set_std_wells_limits.  wi: the list's; control: the controls in force (nw); lim: per well oil, water, gas, liquid, resv (+infinity:
// none); use: per well use_list_target; any / any_resv: some well has a limit (or use_list_target = 0) / a RESV limit
struct StdWellsLimitsLists {
    std::vector<double> lim;
    std::vector<int> use;
    bool any = false, any_resv = false;
};
int std_wells_limits(const opmhip_std_wells_limits* L, size_t nw, const int* wi, const int* control, StdWellsLimitsLists& out, std::string& msg);
// the controls opmhip_set_std_wells_state hands in, with limits in force: 0 .. 7, 2 only with a THP limit (thp_table NULL: none has one), 3 .. 7
// only with that limit, 0 only with use_list_target
int std_wells_limits_check_controls(size_t nw, const int* control, const int* thp_table, const double* lim, const int* use, std::string& msg);
// opmhip_set_std_wells_groups.  wi: the list's; control: the controls in force (nw).  ptr / idx: per group its PRODUCERS, wells ascending
// (an injector may name a group and is ignored by it); of / available: per well; guide: 5 per well; target: 5 per group (+infinity: none);
// mode: per group 0 .. 5; resv: per well, a producer in a group with a RESV target; any: groups are in force; any_resv: some group has a
// RESV target
struct StdWellsGroupsLists {
    int num_groups = 0, nupcol = 0;
    std::vector<int> ptr, idx, of, available, mode, resv;
    std::vector<double> guide, target;
    bool any = false, any_resv = false;
};
int std_wells_groups(const opmhip_std_wells_groups* G, size_t nw, const int* wi, const int* control, StdWellsGroupsLists& out, std::string& msg);
// opmhip_set_std_wells_guide_rates: 5 per well, >= 0 and finite
int std_wells_groups_check_guide_rates(size_t nw, const double* guide_rate, std::string& msg);
// opmhip_set_std_wells_group_targets on the values in force (cur): a NULL array leaves that kind, a NULL mode the modes; out: the new
// target [5 per group], mode, resv and any_resv (the other fields as cur's)
int std_wells_group_targets(const StdWellsGroupsLists& cur, size_t nw, const double* const arr[5], const int* mode, StdWellsGroupsLists& out, std::string& msg);
// the control values 8 opmhip_set_std_wells_state hands in (every other value is the other checks'): an available producer in a group;
// of NULL: no groups in force
int std_wells_groups_check_controls(size_t nw, const int* control, const int* wi, const int* of, const int* available, std::string& msg);
// pref: per well the preferred phase the kernel reads (an injector's is never looked at: oil)
int std_wells_head_model(const opmhip_std_wells_wellbore* wb, size_t nw, size_t np, const int* wi, std::vector<int>& pref, std::string& msg);
// state_set: the perforation pressures exist already
int std_wells_check_perf_state(size_t np, const double* perf_pressure, const double* perf_rates, bool state_set, std::string& msg);

// opmhip_set_std_wells_matrix_add: the schedule of A -= C^T D^-1 B for the list (StandardWell::addWellContributions,
// wells/StandardWell_impl.hpp:1688-1712, on ISTLSolverEbos' clique pattern).  perf_pointers / pos: the list's ranges and the internal
// positions of its perforated cells; fromOrder: internal -> natural (for the text of a refusal); rowptr / col: the device's block-CSR,
// columns ascending.  target[t]: the position of the t-th distinct block some pair (a, b) of one well writes, ascending; its
// contributions are contrib[3 k .. 3 k + 3) = (well, a, b), k in [tptr[t], tptr[t + 1]), a and b counted inside the well, ordered by well
// and then by a * np + b: the order in which opmhip_add_well_contributions adds them.  pairs = tptr.back().
struct StdWellsMatrixAdd {
    std::vector<int> target, tptr, contrib;
    int pairs = 0;
};
int std_wells_matrix_add_check(int on, std::string& msg);
int std_wells_matrix_add_schedule(int nw, const int* perf_pointers, const int* pos, const int* fromOrder, const int* rowptr, const int* col,
                                  StdWellsMatrixAdd& out, std::string& msg);

// ---- analytic aquifers ----
struct AquiferLists {
    int nc = 0;                                // connections
    std::vector<double> par, td, pd;           // AQ_PAR per aquifer; the Carter-Tracy influence tables, concatenated
    std::vector<int> tabptr, need_eq;          // ranges into td / pd; the aquifers without an initial pressure
    std::vector<int> of, pos, cpos, cptr, cconn;   // per connection its aquifer; group_by_cell of the connections
};
int aquifer_lists(const opmhip_aquifers* aq, int Nb, const int* toOrder, AquiferLists& out, std::string& msg);   // aq->num_aquifers != 0
// calculateReservoirEquilibrium (AquiferInterface.hpp:330-373) of one aquifer: its n connections are alpha[i0 .. i0 + n); order: they by
// ascending cell (the element loop); rec: the intensive-quantity records (IQS doubles each) and p the positions of the cells in that order
double aquifer_equilibrium_pressure(const double* alpha, int i0, int n, const int* order, const double* rec, int IQS, const double* depth, const int* p,
                                    double datum);
void aquifer_initial_state(const opmhip_aquifers* aq, const std::vector<double>& par, std::vector<double>& state);
// opm-common's linearInterpolation / linearInterpolationDerivative (not in the reference tree: restated, UNVERIFIED): the interval
// j with x[j] <= xv, the first / last interval outside the table (linear extrapolation); value = slope * (xv - x[j]) + y[j]
int table_interval(const double* x, int n, double xv);
double table_slope(const double* x, const double* y, int n, double xv);
double table_value(const double* x, const double* y, int n, double xv);
// the AQ_STEP scalars of every aquifer for the time step [time, time + dt]
void aquifer_step_scalars(int num, const std::vector<double>& par, const std::vector<int>& tabptr, const std::vector<double>& td, const std::vector<double>& pd,
                          double time, double dt, double* step);
// opmhip_get_aquifers' outputs (each may be NULL) from the state and, for flux_rate, the connections' q4 read back
void aquifer_report(int num, const std::vector<double>& par, const std::vector<int>& ptr, const double* state, const double* q4, double* W_flux,
                    double* pressure, double* flux_rate, double* init_pressure);

}  // namespace opmhip
