// Host set-up of the VFP tables (opmhip_set_vfp_tables) and of the THP limits of the resident standard wells (opmhip_set_std_wells_thp):
// every check of what the caller hands over and the packing of the arrays the kernels read.  Pure host work on its arguments, no context
// and no HIP call, so that it is built and checked without a device (tests/san/vfp_tables_san.cpp).  capi_std_wells.cpp allocates, uploads and
// launches.  A refusal is a code other than OPMHIP_SUCCESS with its text in `msg`, for the caller's fail(); the outputs are then untouched.
#pragma once
#include <string>
#include <vector>

#include "../../include/opmhip.h"

namespace opmhip {

// The descriptor of one table, VFP_DESC ints: kind, deck number, the three types, the five axis sizes (flo, thp, wfr, gfr, alq; an
// injector's last three are 1), where the five axes and the values begin in the double array (an injector's last three axes: -1).
// The values keep the caller's layout, flo fastest: [thp][wfr][gfr][alq][flo] / [thp][flo].
enum { VFP_KIND = 0, VFP_NUM, VFP_FLO_TYPE, VFP_WFR_TYPE, VFP_GFR_TYPE, VFP_N, VFP_AXIS = VFP_N + 5, VFP_VALUES = VFP_AXIS + 5, VFP_DESC };

struct VfpPacked {
    int num = 0;
    std::vector<int> desc;        // num * VFP_DESC
    std::vector<double> dbl;      // every table's axes, then its values
    std::vector<double> datum;    // per table: datum depth (the host's: the wells hand in dh)
};
// t->num_tables != 0
int vfp_pack(const opmhip_vfp_tables* t, VfpPacked& out, std::string& msg);
// the table of that kind and deck number, or -1
int vfp_find(const VfpPacked& P, int kind, int table_num);

// opmhip_set_std_wells_thp for a list of nw wells (wi: per well producer, injected phase, rate component).  table: per well the index into
// P (-1: no limit); wd: per well limit, alq, dh; any: some well has a limit
int std_wells_thp_lists(const opmhip_std_wells_thp* thp, size_t nw, const int* wi, const VfpPacked& P, std::vector<int>& table, std::vector<double>& wd, bool& any,
                        std::string& msg);
// the controls of opmhip_set_std_wells_state with THP limits in force: 0, 1, or 2 for a well that has a limit (table: as above, NULL: none has)
int std_wells_thp_check_controls(size_t nw, const int* control, const int* table, std::string& msg);

}  // namespace opmhip
