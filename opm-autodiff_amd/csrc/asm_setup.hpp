// Host set-up of the assembly (opmhip_set_static, opmhip_set_water_compaction, opmhip_set_endpoint_scaling, opmhip_set_hysteresis,
// opmhip_set_source_cells): the checks of what the caller hands over, the tiles, the launch schedule and the per-lane entry words of
// k_assemble, the packed tables and lists the kernels read.  Pure host work on its arguments, no context and no HIP call, so that it is
// built and checked without a device (tests/san/asm_setup_san.cpp).  capi_asm.cpp allocates, uploads and launches.
// A refusal is a code other than OPMHIP_SUCCESS with its text in `msg`, for the caller's fail(); the outputs are then untouched.
#pragma once
#include <string>
#include <vector>

#include "../../include/opmhip.h"

namespace opmhip {

struct Pattern;   // internal.hpp

// opmhip_set_static's arrays (natural order; thpres / pvtnum / satnum may be NULL): the per-connection data are symmetric - entry (I,J)
// and (J,I) describe the same face; a ghost column's row lives on the neighbouring subdomain and maps to itself -, then every cell's
// volume, porosity and region numbers
int asm_static_check(const Pattern& P, int num_pvt, int num_sat, const double* trans, const double* area, const double* thpres, const double* poro,
                     const double* volume, const int* pvtnum, const int* satnum, std::string& msg);

// What k_assemble is launched by.  row0 [ntiles + 1]: the tiles, whole rows, at most `threads` entries and `max_rows` rows each.
// sched [4 * nsched]: one record per workgroup (first row, end row, first entry, end entry), nsched = 8 * chunk, the last may be empty
// (all zero).  desc [2 * threads * nsched]: per workgroup and lane the column and the entry word (asm_setup.cpp).  split_ok: every
// entry word carries its block's place in the tile's run of the rest or the U stream.
struct AsmPlan {
    std::vector<int> row0, sched, desc;
    int ntiles = 0, nsched = 0;
    bool split_ok = false;
};
int asm_plan(const Pattern& P, int threads, int max_rows, AsmPlan& out, std::string& msg);   // OPMHIP_ANALYSIS_FAILED: a row longer than a tile

// opmhip_set_water_compaction's tables.  desc: per table {np, nsw, pressure at, S_w at, pore-volume multipliers at, transmissibility
// multipliers at | -1}, the places counted in `data`
struct WaterCompactionTables {
    std::vector<int> desc;
    std::vector<double> data;
};
int water_compaction_tables(int num_tables, const int* num_pressure, const int* num_sw, const double* pressure, const double* sw, const double* pv_mult,
                            const double* trans_mult, WaterCompactionTables& out, std::string& msg);

// packed EclEpsConfig (assemble.hip CellStatic::epscfg); krw / kro / krg inside 0 .. 2
inline int eps_config(const opmhip_endpoint_scaling& e) {
    return (e.sat_scaling ? 1 : 0) | (e.three_point_kr ? 2 : 0) | (e.krw << 2) | (e.kro << 4) | (e.krg << 6) | (e.pcw ? 256 : 0) | (e.pcg ? 512 : 0);
}
// One cell's scaled end points.  Field f is src[f][at], or the region's own table value where src or src[f] is NULL; the points must be
// finite and pass end_points_refusal against the region's under the options of cfg (eps_config); they go to v[f * N + pos] (field-major,
// internal order) unless v is NULL.  call / kind: "set_hysteresis", "imbibition " - who refuses, and which curves; cell: its natural id
struct EndPointsCheck {
    const char *call, *kind;
    const double* const* src;
    const double* sat_eps;   // EPS_COUNT per saturation region
    int cfg;
    double* v;
    size_t N;
};
int cell_end_points(const EndPointsCheck& K, size_t at, int cell, int region, size_t pos, std::string& msg);

// opmhip_set_source_cells' list: the distinct cells (internal positions) in the order of first mention, each with the sum of what was
// named for it, in item order (two wells may perforate one cell).  val [distinct][3], dval [distinct][9] (zeros where dsource is NULL)
struct SourceCells {
    std::vector<int> pos;
    std::vector<double> val, dval;
};
int source_cells(int n, const int* cells, const double* source, const double* dsource, int Nloc, const int* toOrder, SourceCells& out, std::string& msg);

}  // namespace opmhip
