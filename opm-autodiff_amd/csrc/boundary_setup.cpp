// Host set-up of the open boundaries (boundary_setup.hpp).  No HIP call: capi_boundary.cpp uploads what is built here.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <utility>

#include "boundary_setup.hpp"
#include "source_lists.hpp"

namespace opmhip {

namespace {
// the text as fail() will cut it
int refuse(std::string& msg, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return OPMHIP_INVALID_ARGUMENT;
}
}  // namespace

int boundary_lists(const opmhip_boundary_conditions* bc, const BoundaryContext& ctx, const int* toOrder, BoundaryLists& out, std::string& msg) {
    const int nf = bc->num_faces;
    if (nf < 0) return refuse(msg, "set_boundary_conditions: num_faces = %d", nf);
    if (ctx.nranks > 1) return refuse(msg, "set_boundary_conditions: decomposed context (%d ranks) - the faces of a subdomain's owned cells are not told from its ghosts', which is not built", ctx.nranks);
    if (ctx.water_compaction)
        return refuse(msg, "set_boundary_conditions: water-induced compaction tables are set - the boundary's transmissibility multiplier (rockCompTransMultiplier, ebos/eclfluxmodule.hh:441) is not built for them");
    if (!bc->cell || !bc->direction || !bc->type || !bc->area || !bc->trans || !bc->depth) return refuse(msg, "set_boundary_conditions: null array (only rate is optional, without RATE faces)");
    std::vector<unsigned char> seen((size_t)ctx.Nb, 0);   // bit d: face d of the cell is listed
    for (int f = 0; f < nf; ++f) {
        const int cell = bc->cell[f], d = bc->direction[f], ty = bc->type[f];
        if (cell < 0 || cell >= ctx.Nb) return refuse(msg, "set_boundary_conditions: face %d: cell %d outside [0, %d)", f, cell, ctx.Nb);
        if (d < 0 || d > 5) return refuse(msg, "set_boundary_conditions: face %d: direction %d outside 0..5 (X-, X+, Y-, Y+, Z-, Z+)", f, d);
        if (ty != OPMHIP_BC_RATE && ty != OPMHIP_BC_FREE) return refuse(msg, "set_boundary_conditions: face %d: unknown type %d (0 RATE, 1 FREE)", f, ty);
        if (seen[cell] & (1u << d)) return refuse(msg, "set_boundary_conditions: face %d: cell %d, direction %d is listed twice", f, cell, d);
        seen[cell] = (unsigned char)(seen[cell] | (1u << d));
        if (!(bc->area[f] > 0.0) || !std::isfinite(bc->area[f])) return refuse(msg, "set_boundary_conditions: face %d: area %g is not positive", f, bc->area[f]);
        if (!(bc->trans[f] >= 0.0) || !std::isfinite(bc->trans[f])) return refuse(msg, "set_boundary_conditions: face %d: transmissibility %g is negative or not finite", f, bc->trans[f]);
        if (!std::isfinite(bc->depth[f])) return refuse(msg, "set_boundary_conditions: face %d: depth is not finite", f);
        if (ty == OPMHIP_BC_FREE && ctx.hysteresis)
            return refuse(msg, "set_boundary_conditions: face %d is FREE in a context with relative-permeability hysteresis - the reference re-evaluates the exterior relative permeabilities with the cell's current material parameters (ebos/eclfluxmodule.hh:452-459), which a captured mobility cannot follow", f);
        if (ty == OPMHIP_BC_RATE) {
            if (!bc->rate) return refuse(msg, "set_boundary_conditions: null array (rate, with a RATE face: %d)", f);
            for (int e = 0; e < 3; ++e)
                if (!std::isfinite(bc->rate[(size_t)3 * f + e])) return refuse(msg, "set_boundary_conditions: face %d: rate %d is not finite", f, e);
        }
    }
    BoundaryLists L;
    L.nf = nf;
    L.type.assign(bc->type, bc->type + nf);
    L.geo.resize((size_t)3 * nf);
    L.rate.assign((size_t)3 * nf, 0.0);
    for (int f = 0; f < nf; ++f) {
        L.geo[(size_t)3 * f] = bc->area[f]; L.geo[(size_t)3 * f + 1] = bc->trans[f]; L.geo[(size_t)3 * f + 2] = bc->depth[f];
        if (L.type[f] == OPMHIP_BC_RATE)
            for (int e = 0; e < 3; ++e) L.rate[(size_t)3 * f + e] = bc->rate[(size_t)3 * f + e];
    }
    group_by_cell(bc->cell, nf, ctx.Nb, toOrder, L.pos, L.cpos, L.cptr, L.cconn);
    L.slot.assign(L.cpos.size(), -1);
    for (size_t t = 0; t < L.cpos.size(); ++t)
        for (int k = L.cptr[t]; k < L.cptr[t + 1]; ++k)
            if (L.type[L.cconn[k]] == OPMHIP_BC_FREE && L.slot[t] < 0) { L.slot[t] = (int)L.fcell.size(); L.fcell.push_back((int)t); }
    out = std::move(L);
    return OPMHIP_SUCCESS;
}

}  // namespace opmhip
