// C-ABI of the fluid-in-place report (include/opmhip.h "fluids in place"): argument checks and plans through fip_setup.hpp, allocation,
// upload and the launches of fip.hip.  Region arrays arrive in the NATURAL cell order; the lists on the device name INTERNAL cell ids.
// Everything goes on the context's one stream.
#include <algorithm>
#include <string>
#include <vector>

#include "capi_guard.hpp"
#include "fip_setup.hpp"
#include "internal.hpp"

using namespace opmhip;

namespace {

// the rows of a set out of d_out's sums: the twelve sums, then RPR / FPR and RPRP / FPRP (updateSummaryRegionValues, :1519-1569)
void fip_rows(const std::vector<double>& sums, int rows, std::vector<double>& out) {
    out.resize((size_t)rows * OPMHIP_FIP_ROW);
    for (int r = 0; r < rows; ++r) {
        const double* s = &sums[(size_t)r * FIP_TERMS];
        double* o = &out[(size_t)r * OPMHIP_FIP_ROW];
        std::copy(s, s + FIP_TERMS, o);
        o[FIP_TERMS] = fip_pressure_average(s[FIP_PRESSURE_HC_PV], s[FIP_HC_PV], s[FIP_PRESSURE_PV], s[FIP_PORE_VOLUME], true);
        o[FIP_TERMS + 1] = fip_pressure_average(s[FIP_PRESSURE_HC_PV], s[FIP_HC_PV], s[FIP_PRESSURE_PV], s[FIP_PORE_VOLUME], false);
    }
}
void fip_hand_over(const std::vector<double>& rows, int max_id, double* regions, double* field) {
    if (regions) std::copy(rows.begin(), rows.begin() + (size_t)max_id * OPMHIP_FIP_ROW, regions);
    if (field) std::copy(rows.begin() + (size_t)max_id * OPMHIP_FIP_ROW, rows.end(), field);
}

}  // namespace

extern "C" {

// replaces: the region arrays of EclGenericOutputBlackoilModule and regionMax (ebos/eclgenericoutputblackoilmodule.cc:1405-1410)
int opmhip_set_fip_regions(opmhip_ctx* c, int num_sets, const int* const* region) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        const Pattern& P = c->pat;
        if (!A.static_set) return fail(c, OPMHIP_NOT_READY, "set_fip_regions before set_static");
        std::vector<int> max_id;
        std::string msg;
        if (int r = fip_regions_check(num_sets, region, P.Nb, c->comm.nranks, P.Nghost, max_id, msg)) return fail(c, r, "%s", msg.c_str());   // the sets in force stay
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        if (num_sets == 0) {
            dev_part_release(c, A.fip);
            return OPMHIP_SUCCESS;
        }
        FipDev fresh;
        const int rc = [&]() -> int {
            int r;
            fresh.sets.resize(num_sets);
            for (int s = 0; s < num_sets; ++s) {
                FipPlan H;
                fip_plan(P.Nb, P.toOrder.data(), region[s], max_id[s], H);
                FipSetDev& S = fresh.sets[s];
                S.max_id = H.max_id; S.ncells = H.ncells; S.npart = H.npart;
                S.level_ptr = H.level_ptr;
                if ((r = dev_upload(c, &S.d_items, H.items)) || (r = dev_upload(c, &S.d_desc, H.desc)) || (r = dev_upload(c, &S.d_result, H.result))) return r;
                fresh.npart = std::max(fresh.npart, H.npart);
                fresh.max_id = std::max(fresh.max_id, H.max_id);
            }
            if ((r = dev_alloc(c, &fresh.d_terms, (size_t)FIP_TERMS * P.Nloc)) || (r = dev_alloc(c, &fresh.d_part, (size_t)FIP_TERMS * fresh.npart)) ||
                (r = dev_alloc(c, &fresh.d_out, (size_t)FIP_TERMS * (fresh.max_id + 1))))
                return r;
            for (hipEvent_t& e : A.fip_ev)
                if (!e) OPMHIP_HIP(c, hipEventCreate(&e));
            return OPMHIP_SUCCESS;
        }();
        if (rc) { dev_part_release(c, fresh); return rc; }
        dev_part_install(c, A.fip, fresh);
        return OPMHIP_SUCCESS;
    });
}

// replaces: the element loop over updateFluidInPlace_ (ebos/ecloutputblackoilmodule.hh:610-697), accumulateRegionSums
// (ebos/eclgenericoutputblackoilmodule.cc:1467-1490) and the pressures of updateSummaryRegionValues (:1519-1569), for one set
int opmhip_fluid_in_place(opmhip_ctx* c, int set, double* regions, double* field) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        FipDev& F = A.fip;
        std::string msg;
        if (int r = fip_call_check("fluid_in_place", A.state_set, (int)F.sets.size(), set, msg)) return fail(c, r, "%s", msg.c_str());
        FipSetDev& S = F.sets[set];
        OPMHIP_HIP(c, hipSetDevice(c->device));
        F.timed = false;
        OPMHIP_HIP(c, hipEventRecord(A.fip_ev[0], c->stream));
        launch_fip_cells(c);
        OPMHIP_HIP(c, hipEventRecord(A.fip_ev[1], c->stream));
        launch_fip_reduce(c, S);
        OPMHIP_HIP(c, hipEventRecord(A.fip_ev[2], c->stream));
        OPMHIP_HIP(c, hipGetLastError());
        std::vector<double> sums((size_t)(S.max_id + 1) * FIP_TERMS), rows;
        OPMHIP_HIP(c, hipMemcpyAsync(sums.data(), F.d_out, sums.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        F.timed = true;
        fip_rows(sums, S.max_id + 1, rows);
        if (S.initial.empty()) S.initial = rows;   // initialInplace_ (:1487-1488)
        fip_hand_over(rows, S.max_id, regions, field);
        return OPMHIP_SUCCESS;
    });
}

// replaces: initialInplace_ as updateSummaryRegionValues reads it for FOE (ebos/eclgenericoutputblackoilmodule.cc:1514-1517)
int opmhip_get_fluid_in_place_initial(opmhip_ctx* c, int set, double* regions, double* field) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        const FipDev& F = c->asmb.fip;
        std::string msg;
        if (int r = fip_call_check("get_fluid_in_place_initial", true, (int)F.sets.size(), set, msg)) return fail(c, r, "%s", msg.c_str());
        const FipSetDev& S = F.sets[set];
        if (S.initial.empty()) return fail(c, OPMHIP_NOT_READY, "get_fluid_in_place_initial before the first fluid_in_place of set %d", set);
        fip_hand_over(S.initial, S.max_id, regions, field);
        return OPMHIP_SUCCESS;
    });
}

// replaces: the per-cell buffers fip_, dynamicPoreVolume_, hydrocarbonPoreVolume_, pressureTimes*Volume_ the restart file is written
// from (ebos/ecloutputblackoilmodule.hh:632-637, 666-693)
int opmhip_get_fluid_in_place_cells(opmhip_ctx* c, double* out) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        const AsmDev& A = c->asmb;
        const Pattern& P = c->pat;
        std::string msg;
        if (int r = fip_call_check("get_fluid_in_place_cells", A.state_set, (int)A.fip.sets.size(), 0, msg)) return fail(c, r, "%s", msg.c_str());
        if (!out) return fail(c, OPMHIP_INVALID_ARGUMENT, "get_fluid_in_place_cells: out == NULL");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        launch_fip_cells(c);
        OPMHIP_HIP(c, hipGetLastError());
        std::vector<double> v((size_t)FIP_TERMS * P.Nloc);
        if (!v.empty()) OPMHIP_HIP(c, hipMemcpyAsync(v.data(), A.fip.d_terms, v.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        for (int f = 0; f < FIP_TERMS; ++f)
            for (int p = 0; p < P.Nb; ++p) out[(size_t)f * P.Nb + P.fromOrder[p]] = v[(size_t)f * P.Nloc + p];
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_fip_info(opmhip_ctx* c, int set, int* info) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        const FipDev& F = c->asmb.fip;
        std::string msg;
        if (int r = fip_call_check("get_fip_info", true, (int)F.sets.size(), set, msg)) return fail(c, r, "%s", msg.c_str());
        if (!info) return fail(c, OPMHIP_INVALID_ARGUMENT, "get_fip_info: info == NULL");
        const FipSetDev& S = F.sets[set];
        const int levels = (int)S.level_ptr.size() - 1;
        info[0] = S.max_id;
        info[1] = S.ncells;
        info[2] = levels > 0 ? S.level_ptr[1] : 0;
        info[3] = levels;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_fip_timings(opmhip_ctx* c, double* ms) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        const AsmDev& A = c->asmb;
        if (!ms) return fail(c, OPMHIP_INVALID_ARGUMENT, "get_fip_timings: ms == NULL");
        if (!A.fip.timed) return fail(c, OPMHIP_NOT_READY, "get_fip_timings before fluid_in_place");
        float a = 0.0f, b = 0.0f;
        OPMHIP_HIP(c, hipEventElapsedTime(&a, A.fip_ev[0], A.fip_ev[1]));
        OPMHIP_HIP(c, hipEventElapsedTime(&b, A.fip_ev[1], A.fip_ev[2]));
        ms[0] = a;
        ms[1] = b;
        return OPMHIP_SUCCESS;
    });
}

}  // extern "C"
