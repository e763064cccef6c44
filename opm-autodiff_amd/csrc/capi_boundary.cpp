// C-ABI of the open boundaries (include/opmhip.h "open boundaries"): argument checks and lists through boundary_setup.hpp, allocation,
// upload and the launches of boundary.hip's kernels.  opmhip_assemble (capi_asm.cpp) applies the list.
#include <algorithm>
#include <string>
#include <vector>

#include "boundary_setup.hpp"
#include "capi_guard.hpp"
#include "internal.hpp"

using namespace opmhip;

static_assert(BC_GEO == 3 && BC_Q == 12, "boundary_setup.cpp packs three doubles per face; opmhip_get_boundary_rates hands out twelve");

extern "C" {

int opmhip_set_boundary_conditions(opmhip_ctx* c, const opmhip_boundary_conditions* bc) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        BoundaryDev& B = A.bc;
        const Pattern& P = c->pat;
        if (!A.static_set) return fail(c, OPMHIP_NOT_READY, "set_boundary_conditions before set_static");
        if (!A.state_set) return fail(c, OPMHIP_NOT_READY, "set_boundary_conditions before set_state: the exterior state of the FREE faces is the state's");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        dev_part_release(c, B);   // whatever happens below, the old list is gone: a refused call leaves no list set
        if (!bc || bc->num_faces == 0) return OPMHIP_SUCCESS;
        BoundaryContext X;
        X.Nb = P.Nb; X.nranks = c->comm.nranks; X.hysteresis = A.hyst_model >= 0; X.water_compaction = A.d_maxsw != nullptr;
        BoundaryLists H;
        std::string msg;
        if (int r = boundary_lists(bc, X, P.toOrder.data(), H, msg)) return fail(c, r, "%s", msg.c_str());
        const int nd = (int)H.cpos.size(), nfc = (int)H.fcell.size();
        BoundaryDev N;
        const int rc = [&]() -> int {
            int r;
            const std::vector<double> zq((size_t)BC_Q * H.nf, 0.0);
            if ((r = dev_upload(c, &N.d_type, H.type)) || (r = dev_upload(c, &N.d_geo, H.geo)) || (r = dev_upload(c, &N.d_rate, H.rate)) || (r = dev_upload(c, &N.d_q, zq)) ||
                (r = dev_upload(c, &N.d_cpos, H.cpos)) || (r = dev_upload(c, &N.d_cptr, H.cptr)) || (r = dev_upload(c, &N.d_cconn, H.cconn)) ||
                (r = dev_upload(c, &N.d_slot, H.slot)) || (r = dev_upload(c, &N.d_fcell, H.fcell)))
                return r;
            if ((r = dev_alloc(c, &N.d_ext, (size_t)nfc * BC_EXT)) || (r = dev_alloc(c, &N.d_save, (size_t)nd * BC_Q))) return r;
            return OPMHIP_SUCCESS;
        }();
        if (rc) { dev_part_release(c, N); return rc; }
        N.nf = H.nf; N.nd = nd; N.nfc = nfc;
        B = N;
        if (nfc > 0) {   // initialFluidStates_ of the cells with a FREE face
            launch_boundary_capture(c);
            OPMHIP_HIP(c, hipGetLastError());
            OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        }
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_boundary_rates(opmhip_ctx* c, double* q12) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        const BoundaryDev& B = c->asmb.bc;
        if (B.nf == 0) return OPMHIP_SUCCESS;
        if (!q12) return fail(c, OPMHIP_INVALID_ARGUMENT, "get_boundary_rates: q12 == NULL");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        OPMHIP_HIP(c, hipMemcpy(q12, B.d_q, (size_t)BC_Q * B.nf * sizeof(double), hipMemcpyDeviceToHost));
        return OPMHIP_SUCCESS;
    });
}

}  // extern "C"
