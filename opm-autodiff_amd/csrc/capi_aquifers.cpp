// C-ABI of the analytic aquifers (include/opmhip.h "analytic aquifers"): argument checks and lists through source_lists.hpp, allocation,
// upload and the launches of assemble.hip's aquifer kernels.  opmhip_assemble and opmhip_end_time_step (capi_asm.cpp) apply the list.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "capi_guard.hpp"
#include "internal.hpp"
#include "source_lists.hpp"

using namespace opmhip;

namespace {
void aquifers_release(opmhip_ctx* c) {   // the stream is idle
    AquifersDev& Q = c->asmb.aq;
    if (Q.h_step) (void)hipHostFree(Q.h_step);
    const hipEvent_t ev = Q.ev_step;   // lives as long as the context
    dev_part_release(c, Q);
    Q.ev_step = ev;
}
}  // namespace

extern "C" {

int opmhip_set_aquifers(opmhip_ctx* c, const opmhip_aquifers* aq) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        AquifersDev& Q = A.aq;
        const Pattern& P = c->pat;
        if (!A.static_set) return fail(c, OPMHIP_NOT_READY, "set_aquifers before set_static");
        if (!A.state_set) return fail(c, OPMHIP_NOT_READY, "set_aquifers before set_state: the aquifers are initialised from the initial solution");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        aquifers_release(c);   // whatever happens below, the old list is gone: a refused call leaves no list set
        if (!aq || aq->num_aquifers == 0) return OPMHIP_SUCCESS;
        if (c->comm.nranks > 1)
            return fail(c, OPMHIP_INVALID_ARGUMENT, "set_aquifers: decomposed context (%d ranks) - alphai_, the equilibrium pressure and W_flux_ are sums over the ranks, which is not built", c->comm.nranks);
        const int na = aq->num_aquifers;
        AquiferLists H;
        std::string msg;
        if (int r = aquifer_lists(aq, P.Nb, P.toOrder.data(), H, msg)) return fail(c, r, "%s", msg.c_str());
        const int nc = H.nc;
        // calculateReservoirEquilibrium (AquiferInterface.hpp:330-373) for the aquifers without an initial pressure
        if (!H.need_eq.empty()) {
            const int IQS = iq_doubles_per_cell(c);
            std::vector<double> depth(P.Nloc), rec;
            OPMHIP_HIP(c, hipMemcpy(depth.data(), A.d_depth, depth.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (int a : H.need_eq) {
                const int i0 = aq->conn_pointers[a], n = aq->conn_pointers[a + 1] - i0;
                std::vector<int> order(n), p(n);
                for (int i = 0; i < n; ++i) order[i] = i0 + i;
                std::sort(order.begin(), order.end(), [&](int x, int y) { return aq->cell[x] < aq->cell[y]; });   // the element loop
                for (int i = 0; i < n; ++i) p[i] = H.pos[order[i]];
                rec.resize((size_t)n * IQS);
                if (n > 0) {
                    const int rc = with_cell_positions(c, "set_aquifers", p, [&]() -> int {
                        launch_iq_gather(c, n, A.d_cell_pos, A.d_stage_cell);
                        OPMHIP_HIP(c, hipGetLastError());
                        OPMHIP_HIP(c, hipMemcpyAsync(rec.data(), A.d_stage_cell, rec.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
                        return OPMHIP_SUCCESS;
                    });
                    if (rc) return rc;
                }
                H.par[(size_t)a * AQ_PAR + AQ_PA0] = aquifer_equilibrium_pressure(aq->alpha, i0, n, order.data(), rec.data(), IQS, depth.data(), p.data(), aq->datum_depth[a]);
            }
        }
        std::vector<double> state;
        aquifer_initial_state(aq, H.par, state);
        const int rc = [&]() -> int {
            int r;
            const std::vector<int> ptr(aq->conn_pointers, aq->conn_pointers + na + 1);
            const std::vector<double> alpha(aq->alpha, aq->alpha + nc), zc((size_t)4 * std::max(nc, 1), 0.0);
            if ((r = dev_upload(c, &Q.d_ptr, ptr)) || (r = dev_upload(c, &Q.d_of, H.of)) || (r = dev_upload(c, &Q.d_pos, H.pos)) || (r = dev_upload(c, &Q.d_alpha, alpha)) ||
                (r = dev_upload(c, &Q.d_par, H.par)) || (r = dev_upload(c, &Q.d_state, state)) || (r = dev_upload(c, &Q.d_q, zc)) ||
                (r = dev_upload(c, &Q.d_cpos, H.cpos)) || (r = dev_upload(c, &Q.d_cptr, H.cptr)) || (r = dev_upload(c, &Q.d_cconn, H.cconn)))
                return r;
            if ((r = dev_alloc(c, &Q.d_pprev, (size_t)nc)) || (r = dev_alloc(c, &Q.d_step, (size_t)na * AQ_STEP)) || (r = dev_alloc(c, &Q.d_save, H.cpos.size() * 4))) return r;
            OPMHIP_HIP(c, hipMemset(Q.d_pprev, 0, (size_t)std::max(nc, 1) * sizeof(double)));
            OPMHIP_HIP(c, hipMemset(Q.d_step, 0, (size_t)na * AQ_STEP * sizeof(double)));
            OPMHIP_HIP(c, hipHostMalloc((void**)&Q.h_step, (size_t)na * AQ_STEP * sizeof(double), hipHostMallocDefault));
            if (!Q.ev_step) OPMHIP_HIP(c, hipEventCreateWithFlags(&Q.ev_step, hipEventDisableTiming));
            OPMHIP_HIP(c, hipDeviceSynchronize());
            return OPMHIP_SUCCESS;
        }();
        if (rc) { aquifers_release(c); return rc; }
        Q.num = na; Q.nc = nc; Q.nd = (int)H.cpos.size();
        Q.h_ptr.assign(aq->conn_pointers, aq->conn_pointers + na + 1);
        Q.h_id.assign(aq->id, aq->id + na);
        Q.h_par = H.par; Q.h_tabptr = H.tabptr; Q.h_td = H.td; Q.h_pd = H.pd;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_aquifers_begin_time_step(opmhip_ctx* c, double time, double dt) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AquifersDev& Q = c->asmb.aq;
        if (Q.num == 0) return OPMHIP_SUCCESS;
        if (!(dt > 0.0) || !std::isfinite(time)) return fail(c, OPMHIP_INVALID_ARGUMENT, "aquifers_begin_time_step: dt must be positive, time finite");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        if (Q.stepped) OPMHIP_HIP(c, hipEventSynchronize(Q.ev_step));   // the last call's copy has read the staging area
        aquifer_step_scalars(Q.num, Q.h_par, Q.h_tabptr, Q.h_td, Q.h_pd, time, dt, Q.h_step);
        OPMHIP_HIP(c, hipMemcpyAsync(Q.d_step, Q.h_step, (size_t)Q.num * AQ_STEP * sizeof(double), hipMemcpyHostToDevice, c->stream));
        OPMHIP_HIP(c, hipEventRecord(Q.ev_step, c->stream));
        if (Q.nc > 0) launch_aquifer_begin(c);
        OPMHIP_HIP(c, hipGetLastError());
        Q.stepped = true;
        Q.step_dt = dt;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_aquifers(opmhip_ctx* c, double* W_flux, double* pressure, double* flux_rate, double* init_pressure) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AquifersDev& Q = c->asmb.aq;
        if (Q.num == 0) return OPMHIP_SUCCESS;
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        std::vector<double> state((size_t)Q.num * AQ_STATE), q((size_t)4 * std::max(Q.nc, 1));
        OPMHIP_HIP(c, hipMemcpy(state.data(), Q.d_state, state.size() * sizeof(double), hipMemcpyDeviceToHost));
        if (flux_rate) OPMHIP_HIP(c, hipMemcpy(q.data(), Q.d_q, q.size() * sizeof(double), hipMemcpyDeviceToHost));
        aquifer_report(Q.num, Q.h_par, Q.h_ptr, state.data(), q.data(), W_flux, pressure, flux_rate, init_pressure);
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_aquifer_rates(opmhip_ctx* c, double* q4) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AquifersDev& Q = c->asmb.aq;
        if (Q.nc == 0) return OPMHIP_SUCCESS;
        if (!q4) return fail(c, OPMHIP_INVALID_ARGUMENT, "get_aquifer_rates: q4 == NULL");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        OPMHIP_HIP(c, hipMemcpy(q4, Q.d_q, (size_t)4 * Q.nc * sizeof(double), hipMemcpyDeviceToHost));
        return OPMHIP_SUCCESS;
    });
}

}  // extern "C"
