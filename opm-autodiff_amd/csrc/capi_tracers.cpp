// C-ABI of the passive tracers (include/opmhip.h "passive tracers"): argument checks through tracers_setup.hpp, allocation, upload and
// the launches of tracers.hip.  Host arrays arrive in the NATURAL cell / entry order, tracer-major; on the device a phase batch's arrays
// are interleaved [cell][tracer of the batch] in the INTERNAL cell order.  Everything goes on the context's one stream.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "capi_guard.hpp"
#include "internal.hpp"
#include "tracers_setup.hpp"

using namespace opmhip;

namespace {

void tracer_connections_release(opmhip_ctx* c) {
    TracersDev& T = c->asmb.tr;
    T.each_conn([c](auto** p) { dev_free(c, p); });
    T.nconn = T.nd = 0;
}
void tracers_release(opmhip_ctx* c) {   // the stream is idle
    TracersDev& T = c->asmb.tr;
    tracer_connections_release(c);
    for (int ph = 0; ph < TRACER_PHASES; ++ph) dev_part_release(c, T.b[ph]);
    T.each_dev([c](auto** p) { dev_free(c, p); });
    T.num = T.maxnt = 0;
    T.begun = false;
    T.phase.clear(); T.slot.clear(); T.lvptr.clear();
}
// natural, tracer-major [g * Nb + cell] <-> a batch's interleaved internal form [pos * nt + slot]
void batch_from_natural(const Pattern& P, const TracerBatchDev& B, const double* nat, std::vector<double>& v) {
    v.resize((size_t)P.Nb * B.nt);
    for (int p = 0; p < P.Nb; ++p)
        for (int t = 0; t < B.nt; ++t) v[(size_t)p * B.nt + t] = nat[(size_t)B.members.g[t] * P.Nb + P.fromOrder[p]];
}
int batch_to_natural(opmhip_ctx* c, const TracerBatchDev& B, const double* d_v, double* nat) {   // the stream is idle
    const Pattern& P = c->pat;
    std::vector<double> v((size_t)P.Nb * B.nt);
    if (v.empty()) return OPMHIP_SUCCESS;
    OPMHIP_HIP(c, hipMemcpy(v.data(), d_v, v.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int p = 0; p < P.Nb; ++p)
        for (int t = 0; t < B.nt; ++t) nat[(size_t)B.members.g[t] * P.Nb + P.fromOrder[p]] = v[(size_t)p * B.nt + t];
    return OPMHIP_SUCCESS;
}

}  // namespace

extern "C" {

int opmhip_set_tracers(opmhip_ctx* c, int num_tracers, const int* phase, const double* concentration) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        TracersDev& T = A.tr;
        const Pattern& P = c->pat;
        if (!A.static_set) return fail(c, OPMHIP_NOT_READY, "set_tracers before set_static");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        tracers_release(c);   // whatever happens below, the old tracers are gone: a refused call leaves none set
        if (num_tracers == 0) return OPMHIP_SUCCESS;
        TracerBatches H;
        std::string msg;
        if (int r = tracer_batches(num_tracers, phase, concentration, P.Nb, A.wet_gas, c->comm.nranks, P.Nghost, H, msg)) return fail(c, r, "%s", msg.c_str());
        TracerLevels L;
        tracer_levels(P.Nb, P.rowptr.data(), P.col.data(), L);
        std::vector<int> ford;
        tracer_face_order(P.Nb, P.rowptr.data(), P.nnzMap.data(), ford);
        const int rc = [&]() -> int {
            int r;
            int maxnt = 0;
            std::vector<double> v;
            for (int ph = 0; ph < TRACER_PHASES; ++ph) {
                TracerBatchDev& B = T.b[ph];
                B.nt = (int)H.members[ph].size();
                for (int t = 0; t < B.nt; ++t) B.members.g[t] = H.members[ph][t];
                if (B.nt == 0) continue;
                maxnt = std::max(maxnt, B.nt);
                batch_from_natural(P, B, concentration, v);
                if ((r = dev_upload(c, &B.d_c, v)) || (r = dev_upload(c, &B.d_c0, v)) || (r = dev_alloc(c, &B.d_s1, v.size()))) return r;
            }
            const size_t nv = (size_t)P.Nb * maxnt;
            if ((r = dev_upload(c, &T.d_lvrows, L.rows)) || (r = dev_upload(c, &T.d_ford, ford))) return r;
            if ((r = dev_alloc(c, &T.d_flag, (size_t)1)) || (r = dev_alloc(c, &T.d_M, (size_t)P.nnzb)) || (r = dev_alloc(c, &T.d_LU, (size_t)P.nnzb)) ||
                (r = dev_alloc(c, &T.d_invd, (size_t)P.Nb)))
                return r;
            for (double** p : {&T.d_res, &T.d_x, &T.d_r, &T.d_rw, &T.d_p, &T.d_v, &T.d_s, &T.d_t, &T.d_y, &T.d_pw})
                if ((r = dev_alloc(c, p, nv))) return r;
            // reductions: at most 256 workgroups of 256 lanes in the first stage, each over a run of whole cells
            T.nblk = std::max(1, std::min(256, (P.Nb + 255) / 256));
            T.cellsPerBlock = (P.Nb + T.nblk - 1) / T.nblk;
            if ((r = dev_alloc(c, &T.d_sc, (size_t)maxnt * 16)) || (r = dev_alloc(c, &T.d_part, (size_t)2 * T.nblk * maxnt))) return r;
            if (!T.h_rec) {
                OPMHIP_HIP(c, hipHostMalloc((void**)&T.h_rec, 4 * sizeof(double), hipHostMallocMapped));
                OPMHIP_HIP(c, hipHostGetDevicePointer((void**)&T.d_rec, T.h_rec, 0));
                for (int i = 0; i < 4; ++i) T.h_rec[i] = 0.0;
            }
            for (hipEvent_t& e : T.ev)
                if (!e) OPMHIP_HIP(c, hipEventCreate(&e));
            T.maxnt = maxnt;
            return OPMHIP_SUCCESS;
        }();
        if (rc) { tracers_release(c); return rc; }
        T.num = num_tracers;
        T.phase = H.phase; T.slot = H.slot; T.lvptr = L.ptr;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_tracer_solver(opmhip_ctx* c, double tolerance, int maxit) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        std::string msg;
        if (int r = tracer_solver_check(tolerance, maxit, msg)) return fail(c, r, "%s", msg.c_str());
        c->asmb.tr.tol = tolerance;
        c->asmb.tr.maxit = maxit;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_tracer_connections(opmhip_ctx* c, int n, const int* cell, const double* rate, const double* injected) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        TracersDev& T = c->asmb.tr;
        const Pattern& P = c->pat;
        if (T.num == 0) return fail(c, OPMHIP_NOT_READY, "set_tracer_connections before set_tracers");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        if (n == 0) {
            OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
            tracer_connections_release(c);
            return OPMHIP_SUCCESS;
        }
        TracerConnLists H;
        std::string msg;
        if (int r = tracer_connections(n, cell, rate, injected, T.num, P.Nb, P.toOrder.data(), H, msg)) return fail(c, r, "%s", msg.c_str());   // the list in force stays
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        tracer_connections_release(c);
        const std::vector<double> hr(rate, rate + (size_t)3 * n), hi(injected, injected + (size_t)T.num * n);
        int r;
        if ((r = dev_upload(c, &T.d_cpos, H.cpos)) || (r = dev_upload(c, &T.d_cptr, H.cptr)) || (r = dev_upload(c, &T.d_cconn, H.cconn)) ||
            (r = dev_upload(c, &T.d_rate, hr)) || (r = dev_upload(c, &T.d_inj, hi))) {
            tracer_connections_release(c);
            return r;
        }
        T.nconn = n;
        T.nd = (int)H.cpos.size();
        return OPMHIP_SUCCESS;
    });
}

int opmhip_tracers_begin_time_step(opmhip_ctx* c) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        TracersDev& T = c->asmb.tr;
        if (T.num == 0) return OPMHIP_SUCCESS;
        if (!c->asmb.state_set) return fail(c, OPMHIP_NOT_READY, "tracers_begin_time_step before set_state");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        for (int ph = 0; ph < TRACER_PHASES; ++ph) launch_tracer_begin(c, ph);
        OPMHIP_HIP(c, hipGetLastError());
        T.begun = true;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_tracers_end_time_step(opmhip_ctx* c, double dt, opmhip_tracer_result* res) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        TracersDev& T = c->asmb.tr;
        if (T.num == 0) return OPMHIP_SUCCESS;
        if (!c->asmb.state_set) return fail(c, OPMHIP_NOT_READY, "tracers_end_time_step before set_state");
        if (!T.begun) return fail(c, OPMHIP_NOT_READY, "tracers_end_time_step before the first opmhip_tracers_begin_time_step");
        if (!(dt > 0.0) || !std::isfinite(dt)) return fail(c, OPMHIP_INVALID_ARGUMENT, "tracers_end_time_step: dt must be positive and finite");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        T.ms[0] = T.ms[1] = T.ms[2] = 0.0;
        T.launches = 0;
        std::vector<opmhip_tracer_result> rb(OPMHIP_TRACERS_MAX_PER_PHASE);
        std::string pivots;
        for (int ph = 0; ph < TRACER_PHASES; ++ph) {
            const TracerBatchDev& B = T.b[ph];
            if (B.nt == 0) continue;
            OPMHIP_HIP(c, hipEventRecord(T.ev[0], c->stream));
            launch_tracer_system(c, ph, dt);
            OPMHIP_HIP(c, hipGetLastError());
            bool pivot = false;
            if (int r = tracer_solve_batch(c, ph, rb.data(), &pivot)) return r;
            if (pivot) pivots += (pivots.empty() ? "" : ", ") + std::to_string(ph);
            if (res)
                for (int t = 0; t < B.nt; ++t) res[B.members.g[t]] = rb[t];
        }
        if (!pivots.empty())
            (void)fail(c, OPMHIP_SUCCESS, "tracers_end_time_step: the ILU0 of phase %s met a pivot that is zero or not finite (replaced by 1; reported as not converged)", pivots.c_str());
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_tracers(opmhip_ctx* c, double* concentration) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        TracersDev& T = c->asmb.tr;
        if (T.num == 0) return OPMHIP_SUCCESS;
        if (!concentration) return fail(c, OPMHIP_INVALID_ARGUMENT, "get_tracers: concentration == NULL");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        for (int ph = 0; ph < TRACER_PHASES; ++ph)
            if (T.b[ph].nt > 0)
                if (int r = batch_to_natural(c, T.b[ph], T.b[ph].d_c, concentration)) return r;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_tracer_storage(opmhip_ctx* c, double* storage1, double* concentration_initial) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        TracersDev& T = c->asmb.tr;
        if (T.num == 0) return OPMHIP_SUCCESS;
        if (!T.begun) return fail(c, OPMHIP_NOT_READY, "get_tracer_storage before the first opmhip_tracers_begin_time_step");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        for (int ph = 0; ph < TRACER_PHASES; ++ph) {
            if (T.b[ph].nt == 0) continue;
            if (storage1)
                if (int r = batch_to_natural(c, T.b[ph], T.b[ph].d_s1, storage1)) return r;
            if (concentration_initial)
                if (int r = batch_to_natural(c, T.b[ph], T.b[ph].d_c0, concentration_initial)) return r;
        }
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_tracer_system(opmhip_ctx* c, int phase, double dt, double* matrix, double* residual) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        TracersDev& T = c->asmb.tr;
        const Pattern& P = c->pat;
        if (phase < 0 || phase >= TRACER_PHASES) return fail(c, OPMHIP_INVALID_ARGUMENT, "get_tracer_system: phase %d", phase);
        if (T.num == 0 || T.b[phase].nt == 0) return fail(c, OPMHIP_INVALID_ARGUMENT, "get_tracer_system: no tracer of phase %d is set", phase);
        if (!c->asmb.state_set || !T.begun) return fail(c, OPMHIP_NOT_READY, "get_tracer_system before the first opmhip_tracers_begin_time_step");
        if (!(dt > 0.0) || !std::isfinite(dt)) return fail(c, OPMHIP_INVALID_ARGUMENT, "get_tracer_system: dt must be positive and finite");
        if (!matrix || !residual) return fail(c, OPMHIP_INVALID_ARGUMENT, "get_tracer_system: null array");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        const TracerBatchDev& B = T.b[phase];
        launch_tracer_system(c, phase, dt);   // into the solve's scratch arrays: nothing of the tracers' state is touched
        OPMHIP_HIP(c, hipGetLastError());
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        std::vector<double> m(P.nnzb), r((size_t)P.Nb * B.nt);
        if (!m.empty()) OPMHIP_HIP(c, hipMemcpy(m.data(), T.d_M, m.size() * sizeof(double), hipMemcpyDeviceToHost));
        if (!r.empty()) OPMHIP_HIP(c, hipMemcpy(r.data(), T.d_res, r.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int k = 0; k < P.nnzb; ++k) matrix[P.nnzMap[k]] = m[k];
        for (int p = 0; p < P.Nb; ++p)
            for (int t = 0; t < B.nt; ++t) residual[(size_t)t * P.Nb + P.fromOrder[p]] = r[(size_t)p * B.nt + t];
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_tracer_timings(opmhip_ctx* c, double* ms, int* info) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    const TracersDev& T = c->asmb.tr;
    if (ms) for (int i = 0; i < 3; ++i) ms[i] = T.ms[i];
    if (info) { info[0] = T.lvptr.empty() ? 0 : (int)T.lvptr.size() - 1; info[1] = T.launches; }
    return OPMHIP_SUCCESS;
}

}  // extern "C"
