// C-ABI, the device-resident standard wells and the VFP tables their THP control reads (include/opmhip.h: opmhip_set_std_wells ...
// opmhip_get_std_wells_groups, opmhip_set_vfp_tables, opmhip_vfp_probe).  Every check of what the caller hands over is host work of
// source_lists.cpp / vfp_tables.cpp; this unit allocates, uploads and launches (std_wells.hip).
//
// A feature's device state is one part of StdWellsDev (internal.hpp), its arrays named once.  Its setter builds a fresh part apart, discards it
// (dev_part_release) if an array cannot be had, and installs it (dev_part_install) once all of them exist: a refused call leaves the
// previous setting in force.  opmhip_set_std_wells and opmhip_set_std_wells_head_model release first instead: the old list or model is
// gone whatever happens.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "capi_guard.hpp"
#include "internal.hpp"
#include "source_lists.hpp"
#include "vfp_tables.hpp"

using namespace opmhip;

namespace {
void std_wells_release(opmhip_ctx* c) {   // the stream is idle
    StdWellsDev& S = c->wells.sw;
    dev_part_release(c, S.lim);
    dev_part_release(c, S.grp);
    dev_part_release(c, S.ma);   // (in_matrix is a fact about the matrix: it stays until the next assemble, so that these wells are not applied a second time)
    dev_part_release(c, S.cf);
    dev_part_release(c, S.vo);
    dev_part_release(c, S.thp);
    dev_part_release(c, S.wb);
    S.h_vp.clear(); S.h_pos.clear();
    dev_free(c, &S.d_wi); dev_free(c, &S.d_wd); dev_free(c, &S.d_tw); dev_free(c, &S.d_dz); dev_free(c, &S.d_head); dev_free(c, &S.d_pr);
    dev_free(c, &S.d_pack); dev_free(c, &S.d_saved); dev_free(c, &S.d_Dmat);
    dev_free(c, &S.d_cpos); dev_free(c, &S.d_cptr); dev_free(c, &S.d_cperf); dev_free(c, &S.d_save);
    S.h_wi.clear(); S.h_wd.clear();
    S.num = S.nperf = S.nd = 0;
    S.initialised = S.assembled = false;
    c->wells.num_wells = 0;   // no operator form of the list left behind for later products
}
// the controls in force, read back (the stream is idle)
int std_wells_controls_now(opmhip_ctx* c, std::vector<int>& control) {
    const StdWellsDev& S = c->wells.sw;
    std::vector<double> hc(S.num);
    OPMHIP_HIP(c, hipMemcpy(hc.data(), S.control(), hc.size() * sizeof(double), hipMemcpyDeviceToHost));
    control.resize(S.num);
    for (int w = 0; w < S.num; ++w) control[w] = (int)hc[w];
    return OPMHIP_SUCCESS;
}
// the targets, the modes and the RESV flags of H to the device arrays in force (the stream is idle)
int std_wells_group_targets_upload(opmhip_ctx* c, const StdWellsGroupsLists& H) {
    StdWellsDev& S = c->wells.sw;
    if (H.any_resv && !c->asmb.d_resv)
        if (int r = dev_alloc(c, &c->asmb.d_resv, (size_t)RESV_MAX_PARTS * 8 + RESV_OUT)) return r;
    std::vector<double> mode(H.mode.begin(), H.mode.end());
    OPMHIP_HIP(c, hipMemcpy(S.grp.d_target, H.target.data(), H.target.size() * sizeof(double), hipMemcpyHostToDevice));
    OPMHIP_HIP(c, hipMemcpy(S.grp.d_state, mode.data(), mode.size() * sizeof(double), hipMemcpyHostToDevice));
    OPMHIP_HIP(c, hipMemcpy(S.grp.d_resv, H.resv.data(), H.resv.size() * sizeof(int), hipMemcpyHostToDevice));
    OPMHIP_HIP(c, hipDeviceSynchronize());
    return OPMHIP_SUCCESS;
}
}  // namespace

// On the context's stream, in the order of the callers' other copies.  The well state of the last accepted step (x | control) and, under
// the well-bore head model, the perforation pressures and stored rates the next heads are formed from
int opmhip::std_wells_save_state(opmhip_ctx* c) {
    StdWellsDev& S = c->wells.sw;
    if (S.num > 0) OPMHIP_HIP(c, hipMemcpyAsync(S.d_saved, S.d_pack, (size_t)SW_SAVED * S.num * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (S.grp.on)   // the groups' modes and the NUPCOL rates go with the controls
        OPMHIP_HIP(c, hipMemcpyAsync(S.grp.d_saved, S.grp.d_state, ((size_t)S.grp.num + 3 * (size_t)S.num) * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (S.wb.on) {
        OPMHIP_HIP(c, hipMemcpyAsync(S.wb.d_saved, S.wb.d_state, (size_t)4 * S.nperf * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        S.wb.state_saved = S.wb.state_set;
        S.wb.initialised_saved = S.initialised;
    }
    return OPMHIP_SUCCESS;
}
int opmhip::std_wells_restore_state(opmhip_ctx* c) {
    StdWellsDev& S = c->wells.sw;
    if (S.num > 0) {
        OPMHIP_HIP(c, hipMemcpyAsync(S.d_pack, S.d_saved, (size_t)SW_SAVED * S.num * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        S.assembled = false;
    }
    if (S.grp.on)
        OPMHIP_HIP(c, hipMemcpyAsync(S.grp.d_state, S.grp.d_saved, ((size_t)S.grp.num + 3 * (size_t)S.num) * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (S.wb.on) {
        OPMHIP_HIP(c, hipMemcpyAsync(S.wb.d_state, S.wb.d_saved, (size_t)4 * S.nperf * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        S.wb.state_set = S.wb.state_saved;
        S.initialised = S.wb.initialised_saved;   // a first step given up: the retry takes the bottom-hole pressures from the cells again, as a run that never tried it
    }
    return OPMHIP_SUCCESS;
}

// The zero-pivot flags as the caller has just read them back, where the host waits for the stream anyway.  A singular D clears the list and is
// INVALID_ARGUMENT - the operator is never applied with a broken inverse.
int opmhip::std_wells_check(opmhip_ctx* c, const double* h) {
    StdWellsDev& S = c->wells.sw;
    for (int w = 0; w < S.num; ++w)
        if (h[w] != 0.0) {
            const int col = (int)h[w] - 1;
            std_wells_release(c);
            // (capi.py's HipModel._check knows a cleared list by the words "std_wells" and "the list is cleared" of this text: change both together)
            return fail(c, OPMHIP_INVALID_ARGUMENT, "std_wells: D of well %d is singular (no non-zero pivot in column %d of its elimination - a rate target on a component none of its "
                        "completions can flow?); the list is cleared", w, col);
        }
    return OPMHIP_SUCCESS;
}

extern "C" {

int opmhip_set_std_wells(opmhip_ctx* c, const opmhip_std_wells* sw) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        WellsDev& W = c->wells;
        StdWellsDev& S = W.sw;
        const Pattern& P = c->pat;
        if (!A.static_set) return fail(c, OPMHIP_NOT_READY, "set_std_wells before set_static");
        if (!A.state_set) return fail(c, OPMHIP_NOT_READY, "set_std_wells before set_state: the wells start from the reservoir state present");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        std_wells_release(c);   // whatever happens below, the old list is gone: a refused call leaves no list set
        if (!sw || sw->num_wells == 0) return OPMHIP_SUCCESS;
        if (c->comm.nranks > 1)
            return fail(c, OPMHIP_INVALID_ARGUMENT, "set_std_wells: decomposed context (%d ranks) - the per-well sums over the ranks are not built; hand the wells over as a host list (opmhip_wells.distributed)", c->comm.nranks);
        StdWellsLists H;
        std::string msg;
        if (int r = std_wells_lists(sw, P.Nb, P.toOrder.data(), H, msg)) return fail(c, r, "%s", msg.c_str());
        const int nw = sw->num_wells, np = sw->perf_pointers[nw];
        const int rc = [&]() -> int {
            int r;
            // WellsDev's arrays sized for the list: written by kernels from now on.  What they held of a host list is gone: the record of it
            // is emptied, so that a later host list is copied again
            if ((size_t)nw > W.cap_wells) {
                dev_free(c, &W.d_val_pointers); dev_free(c, &W.d_D); dev_free(c, &W.d_res); dev_free(c, &W.d_xw); dev_free(c, &W.d_bx);
                W.cap_wells = 0;
                if ((r = dev_alloc(c, &W.d_val_pointers, (size_t)nw + 1)) || (r = dev_alloc(c, &W.d_D, (size_t)nw * 16)) || (r = dev_alloc(c, &W.d_res, (size_t)nw * 4)) ||
                    (r = dev_alloc(c, &W.d_xw, (size_t)nw * 4)) || (r = dev_alloc(c, &W.d_bx, (size_t)nw * 4)))
                    return r;
                W.cap_wells = nw;
            }
            if ((size_t)np > W.cap_perf) {
                dev_free(c, &W.d_Ccols); dev_free(c, &W.d_Bcols); dev_free(c, &W.d_C); dev_free(c, &W.d_B);
                W.cap_perf = 0;
                if ((r = dev_alloc(c, &W.d_Ccols, (size_t)np)) || (r = dev_alloc(c, &W.d_Bcols, (size_t)np)) || (r = dev_alloc(c, &W.d_C, (size_t)np * 12)) ||
                    (r = dev_alloc(c, &W.d_B, (size_t)np * 12)))
                    return r;
                W.cap_perf = np;
            }
            W.h_vp.clear(); W.h_D.clear(); W.h_cc.clear(); W.h_bc.clear(); W.h_C.clear(); W.h_B.clear();
            OPMHIP_HIP(c, hipMemcpy(W.d_val_pointers, sw->perf_pointers, ((size_t)nw + 1) * sizeof(int), hipMemcpyHostToDevice));
            OPMHIP_HIP(c, hipMemcpy(W.d_Ccols, H.pos.data(), (size_t)np * sizeof(int), hipMemcpyHostToDevice));
            OPMHIP_HIP(c, hipMemcpy(W.d_Bcols, H.pos.data(), (size_t)np * sizeof(int), hipMemcpyHostToDevice));
            OPMHIP_HIP(c, hipMemset(W.d_D, 0, (size_t)nw * 16 * sizeof(double)));
            OPMHIP_HIP(c, hipMemset(W.d_B, 0, (size_t)np * 12 * sizeof(double)));
            OPMHIP_HIP(c, hipMemset(W.d_C, 0, (size_t)np * 12 * sizeof(double)));
            OPMHIP_HIP(c, hipMemset(W.d_xw, 0, (size_t)nw * 4 * sizeof(double)));
            const std::vector<double> tw(sw->tw, sw->tw + np), dz(sw->dz, sw->dz + np), zp((size_t)15 * np, 0.0), zw((size_t)16 * nw, 0.0);
            if ((r = dev_upload(c, &S.d_wi, H.wi)) || (r = dev_upload(c, &S.d_wd, H.wd)) || (r = dev_upload(c, &S.d_tw, tw)) || (r = dev_upload(c, &S.d_dz, dz)) ||
                (r = dev_upload(c, &S.d_head, std::vector<double>(np, 0.0))) || (r = dev_upload(c, &S.d_pr, zp)) || (r = dev_upload(c, &S.d_pack, H.pack)) ||
                (r = dev_upload(c, &S.d_saved, std::vector<double>((size_t)SW_SAVED * nw, 0.0))) || (r = dev_upload(c, &S.d_Dmat, zw)) || (r = dev_upload(c, &S.d_cpos, H.cpos)) ||
                (r = dev_upload(c, &S.d_cptr, H.cptr)) || (r = dev_upload(c, &S.d_cperf, H.cperf)) || (r = dev_alloc(c, &S.d_save, H.cpos.size() * 12)))
                return r;
            OPMHIP_HIP(c, hipMemcpy(S.d_saved, H.pack.data(), (size_t)SW_SAVED * nw * sizeof(double), hipMemcpyHostToDevice));
            OPMHIP_HIP(c, hipDeviceSynchronize());
            return OPMHIP_SUCCESS;
        }();
        if (rc) { std_wells_release(c); return rc; }
        S.num = nw; S.nperf = np; S.nd = (int)H.cpos.size();
        S.h_wi = std::move(H.wi); S.h_wd = std::move(H.wd);
        S.h_vp.assign(sw->perf_pointers, sw->perf_pointers + nw + 1);
        S.h_pos = std::move(H.pos);
        return OPMHIP_SUCCESS;
    });
}

int opmhip_std_wells_begin_iteration(opmhip_ctx* c, int iteration) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        StdWellsDev& S = c->wells.sw;
        if (S.num == 0) return OPMHIP_SUCCESS;
        if (iteration < 0) return fail(c, OPMHIP_INVALID_ARGUMENT, "std_wells_begin_iteration: iteration = %d", iteration);
        OPMHIP_HIP(c, hipSetDevice(c->device));
        if (iteration == 0) {   // calculateExplicitQuantities, prepareTimeStep
            if (S.wb.on) {   // computeWellConnectionPressures, from the well state the time step starts with
                launch_std_wells_wellbore(c, !S.initialised, !S.wb.state_set);
                S.wb.state_set = true;
            }
            if (S.lim.resv || S.grp.resv) launch_std_wells_resv(c);   // RateConverter::defineState and the coefficients, from the state the time step starts with
            if (S.grp.on) launch_std_wells_groups(c, 0, false);   // the group record the wells alone read, frozen through their solve
            launch_std_wells_solve(c, !S.initialised);
            S.initialised = true;
        }
        // the groups' check, then group data in one launch.  The reference's group data in FRONT of the check is elided: the check reads the present
        // rates only, and all that pass would leave - the NUPCOL copy under the same condition and the record - the data behind the check overwrites
        if (S.grp.on) launch_std_wells_groups(c, iteration, true);
        launch_std_wells_controls(c);   // updateWellControls: [every well's group check,] the individual checks
        if (S.grp.on) launch_std_wells_groups(c, iteration, false);   // group data: what the assembly reads
        OPMHIP_HIP(c, hipGetLastError());
        S.assembled = false;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_std_wells_apply_residual(opmhip_ctx* c) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        WellsDev& W = c->wells;
        if (W.sw.num == 0) return fail(c, OPMHIP_NOT_READY, "std_wells_apply_residual: no resident list (opmhip_set_std_wells)");
        if (!W.sw.assembled || !c->asmb.assembled) return fail(c, OPMHIP_NOT_READY, "std_wells_apply_residual before opmhip_assemble: there is no r_w");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        const StdWellsOperatorForm form(W);
        launch_wells_residual(c, W.sw.rw(), c->d_b);   // wellModel().apply(r): r -= C^T D^-1 r_w
        OPMHIP_HIP(c, hipGetLastError());
        return OPMHIP_SUCCESS;
    });
}

int opmhip_std_wells_update(opmhip_ctx* c, double relax) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        WellsDev& W = c->wells;
        if (W.sw.num == 0) return fail(c, OPMHIP_NOT_READY, "std_wells_update: no resident list (opmhip_set_std_wells)");
        if (!c->have_result) return fail(c, OPMHIP_NOT_READY, "std_wells_update before a solve");
        if (!W.sw.assembled) return fail(c, OPMHIP_NOT_READY, "std_wells_update before opmhip_assemble: there is no r_w");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        {
            const StdWellsOperatorForm form(W);
            const int rc = launch_wells_recover(c, W.sw.rw(), c->d_x, W.d_xw);   // x_w = D^-1 (r_w - B x)
            if (rc) return rc;
        }
        launch_std_wells_axpy(c, relax);
        OPMHIP_HIP(c, hipGetLastError());
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_std_wells_matrix_add(opmhip_ctx* c, int on) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        StdWellsDev& S = c->wells.sw;
        const Pattern& P = c->pat;
        if (S.num == 0) return fail(c, OPMHIP_NOT_READY, "set_std_wells_matrix_add: no resident list (opmhip_set_std_wells)");
        std::string msg;   // everything is looked at before anything changes: a refused call leaves the switch as it was
        if (int r = std_wells_matrix_add_check(on, msg)) return fail(c, r, "%s", msg.c_str());
        StdWellsMatrixAdd H;
        if (on)
            if (int r = std_wells_matrix_add_schedule(S.num, S.h_vp.data(), S.h_pos.data(), P.fromOrder.data(), P.rowptr.data(), P.col.data(), H, msg))
                return fail(c, r, "%s", msg.c_str());
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        SwMatrixAddDev N;
        if (on) {
            int r;
            if ((r = dev_upload(c, &N.d_target, H.target)) || (r = dev_upload(c, &N.d_tptr, H.tptr)) || (r = dev_upload(c, &N.d_contrib, H.contrib))) {
                dev_part_release(c, N);
                return r;
            }
            OPMHIP_HIP(c, hipDeviceSynchronize());
        }
        N.targets = (int)H.target.size(); N.pairs = H.pairs;
        N.h_target = std::move(H.target); N.h_tptr = std::move(H.tptr); N.h_contrib = std::move(H.contrib);
        N.on = on != 0;
        dev_part_install(c, S.ma, N);   // (in_matrix is a fact about the matrix: it stays until the next assemble)
        return OPMHIP_SUCCESS;
    });
}

int opmhip_std_wells_add_to_matrix(opmhip_ctx* c) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        StdWellsDev& S = c->wells.sw;
        if (S.num == 0) return fail(c, OPMHIP_NOT_READY, "std_wells_add_to_matrix: no resident list (opmhip_set_std_wells)");
        if (!S.ma.on) return fail(c, OPMHIP_NOT_READY, "std_wells_add_to_matrix: the list's matrix-add form is not switched on (opmhip_set_std_wells_matrix_add)");
        if (!S.assembled || !c->asmb.assembled) return fail(c, OPMHIP_NOT_READY, "std_wells_add_to_matrix before opmhip_assemble: there are no B, C and D^-1");
        if (S.in_matrix) return fail(c, OPMHIP_NOT_READY, "std_wells_add_to_matrix: the wells of the last opmhip_assemble are in the matrix already - a second call would subtract them twice");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        launch_std_wells_add_to_matrix(c);   // A -= C^T D^-1 B
        OPMHIP_HIP(c, hipGetLastError());
        c->factored = false;
        S.in_matrix = true;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_std_wells_matrix_add(opmhip_ctx* c, int info[4]) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        const StdWellsDev& S = c->wells.sw;
        if (!info) return fail(c, OPMHIP_INVALID_ARGUMENT, "get_std_wells_matrix_add: null array");
        info[0] = S.ma.on ? 1 : 0; info[1] = S.ma.targets; info[2] = S.ma.pairs; info[3] = S.in_matrix ? 1 : 0;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_std_wells(opmhip_ctx* c, double* x, int* control, double* res_well) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        StdWellsDev& S = c->wells.sw;
        if (S.num == 0) return OPMHIP_SUCCESS;
        OPMHIP_HIP(c, hipSetDevice(c->device));
        const size_t nw = S.num;
        std::vector<double> h(SW_PACK * nw);
        OPMHIP_HIP(c, hipMemcpyAsync(h.data(), S.d_pack, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        const int rc = std_wells_check(c, &h[SW_FLAG * nw]);
        if (rc) return rc;
        if (x) std::memcpy(x, &h[SW_X * nw], 4 * nw * sizeof(double));
        if (control)
            for (size_t w = 0; w < nw; ++w) control[w] = (int)h[SW_CONTROL * nw + w];   // 0 rate, 1 bhp, 2 thp, 3 .. 7 orat, wrat, grat, lrat, resv, 8 grup
        if (res_well) std::memcpy(res_well, &h[SW_RW * nw], 4 * nw * sizeof(double));
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_std_wells_state(opmhip_ctx* c, const double* x, const int* control, const double* rate_target) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        StdWellsDev& S = c->wells.sw;
        if (S.num == 0) return fail(c, OPMHIP_NOT_READY, "set_std_wells_state: no resident list (opmhip_set_std_wells)");
        const size_t nw = S.num;
        std::string msg;
        // control 8 (grup) exists with groups in force, for an available producer in a group; the other checks then see that well under 1
        std::vector<int> others;
        const int* const handed_in = control;
        if (control) {
            if (int r = std_wells_groups_check_controls(nw, control, S.h_wi.data(), S.grp.on ? S.grp.h.of.data() : nullptr, S.grp.on ? S.grp.h.available.data() : nullptr, msg))
                return fail(c, r, "%s", msg.c_str());
            if (S.grp.on) {
                others.assign(control, control + nw);
                for (size_t w = 0; w < nw; ++w)
                    if (others[w] == 8) others[w] = 1;
                control = others.data();
            }
        }
        if (S.lim.on) {   // controls 3 .. 7 exist, for the wells that have that limit
            if (int r = std_wells_limits_check_controls(nw, control, S.thp.on ? S.thp.h_table.data() : nullptr, S.lim.h_lim.data(), S.lim.h_use.data(), msg)) return fail(c, r, "%s", msg.c_str());
            if (int r = std_wells_check_state(nw, x, nullptr, rate_target, msg)) return fail(c, r, "%s", msg.c_str());
        } else if (S.thp.on) {   // control 2 exists, for the wells that have a limit; everything else is looked at as before
            if (int r = std_wells_thp_check_controls(nw, control, S.thp.h_table.data(), msg)) return fail(c, r, "%s", msg.c_str());
            if (int r = std_wells_check_state(nw, x, nullptr, rate_target, msg)) return fail(c, r, "%s", msg.c_str());
        } else if (int r = std_wells_check_state(nw, x, control, rate_target, msg)) return fail(c, r, "%s", msg.c_str());
        S.assembled = false;   // from here on the device state changes: nothing a refusal above could have left half done
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));   // rare: events and restarts
        if (x) OPMHIP_HIP(c, hipMemcpy(S.x(), x, 4 * nw * sizeof(double), hipMemcpyHostToDevice));
        if (control) {
            std::vector<double> h(nw);
            for (size_t w = 0; w < nw; ++w) h[w] = handed_in[w];
            OPMHIP_HIP(c, hipMemcpy(S.control(), h.data(), nw * sizeof(double), hipMemcpyHostToDevice));
        }
        if (rate_target) {
            for (size_t w = 0; w < nw; ++w) S.h_wd[2 * w] = rate_target[w];
            OPMHIP_HIP(c, hipMemcpy(S.d_wd, S.h_wd.data(), S.h_wd.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        OPMHIP_HIP(c, hipDeviceSynchronize());
        S.assembled = false;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_std_wells_blocks(opmhip_ctx* c, double* head, double* D, double* Dinv, double* B, double* C, double* rates, double* xw) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        const WellsDev& W = c->wells;
        const StdWellsDev& S = W.sw;
        if (S.num == 0) return OPMHIP_SUCCESS;
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        const size_t nw = S.num, np = S.nperf;
        if (head) OPMHIP_HIP(c, hipMemcpy(head, S.d_head, np * sizeof(double), hipMemcpyDeviceToHost));
        if (D) OPMHIP_HIP(c, hipMemcpy(D, S.d_Dmat, nw * 16 * sizeof(double), hipMemcpyDeviceToHost));
        if (Dinv) OPMHIP_HIP(c, hipMemcpy(Dinv, W.d_D, nw * 16 * sizeof(double), hipMemcpyDeviceToHost));
        if (B) OPMHIP_HIP(c, hipMemcpy(B, W.d_B, np * 12 * sizeof(double), hipMemcpyDeviceToHost));
        if (C) OPMHIP_HIP(c, hipMemcpy(C, W.d_C, np * 12 * sizeof(double), hipMemcpyDeviceToHost));
        if (rates) OPMHIP_HIP(c, hipMemcpy(rates, S.d_pr, np * 15 * sizeof(double), hipMemcpyDeviceToHost));
        if (xw) OPMHIP_HIP(c, hipMemcpy(xw, W.d_xw, nw * 4 * sizeof(double), hipMemcpyDeviceToHost));
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_std_wells_crossflow(opmhip_ctx* c, const int* allow) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        StdWellsDev& S = c->wells.sw;
        if (S.num == 0) return fail(c, OPMHIP_NOT_READY, "set_std_wells_crossflow: no resident list (opmhip_set_std_wells)");
        const size_t nw = S.num, np = S.nperf;
        bool any = false;
        std::string msg;   // everything is looked at before anything changes: a refused call leaves the flags as they were
        if (int r = std_wells_check_crossflow(nw, allow, S.h_wi.data(), any, msg)) return fail(c, r, "%s", msg.c_str());
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        SwCrossflowDev N;
        if (any) {
            int r;
            if ((r = dev_upload(c, &N.d_allow, std::vector<int>(allow, allow + nw))) || (r = dev_upload(c, &N.d_dq, std::vector<double>(9 * np, 0.0)))) {
                dev_part_release(c, N);
                return r;
            }
            OPMHIP_HIP(c, hipDeviceSynchronize());
        }
        N.on = any;
        dev_part_install(c, S.cf, N);
        S.assembled = false;   // the blocks of the last assembly are no longer the model's
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_std_wells_rate_dq(opmhip_ctx* c, double* dq) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        const StdWellsDev& S = c->wells.sw;
        if (S.num == 0 || !dq) return OPMHIP_SUCCESS;
        const size_t np = S.nperf;
        if (!S.cf.on) { std::memset(dq, 0, 9 * np * sizeof(double)); return OPMHIP_SUCCESS; }
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        OPMHIP_HIP(c, hipMemcpy(dq, S.cf.d_dq, 9 * np * sizeof(double), hipMemcpyDeviceToHost));
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_std_wells_vaporised_oil(opmhip_ctx* c, int on) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        StdWellsDev& S = c->wells.sw;
        if (S.num == 0) return fail(c, OPMHIP_NOT_READY, "set_std_wells_vaporised_oil: no resident list (opmhip_set_std_wells)");
        std::string msg;   // everything is looked at before anything changes: a refused call leaves the switch as it was
        if (int r = std_wells_check_vaporised_oil(on, c->asmb.wet_gas, msg)) return fail(c, r, "%s", msg.c_str());
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        SwVaporisedOilDev N;
        if (on) {
            if (int r = dev_upload(c, &N.d_sol, std::vector<double>(2 * (size_t)S.num, 0.0))) {
                dev_part_release(c, N);
                return r;
            }
            OPMHIP_HIP(c, hipDeviceSynchronize());
        }
        N.on = on != 0;
        dev_part_install(c, S.vo, N);
        S.assembled = false;   // the blocks of the last assembly are no longer the model's
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_std_wells_solution_rates(opmhip_ctx* c, double* dissolved_gas, double* vaporised_oil) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        const StdWellsDev& S = c->wells.sw;
        if (S.num == 0) return OPMHIP_SUCCESS;
        const size_t nw = S.num;
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        if (!S.vo.on) {   // the default model's kernels form neither
            if (dissolved_gas) std::memset(dissolved_gas, 0, nw * sizeof(double));
            if (vaporised_oil) std::memset(vaporised_oil, 0, nw * sizeof(double));
            return OPMHIP_SUCCESS;
        }
        if (dissolved_gas) OPMHIP_HIP(c, hipMemcpy(dissolved_gas, S.vo.d_sol, nw * sizeof(double), hipMemcpyDeviceToHost));
        if (vaporised_oil) OPMHIP_HIP(c, hipMemcpy(vaporised_oil, S.vo.d_sol + nw, nw * sizeof(double), hipMemcpyDeviceToHost));
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_std_wells_head_model(opmhip_ctx* c, const opmhip_std_wells_wellbore* wb) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        StdWellsDev& S = c->wells.sw;
        if (S.num == 0) return fail(c, OPMHIP_NOT_READY, "set_std_wells_head_model: no resident list (opmhip_set_std_wells)");
        const size_t nw = S.num, np = S.nperf;
        std::vector<int> pref;
        std::string msg;   // everything is looked at before anything changes: a refused call leaves the model as it was
        if (wb)
            if (int r = std_wells_head_model(wb, nw, np, S.h_wi.data(), pref, msg)) return fail(c, r, "%s", msg.c_str());
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        dev_part_release(c, S.wb);
        S.assembled = false;   // the heads the last assembly used are no longer the model's
        if (!wb) return OPMHIP_SUCCESS;
        const int rc = [&]() -> int {
            int r;
            const std::vector<double> depth(wb->perf_depth, wb->perf_depth + np), ref(wb->ref_depth, wb->ref_depth + nw);
            if ((r = dev_upload(c, &S.wb.d_depth, depth)) || (r = dev_upload(c, &S.wb.d_ref, ref)) || (r = dev_upload(c, &S.wb.d_pref, pref)) ||
                (r = dev_upload(c, &S.wb.d_state, std::vector<double>(4 * np, 0.0))) || (r = dev_upload(c, &S.wb.d_saved, std::vector<double>(4 * np, 0.0))) ||
                (r = dev_upload(c, &S.wb.d_out, std::vector<double>(5 * np, 0.0))) || (r = dev_upload(c, &S.wb.d_scratch, std::vector<double>(8 * np, 0.0))))
                return r;
            OPMHIP_HIP(c, hipDeviceSynchronize());
            return OPMHIP_SUCCESS;
        }();
        if (rc) { dev_part_release(c, S.wb); return rc; }
        S.wb.on = true;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_std_wells_wellbore(opmhip_ctx* c, double* density, double* p_avg, double* mixture, double* perf_pressure, double* perf_rates, int* perf_state_set) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        const StdWellsDev& S = c->wells.sw;
        if (perf_state_set) *perf_state_set = S.wb.on && S.wb.state_set ? 1 : 0;
        if (!S.wb.on) return OPMHIP_SUCCESS;
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        const size_t np = S.nperf;
        if (density) OPMHIP_HIP(c, hipMemcpy(density, S.wb.d_out, np * sizeof(double), hipMemcpyDeviceToHost));
        if (p_avg) OPMHIP_HIP(c, hipMemcpy(p_avg, S.wb.d_out + np, np * sizeof(double), hipMemcpyDeviceToHost));
        if (mixture) OPMHIP_HIP(c, hipMemcpy(mixture, S.wb.d_out + 2 * np, 3 * np * sizeof(double), hipMemcpyDeviceToHost));
        if (perf_pressure) OPMHIP_HIP(c, hipMemcpy(perf_pressure, S.wb.d_state, np * sizeof(double), hipMemcpyDeviceToHost));
        if (perf_rates) OPMHIP_HIP(c, hipMemcpy(perf_rates, S.wb.d_state + np, 3 * np * sizeof(double), hipMemcpyDeviceToHost));
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_std_wells_perf_state(opmhip_ctx* c, const double* perf_pressure, const double* perf_rates) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        StdWellsDev& S = c->wells.sw;
        if (!S.wb.on) return fail(c, OPMHIP_NOT_READY, "set_std_wells_perf_state: the well-bore head model is not in force (opmhip_set_std_wells_head_model)");
        const size_t np = S.nperf;
        if (!perf_pressure && !perf_rates) return OPMHIP_SUCCESS;   // nothing handed in: nothing changes, the pressures still come from the cells if they have not yet
        std::string msg;
        if (int r = std_wells_check_perf_state(np, perf_pressure, perf_rates, S.wb.state_set, msg)) return fail(c, r, "%s", msg.c_str());
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));   // rare: restarts
        if (perf_pressure) OPMHIP_HIP(c, hipMemcpy(S.wb.d_state, perf_pressure, np * sizeof(double), hipMemcpyHostToDevice));
        if (perf_rates) OPMHIP_HIP(c, hipMemcpy(S.wb.d_state + np, perf_rates, 3 * np * sizeof(double), hipMemcpyHostToDevice));
        else if (!S.wb.state_set) OPMHIP_HIP(c, hipMemset(S.wb.d_state + np, 0, 3 * np * sizeof(double)));
        OPMHIP_HIP(c, hipDeviceSynchronize());
        S.wb.state_set = true;
        return OPMHIP_SUCCESS;
    });
}

// ---- VFP tables, the THP limit of the resident wells ---------------------------------------------------------------------------------------
int opmhip_set_vfp_tables(opmhip_ctx* c, const opmhip_vfp_tables* tables) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        VfpDev& V = c->asmb.vfp;
        if (c->wells.sw.thp.on)
            return fail(c, OPMHIP_INVALID_ARGUMENT, "set_vfp_tables: the resident wells hold THP limits that name the tables in force; switch them off first (opmhip_set_std_wells_thp(NULL))");
        VfpPacked P;
        if (tables && tables->num_tables != 0) {   // everything is looked at before anything changes: a refused call leaves the previous set in force
            std::string msg;
            if (int r = vfp_pack(tables, P, msg)) return fail(c, r, "%s", msg.c_str());
        }
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        VfpDev N;
        if (P.num > 0) {
            int r;
            if ((r = dev_upload(c, &N.d_desc, P.desc)) || (r = dev_upload(c, &N.d_dbl, P.dbl))) {
                dev_part_release(c, N);
                return r;
            }
            OPMHIP_HIP(c, hipDeviceSynchronize());
        }
        N.h = std::move(P);
        dev_part_install(c, V, N);
        return OPMHIP_SUCCESS;
    });
}

int opmhip_vfp_probe(opmhip_ctx* c, int kind, int table_num, int n, const double* aqua, const double* liquid, const double* vapour, const double* thp,
                     const double* alq, const double* bhp_target, double* out) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        const VfpDev& V = c->asmb.vfp;
        if (V.h.num == 0) return fail(c, OPMHIP_NOT_READY, "vfp_probe before set_vfp_tables");
        const int table = vfp_find(V.h, kind, table_num);
        if (table < 0) return fail(c, OPMHIP_INVALID_ARGUMENT, "vfp_probe: there is no table %d of kind %d (0 VFPPROD, 1 VFPINJ)", table_num, kind);
        if (n < 0 || (n > 0 && (!aqua || !liquid || !vapour || !thp || !out || (kind == 0 && !alq)))) return fail(c, OPMHIP_INVALID_ARGUMENT, "vfp_probe: null array");
        if (n == 0) return OPMHIP_SUCCESS;
        OPMHIP_HIP(c, hipSetDevice(c->device));
        struct Scratch { double *in = nullptr, *out = nullptr; ~Scratch() { if (in) (void)hipFree(in); if (out) (void)hipFree(out); } } S;
        OPMHIP_HIP(c, hipMalloc((void**)&S.in, (size_t)6 * n * sizeof(double)));
        OPMHIP_HIP(c, hipMalloc((void**)&S.out, (size_t)10 * n * sizeof(double)));
        const double* src[6] = {aqua, liquid, vapour, thp, kind == 0 ? alq : nullptr, bhp_target};
        for (int k = 0; k < 6; ++k) {
            if (src[k]) OPMHIP_HIP(c, hipMemcpyAsync(S.in + (size_t)k * n, src[k], (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
            else OPMHIP_HIP(c, hipMemsetAsync(S.in + (size_t)k * n, 0, (size_t)n * sizeof(double), c->stream));
        }
        launch_vfp_probe(c, table, n, S.in, bhp_target != nullptr, S.out);
        OPMHIP_HIP(c, hipGetLastError());
        OPMHIP_HIP(c, hipMemcpyAsync(out, S.out, (size_t)10 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_std_wells_thp(opmhip_ctx* c, const opmhip_std_wells_thp* thp) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        StdWellsDev& S = c->wells.sw;
        const VfpDev& V = c->asmb.vfp;
        if (S.num == 0) return fail(c, OPMHIP_NOT_READY, "set_std_wells_thp: no resident list (opmhip_set_std_wells)");
        if (thp && V.h.num == 0) return fail(c, OPMHIP_NOT_READY, "set_std_wells_thp: no VFP tables (opmhip_set_vfp_tables)");
        const size_t nw = S.num;
        std::vector<int> table(nw, -1);
        std::vector<double> wd;
        bool any = false;
        std::string msg;   // everything is looked at before anything changes: a refused call leaves the previous values in force
        if (thp)
            if (int r = std_wells_thp_lists(thp, nw, S.h_wi.data(), V.h, table, wd, any, msg)) return fail(c, r, "%s", msg.c_str());
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        if (S.thp.on) {   // a well under THP control keeps its limit: the control row would have no table to read
            std::vector<double> ctl(nw);
            OPMHIP_HIP(c, hipMemcpy(ctl.data(), S.control(), nw * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t w = 0; w < nw; ++w)
                if (ctl[w] == 2.0 && table[w] < 0)
                    return fail(c, OPMHIP_INVALID_ARGUMENT, "set_std_wells_thp: well %zu is under THP control and would lose its limit; put it under another control first (opmhip_set_std_wells_state)", w);
        }
        SwThpDev N;
        if (any) {
            int r;
            if ((r = dev_upload(c, &N.d_table, table)) || (r = dev_upload(c, &N.d_wd, wd)) || (r = dev_upload(c, &N.d_out, std::vector<double>(3 * nw, 0.0)))) {
                dev_part_release(c, N);
                return r;
            }
            OPMHIP_HIP(c, hipDeviceSynchronize());
            N.h_table = std::move(table);
        }
        N.on = any;
        dev_part_install(c, S.thp, N);
        S.assembled = false;   // the control rows of the last assembly are no longer the model's
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_std_wells_thp(opmhip_ctx* c, double* thp, double* dp, double* bhp_from_thp) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        const StdWellsDev& S = c->wells.sw;
        if (S.num == 0) return OPMHIP_SUCCESS;
        const size_t nw = S.num;
        std::vector<double> h(3 * nw, 0.0);
        if (S.thp.on) {
            OPMHIP_HIP(c, hipSetDevice(c->device));
            OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
            OPMHIP_HIP(c, hipMemcpy(h.data(), S.thp.d_out, h.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t w = 0; w < nw; ++w)
                if (S.thp.h_table[w] < 0) h[w] = h[nw + w] = h[2 * nw + w] = 0.0;
        }
        if (thp) std::memcpy(thp, &h[0], nw * sizeof(double));
        if (dp) std::memcpy(dp, &h[nw], nw * sizeof(double));
        if (bhp_from_thp) std::memcpy(bhp_from_thp, &h[2 * nw], nw * sizeof(double));
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_std_wells_limits(opmhip_ctx* c, const opmhip_std_wells_limits* limits) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        StdWellsDev& S = c->wells.sw;
        if (S.num == 0) return fail(c, OPMHIP_NOT_READY, "set_std_wells_limits: no resident list (opmhip_set_std_wells)");
        const size_t nw = S.num;
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        std::vector<int> control;   // the controls in force: a limit a well is under control of stays
        if (int r = std_wells_controls_now(c, control)) return r;
        StdWellsLimitsLists H;
        std::string msg;   // everything is looked at before anything changes: a refused call leaves the previous values in force
        if (int r = std_wells_limits(limits, nw, S.h_wi.data(), control.data(), H, msg)) return fail(c, r, "%s", msg.c_str());
        SwLimitsDev N;
        if (H.any) {
            int r;
            if ((r = dev_upload(c, &N.d_lim, H.lim)) || (r = dev_upload(c, &N.d_use, H.use)) || (r = dev_upload(c, &N.d_out, std::vector<double>(4 * nw + 5, 0.0))) ||
                (H.any_resv && !c->asmb.d_resv && (r = dev_alloc(c, &c->asmb.d_resv, (size_t)RESV_MAX_PARTS * 8 + RESV_OUT)))) {
                dev_part_release(c, N);
                return r;
            }
            OPMHIP_HIP(c, hipDeviceSynchronize());
            N.h_lim = std::move(H.lim); N.h_use = std::move(H.use);
        }
        N.on = H.any; N.resv = H.any_resv;
        dev_part_install(c, S.lim, N);
        S.assembled = false;   // the blocks of the last assembly are no longer the model's
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_std_wells_resv(opmhip_ctx* c, double* averages, double* coeff, double* resv_current) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        const StdWellsDev& S = c->wells.sw;
        if (S.num == 0) return OPMHIP_SUCCESS;
        const size_t nw = S.num;
        std::vector<double> h(4 * nw + 5, 0.0);
        if (S.lim.on || S.grp.on) {   // (a list with groups and without limits keeps them in its own array)
            OPMHIP_HIP(c, hipSetDevice(c->device));
            OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
            OPMHIP_HIP(c, hipMemcpy(h.data(), S.lim.on ? S.lim.d_out : S.grp.d_out, h.size() * sizeof(double), hipMemcpyDeviceToHost));
        }
        if (averages) std::memcpy(averages, &h[4 * nw], 5 * sizeof(double));
        if (coeff) std::memcpy(coeff, &h[0], 3 * nw * sizeof(double));
        if (resv_current) std::memcpy(resv_current, &h[3 * nw], nw * sizeof(double));
        return OPMHIP_SUCCESS;
    });
}

// ---- group production control (include/opmhip.h: opmhip_set_std_wells_groups) ----

int opmhip_set_std_wells_groups(opmhip_ctx* c, const opmhip_std_wells_groups* groups) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        StdWellsDev& S = c->wells.sw;
        // (in front of the no-list check: a decomposed context can never hold a list, and the caller is told why)
        if (c->comm.nranks > 1)
            return fail(c, OPMHIP_INVALID_ARGUMENT, "set_std_wells_groups: decomposed context (%d ranks) - refused as the resident list itself is (opmhip_set_std_wells)", c->comm.nranks);
        if (S.num == 0) return fail(c, OPMHIP_NOT_READY, "set_std_wells_groups: no resident list (opmhip_set_std_wells)");
        const size_t nw = S.num;
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        std::vector<int> control;
        if (int r = std_wells_controls_now(c, control)) return r;
        StdWellsGroupsLists H;
        std::string msg;   // everything is looked at before anything changes: a refused call leaves the previous values in force
        if (int r = std_wells_groups(groups, nw, S.h_wi.data(), control.data(), H, msg)) return fail(c, r, "%s", msg.c_str());
        SwGroupsDev N;
        if (H.any) {
            const size_t ng = H.num_groups;
            std::vector<double> state(ng + 3 * nw, 0.0);
            for (size_t g = 0; g < ng; ++g) state[g] = H.mode[g];
            int r;
            if ((r = dev_upload(c, &N.d_ptr, H.ptr)) || (r = dev_upload(c, &N.d_idx, H.idx)) || (r = dev_upload(c, &N.d_of, H.of)) ||
                (r = dev_upload(c, &N.d_avail, H.available)) || (r = dev_upload(c, &N.d_resv, H.resv)) || (r = dev_upload(c, &N.d_guide, H.guide)) ||
                (r = dev_upload(c, &N.d_target, H.target)) || (r = dev_upload(c, &N.d_state, state)) || (r = dev_upload(c, &N.d_saved, state)) ||
                (r = dev_upload(c, &N.d_rec, std::vector<double>(8 * ng, 0.0))) || (r = dev_upload(c, &N.d_out, std::vector<double>(4 * nw + 5, 0.0))) ||
                (H.any_resv && !c->asmb.d_resv && (r = dev_alloc(c, &c->asmb.d_resv, (size_t)RESV_MAX_PARTS * 8 + RESV_OUT)))) {
                dev_part_release(c, N);
                return r;
            }
            OPMHIP_HIP(c, hipDeviceSynchronize());
        }
        N.on = H.any; N.resv = H.any_resv; N.num = H.num_groups; N.nupcol = H.nupcol;
        N.h = std::move(H);
        dev_part_install(c, S.grp, N);
        S.assembled = false;   // the blocks of the last assembly are no longer the model's
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_std_wells_guide_rates(opmhip_ctx* c, const double* guide_rate) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        StdWellsDev& S = c->wells.sw;
        if (S.num == 0 || !S.grp.on) return fail(c, OPMHIP_NOT_READY, "set_std_wells_guide_rates: no groups in force (opmhip_set_std_wells_groups)");
        std::string msg;
        if (int r = std_wells_groups_check_guide_rates(S.num, guide_rate, msg)) return fail(c, r, "%s", msg.c_str());
        S.assembled = false;
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        S.grp.h.guide.assign(guide_rate, guide_rate + 5 * (size_t)S.num);
        OPMHIP_HIP(c, hipMemcpy(S.grp.d_guide, guide_rate, 5 * (size_t)S.num * sizeof(double), hipMemcpyHostToDevice));
        OPMHIP_HIP(c, hipDeviceSynchronize());
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_std_wells_group_targets(opmhip_ctx* c, const double* oil_target, const double* water_target, const double* gas_target, const double* liquid_target,
                                       const double* resv_target, const int* mode) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        StdWellsDev& S = c->wells.sw;
        if (S.num == 0 || !S.grp.on) return fail(c, OPMHIP_NOT_READY, "set_std_wells_group_targets: no groups in force (opmhip_set_std_wells_groups)");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        // the modes in force are the device's: a group may have switched since they were handed in
        std::vector<double> now(S.grp.num);
        OPMHIP_HIP(c, hipMemcpy(now.data(), S.grp.d_state, now.size() * sizeof(double), hipMemcpyDeviceToHost));
        StdWellsGroupsLists cur = S.grp.h, H;
        for (int g = 0; g < S.grp.num; ++g) cur.mode[g] = (int)now[g];
        const double* arr[5] = {oil_target, water_target, gas_target, liquid_target, resv_target};
        std::string msg;
        if (int r = std_wells_group_targets(cur, S.num, arr, mode, H, msg)) return fail(c, r, "%s", msg.c_str());
        S.assembled = false;
        if (int r = std_wells_group_targets_upload(c, H)) return r;
        S.grp.resv = H.any_resv;
        S.grp.h = std::move(H);
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_std_wells_groups(opmhip_ctx* c, int* mode, double* rates, double* voidage, double* reduction, double* guide_sum, double* nupcol_rates) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        const StdWellsDev& S = c->wells.sw;
        if (S.num == 0 || !S.grp.on) return OPMHIP_SUCCESS;
        const size_t ng = S.grp.num, nw = S.num;
        std::vector<double> st(ng + 3 * nw), rec(8 * ng);
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipMemcpyAsync(st.data(), S.grp.d_state, st.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        OPMHIP_HIP(c, hipMemcpyAsync(rec.data(), S.grp.d_rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        for (size_t g = 0; g < ng; ++g) {
            if (mode) mode[g] = (int)st[g];
            if (voidage) voidage[g] = rec[8 * g + 3];
            if (guide_sum) guide_sum[g] = rec[8 * g + 7];
            for (int k = 0; k < 3; ++k) {
                if (rates) rates[3 * g + k] = rec[8 * g + k];
                if (reduction) reduction[3 * g + k] = rec[8 * g + 4 + k];
            }
        }
        if (nupcol_rates) std::memcpy(nupcol_rates, &st[ng], 3 * nw * sizeof(double));
        return OPMHIP_SUCCESS;
    });
}

}  // extern "C"
