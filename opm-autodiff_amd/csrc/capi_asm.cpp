// C-ABI, assembly half (include/opmhip.h "assembly" section): fluid tables, static grid data, state, linearisation,
// convergence norms, Newton update.  Host arrays arrive in the NATURAL cell / entry order and are permuted on upload.
#include <climits>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "asm_setup.hpp"
#include "capi_guard.hpp"
#include "fluid_tables.hpp"
#include "internal.hpp"

using namespace opmhip;

namespace {

// an array that lives from its first use on
template <class T>
int dev_ensure(opmhip_ctx* c, T** p, size_t count) {
    return *p ? OPMHIP_SUCCESS : dev_alloc(c, p, count);
}
// host-side permutation of a per-cell array natural -> internal
template <class T>
std::vector<T> cells_to_internal(const Pattern& P, const T* nat, int width = 1) {
    std::vector<T> v((size_t)P.Nloc * width);
    for (int p = 0; p < P.Nloc; ++p)
        for (int q = 0; q < width; ++q) v[(size_t)p * width + q] = nat[(size_t)P.fromOrder[p] * width + q];
    return v;
}
// a host array in the internal order to its device array, allocated with the first one
template <class T>
int upload_internal(opmhip_ctx* c, T** dst, const std::vector<T>& v) {
    if (int rc = dev_ensure(c, dst, v.size())) return rc;
    // the context's stream is non-blocking: an assembly enqueued earlier may still read this array
    OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
    OPMHIP_HIP(c, hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return OPMHIP_SUCCESS;
}
template <class T>
int upload_cells(opmhip_ctx* c, T** dst, const T* nat, int width = 1) {
    return upload_internal(c, dst, cells_to_internal(c->pat, nat, width));
}
int upload_entries(opmhip_ctx* c, double** dst, const double* nat) {
    const Pattern& P = c->pat;
    std::vector<double> v(P.nnzb);
    for (int k = 0; k < P.nnzb; ++k) v[k] = nat[P.nnzMap[k]];
    return upload_internal(c, dst, v);
}
// a per-cell array of the device (internal order) in the caller's natural order; none on the device: zeros.  out NULL: not asked for.
// The stream is idle
int download_cells(opmhip_ctx* c, const double* dev, double* out) {
    const Pattern& P = c->pat;
    if (!out) return OPMHIP_SUCCESS;
    if (!dev) { std::fill(out, out + P.Nloc, 0.0); return OPMHIP_SUCCESS; }
    std::vector<double> tmp(P.Nloc);
    OPMHIP_HIP(c, hipMemcpy(tmp.data(), dev, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int pos = 0; pos < P.Nloc; ++pos) out[P.fromOrder[pos]] = tmp[pos];
    return OPMHIP_SUCCESS;
}
// the cached intensive quantities follow what the call has changed; the host waits for them
int refresh_iq(opmhip_ctx* c) {
    launch_iq_update(c);
    OPMHIP_HIP(c, hipGetLastError());
    OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
    return OPMHIP_SUCCESS;
}
// A probe kernel on n points: the host arrays `in` (n doubles each) side by side in device scratch, `extra` doubles behind them for the
// launcher's own use, launch(d_in, d_out), width doubles per point back into `out`.  The scratch goes with the call
template <class F>
int run_probe(opmhip_ctx* c, int n, std::initializer_list<const double*> in, size_t extra, int width, double* out, F&& launch) {
    struct Scratch { double *in = nullptr, *out = nullptr; ~Scratch() { if (in) (void)hipFree(in); if (out) (void)hipFree(out); } } S;
    OPMHIP_HIP(c, hipMalloc((void**)&S.in, (in.size() * n + extra) * sizeof(double)));
    OPMHIP_HIP(c, hipMalloc((void**)&S.out, (size_t)width * n * sizeof(double)));
    size_t k = 0;
    for (const double* h : in) OPMHIP_HIP(c, hipMemcpyAsync(S.in + n * k++, h, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (int rc = launch(S.in, S.out)) return rc;
    OPMHIP_HIP(c, hipGetLastError());
    OPMHIP_HIP(c, hipMemcpyAsync(out, S.out, (size_t)width * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
    return OPMHIP_SUCCESS;
}
}  // namespace

int opmhip::stage_cell_positions(opmhip_ctx* c, const std::vector<int>& pos) {
    AsmDev& A = c->asmb;
    if (pos.size() > A.cell_pos_cap) {
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        dev_free(c, &A.d_cell_pos);
        A.cell_pos_cap = 0;
        const size_t cap = std::max<size_t>(256, 2 * pos.size());
        int rc = dev_alloc(c, &A.d_cell_pos, cap);
        if (rc) return rc;
        A.cell_pos_cap = cap;
    }
    OPMHIP_HIP(c, hipMemcpyAsync(A.d_cell_pos, pos.data(), pos.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    return OPMHIP_SUCCESS;
}

extern "C" {

int opmhip_set_fluid(opmhip_ctx* c, const opmhip_fluid* fluid) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        OPMHIP_HIP(c, hipSetDevice(c->device));
        AsmDev& A = c->asmb;
        // "setup, once": set_static sizes the intensive-quantity cache for THIS fluid's record layout and checks the region
        // arrays against ITS table counts - another fluid afterwards would let the 19-field kernels write past 17-field buffers
        if (A.static_set)
            return fail(c, OPMHIP_INVALID_ARGUMENT, "set_fluid: the static data of this context is already set (opmhip_set_static) - the fluid cannot be replaced any more");
        FluidTables T;
        const std::string msg = build_fluid_tables(fluid, T);
        if (!msg.empty()) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_fluid: %s", msg.c_str());
        int rc;
        if (A.fluid_set) {   // replaced before set_static: the old blobs go back (no kernel can be using them yet except a probe, which synchronises)
            OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
            dev_free(c, &A.d_tab_dbl);
            dev_free(c, &A.d_tab_idx);
        }
        if ((rc = dev_upload(c, &A.d_tab_dbl, T.dbl))) return rc;
        if ((rc = dev_upload(c, &A.d_tab_idx, T.idx))) return rc;
        A.tab_ndbl = (int)T.dbl.size();
        A.tab_nidx = (int)T.idx.size();
        A.rock_pref = T.rock_pref;
        A.rock_cr = T.rock_cr;
        A.num_pvt = T.num_pvt;
        A.num_sat = T.num_sat;
        A.num_rock = T.num_rock;
        A.rock_desc = T.rock_desc;
        A.wet_gas = T.wet_gas;
        A.pc_scaling = T.pc_scaling;
        A.ext = T.wet_gas || T.num_rock > 0 || T.pc_scaling;   // extended intensive-quantity record
        A.sat_eps.resize((size_t)T.num_sat * EPS_COUNT);
        for (int s = 0; s < T.num_sat; ++s) sat_end_points(T, s, &A.sat_eps[(size_t)s * EPS_COUNT]);
        A.fluid_set = true;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_static(opmhip_ctx* c, const double* trans, const double* area, const double* thpres, const double* poro,
                      const double* volume, const double* depth, const int* pvtnum, const int* satnum, const double* rsmax) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        if (!c->pattern_set) return fail(c, OPMHIP_NOT_READY, "set_static before set_pattern");
        if (!c->asmb.fluid_set) return fail(c, OPMHIP_NOT_READY, "set_static before set_fluid");
        if (!trans || !area || !poro || !volume || !depth) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_static: null array");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        const Pattern& P = c->pat;
        AsmDev& A = c->asmb;
        std::string msg;
        int rc;
        if ((rc = asm_static_check(P, A.num_pvt, A.num_sat, trans, area, thpres, poro, volume, pvtnum, satnum, msg))) return fail(c, rc, "%s", msg.c_str());
        if ((rc = upload_entries(c, &A.d_trans, trans))) return rc;
        if ((rc = upload_entries(c, &A.d_area, area))) return rc;
        if (thpres) { if ((rc = upload_entries(c, &A.d_thpres, thpres))) return rc; } else A.d_thpres = nullptr;
        if ((rc = upload_cells(c, &A.d_poro, poro))) return rc;
        if ((rc = upload_cells(c, &A.d_volume, volume))) return rc;
        if ((rc = upload_cells(c, &A.d_depth, depth))) return rc;
        if (pvtnum) { if ((rc = upload_cells(c, &A.d_pvtnum, pvtnum))) return rc; } else A.d_pvtnum = nullptr;
        if (satnum) { if ((rc = upload_cells(c, &A.d_satnum, satnum))) return rc; } else A.d_satnum = nullptr;
        // DRSDT in force (opmhip_set_composition_change_limits): the cap array belongs to the library - lastRs + rate * dt, written by
        // begin_time_step - and must neither be overwritten nor withdrawn here
        if (A.drsdt_on) {
            if (rsmax) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_static: rsmax handed in while DRSDT is in force (opmhip_set_composition_change_limits owns the dissolution cap)");
        } else if (rsmax) { if ((rc = upload_cells(c, &A.d_rsmax, rsmax))) return rc; }
        else { OPMHIP_HIP(c, hipStreamSynchronize(c->stream)); dev_free(c, &A.d_rsmax); }
        if (!A.d_pv) {
            const size_t Nb = P.Nloc, IQS = iq_doubles_per_cell(c);  // per-cell state includes the ghost cells
            if ((rc = dev_alloc(c, &A.d_pv, Nb * 3)) || (rc = dev_alloc(c, &A.d_iq, Nb * IQS)) || (rc = dev_alloc(c, &A.d_storageOld, Nb * 3)) ||
                (rc = dev_alloc(c, &A.d_invb, Nb * 3)) || (rc = dev_alloc(c, &A.d_drift, Nb * 3)) || (rc = dev_alloc(c, &A.d_source, Nb * 3)) ||
                (rc = dev_alloc(c, &A.d_dsource, Nb * 9)) || (rc = dev_alloc(c, &A.d_meaning, Nb)) || (rc = dev_alloc(c, &A.d_wasSwitched, Nb)) ||
                (rc = dev_alloc(c, &A.d_pv_prev, Nb * 3)) || (rc = dev_alloc(c, &A.d_meaning_prev, Nb)) || (rc = dev_alloc(c, &A.d_stage_u8, Nb)) ||
                (rc = dev_alloc(c, &A.d_nswitched, (size_t)1)) || (rc = dev_alloc(c, &A.d_conv_part, ((Nb + 255) / 256) * 10)) ||
                (rc = dev_alloc(c, &A.d_conv_out, (size_t)16)) || (rc = dev_alloc(c, &A.d_stage_cell, Nb * IQS)))
                return rc;
            OPMHIP_HIP(c, hipMemsetAsync(A.d_drift, 0, Nb * 3 * sizeof(double), c->stream));
            OPMHIP_HIP(c, hipMemsetAsync(A.d_source, 0, Nb * 3 * sizeof(double), c->stream));
            OPMHIP_HIP(c, hipMemsetAsync(A.d_dsource, 0, Nb * 9 * sizeof(double), c->stream));
            OPMHIP_HIP(c, hipMemsetAsync(A.d_storageOld, 0, Nb * 3 * sizeof(double), c->stream));
            OPMHIP_HIP(c, hipMemsetAsync(A.d_wasSwitched, 0, Nb, c->stream));
            OPMHIP_HIP(c, hipStreamSynchronize(c->stream));   // (fills on the context's stream, complete before anything else can reach these arrays: capi.cpp, alloc_system)
            // k_assemble's tiles, launch schedule and per-lane entry words (asm_setup.hpp)
            AsmPlan plan;
            if ((rc = asm_plan(P, asm_threads(), asm_max_rows(), plan, msg))) return fail(c, rc, "%s", msg.c_str());
            A.ntiles = plan.ntiles; A.nsched = plan.nsched; A.split_ok = plan.split_ok;
            if ((rc = dev_upload(c, &A.d_asm_sched, plan.sched)) || (rc = dev_upload(c, &A.d_asm_desc, plan.desc))) return rc;
        }
        A.static_set = true;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_problem_extras(opmhip_ctx* c, const double* rvmax, const int* rocknum, const double* overburden) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.static_set) return fail(c, OPMHIP_NOT_READY, "set_problem_extras before set_static");
        if ((rvmax || rocknum || overburden) && !A.ext)
            return fail(c, OPMHIP_INVALID_ARGUMENT, "set_problem_extras: the fluid has neither PVTG nor ROCKTAB tables - nothing these arrays could act on");
        int rockMax = -1;
        if (rocknum) {
            // tables: ROCKTAB of the fluid, else those of opmhip_set_water_compaction - which may still be to come (it needs the
            // state): then the indices are checked when it arrives
            const int limit = A.num_rock > 0 ? A.num_rock : (A.num_wc > 0 ? A.num_wc : INT_MAX);
            for (int i = 0; i < c->pat.Nloc; ++i) {
                if (rocknum[i] < 0 || rocknum[i] >= limit) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_problem_extras: rocknum[%d] out of range", i);
                rockMax = std::max(rockMax, rocknum[i]);
            }
        }
        A.h_rocknum_max = rockMax;
        OPMHIP_HIP(c, hipSetDevice(c->device));
        int rc;
        // an array that is withdrawn goes back to the allocator (an assembly enqueued earlier may still read it: sync first)
        if (!rvmax || !rocknum || !overburden) OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        // DRVDT in force: the cap array is the library's (lastRv + rate * dt); re-sending rocknum / overburden must leave it alone
        if (A.drvdt_on) {
            if (rvmax) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_problem_extras: rvmax handed in while DRVDT is in force (opmhip_set_composition_change_limits owns the vaporisation cap)");
        } else if (rvmax) { if ((rc = upload_cells(c, &A.d_rvmax, rvmax))) return rc; } else dev_free(c, &A.d_rvmax);
        if (rocknum) { if ((rc = upload_cells(c, &A.d_rocknum, rocknum))) return rc; } else dev_free(c, &A.d_rocknum);
        if (overburden) { if ((rc = upload_cells(c, &A.d_overburden, overburden))) return rc; } else dev_free(c, &A.d_overburden);
        return A.state_set ? refresh_iq(c) : OPMHIP_SUCCESS;   // the cached intensive quantities depend on these arrays
    });
}

int opmhip_set_pcw(opmhip_ctx* c, const double* pcw) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.static_set) return fail(c, OPMHIP_NOT_READY, "set_pcw before set_static");
        if (pcw && A.d_eps) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_pcw: opmhip_set_endpoint_scaling is in force - PCW is its points[OPMHIP_EPS_MAXPCOW]");
        if (pcw && !A.pc_scaling)
            return fail(c, OPMHIP_INVALID_ARGUMENT, "set_pcw: the fluid was set without pc_scaling - its capillary pressure curves have no per-cell end point");
        if (pcw)
            for (int i = 0; i < c->pat.Nloc; ++i)
                if (!std::isfinite(pcw[i])) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_pcw: pcw[%d] is not finite", i);
        OPMHIP_HIP(c, hipSetDevice(c->device));
        int rc;
        if (pcw) { if ((rc = upload_cells(c, &A.d_pcw, pcw))) return rc; }
        else if (A.d_pcw) {
            OPMHIP_HIP(c, hipStreamSynchronize(c->stream));   // an assembly enqueued earlier may still read it
            dev_free(c, &A.d_pcw);
        }
        return A.state_set ? refresh_iq(c) : OPMHIP_SUCCESS;   // the cached intensive quantities depend on it
    });
}

int opmhip_sat_end_points(opmhip_ctx* c, int sat_region, double* out) {
    if (!c || !out) return OPMHIP_INVALID_ARGUMENT;
    const AsmDev& A = c->asmb;
    if (!A.fluid_set) return fail(c, OPMHIP_NOT_READY, "sat_end_points before set_fluid");
    if (sat_region < 0 || sat_region >= A.num_sat) return fail(c, OPMHIP_INVALID_ARGUMENT, "sat_end_points: region out of range");
    for (int f = 0; f < EPS_COUNT; ++f) out[f] = A.sat_eps[(size_t)sat_region * EPS_COUNT + f];
    return OPMHIP_SUCCESS;
}

int opmhip_set_endpoint_scaling(opmhip_ctx* c, const opmhip_endpoint_scaling* e) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    static_assert((int)OPMHIP_EPS_COUNT == (int)EPS_COUNT, "public and internal end-point indices");
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        const Pattern& P = c->pat;
        if (!A.static_set) return fail(c, OPMHIP_NOT_READY, "set_endpoint_scaling before set_static");
        if (e && !A.pc_scaling)
            return fail(c, OPMHIP_INVALID_ARGUMENT, "set_endpoint_scaling: the fluid was set without pc_scaling - its saturation functions have no per-cell end points");
        if (e && A.d_pcw) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_endpoint_scaling: opmhip_set_pcw is in force - hand PCW in as points[OPMHIP_EPS_MAXPCOW] with pcw = 1 instead");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        if (!e) {
            if (A.d_eps) { OPMHIP_HIP(c, hipStreamSynchronize(c->stream)); dev_free(c, &A.d_eps); }
            A.epscfg = 0;
        } else {
            if (e->krw < 0 || e->krw > 2 || e->kro < 0 || e->kro > 2 || e->krg < 0 || e->krg > 2)
                return fail(c, OPMHIP_INVALID_ARGUMENT, "set_endpoint_scaling: krw / kro / krg must be 0, 1 or 2");
            const int N = P.Nloc;
            std::vector<int> satnum(N, 0);   // internal order, as on the device
            if (A.d_satnum) {
                OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
                OPMHIP_HIP(c, hipMemcpy(satnum.data(), A.d_satnum, (size_t)N * sizeof(int), hipMemcpyDeviceToHost));
            }
            // with hysteresis in force the imbibition curves are scaled by the same options: their points are checked again
            std::vector<int> imbnum;
            std::vector<double> imbpts;
            if (A.d_hyst) {
                imbnum.resize(N);
                OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
                OPMHIP_HIP(c, hipMemcpy(imbnum.data(), A.d_imbnum, (size_t)N * sizeof(int), hipMemcpyDeviceToHost));
                if (A.d_eps_imb) {
                    imbpts.resize((size_t)EPS_COUNT * N);
                    OPMHIP_HIP(c, hipMemcpy(imbpts.data(), A.d_eps_imb, imbpts.size() * sizeof(double), hipMemcpyDeviceToHost));
                }
            }
            std::vector<double> v((size_t)EPS_COUNT * N);   // field-major, internal order
            const double* imbsrc[EPS_COUNT];
            for (int f = 0; f < EPS_COUNT; ++f) imbsrc[f] = imbpts.empty() ? nullptr : &imbpts[(size_t)f * N];
            const int cfg = eps_config(*e);
            const EndPointsCheck drainage{"set_endpoint_scaling", "", e->points, A.sat_eps.data(), cfg, v.data(), (size_t)N};
            const EndPointsCheck imbibition{"set_endpoint_scaling", "imbibition ", imbsrc, A.sat_eps.data(), cfg, nullptr, (size_t)N};
            std::string msg;
            int rc;
            for (int pos = 0; pos < N; ++pos) {
                const int i = P.fromOrder[pos];   // natural id (ghost cells keep their place behind the owned ones)
                if ((rc = cell_end_points(drainage, i, i, satnum[pos], pos, msg))) return fail(c, rc, "%s", msg.c_str());
                if (A.d_hyst && (rc = cell_end_points(imbibition, pos, i, imbnum[pos], pos, msg))) return fail(c, rc, "%s", msg.c_str());
            }
            if ((rc = upload_internal(c, &A.d_eps, v))) return rc;
            A.epscfg = cfg;
        }
        return A.state_set ? refresh_iq(c) : OPMHIP_SUCCESS;   // the cached intensive quantities depend on it
    });
}

int opmhip_sat_probe(opmhip_ctx* c, int sat_region, const opmhip_endpoint_scaling* e, int n, const double* sw, const double* sg, double* out) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.fluid_set) return fail(c, OPMHIP_NOT_READY, "sat_probe before set_fluid");
        if (n < 0 || (n > 0 && (!sw || !sg || !out))) return fail(c, OPMHIP_INVALID_ARGUMENT, "sat_probe: null array");
        if (sat_region < 0 || sat_region >= A.num_sat) return fail(c, OPMHIP_INVALID_ARGUMENT, "sat_probe: region out of range");
        if (e && (e->krw < 0 || e->krw > 2 || e->kro < 0 || e->kro > 2 || e->krg < 0 || e->krg > 2))
            return fail(c, OPMHIP_INVALID_ARGUMENT, "sat_probe: krw / kro / krg must be 0, 1 or 2");
        if (n == 0) return OPMHIP_SUCCESS;
        OPMHIP_HIP(c, hipSetDevice(c->device));
        double pts[EPS_COUNT];
        int cfg = -1;
        if (e) {
            for (int f = 0; f < EPS_COUNT; ++f) pts[f] = e->points[f] ? e->points[f][0] : A.sat_eps[(size_t)sat_region * EPS_COUNT + f];
            cfg = eps_config(*e);
        }
        return run_probe(c, n, {sw, sg}, EPS_COUNT, 5, out, [&](double* d_in, double* d_out) -> int {   // the points ride behind the inputs
            double* d_eps = d_in + (size_t)2 * n;
            if (e) OPMHIP_HIP(c, hipMemcpyAsync(d_eps, pts, sizeof pts, hipMemcpyHostToDevice, c->stream));
            return launch_sat_probe(c, sat_region, cfg, d_eps, n, d_in, d_out);
        });
    });
}

int opmhip_fluid_probe(opmhip_ctx* c, int pvt_region, int sat_region, int n, const double* p, const double* rs, const double* sw,
                       const double* sg, double* out) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.fluid_set) return fail(c, OPMHIP_NOT_READY, "fluid_probe before set_fluid");
        if (n < 0 || (n > 0 && (!p || !rs || !sw || !sg || !out))) return fail(c, OPMHIP_INVALID_ARGUMENT, "fluid_probe: null array");
        if (pvt_region < 0 || pvt_region >= A.num_pvt || sat_region < 0 || sat_region >= A.num_sat)
            return fail(c, OPMHIP_INVALID_ARGUMENT, "fluid_probe: region out of range");
        if (n == 0) return OPMHIP_SUCCESS;
        OPMHIP_HIP(c, hipSetDevice(c->device));
        return run_probe(c, n, {p, rs, sw, sg}, 0, 8, out, [&](double* d_in, double* d_out) { return launch_fluid_probe(c, pvt_region, sat_region, n, d_in, d_out); });
    });
}

int opmhip_gas_probe(opmhip_ctx* c, int pvt_region, int n, const double* p, const double* rv, double* out) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.fluid_set) return fail(c, OPMHIP_NOT_READY, "gas_probe before set_fluid");
        if (n < 0 || (n > 0 && (!p || !rv || !out))) return fail(c, OPMHIP_INVALID_ARGUMENT, "gas_probe: null array");
        if (pvt_region < 0 || pvt_region >= A.num_pvt) return fail(c, OPMHIP_INVALID_ARGUMENT, "gas_probe: region out of range");
        if (n == 0) return OPMHIP_SUCCESS;
        OPMHIP_HIP(c, hipSetDevice(c->device));
        return run_probe(c, n, {p, rv}, 0, 3, out, [&](double* d_in, double* d_out) { return launch_gas_probe(c, pvt_region, n, d_in, d_out); });
    });
}

int opmhip_set_state(opmhip_ctx* c, const double* pv, const unsigned char* meaning) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        if (!c->asmb.static_set) return fail(c, OPMHIP_NOT_READY, "set_state before set_static");
        if (!pv || !meaning) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_state: null array");
        for (int i = 0; i < c->pat.Nloc; ++i)
            if (meaning[i] > (c->asmb.wet_gas ? OPMHIP_SW_PG_RV : OPMHIP_SW_PO_RS))
                return fail(c, OPMHIP_INVALID_ARGUMENT, "set_state: meaning[%d] = %d is not valid (Sw_po_Sg, Sw_po_Rs; Sw_pg_Rv only with a PVTG fluid)", i, (int)meaning[i]);
        OPMHIP_HIP(c, hipSetDevice(c->device));
        AsmDev& A = c->asmb;
        OPMHIP_HIP(c, hipMemcpyAsync(c->d_stageV, pv, (size_t)c->pat.Nloc * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        launch_vec_to_internal(c, c->d_stageV, A.d_pv, c->pat.Nloc);
        OPMHIP_HIP(c, hipMemcpyAsync(A.d_stage_u8, meaning, (size_t)c->pat.Nloc, hipMemcpyHostToDevice, c->stream));
        launch_u8_to_internal(c, A.d_stage_u8, A.d_meaning);
        OPMHIP_HIP(c, hipMemsetAsync(A.d_wasSwitched, 0, c->pat.Nloc, c->stream));
        if (int rc = refresh_iq(c)) return rc;
        A.state_set = true;
        A.prev_set = false;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_advance_time_level(opmhip_ctx* c) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.state_set) return fail(c, OPMHIP_NOT_READY, "advance_time_level before set_state");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        // ghost cells included: a later update_failed needs no communication
        OPMHIP_HIP(c, hipMemcpyAsync(A.d_pv_prev, A.d_pv, (size_t)c->pat.Nloc * 3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        OPMHIP_HIP(c, hipMemcpyAsync(A.d_meaning_prev, A.d_meaning, (size_t)c->pat.Nloc, hipMemcpyDeviceToDevice, c->stream));
        if (int rc = std_wells_save_state(c)) return rc;
        A.prev_set = true;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_relative_change(opmhip_ctx* c, double* relative_change) {
    if (!c || !relative_change) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.prev_set) return fail(c, OPMHIP_NOT_READY, "relative_change before advance_time_level: there is no old time level to compare with");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        int rc;
        if ((rc = dev_ensure(c, &A.d_rc, (size_t)2 * 256 + 2))) return rc;
        if ((rc = launch_relative_change(c))) return rc;
        double h[2];
        OPMHIP_HIP(c, hipMemcpyAsync(h, A.d_rc + 2 * 256, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        *relative_change = h[1] > 0.0 ? h[0] / h[1] : 0.0;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_update_failed(opmhip_ctx* c) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.prev_set) return fail(c, OPMHIP_NOT_READY, "update_failed before advance_time_level");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipMemcpyAsync(A.d_pv, A.d_pv_prev, (size_t)c->pat.Nloc * 3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        OPMHIP_HIP(c, hipMemcpyAsync(A.d_meaning, A.d_meaning_prev, (size_t)c->pat.Nloc, hipMemcpyDeviceToDevice, c->stream));
        OPMHIP_HIP(c, hipMemsetAsync(A.d_wasSwitched, 0, c->pat.Nloc, c->stream));
        launch_iq_update(c);
        OPMHIP_HIP(c, hipGetLastError());
        if (int rc = std_wells_restore_state(c)) return rc;
        A.assembled = false;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_composition_change_limits(opmhip_ctx* c, const double* drsdt, const int* drsdt_all, const double* drvdt) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.state_set) return fail(c, OPMHIP_NOT_READY, "set_composition_change_limits before set_state: lastRs / lastRv are taken from the initial solution");
        if (drvdt && !A.wet_gas) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_composition_change_limits: DRVDT needs a fluid with PVTG");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        const size_t N = c->pat.Nloc;
        int rc;
        auto put = [&](double** dst, const double* src) -> int {
            if ((rc = dev_ensure(c, dst, (size_t)A.num_pvt))) return rc;
            OPMHIP_HIP(c, hipMemcpy(*dst, src, (size_t)A.num_pvt * sizeof(double), hipMemcpyHostToDevice));
            return OPMHIP_SUCCESS;
        };
        A.drsdt_on = drsdt != nullptr;
        A.drvdt_on = drvdt != nullptr;
        if (drsdt) {
            if ((rc = put(&A.d_drsdt, drsdt))) return rc;
            std::vector<int> all(A.num_pvt, 0);
            if (drsdt_all) all.assign(drsdt_all, drsdt_all + A.num_pvt);
            if ((rc = dev_ensure(c, &A.d_drsdt_all, (size_t)A.num_pvt))) return rc;
            OPMHIP_HIP(c, hipMemcpy(A.d_drsdt_all, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice));
            if ((rc = dev_ensure(c, &A.d_lastRs, N))) return rc;
            if ((rc = dev_ensure(c, &A.d_rsmax, N))) return rc;
        } else if (A.d_lastRs) {   // the keyword went out of force: no cap any more
            dev_free(c, &A.d_lastRs);
            dev_free(c, &A.d_rsmax);
        }
        if (drvdt) {
            if ((rc = put(&A.d_drvdt, drvdt))) return rc;
            if ((rc = dev_ensure(c, &A.d_lastRv, N))) return rc;
            if ((rc = dev_ensure(c, &A.d_rvmax, N))) return rc;
        } else if (A.d_lastRv) {
            dev_free(c, &A.d_lastRv);
            dev_free(c, &A.d_rvmax);
        }
        A.storage_frozen = false;
        if (A.drsdt_on || A.drvdt_on) {
            launch_last_rs_rv(c);            // updateCompositionChangeLimits_ on the initial solution (eclproblem.hh:1811)
            launch_set_limits(c, 0.0);       // until the first begin_time_step: the caps of the state itself
        }
        return refresh_iq(c);
    });
}

int opmhip_set_irreversible_compaction(opmhip_ctx* c, int enable) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.state_set) return fail(c, OPMHIP_NOT_READY, "set_irreversible_compaction before set_state: the minimum pressure starts from the initial solution");
        if (enable && A.num_rock <= 0) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_irreversible_compaction: the fluid has no ROCKTAB tables");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        if (!enable) dev_free(c, &A.d_minpo);
        else {
            int rc;
            if ((rc = dev_ensure(c, &A.d_minpo, (size_t)c->pat.Nloc))) return rc;
            launch_min_pressure(c, true);
        }
        return refresh_iq(c);
    });
}

int opmhip_set_vappars(opmhip_ctx* c, int enable, double vap1, double vap2) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.state_set) return fail(c, OPMHIP_NOT_READY, "set_vappars before set_state: the maximum oil saturation starts from the initial solution");
        if (enable && !A.ext) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_vappars: needs a context with the extended record (a fluid with PVTG, ROCKTAB or pc_scaling)");
        if (enable && (!(vap1 >= 0.0) || !(vap2 >= 0.0))) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_vappars: the exponents must not be negative");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        if (!enable) dev_free(c, &A.d_maxso);
        else {
            int rc;
            if ((rc = dev_ensure(c, &A.d_maxso, (size_t)c->pat.Nloc))) return rc;
            A.vap1 = vap1; A.vap2 = vap2;
            launch_max_oil_saturation(c, true);
        }
        return refresh_iq(c);
    });
}

int opmhip_set_water_compaction(opmhip_ctx* c, int num_tables, const int* num_pressure, const int* num_sw, const double* pressure, const double* sw,
                                const double* pv_mult, const double* trans_mult) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.state_set) return fail(c, OPMHIP_NOT_READY, "set_water_compaction before set_state: the initial and the maximum water saturation start from the initial solution");
        if (num_tables < 0 || (num_tables > 0 && (!num_pressure || !num_sw || !pressure || !sw || !pv_mult)))
            return fail(c, OPMHIP_INVALID_ARGUMENT, "set_water_compaction: null table array");
        if (num_tables > 0 && !A.ext) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_water_compaction: needs a context with the extended record (a fluid with PVTG or pc_scaling)");
        if (num_tables > 0 && A.num_rock > 0) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_water_compaction: the fluid has ROCKTAB tables (the reference reads the one or the other)");
        WaterCompactionTables W;
        std::string msg;
        if (int r = water_compaction_tables(num_tables, num_pressure, num_sw, pressure, sw, pv_mult, trans_mult, W, msg)) return fail(c, r, "%s", msg.c_str());
        if (num_tables > 0 && A.h_rocknum_max >= num_tables) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_water_compaction: a cell's rock-table index is %d, %d tables given", A.h_rocknum_max, num_tables);
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        dev_free(c, &A.d_wcdesc); dev_free(c, &A.d_wcdata);
        if (num_tables == 0) { dev_free(c, &A.d_maxsw); dev_free(c, &A.d_sw0); }
        else {
            int rc;
            if ((rc = dev_upload(c, &A.d_wcdesc, W.desc)) || (rc = dev_upload(c, &A.d_wcdata, W.data))) return rc;
            if ((rc = dev_ensure(c, &A.d_maxsw, (size_t)c->pat.Nloc))) return rc;
            if ((rc = dev_ensure(c, &A.d_sw0, (size_t)c->pat.Nloc))) return rc;
            launch_max_water_saturation(c, true);
        }
        A.num_wc = num_tables;
        return refresh_iq(c);
    });
}

int opmhip_get_max_water_saturation(opmhip_ctx* c, double* max_sw) {
    if (!c || !max_sw) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.static_set) return fail(c, OPMHIP_NOT_READY, "get_max_water_saturation before set_static");
        if (A.d_maxsw) {
            OPMHIP_HIP(c, hipSetDevice(c->device));
            OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        }
        return download_cells(c, A.d_maxsw, max_sw);
    });
}

int opmhip_begin_time_step(opmhip_ctx* c, double dt) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!(dt > 0.0)) return fail(c, OPMHIP_INVALID_ARGUMENT, "begin_time_step: dt must be positive");
        const bool limits = A.drsdt_on || A.drvdt_on;
        if ((A.drsdt_on && (!A.d_rsmax || !A.d_lastRs)) || (A.drvdt_on && (!A.d_rvmax || !A.d_lastRv)))
            return fail(c, OPMHIP_UNKNOWN_ERROR, "begin_time_step: DRSDT / DRVDT is in force but its cap array is gone (internal error)");
        if (!limits && !A.d_minpo && !A.d_maxso && !A.d_maxsw && !A.d_hyst) return OPMHIP_SUCCESS;
        if (!A.state_set) return fail(c, OPMHIP_NOT_READY, "begin_time_step before set_state");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        if (A.d_maxsw) launch_max_water_saturation(c, false);   // updateMaxWaterSaturation_ (eclproblem.hh:1056)
        if (A.d_minpo) launch_min_pressure(c, false);     // updateMinPressure_: from the intensive quantities of the state as it is
        if (A.d_hyst) launch_hyst_update(c);              // updateHysteresis_ (eclproblem.hh:1060, 2603-2626)
        if (A.d_maxso) launch_max_oil_saturation(c, false);   // updateMaxOilSaturation_
        A.storage_frozen = false;
        if (limits) {
            launch_set_limits(c, 0.0);                    // time index 1: lastRs / lastRv without the increment
            launch_iq_update(c);
            launch_storage_old(c);
            A.storage_frozen = true;
            launch_set_limits(c, dt);                     // time index 0: + DRSDT * dt
        }
        launch_iq_update(c);
        OPMHIP_HIP(c, hipGetLastError());
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_hysteresis(opmhip_ctx* c, int kr_model, const int* imbnum, const opmhip_endpoint_scaling* imb) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        const Pattern& P = c->pat;
        if (!A.static_set) return fail(c, OPMHIP_NOT_READY, "set_hysteresis before set_static");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        const int N = P.Nloc;
        if (kr_model < 0) {   // the keyword is not in force
            A.hyst_model = -1;
            dev_free(c, &A.d_hyst);
            dev_free(c, &A.d_imbnum);
            dev_free(c, &A.d_eps_imb);
        } else {
            if (kr_model > 1) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_hysteresis: EHYSTR item 2 = %d - only the Carlson models 0 and 1 are supported (as in the reference, PartiallySupportedFlowKeywords.cpp:301)", kr_model);
            if (!A.ext) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_hysteresis: needs a context with the extended record (a fluid with PVTG, ROCKTAB or pc_scaling)");
            if (!imbnum) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_hysteresis: imbnum is NULL");
            if (imb && !A.d_eps) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_hysteresis: scaled end points of the imbibition curves without opmhip_set_endpoint_scaling in force");
            for (int i = 0; i < N; ++i)
                if (imbnum[i] < 0 || imbnum[i] >= A.num_sat) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_hysteresis: imbnum[%d] out of range", i);
            int rc;
            // every refusal comes before the first upload: a refused call leaves the previous settings in force
            std::vector<double> v(imb ? (size_t)EPS_COUNT * N : 0);   // field-major, internal order
            if (A.d_eps) {   // the imbibition curves are scaled by the options of opmhip_set_endpoint_scaling: the same checks
                const EndPointsCheck K{"set_hysteresis", "imbibition ", imb ? imb->points : nullptr, A.sat_eps.data(), A.epscfg, imb ? v.data() : nullptr, (size_t)N};
                std::string msg;
                for (int pos = 0; pos < N; ++pos) {
                    const int i = P.fromOrder[pos];
                    if ((rc = cell_end_points(K, i, i, imbnum[i], pos, msg))) return fail(c, rc, "%s", msg.c_str());
                }
            }
            if ((rc = upload_cells(c, &A.d_imbnum, imbnum))) return rc;
            if (imb) { if ((rc = upload_internal(c, &A.d_eps_imb, v))) return rc; }
            else dev_free(c, &A.d_eps_imb);
            // "nothing seen yet": turning points 2, shifts 0 - the first begin_time_step sets them (or opmhip_set_hysteresis_params)
            std::vector<double> h((size_t)4 * N, 0.0);
            for (int q = 0; q < N; ++q) h[q] = h[(size_t)2 * N + q] = 2.0;
            if ((rc = upload_internal(c, &A.d_hyst, h))) return rc;
            A.hyst_model = kr_model;
        }
        return A.state_set ? refresh_iq(c) : OPMHIP_SUCCESS;
    });
}

int opmhip_get_hysteresis(opmhip_ctx* c, double* sw_ow, double* delta_ow, double* sw_go, double* delta_go) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.d_hyst) return fail(c, OPMHIP_NOT_READY, "get_hysteresis: opmhip_set_hysteresis is not in force");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        double* out[4] = {sw_ow, delta_ow, sw_go, delta_go};   // d_hyst is [4][Nloc]
        for (int f = 0; f < 4; ++f)
            if (int rc = download_cells(c, A.d_hyst + (size_t)f * c->pat.Nloc, out[f])) return rc;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_hysteresis_params(opmhip_ctx* c, const double* sw_ow, const double* sw_go) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.d_hyst) return fail(c, OPMHIP_NOT_READY, "set_hysteresis_params: opmhip_set_hysteresis is not in force");
        if (!sw_ow || !sw_go) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_hysteresis_params: null array");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));   // the staging area may still be read by an earlier download
        const size_t N = c->pat.Nloc;
        const std::vector<double> a = cells_to_internal(c->pat, sw_ow), b = cells_to_internal(c->pat, sw_go);
        OPMHIP_HIP(c, hipMemcpy(A.d_stage_cell, a.data(), N * sizeof(double), hipMemcpyHostToDevice));   // staged as [2][Nloc]
        OPMHIP_HIP(c, hipMemcpy(A.d_stage_cell + N, b.data(), N * sizeof(double), hipMemcpyHostToDevice));
        launch_hyst_update(c, A.d_stage_cell, A.d_stage_cell + N);
        if (A.state_set) launch_iq_update(c);
        OPMHIP_HIP(c, hipGetLastError());
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_trackers(opmhip_ctx* c, double* last_rs, double* last_rv, double* min_po, double* max_so) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.static_set) return fail(c, OPMHIP_NOT_READY, "get_trackers before set_static");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        int rc;
        if ((rc = download_cells(c, A.d_lastRs, last_rs)) || (rc = download_cells(c, A.d_lastRv, last_rv)) || (rc = download_cells(c, A.d_minpo, min_po)) ||
            (rc = download_cells(c, A.d_maxso, max_so)))
            return rc;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_end_time_step(opmhip_ctx* c, double dt) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.assembled) return fail(c, OPMHIP_NOT_READY, "end_time_step before assemble: no residual of an accepted step on the device");
        if (!(dt > 0.0)) return fail(c, OPMHIP_INVALID_ARGUMENT, "end_time_step: dt must be positive");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        if (A.drsdt_on || A.drvdt_on) launch_last_rs_rv(c);   // updateCompositionChangeLimits_ (eclproblem.hh:1125)
        A.storage_frozen = false;
        if (A.aq.num > 0) {   // aquiferModel_.endTimeStep (eclproblem.hh:1101-1135 -> BlackoilAquiferModel_impl.hpp)
            launch_aquifer_end(c, dt);
            OPMHIP_HIP(c, hipGetLastError());
        }
        if (!A.drift_enabled) return OPMHIP_SUCCESS;
        launch_drift_update(c, dt);
        OPMHIP_HIP(c, hipGetLastError());
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_drift_compensation(opmhip_ctx* c, int enable, double max_compensation) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        if (enable && !(max_compensation > 0.0)) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_drift_compensation: max_compensation must be positive");
        c->asmb.drift_enabled = enable != 0;
        if (enable) c->asmb.max_compensation = max_compensation;
        if (c->asmb.d_drift) {   // switching it on or off starts from a clean slate, like a fresh EclProblem
            OPMHIP_HIP(c, hipSetDevice(c->device));
            OPMHIP_HIP(c, hipMemsetAsync(c->asmb.d_drift, 0, (size_t)c->pat.Nloc * 3 * sizeof(double), c->stream));
        }
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_state(opmhip_ctx* c, double* pv, unsigned char* meaning) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        if (!c->asmb.state_set) return fail(c, OPMHIP_NOT_READY, "get_state before set_state");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        AsmDev& A = c->asmb;
        if (pv) {
            launch_vec_to_natural(c, A.d_pv, c->d_stageV, c->pat.Nloc);
            OPMHIP_HIP(c, hipMemcpyAsync(pv, c->d_stageV, (size_t)c->pat.Nloc * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        if (meaning) {
            launch_u8_to_natural(c, A.d_meaning, A.d_stage_u8);
            OPMHIP_HIP(c, hipMemcpyAsync(meaning, A.d_stage_u8, (size_t)c->pat.Nloc, hipMemcpyDeviceToHost, c->stream));
        }
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_source(opmhip_ctx* c, const double* source, const double* dsource) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        if (!c->asmb.static_set) return fail(c, OPMHIP_NOT_READY, "set_source before set_static");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        AsmDev& A = c->asmb;
        const size_t Nb = c->pat.Nloc;
        int rc;
        if (source) { if ((rc = upload_cells(c, &A.d_source, source, 3))) return rc; }
        else OPMHIP_HIP(c, hipMemsetAsync(A.d_source, 0, Nb * 3 * sizeof(double), c->stream));
        if (dsource) { if ((rc = upload_cells(c, &A.d_dsource, dsource, 9))) return rc; }
        else OPMHIP_HIP(c, hipMemsetAsync(A.d_dsource, 0, Nb * 9 * sizeof(double), c->stream));
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_source_cells(opmhip_ctx* c, int n, const int* cells, const double* source, const double* dsource) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        if (!c->asmb.static_set) return fail(c, OPMHIP_NOT_READY, "set_source_cells before set_static");
        if (n < 0 || (n > 0 && (!cells || !source))) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_source_cells: n = %d, cells / source missing", n);
        OPMHIP_HIP(c, hipSetDevice(c->device));
        AsmDev& A = c->asmb;
        const Pattern& P = c->pat;
        SourceCells S;
        std::string msg;
        if (int r = source_cells(n, cells, source, dsource, P.Nloc, P.toOrder.data(), S, msg)) return fail(c, r, "%s", msg.c_str());
        const size_t Nloc = P.Nloc, m = S.pos.size();
        OPMHIP_HIP(c, hipMemsetAsync(A.d_source, 0, Nloc * 3 * sizeof(double), c->stream));   // behind whatever assembly still reads them: same stream
        OPMHIP_HIP(c, hipMemsetAsync(A.d_dsource, 0, Nloc * 9 * sizeof(double), c->stream));
        if (m == 0) return OPMHIP_SUCCESS;
        return with_cell_positions(c, "set_source_cells", S.pos, [&]() -> int {
            // values staged in d_stage_cell (Nloc * IQS doubles >= 12 per distinct cell)
            OPMHIP_HIP(c, hipMemcpyAsync(A.d_stage_cell, S.val.data(), m * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
            OPMHIP_HIP(c, hipMemcpyAsync(A.d_stage_cell + m * 3, S.dval.data(), m * 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
            launch_source_scatter(c, (int)m, A.d_cell_pos, A.d_stage_cell, A.d_stage_cell + m * 3);
            OPMHIP_HIP(c, hipGetLastError());
            return OPMHIP_SUCCESS;
        });
    });
}

int opmhip_assemble(opmhip_ctx* c, double dt, int iteration, double* jac, double* residual) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        if (!c->asmb.state_set) return fail(c, OPMHIP_NOT_READY, "assemble before set_state");
        if (!(dt > 0.0) || iteration < 0) return fail(c, OPMHIP_INVALID_ARGUMENT, "assemble: dt must be positive, iteration >= 0");
        const AquifersDev& Q = c->asmb.aq;
        StdWellsDev& SW = c->wells.sw;
        if (Q.num > 0 && !Q.stepped) return fail(c, OPMHIP_NOT_READY, "assemble: aquifers are set but opmhip_aquifers_begin_time_step was not called");
        if (Q.num > 0 && dt != Q.step_dt) return fail(c, OPMHIP_INVALID_ARGUMENT, "assemble: dt = %.17g, the aquifers' time step was begun with dt = %.17g", dt, Q.step_dt);
        const BoundaryDev& BC = c->asmb.bc;
        if (BC.nf > 0 && ((BC.nfc > 0 && c->asmb.hyst_model >= 0) || c->asmb.d_maxsw))
            return fail(c, OPMHIP_INVALID_ARGUMENT, "assemble: hysteresis or water-induced compaction was set behind opmhip_set_boundary_conditions, which refuses them");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        c->asmb.last_dt = dt;
        c->asmb.last_iteration = iteration;
        SW.in_matrix = false;   // a new Jacobian: the matrix-add form's wells are not in it yet
        if (SW.num > 0) { launch_std_wells_assemble(c); SW.assembled = true; }   // wellModel().assemble: rates first, then the aquifers (the host order)
        if (Q.nd > 0) launch_aquifer_apply(c);     // aquiferModel_.addToSource (ebos/eclproblem.hh:1843)
        if (BC.nd > 0) launch_boundary_apply(c);   // EclProblem::boundary (ebos/eclproblem.hh:1602-1671): the faces' rates out of the boundary cells' source
        launch_assemble(c, dt, iteration);
        if (BC.nd > 0) launch_boundary_restore(c); // innermost: the save areas nest
        if (Q.nd > 0) launch_aquifer_restore(c);   // the caller's source arrays as the caller left them
        if (SW.num > 0) launch_std_wells_restore(c);
        OPMHIP_HIP(c, hipGetLastError());
        c->system_loaded = true;
        c->factored = false;
        c->asmb.assembled = true;
        if (jac) {
            ensure_A(c);
            launch_unpermute_blocks(c, c->d_A, c->d_stageA);
            OPMHIP_HIP(c, hipMemcpyAsync(jac, c->d_stageA, (size_t)c->pat.nnzb * BB * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        if (residual) {
            launch_vec_to_natural(c, c->d_b, c->d_stageV);
            OPMHIP_HIP(c, hipMemcpyAsync(residual, c->d_stageV, (size_t)c->pat.Nb * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        if (jac || residual) OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        return OPMHIP_SUCCESS;
    });
}

int opmhip_iq_fields(opmhip_ctx* c) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return iq_doubles_per_cell(c) / 4;
}

int opmhip_get_iq(opmhip_ctx* c, double* out) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        if (!c->asmb.state_set) return fail(c, OPMHIP_NOT_READY, "get_iq before set_state");
        if (!out) return fail(c, OPMHIP_INVALID_ARGUMENT, "get_iq: out == NULL");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        launch_iq_to_natural(c, c->asmb.d_stage_cell);
        OPMHIP_HIP(c, hipMemcpyAsync(out, c->asmb.d_stage_cell, (size_t)c->pat.Nloc * iq_doubles_per_cell(c) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_iq_cells(opmhip_ctx* c, int n, const int* cells, double* out) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        if (!c->asmb.state_set) return fail(c, OPMHIP_NOT_READY, "get_iq_cells before set_state");
        if (n < 0 || (n > 0 && (!cells || !out))) return fail(c, OPMHIP_INVALID_ARGUMENT, "get_iq_cells: n = %d, cells / out missing", n);
        if (n == 0) return OPMHIP_SUCCESS;
        const Pattern& P = c->pat;
        if (n > P.Nloc) return fail(c, OPMHIP_INVALID_ARGUMENT, "get_iq_cells: %d cells asked for, the grid has %d (opmhip_get_iq copies them all)", n, P.Nloc);
        std::vector<int> pos(n);
        for (int i = 0; i < n; ++i) {
            if (cells[i] < 0 || cells[i] >= P.Nloc) return fail(c, OPMHIP_INVALID_ARGUMENT, "get_iq_cells: cell %d of %d", cells[i], P.Nloc);
            pos[i] = P.toOrder[cells[i]];
        }
        OPMHIP_HIP(c, hipSetDevice(c->device));
        return with_cell_positions(c, "get_iq_cells", pos, [&]() -> int {
            launch_iq_gather(c, n, c->asmb.d_cell_pos, c->asmb.d_stage_cell);
            OPMHIP_HIP(c, hipGetLastError());
            OPMHIP_HIP(c, hipMemcpyAsync(out, c->asmb.d_stage_cell, (size_t)n * iq_doubles_per_cell(c) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            return OPMHIP_SUCCESS;
        });
    });
}

int opmhip_convergence(opmhip_ctx* c, double dt, double tol_cnv, double* out) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        if (!c->asmb.assembled) return fail(c, OPMHIP_NOT_READY, "convergence before assemble");
        if (!out) return fail(c, OPMHIP_INVALID_ARGUMENT, "convergence: out == NULL");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        const int rcc = launch_convergence(c, dt, tol_cnv);
        if (rcc) return rcc;
        OPMHIP_HIP(c, hipGetLastError());
        double h[16];
        OPMHIP_HIP(c, hipMemcpyAsync(h, c->asmb.d_conv_out, 11 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < 11; ++i) out[i] = h[i];
        // CNV_c = B_avg dt maxCoeff ; MB_c = |B_avg R_sum| dt / pvSum   (flow/BlackoilModelEbos.hpp:797-801)
        for (int e = 0; e < 3; ++e) {
            out[11 + e] = h[6 + e] * dt * h[3 + e];
            out[14 + e] = std::fabs(h[6 + e] * h[e]) * dt / h[9];
        }
        return OPMHIP_SUCCESS;
    });
}

int opmhip_reservoir_averages(opmhip_ctx* c, double* out) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        AsmDev& A = c->asmb;
        if (!A.state_set) return fail(c, OPMHIP_NOT_READY, "reservoir_averages before set_state");
        if (!out) return fail(c, OPMHIP_INVALID_ARGUMENT, "reservoir_averages: out == NULL");
        if (c->comm.nranks > 1 || c->pat.Nghost > 0)
            return fail(c, OPMHIP_INVALID_ARGUMENT, "reservoir_averages: a decomposed context (the sums over the ranks are not formed)");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        int rc;
        if ((rc = dev_ensure(c, &A.d_resv, (size_t)RESV_MAX_PARTS * 8 + RESV_OUT))) return rc;
        launch_reservoir_averages(c);
        OPMHIP_HIP(c, hipGetLastError());
        double h[RESV_OUT];
        OPMHIP_HIP(c, hipMemcpyAsync(h, A.d_resv + (size_t)RESV_MAX_PARTS * 8, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        if (!(h[5] > 0.0)) return fail(c, OPMHIP_INVALID_ARGUMENT, "reservoir_averages: the field's pore volume is %.17g, not > 0", h[5]);
        for (int i = 0; i < 5; ++i) out[i] = h[i];
        return OPMHIP_SUCCESS;
    });
}

int opmhip_update(opmhip_ctx* c, const double* dx, double relax, int* num_switched) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        if (!c->asmb.state_set) return fail(c, OPMHIP_NOT_READY, "update before set_state");
        if (!dx && !c->have_result) return fail(c, OPMHIP_NOT_READY, "update: dx == NULL but no solve result is resident");
        OPMHIP_HIP(c, hipSetDevice(c->device));
        const double* d_dx = c->d_x;
        if (dx) {
            OPMHIP_HIP(c, hipMemcpyAsync(c->d_stageV, dx, (size_t)c->pat.Nb * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
            launch_vec_to_internal(c, c->d_stageV, c->d_t);
            d_dx = c->d_t;
        }
        launch_newton_update(c, d_dx, relax);
        int rcg = launch_ghost_refresh(c);
        if (rcg) return rcg;
        OPMHIP_HIP(c, hipGetLastError());
        if (num_switched) {
            OPMHIP_HIP(c, hipMemcpyAsync(num_switched, c->asmb.d_nswitched, sizeof(int), hipMemcpyDeviceToHost, c->stream));
            OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        }
        return OPMHIP_SUCCESS;
    });
}

}  // extern "C"
