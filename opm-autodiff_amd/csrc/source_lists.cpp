// Host set-up of the resident standard wells and analytic aquifers (source_lists.hpp).  No HIP call: capi_std_wells.cpp and capi_aquifers.cpp upload what is
// built here.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <limits>
#include <utility>

#include "internal.hpp"
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

void group_by_cell(const int* cell, int n, int Nb, const int* toOrder, std::vector<int>& pos, std::vector<int>& cpos, std::vector<int>& cptr,
                   std::vector<int>& items) {
    pos.assign(n, 0); items.assign(n, 0); cpos.clear();
    std::vector<int> slot(Nb, -1), count;
    for (int i = 0; i < n; ++i) {
        pos[i] = toOrder[cell[i]];
        if (slot[cell[i]] < 0) { slot[cell[i]] = (int)cpos.size(); cpos.push_back(pos[i]); count.push_back(0); }
        count[slot[cell[i]]]++;
    }
    cptr.assign(cpos.size() + 1, 0);
    for (size_t t = 0; t < cpos.size(); ++t) cptr[t + 1] = cptr[t] + count[t];
    std::vector<int> fill(cptr.begin(), cptr.end() - 1);
    for (int i = 0; i < n; ++i) items[fill[slot[cell[i]]]++] = i;
}

// ---- standard wells ----
int std_wells_lists(const opmhip_std_wells* sw, int Nb, const int* toOrder, StdWellsLists& out, std::string& msg) {
    const int nw = sw->num_wells;
    if (nw < 0) return refuse(msg, "set_std_wells: num_wells = %d", nw);
    if (!sw->perf_pointers || !sw->cell || !sw->tw || !sw->dz || !sw->producer || !sw->inj_phase || !sw->rate_component || !sw->rate_target || !sw->bhp_limit || !sw->control)
        return refuse(msg, "set_std_wells: null array (only x is optional)");
    if (sw->perf_pointers[0] != 0) return refuse(msg, "set_std_wells: inconsistent pointers (perf_pointers[0] = %d, not 0)", sw->perf_pointers[0]);
    for (int w = 0; w < nw; ++w) {
        if (sw->perf_pointers[w + 1] <= sw->perf_pointers[w]) return refuse(msg, "set_std_wells: inconsistent pointers (well %d has no perforation)", w);
        if (sw->producer[w] != 0 && sw->producer[w] != 1) return refuse(msg, "set_std_wells: producer[%d] = %d (1 producer, 0 injector)", w, sw->producer[w]);
        if (!sw->producer[w] && (sw->inj_phase[w] < 0 || sw->inj_phase[w] > 2))
            return refuse(msg, "set_std_wells: unknown phase: inj_phase[%d] = %d (0 water, 1 oil, 2 gas)", w, sw->inj_phase[w]);
        if (sw->rate_component[w] < 0 || sw->rate_component[w] > 2)
            return refuse(msg, "set_std_wells: unknown component: rate_component[%d] = %d (0 oil, 1 water, 2 gas)", w, sw->rate_component[w]);
        if (sw->control[w] != 0 && sw->control[w] != 1) return refuse(msg, "set_std_wells: control[%d] = %d (0 rate, 1 bhp)", w, sw->control[w]);
        if (!std::isfinite(sw->rate_target[w]) || !std::isfinite(sw->bhp_limit[w])) return refuse(msg, "set_std_wells: rate target / bhp limit of well %d is not finite", w);
    }
    const int np = sw->perf_pointers[nw];
    for (int p = 0; p < np; ++p) {
        const int cell = sw->cell[p];
        if (cell < 0 || cell >= Nb) return refuse(msg, "set_std_wells: perforation %d names cell %d, outside [0, %d)", p, cell, Nb);
        if (!std::isfinite(sw->tw[p]) || !std::isfinite(sw->dz[p])) return refuse(msg, "set_std_wells: tw / dz of perforation %d is not finite", p);
    }
    // the perforated cells in the internal order; the distinct ones, each with its perforations in perforation order
    group_by_cell(sw->cell, np, Nb, toOrder, out.pos, out.cpos, out.cptr, out.cperf);
    out.wi.assign((size_t)3 * nw, 0);
    out.wd.assign((size_t)2 * nw, 0.0);
    out.pack.assign((size_t)SW_PACK * nw, 0.0);
    for (int w = 0; w < nw; ++w) {
        out.wi[3 * w] = sw->producer[w]; out.wi[3 * w + 1] = sw->producer[w] ? 0 : sw->inj_phase[w]; out.wi[3 * w + 2] = sw->rate_component[w];
        out.wd[2 * w] = sw->rate_target[w]; out.wd[2 * w + 1] = sw->bhp_limit[w];
        for (int i = 0; i < 4; ++i) out.pack[(size_t)SW_X * nw + 4 * w + i] = sw->x ? sw->x[(size_t)4 * w + i] : 0.0;
        out.pack[(size_t)SW_CONTROL * nw + w] = sw->control[w];
    }
    return OPMHIP_SUCCESS;
}

int std_wells_check_state(size_t nw, const double* x, const int* control, const double* rate_target, std::string& msg) {
    if (control)
        for (size_t w = 0; w < nw; ++w)
            if (control[w] != 0 && control[w] != 1) return refuse(msg, "set_std_wells_state: control[%zu] = %d (0 rate, 1 bhp)", w, control[w]);
    if (rate_target)
        for (size_t w = 0; w < nw; ++w)
            if (!std::isfinite(rate_target[w])) return refuse(msg, "set_std_wells_state: rate_target[%zu] is not finite", w);
    if (x)
        for (size_t i = 0; i < 4 * nw; ++i)
            if (!std::isfinite(x[i])) return refuse(msg, "set_std_wells_state: x[%zu] is not finite", i);
    return OPMHIP_SUCCESS;
}

int std_wells_limits(const opmhip_std_wells_limits* L, size_t nw, const int* wi, const int* control, StdWellsLimitsLists& out, std::string& msg) {
    static const char* const name[5] = {"oil_rate", "water_rate", "gas_rate", "liquid_rate", "resv_rate"};
    const double inf = std::numeric_limits<double>::infinity();
    StdWellsLimitsLists H;
    H.lim.assign(5 * nw, inf);
    H.use.assign(nw, 1);
    if (L) {
        const double* arr[5] = {L->oil_rate, L->water_rate, L->gas_rate, L->liquid_rate, L->resv_rate};
        for (size_t w = 0; w < nw; ++w) {
            const bool producer = wi[3 * w] != 0;
            const int use = L->use_list_target ? L->use_list_target[w] : 1;
            if (use != 0 && use != 1) return refuse(msg, "set_std_wells_limits: use_list_target[%zu] = %d (0 / 1)", w, use);
            H.use[w] = use;
            if (!use) H.any = true;
            for (int k = 0; k < 5; ++k) {
                if (!arr[k]) continue;
                const double v = arr[k][w];
                if (!(v > 0.0)) return refuse(msg, "set_std_wells_limits: %s[%zu] = %g is not > 0 (+infinity: no such limit)", name[k], w, v);
                if (v == inf) continue;
                if (!producer && k != 4) return refuse(msg, "set_std_wells_limits: %s[%zu] is a producer's limit, well %zu is an injector (its limits: the list's rate target and resv_rate)", name[k], w, w);
                if (producer && use && k < 3 && wi[3 * w + 2] == k)
                    return refuse(msg, "set_std_wells_limits: %s[%zu] limits the component the list's own target already names (use_list_target = 0 takes that one out)", name[k], w);
                H.lim[5 * w + k] = v;
                H.any = true;
                if (k == 4) H.any_resv = true;
            }
        }
    }
    for (size_t w = 0; w < nw; ++w) {
        if (control[w] == 0 && !H.use[w]) return refuse(msg, "set_std_wells_limits: use_list_target[%zu] = 0 for a well under control 0, the list's own target", w);
        if (control[w] >= 3 && control[w] <= 7 && !(H.lim[5 * w + control[w] - 3] < inf))
            return refuse(msg, "set_std_wells_limits: well %zu is under control %d (%s): that limit cannot be taken away", w, control[w], name[control[w] - 3]);
    }
    out = std::move(H);
    return OPMHIP_SUCCESS;
}

int std_wells_limits_check_controls(size_t nw, const int* control, const int* thp_table, const double* lim, const int* use, std::string& msg) {
    if (!control) return OPMHIP_SUCCESS;
    for (size_t w = 0; w < nw; ++w) {
        const int k = control[w];
        if (k < 0 || k > 7) return refuse(msg, "set_std_wells_state: control[%zu] = %d (0 rate, 1 bhp, 2 thp, 3 orat, 4 wrat, 5 grat, 6 lrat, 7 resv)", w, k);
        if (k == 0 && !use[w]) return refuse(msg, "set_std_wells_state: control[%zu] = 0 for a well whose own target is not a limit (use_list_target = 0)", w);
        if (k == 2 && (!thp_table || thp_table[w] < 0))
            return refuse(msg, "set_std_wells_state: control[%zu] = 2 (thp) for a well without a THP limit (opmhip_set_std_wells_thp)", w);
        if (k >= 3 && !(lim[5 * w + k - 3] < std::numeric_limits<double>::infinity()))
            return refuse(msg, "set_std_wells_state: control[%zu] = %d for a well without that limit (opmhip_set_std_wells_limits)", w, k);
    }
    return OPMHIP_SUCCESS;
}

// ---- group production control ----
namespace {
const char* const group_target_name[5] = {"oil_target", "water_target", "gas_target", "liquid_target", "resv_target"};
// the targets' and the modes' part of a groups record, into H (whose `of` and `ptr` / `idx` stand): what both setters look at
int group_targets_into(const char* who, const double* const arr[5], const int* mode, size_t nw, StdWellsGroupsLists& H, std::string& msg) {
    const double inf = std::numeric_limits<double>::infinity();
    const int ng = H.num_groups;
    for (int g = 0; g < ng; ++g)
        for (int k = 0; k < 5; ++k) {
            if (!arr[k]) continue;
            const double v = arr[k][g];
            if (!(v > 0.0)) return refuse(msg, "%s: %s[%d] = %g is not > 0 (+infinity: no such target)", who, group_target_name[k], g, v);
            H.target[5 * (size_t)g + k] = v;
        }
    if (mode)
        for (int g = 0; g < ng; ++g) {
            if (mode[g] < 0 || mode[g] > 5) return refuse(msg, "%s: mode[%d] = %d (0 none, 1 orat, 2 wrat, 3 grat, 4 lrat, 5 resv)", who, g, mode[g]);
            H.mode[g] = mode[g];
        }
    for (int g = 0; g < ng; ++g)
        if (H.mode[g] != 0 && !(H.target[5 * (size_t)g + H.mode[g] - 1] < inf))
            return refuse(msg, "%s: group %d is under mode %d (%s) and has no such target", who, g, H.mode[g], group_target_name[H.mode[g] - 1]);
    H.resv.assign(nw, 0);
    H.any_resv = false;
    for (int g = 0; g < ng; ++g)
        if (H.target[5 * (size_t)g + 4] < inf) {
            H.any_resv = true;
            for (int k = H.ptr[g]; k < H.ptr[g + 1]; ++k) H.resv[H.idx[k]] = 1;
        }
    return OPMHIP_SUCCESS;
}
}  // namespace

int std_wells_groups_check_guide_rates(size_t nw, const double* guide_rate, std::string& msg) {
    if (!guide_rate) return refuse(msg, "set_std_wells_guide_rates: null array");
    for (size_t i = 0; i < 5 * nw; ++i)
        if (!std::isfinite(guide_rate[i]) || guide_rate[i] < 0.0)
            return refuse(msg, "set_std_wells_guide_rates: guide_rate[%zu] = %g (well %zu) is negative or not finite", i, guide_rate[i], i / 5);
    return OPMHIP_SUCCESS;
}

int std_wells_groups_check_controls(size_t nw, const int* control, const int* wi, const int* of, const int* available, std::string& msg) {
    if (!control) return OPMHIP_SUCCESS;
    for (size_t w = 0; w < nw; ++w) {
        if (control[w] != 8) continue;
        if (!of) return refuse(msg, "set_std_wells_state: control[%zu] = 8 (grup) without groups in force (opmhip_set_std_wells_groups)", w);
        if (!wi[3 * w]) return refuse(msg, "set_std_wells_state: control[%zu] = 8 (grup) for an injector", w);
        if (of[w] < 0) return refuse(msg, "set_std_wells_state: control[%zu] = 8 (grup) for a well without a group", w);
        if (!available[w]) return refuse(msg, "set_std_wells_state: control[%zu] = 8 (grup) for a well that is not available for group control", w);
    }
    return OPMHIP_SUCCESS;
}

int std_wells_groups(const opmhip_std_wells_groups* G, size_t nw, const int* wi, const int* control, StdWellsGroupsLists& out, std::string& msg) {
    StdWellsGroupsLists H;
    if (G && G->num_groups < 0) return refuse(msg, "set_std_wells_groups: num_groups = %d", G->num_groups);
    if (G && G->num_groups > 0) {
        const int ng = G->num_groups;
        if (!G->well_group || !G->guide_rate) return refuse(msg, "set_std_wells_groups: null array (well_group and guide_rate are needed)");
        if (G->nupcol < 0) return refuse(msg, "set_std_wells_groups: nupcol = %d is not >= 0", G->nupcol);
        H.num_groups = ng; H.nupcol = G->nupcol; H.any = true;
        H.of.assign(G->well_group, G->well_group + nw);
        H.available.assign(nw, 1);
        for (size_t w = 0; w < nw; ++w) {
            if (H.of[w] < -1 || H.of[w] >= ng) return refuse(msg, "set_std_wells_groups: well_group[%zu] = %d is outside [-1, %d)", w, H.of[w], ng);
            if (G->available) {
                if (G->available[w] != 0 && G->available[w] != 1) return refuse(msg, "set_std_wells_groups: available[%zu] = %d (0 / 1)", w, G->available[w]);
                H.available[w] = G->available[w];
            }
        }
        if (std_wells_groups_check_guide_rates(nw, G->guide_rate, msg)) {
            msg.replace(0, msg.find(':'), "set_std_wells_groups");
            return OPMHIP_INVALID_ARGUMENT;
        }
        H.guide.assign(G->guide_rate, G->guide_rate + 5 * nw);
        // per group its producers, wells ascending
        H.ptr.assign((size_t)ng + 1, 0);
        for (size_t w = 0; w < nw; ++w)
            if (H.of[w] >= 0 && wi[3 * w]) H.ptr[H.of[w] + 1]++;
        for (int g = 0; g < ng; ++g) H.ptr[g + 1] += H.ptr[g];
        H.idx.assign(H.ptr[ng], 0);
        std::vector<int> fill(H.ptr.begin(), H.ptr.end() - 1);
        for (size_t w = 0; w < nw; ++w)
            if (H.of[w] >= 0 && wi[3 * w]) H.idx[fill[H.of[w]]++] = (int)w;
        H.target.assign((size_t)5 * ng, std::numeric_limits<double>::infinity());
        H.mode.assign(ng, 0);
        const double* arr[5] = {G->oil_target, G->water_target, G->gas_target, G->liquid_target, G->resv_target};
        if (int r = group_targets_into("set_std_wells_groups", arr, G->mode, nw, H, msg)) return r;
        for (size_t w = 0; w < nw; ++w)
            if (control[w] == 8 && (!wi[3 * w] || H.of[w] < 0 || !H.available[w]))
                return refuse(msg, "set_std_wells_groups: well %zu is under control 8 (grup): it must stay an available producer in a group", w);
    } else {
        for (size_t w = 0; w < nw; ++w)
            if (control[w] == 8) return refuse(msg, "set_std_wells_groups: well %zu is under control 8 (grup): the groups cannot be removed", w);
    }
    out = std::move(H);
    return OPMHIP_SUCCESS;
}

int std_wells_group_targets(const StdWellsGroupsLists& cur, size_t nw, const double* const arr[5], const int* mode, StdWellsGroupsLists& out, std::string& msg) {
    StdWellsGroupsLists H = cur;
    if (int r = group_targets_into("set_std_wells_group_targets", arr, mode, nw, H, msg)) return r;
    out = std::move(H);
    return OPMHIP_SUCCESS;
}

int std_wells_check_crossflow(size_t nw, const int* allow, const int* wi, bool& any, std::string& msg) {
    bool some = false;
    if (allow)
        for (size_t w = 0; w < nw; ++w) {
            if (allow[w] != 0 && allow[w] != 1) return refuse(msg, "set_std_wells_crossflow: allow[%zu] = %d (0 off, 1 on)", w, allow[w]);
            some = some || allow[w] == 1;
        }
    if (some)
        for (size_t w = 0; w < nw; ++w)
            if (allow[w] && !wi[3 * w])
                return refuse(msg, "set_std_wells_crossflow: well %zu is an injector - crossflow is modelled for producers only (the injected composition is fixed)", w);
    any = some;
    return OPMHIP_SUCCESS;
}

int std_wells_check_vaporised_oil(int on, bool has_pvtg, std::string& msg) {
    if (on != 0 && on != 1) return refuse(msg, "set_std_wells_vaporised_oil: on = %d (0 off, 1 on)", on);
    if (!has_pvtg)
        return refuse(msg, "set_std_wells_vaporised_oil: the context's fluid has no PVTG - its intensive-quantity records hold no Rv for the rate model to read");
    return OPMHIP_SUCCESS;
}

int std_wells_head_model(const opmhip_std_wells_wellbore* wb, size_t nw, size_t np, const int* wi, std::vector<int>& pref, std::string& msg) {
    if (!wb->perf_depth || !wb->ref_depth || !wb->preferred_phase) return refuse(msg, "set_std_wells_head_model: null array");
    for (size_t p = 0; p < np; ++p)
        if (!std::isfinite(wb->perf_depth[p])) return refuse(msg, "set_std_wells_head_model: perf_depth[%zu] is not finite", p);
    for (size_t w = 0; w < nw; ++w)
        if (!std::isfinite(wb->ref_depth[w])) return refuse(msg, "set_std_wells_head_model: ref_depth[%zu] is not finite", w);
    for (size_t w = 0; w < nw; ++w)
        if (wi[3 * w] && (wb->preferred_phase[w] < 0 || wb->preferred_phase[w] > 2))
            return refuse(msg, "set_std_wells_head_model: unknown phase: preferred_phase[%zu] = %d (0 water, 1 oil, 2 gas)", w, wb->preferred_phase[w]);
    pref.resize(nw);
    for (size_t w = 0; w < nw; ++w) pref[w] = wi[3 * w] ? wb->preferred_phase[w] : 1;
    return OPMHIP_SUCCESS;
}

int std_wells_check_perf_state(size_t np, const double* perf_pressure, const double* perf_rates, bool state_set, std::string& msg) {
    if (perf_pressure)
        for (size_t p = 0; p < np; ++p)
            if (!std::isfinite(perf_pressure[p])) return refuse(msg, "set_std_wells_perf_state: perf_pressure[%zu] is not finite", p);
    if (perf_rates)
        for (size_t i = 0; i < 3 * np; ++i)
            if (!std::isfinite(perf_rates[i])) return refuse(msg, "set_std_wells_perf_state: perf_rates[%zu] is not finite", i);
    if (!state_set && !perf_pressure && perf_rates)
        return refuse(msg, "set_std_wells_perf_state: rates alone before the perforation pressures exist (they are taken from the cells at the first begin_iteration(0))");
    return OPMHIP_SUCCESS;
}

int std_wells_matrix_add_check(int on, std::string& msg) {
    if (on != 0 && on != 1) return refuse(msg, "set_std_wells_matrix_add: on = %d (0 off, 1 on)", on);
    return OPMHIP_SUCCESS;
}

int std_wells_matrix_add_schedule(int nw, const int* perf_pointers, const int* pos, const int* fromOrder, const int* rowptr, const int* col,
                                  StdWellsMatrixAdd& out, std::string& msg) {
    struct Pair { int entry, well, a, b; };
    std::vector<Pair> pairs;
    for (int w = 0; w < nw; ++w) {
        const int pb = perf_pointers[w], np = perf_pointers[w + 1] - pb;
        for (int a = 0; a < np; ++a) {
            const int row = pos[pb + a];
            const int* lo = col + rowptr[row];
            const int* hi = col + rowptr[row + 1];
            for (int b = 0; b < np; ++b) {
                const int* it = std::lower_bound(lo, hi, pos[pb + b]);
                if (it == hi || *it != pos[pb + b])
                    return refuse(msg, "set_std_wells_matrix_add: block (%d, %d) of well %d is not in the pattern given to set_pattern: the form needs every pair of a "
                                       "well's perforated cells there (the clique pattern)", fromOrder[row], fromOrder[pos[pb + b]], w);
                pairs.push_back({(int)(it - col), w, a, b});
            }
        }
    }
    // by block; the pairs of one block stay in the order they were listed in: by well, then by a * np + b
    std::stable_sort(pairs.begin(), pairs.end(), [](const Pair& x, const Pair& y) { return x.entry < y.entry; });
    StdWellsMatrixAdd H;
    H.contrib.reserve(3 * pairs.size());
    for (size_t k = 0; k < pairs.size(); ++k) {
        if (k == 0 || pairs[k].entry != pairs[k - 1].entry) {
            H.target.push_back(pairs[k].entry);
            H.tptr.push_back((int)k);
        }
        H.contrib.push_back(pairs[k].well); H.contrib.push_back(pairs[k].a); H.contrib.push_back(pairs[k].b);
    }
    H.tptr.push_back((int)pairs.size());
    H.pairs = (int)pairs.size();
    out = std::move(H);
    return OPMHIP_SUCCESS;
}

// ---- analytic aquifers ----
int aquifer_lists(const opmhip_aquifers* aq, int Nb, const int* toOrder, AquiferLists& out, std::string& msg) {
    const int na = aq->num_aquifers;
    if (na < 0) return refuse(msg, "set_aquifers: num_aquifers = %d", na);
    if (!aq->type || !aq->id || !aq->conn_pointers || !aq->time_constant || !aq->water_density || !aq->datum_depth)
        return refuse(msg, "set_aquifers: null array (type, id, conn_pointers, time_constant, water_density, datum_depth are mandatory)");
    if (aq->conn_pointers[0] != 0) return refuse(msg, "set_aquifers: conn_pointers[0] = %d, not 0", aq->conn_pointers[0]);
    bool anyCT = false, anyFet = false;
    for (int a = 0; a < na; ++a) {
        if (aq->conn_pointers[a + 1] < aq->conn_pointers[a]) return refuse(msg, "set_aquifers: conn_pointers descend at aquifer %d", a);
        if (aq->type[a] != 0 && aq->type[a] != 1) return refuse(msg, "set_aquifers: type[%d] = %d (0 Carter-Tracy, 1 Fetkovich)", a, aq->type[a]);
        if (aq->type[a] == 0 && anyFet) return refuse(msg, "set_aquifers: Carter-Tracy aquifer %d behind a Fetkovich one (Carter-Tracy first: the order of addToSource)", a);
        (aq->type[a] == 0 ? anyCT : anyFet) = true;
    }
    const int nc = aq->conn_pointers[na];
    if (nc > 0 && (!aq->cell || !aq->alpha)) return refuse(msg, "set_aquifers: null array (cell / alpha)");
    if (anyCT && (!aq->influx_constant || !aq->table_pointers || !aq->td || !aq->pd))
        return refuse(msg, "set_aquifers: null array (a Carter-Tracy aquifer needs influx_constant, table_pointers, td, pd)");
    if (anyFet && (!aq->prod_index || !aq->total_compr || !aq->initial_watvolume))
        return refuse(msg, "set_aquifers: null array (a Fetkovich aquifer needs prod_index, total_compr, initial_watvolume)");
    if (aq->has_restart && (!aq->restart_W_flux || (anyFet && !aq->restart_pressure)))
        return refuse(msg, "set_aquifers: null array (has_restart without restart_W_flux / restart_pressure)");
    AquiferLists L;
    L.nc = nc;
    L.par.assign((size_t)na * AQ_PAR, 0.0);
    L.tabptr.assign(na + 1, 0);
    for (int a = 0; a < na; ++a) {
        double* p = &L.par[(size_t)a * AQ_PAR];
        if (!(aq->time_constant[a] > 0.0)) return refuse(msg, "set_aquifers: aquifer %d has time constant Tc = %g, must be positive", a, aq->time_constant[a]);
        const bool has_p = !aq->has_initial_pressure || aq->has_initial_pressure[a];
        if (has_p && !aq->initial_pressure) return refuse(msg, "set_aquifers: null array (initial_pressure)");
        const bool restart = aq->has_restart && aq->has_restart[a];
        p[AQ_TYPE] = aq->type[a]; p[AQ_TC] = aq->time_constant[a]; p[AQ_RHOW] = aq->water_density[a]; p[AQ_DATUM] = aq->datum_depth[a];
        p[AQ_PA0] = has_p ? aq->initial_pressure[a] : 0.0;
        if (!has_p) L.need_eq.push_back(a);
        L.tabptr[a + 1] = L.tabptr[a];
        if (aq->type[a] == 0) {
            if (restart) return refuse(msg, "set_aquifers: restart data for Carter-Tracy aquifer %d - restart-based initialisation is not supported for Carter-Tracy aquifers (as in the reference)", a);
            p[AQ_BETA] = aq->influx_constant[a];
            const int t0 = aq->table_pointers[a], t1 = aq->table_pointers[a + 1];
            if (t0 < 0 || t1 - t0 < 2) return refuse(msg, "set_aquifers: the influence table of aquifer %d has fewer than two nodes", a);
            for (int i = t0 + 1; i < t1; ++i)
                if (!(aq->td[i] > aq->td[i - 1])) return refuse(msg, "set_aquifers: the influence table of aquifer %d is not ascending at node %d", a, i - t0);
            L.td.insert(L.td.end(), aq->td + t0, aq->td + t1);
            L.pd.insert(L.pd.end(), aq->pd + t0, aq->pd + t1);
            L.tabptr[a + 1] = (int)L.td.size();
        } else {
            p[AQ_PI] = aq->prod_index[a];
            p[AQ_CV] = aq->total_compr[a] * aq->initial_watvolume[a];
            if (!(p[AQ_CV] > 0.0)) return refuse(msg, "set_aquifers: Fetkovich aquifer %d has total_compr * initial_watvolume = %g, must be positive", a, p[AQ_CV]);
        }
    }
    // connections; the distinct connected cells, each with its connections in aquifer order (= ascending connection number)
    L.of.assign(nc, 0);
    {
        std::vector<int> seen(Nb, -1);
        for (int a = 0; a < na; ++a)
            for (int i = aq->conn_pointers[a]; i < aq->conn_pointers[a + 1]; ++i) {
                const int cell = aq->cell[i];
                if (cell < 0 || cell >= Nb) return refuse(msg, "set_aquifers: connection %d of aquifer %d names cell %d, outside [0, %d)", i - aq->conn_pointers[a], a, cell, Nb);
                if (seen[cell] == a) return refuse(msg, "set_aquifers: cell %d is repeated within aquifer %d (one connection per cell)", cell, a);
                seen[cell] = a;
                L.of[i] = a;
            }
    }
    group_by_cell(aq->cell, nc, Nb, toOrder, L.pos, L.cpos, L.cptr, L.cconn);
    out = std::move(L);
    return OPMHIP_SUCCESS;
}

double aquifer_equilibrium_pressure(const double* alpha, int i0, int n, const int* order, const double* rec, int IQS, const double* depth, const int* p,
                                    double datum) {
    double sumAlpha = 0.0, sumPw = 0.0;
    for (int i = i0; i < i0 + n; ++i) sumAlpha += alpha[i];
    for (int i = 0; i < n; ++i) {
        const double pw = rec[(size_t)i * IQS + 4 * (F_P + WATER)], rho = rec[(size_t)i * IQS + 4 * (F_RHO + WATER)];
        const double gdz = GRAVITY * (depth[p[i]] - datum);
        sumPw += alpha[order[i]] * (pw - rho * gdz);
    }
    return sumPw / sumAlpha;
}

void aquifer_initial_state(const opmhip_aquifers* aq, const std::vector<double>& par, std::vector<double>& state) {
    const int na = aq->num_aquifers;
    state.assign((size_t)na * AQ_STATE, 0.0);
    for (int a = 0; a < na; ++a) {
        const bool restart = aq->has_restart && aq->has_restart[a];
        state[(size_t)a * AQ_STATE + AQ_WFLUX] = restart ? aq->restart_W_flux[a] : 0.0;
        state[(size_t)a * AQ_STATE + AQ_AUX] = aq->type[a] == 0 ? 0.0 : (restart ? aq->restart_pressure[a] : par[(size_t)a * AQ_PAR + AQ_PA0]);
    }
}

int table_interval(const double* x, int n, double xv) {
    const int j = (int)(std::upper_bound(x, x + n, xv) - x) - 1;
    return std::min(std::max(j, 0), n - 2);
}
double table_slope(const double* x, const double* y, int n, double xv) {
    const int j = table_interval(x, n, xv);
    return (y[j + 1] - y[j]) / (x[j + 1] - x[j]);
}
double table_value(const double* x, const double* y, int n, double xv) {
    const int j = table_interval(x, n, xv);
    return (y[j + 1] - y[j]) / (x[j + 1] - x[j]) * (xv - x[j]) + y[j];
}

void aquifer_step_scalars(int num, const std::vector<double>& par, const std::vector<int>& tabptr, const std::vector<double>& td, const std::vector<double>& pd,
                          double time, double dt, double* step) {
    for (int a = 0; a < num; ++a) {
        const double* p = &par[(size_t)a * AQ_PAR];
        double* s = step + (size_t)a * AQ_STEP;
        s[AQ_TD] = s[AQ_PITD] = s[AQ_PITDPRIME] = s[AQ_COEF] = 0.0;
        if (p[AQ_TYPE] == 0.0) {   // calculateEqnConstants (AquiferCarterTracy.hpp:150-153)
            const double td_plus_dt = (dt + time) / p[AQ_TC];
            const int t0 = tabptr[a], n = tabptr[a + 1] - t0;
            s[AQ_TD] = time / p[AQ_TC];
            s[AQ_PITD] = table_value(&td[t0], &pd[t0], n, td_plus_dt);
            s[AQ_PITDPRIME] = table_slope(&td[t0], &pd[t0], n, td_plus_dt);
        } else {                   // AquiferFetkovich.hpp:143-144
            const double td_Tc = dt / p[AQ_TC];
            s[AQ_COEF] = (1 - std::exp(-td_Tc)) / td_Tc;
        }
    }
}

void aquifer_report(int num, const std::vector<double>& par, const std::vector<int>& ptr, const double* state, const double* q4, double* W_flux,
                    double* pressure, double* flux_rate, double* init_pressure) {
    for (int a = 0; a < num; ++a) {
        const double* p = &par[(size_t)a * AQ_PAR];
        if (W_flux) W_flux[a] = state[(size_t)a * AQ_STATE + AQ_WFLUX];
        if (pressure) pressure[a] = p[AQ_TYPE] == 0.0 ? p[AQ_PA0] : state[(size_t)a * AQ_STATE + AQ_AUX];
        if (init_pressure) init_pressure[a] = p[AQ_PA0];
        if (flux_rate) {
            double f = 0.0;
            for (int i = ptr[a]; i < ptr[a + 1]; ++i) f += q4[(size_t)4 * i];
            flux_rate[a] = f;
        }
    }
}

}  // namespace opmhip
