// Host set-up of the passive tracers: see tracers_setup.hpp.  No HIP types, no context.
#include "tracers_setup.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "source_lists.hpp"

namespace opmhip {

namespace {
std::string text(const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
    char buf[320];
    std::snprintf(buf, sizeof buf, fmt, a, b, c);
    return buf;
}
}  // namespace

int tracer_batches(int num_tracers, const int* phase, const double* concentration, int Nb, bool has_pvtg, int nranks, int nghost, TracerBatches& out,
                   std::string& msg) {
    if (num_tracers < 0) { msg = text("set_tracers: num_tracers = %lld", num_tracers); return OPMHIP_INVALID_ARGUMENT; }
    if (!phase || !concentration) { msg = "set_tracers: null array"; return OPMHIP_INVALID_ARGUMENT; }
    if (nranks > 1 || nghost > 0) {
        msg = text("set_tracers: decomposed context (%lld ranks, %lld ghost cells) - the reference's tracer model gives up on parallel runs "
                   "(eclgenerictracermodel.cc:105-111) and the transport solve across the ranks is not built", nranks, nghost);
        return OPMHIP_INVALID_ARGUMENT;
    }
    TracerBatches B;
    B.phase.assign(phase, phase + num_tracers);
    B.slot.resize(num_tracers);
    for (int t = 0; t < num_tracers; ++t) {
        const int ph = phase[t];
        if (ph < 0 || ph > 2) { msg = text("set_tracers: tracer %lld has phase %lld (0 water, 1 oil, 2 gas)", t, ph); return OPMHIP_INVALID_ARGUMENT; }
        if (ph == 2) {
            msg = text("set_tracers: tracer %lld is a gas tracer - the library's fluid always carries dissolved gas, and the reference refuses gas "
                       "tracers under DISGAS (ecltracermodel.hh:465-467)", t);
            return OPMHIP_INVALID_ARGUMENT;
        }
        if (ph == 1 && has_pvtg) {
            msg = text("set_tracers: tracer %lld is an oil tracer on a fluid with PVTG - vaporised oil would carry it in the gas phase, which the "
                       "reference refuses (ecltracermodel.hh:455-457)", t);
            return OPMHIP_INVALID_ARGUMENT;
        }
        B.slot[t] = (int)B.members[ph].size();
        B.members[ph].push_back(t);
        if ((int)B.members[ph].size() > OPMHIP_TRACERS_MAX_PER_PHASE) {
            msg = text("set_tracers: more than %lld tracers of phase %lld", OPMHIP_TRACERS_MAX_PER_PHASE, ph);
            return OPMHIP_INVALID_ARGUMENT;
        }
    }
    for (long long i = 0; i < (long long)num_tracers * Nb; ++i)
        if (!std::isfinite(concentration[i])) {
            msg = text("set_tracers: the concentration of tracer %lld in cell %lld is not finite", i / Nb, i % Nb);
            return OPMHIP_INVALID_ARGUMENT;
        }
    out = std::move(B);
    return OPMHIP_SUCCESS;
}

int tracer_solver_check(double tolerance, int maxit, std::string& msg) {
    if (!(tolerance > 0.0) || !std::isfinite(tolerance)) { msg = "set_tracer_solver: the tolerance must be positive and finite"; return OPMHIP_INVALID_ARGUMENT; }
    if (maxit < 1) { msg = text("set_tracer_solver: maxit = %lld", maxit); return OPMHIP_INVALID_ARGUMENT; }
    return OPMHIP_SUCCESS;
}

void tracer_levels(int Nb, const int* rowptr, const int* col, TracerLevels& out) {
    std::vector<int> level(Nb > 0 ? Nb : 0, 0);
    int nlev = 0;
    for (int i = 0; i < Nb; ++i) {
        int l = 0;
        for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) {
            const int j = col[k];
            if (j < i) l = std::max(l, level[j] + 1);
        }
        level[i] = l;
        nlev = std::max(nlev, l + 1);
    }
    out.ptr.assign((size_t)nlev + 1, 0);
    for (int i = 0; i < Nb; ++i) out.ptr[(size_t)level[i] + 1]++;
    for (int l = 0; l < nlev; ++l) out.ptr[(size_t)l + 1] += out.ptr[l];
    out.rows.assign(Nb > 0 ? Nb : 0, 0);
    std::vector<int> at(out.ptr.begin(), out.ptr.end() - 1);
    for (int i = 0; i < Nb; ++i) out.rows[at[level[i]]++] = i;
}

void tracer_face_order(int Nb, const int* rowptr, const int* nnzMap, std::vector<int>& ford) {
    ford.resize(Nb > 0 ? rowptr[Nb] : 0);
    for (int p = 0; p < Nb; ++p) {
        const int kb = rowptr[p], ke = rowptr[p + 1];
        for (int k = kb; k < ke; ++k) ford[k] = k;
        std::sort(ford.begin() + kb, ford.begin() + ke, [&](int x, int y) { return nnzMap[x] < nnzMap[y]; });
    }
}

int tracer_connections(int n, const int* cell, const double* rate, const double* injected, int num_tracers, int Nb, const int* toOrder,
                       TracerConnLists& out, std::string& msg) {
    if (n < 0) { msg = text("set_tracer_connections: n = %lld", n); return OPMHIP_INVALID_ARGUMENT; }
    if (!cell || !rate || !injected) { msg = "set_tracer_connections: null array"; return OPMHIP_INVALID_ARGUMENT; }
    for (int i = 0; i < n; ++i) {
        if (cell[i] < 0 || cell[i] >= Nb) { msg = text("set_tracer_connections: connection %lld names cell %lld outside [0, %lld)", i, cell[i], Nb); return OPMHIP_INVALID_ARGUMENT; }
        for (int ph = 0; ph < 3; ++ph)
            if (!std::isfinite(rate[(size_t)3 * i + ph])) { msg = text("set_tracer_connections: a rate of connection %lld is not finite", i); return OPMHIP_INVALID_ARGUMENT; }
    }
    for (long long i = 0; i < (long long)num_tracers * n; ++i)
        if (!std::isfinite(injected[i])) {
            msg = text("set_tracer_connections: the injected concentration of tracer %lld at connection %lld is not finite", i / n, i % n);
            return OPMHIP_INVALID_ARGUMENT;
        }
    TracerConnLists L;
    group_by_cell(cell, n, Nb, toOrder, L.pos, L.cpos, L.cptr, L.cconn);
    out = std::move(L);
    return OPMHIP_SUCCESS;
}

}  // namespace opmhip
