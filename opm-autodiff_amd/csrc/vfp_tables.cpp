// Host set-up of the VFP tables and of the resident standard wells' THP limits (vfp_tables.hpp).  No HIP call: capi_std_wells.cpp uploads what
// is built here.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <utility>

#include "vfp_tables.hpp"

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
const char* const AXIS_NAME[5] = {"flo", "thp", "wfr", "gfr", "alq"};
}  // namespace

int vfp_pack(const opmhip_vfp_tables* t, VfpPacked& out, std::string& msg) {
    const int nt = t->num_tables;
    if (nt < 0) return refuse(msg, "set_vfp_tables: num_tables = %d", nt);
    if (!t->kind || !t->table_num || !t->flo_type || !t->wfr_type || !t->gfr_type || !t->datum_depth || !t->axis_sizes || !t->axis_pointers || !t->axes ||
        !t->value_pointers || !t->values)
        return refuse(msg, "set_vfp_tables: null array");
    if (t->axis_pointers[0] != 0 || t->value_pointers[0] != 0)
        return refuse(msg, "set_vfp_tables: inconsistent pointers (axis_pointers[0] = %d, value_pointers[0] = %d, not 0)", t->axis_pointers[0], t->value_pointers[0]);
    VfpPacked P;
    P.num = nt;
    P.desc.assign((size_t)nt * VFP_DESC, 0);
    P.datum.assign(nt, 0.0);
    for (int k = 0; k < nt; ++k) {
        const int kind = t->kind[k];
        if (kind != 0 && kind != 1) return refuse(msg, "set_vfp_tables: unknown kind: kind[%d] = %d (0 VFPPROD, 1 VFPINJ)", k, kind);
        if (t->table_num[k] <= 0) return refuse(msg, "set_vfp_tables: table_num[%d] = %d (the deck's number, > 0)", k, t->table_num[k]);
        for (int j = 0; j < k; ++j)
            if (t->kind[j] == kind && t->table_num[j] == t->table_num[k])
                return refuse(msg, "set_vfp_tables: duplicate number: tables %d and %d are both %s %d", j, k, kind ? "VFPINJ" : "VFPPROD", t->table_num[k]);
        if (t->flo_type[k] < 0 || t->flo_type[k] > 2)
            return refuse(msg, "set_vfp_tables: unknown type: flo_type[%d] = %d (%s)", k, t->flo_type[k], kind ? "0 OIL, 1 WAT, 2 GAS" : "0 OIL, 1 LIQ, 2 GAS");
        if (!kind && (t->wfr_type[k] < 0 || t->wfr_type[k] > 2)) return refuse(msg, "set_vfp_tables: unknown type: wfr_type[%d] = %d (0 WOR, 1 WCT, 2 WGR)", k, t->wfr_type[k]);
        if (!kind && (t->gfr_type[k] < 0 || t->gfr_type[k] > 2)) return refuse(msg, "set_vfp_tables: unknown type: gfr_type[%d] = %d (0 GOR, 1 GLR, 2 OGR)", k, t->gfr_type[k]);
        if (!std::isfinite(t->datum_depth[k])) return refuse(msg, "set_vfp_tables: datum_depth[%d] is not finite", k);
        const int naxes = kind ? 2 : 5;
        long long sum = 0, prod = 1;
        int* d = &P.desc[(size_t)k * VFP_DESC];
        for (int a = 0; a < 5; ++a) {
            const int n = a < naxes ? t->axis_sizes[5 * k + a] : 1;
            if (n < 1) return refuse(msg, "set_vfp_tables: empty axis: table %d has %d %s entries", k, n, AXIS_NAME[a]);
            d[VFP_N + a] = n;
            if (a < naxes) sum += n;
            prod *= n;
            if (prod > (1 << 28)) return refuse(msg, "set_vfp_tables: table %d is too large", k);
        }
        const long long a0 = t->axis_pointers[k], a1 = t->axis_pointers[k + 1], v0 = t->value_pointers[k], v1 = t->value_pointers[k + 1];
        if (a1 - a0 != sum) return refuse(msg, "set_vfp_tables: inconsistent pointers (table %d: axis_pointers give %lld entries, axis_sizes %lld)", k, a1 - a0, sum);
        if (v1 - v0 != prod) return refuse(msg, "set_vfp_tables: inconsistent pointers (table %d: value_pointers give %lld values, axis_sizes %lld)", k, v1 - v0, prod);
        d[VFP_KIND] = kind; d[VFP_NUM] = t->table_num[k]; d[VFP_FLO_TYPE] = t->flo_type[k];
        d[VFP_WFR_TYPE] = kind ? 0 : t->wfr_type[k]; d[VFP_GFR_TYPE] = kind ? 0 : t->gfr_type[k];
        const double* ax = t->axes + a0;
        for (int a = 0; a < 5; ++a) {
            if (a >= naxes) { d[VFP_AXIS + a] = -1; continue; }
            const int n = d[VFP_N + a];
            for (int i = 0; i < n; ++i) {
                if (!std::isfinite(ax[i])) return refuse(msg, "set_vfp_tables: table %d: %s axis entry %d is not finite", k, AXIS_NAME[a], i);
                if (i > 0 && ax[i] < ax[i - 1]) return refuse(msg, "set_vfp_tables: table %d: the %s axis decreases at entry %d", k, AXIS_NAME[a], i);
            }
            d[VFP_AXIS + a] = (int)P.dbl.size();
            P.dbl.insert(P.dbl.end(), ax, ax + n);
            ax += n;
        }
        const double* val = t->values + v0;
        for (long long i = 0; i < prod; ++i)
            if (!std::isfinite(val[i])) return refuse(msg, "set_vfp_tables: table %d: value %lld is not finite", k, i);
        d[VFP_VALUES] = (int)P.dbl.size();
        P.dbl.insert(P.dbl.end(), val, val + prod);
        P.datum[k] = t->datum_depth[k];
        if (P.dbl.size() > (size_t)(1 << 29)) return refuse(msg, "set_vfp_tables: the tables are too large");
    }
    out = std::move(P);
    return OPMHIP_SUCCESS;
}

int vfp_find(const VfpPacked& P, int kind, int table_num) {
    for (int k = 0; k < P.num; ++k)
        if (P.desc[(size_t)k * VFP_DESC + VFP_KIND] == kind && P.desc[(size_t)k * VFP_DESC + VFP_NUM] == table_num) return k;
    return -1;
}

int std_wells_thp_lists(const opmhip_std_wells_thp* thp, size_t nw, const int* wi, const VfpPacked& P, std::vector<int>& table, std::vector<double>& wd, bool& any,
                        std::string& msg) {
    if (!thp->vfp_table || !thp->thp_limit || !thp->alq || !thp->dh) return refuse(msg, "set_std_wells_thp: null array");
    std::vector<int> tab(nw, -1);
    std::vector<double> d(3 * nw, 0.0);
    bool some = false;
    for (size_t w = 0; w < nw; ++w) {
        const int num = thp->vfp_table[w];
        if (num == 0) continue;
        const int kind = wi[3 * w] ? 0 : 1;
        const int k = num > 0 ? vfp_find(P, kind, num) : -1;
        if (k < 0) return refuse(msg, "set_std_wells_thp: well %zu (%s) names %s table %d, which does not exist", w, kind ? "an injector" : "a producer", kind ? "VFPINJ" : "VFPPROD", num);
        if (P.desc[(size_t)k * VFP_DESC + VFP_N + 1] < 2)
            return refuse(msg, "set_std_wells_thp: well %zu: the THP axis of %s table %d has fewer than two entries (the inverse look-up reads two)", w, kind ? "VFPINJ" : "VFPPROD", num);
        if (!std::isfinite(thp->thp_limit[w]) || !std::isfinite(thp->alq[w]) || !std::isfinite(thp->dh[w]))
            return refuse(msg, "set_std_wells_thp: limit, alq or dh of well %zu is not finite", w);
        tab[w] = k;
        d[3 * w] = thp->thp_limit[w]; d[3 * w + 1] = thp->alq[w]; d[3 * w + 2] = thp->dh[w];
        some = true;
    }
    table = std::move(tab);
    wd = std::move(d);
    any = some;
    return OPMHIP_SUCCESS;
}

int std_wells_thp_check_controls(size_t nw, const int* control, const int* table, std::string& msg) {
    if (!control) return OPMHIP_SUCCESS;
    for (size_t w = 0; w < nw; ++w) {
        if (control[w] < 0 || control[w] > 2) return refuse(msg, "set_std_wells_state: control[%zu] = %d (0 rate, 1 bhp, 2 thp)", w, control[w]);
        if (control[w] == 2 && (!table || table[w] < 0))
            return refuse(msg, "set_std_wells_state: control[%zu] = 2 (thp) for a well without a THP limit (opmhip_set_std_wells_thp)", w);
    }
    return OPMHIP_SUCCESS;
}

}  // namespace opmhip
