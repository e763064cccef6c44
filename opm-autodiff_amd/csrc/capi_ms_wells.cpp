// C-ABI, the device-resident multisegment wells (include/opmhip.h: opmhip_set_ms_wells, opmhip_get_ms_wells_info,
// opmhip_set_ms_wells_form, opmhip_get_ms_wells_form_info).  Every check of what the caller hands over and the list's layout are host
// work of ms_wells_setup.cpp; this unit compares the list with the one in force, allocates, uploads and launches (wells_operator.hip).
#include <string>
#include <vector>

#include "capi_guard.hpp"
#include "internal.hpp"

using namespace opmhip;

namespace {
void ms_wells_clear(opmhip_ctx* c) {
    MsWellsDev& S = c->wells.ms;
    S.num = S.maxM = 0;
    S.flag_pending = false;
}
void ms_wells_release(opmhip_ctx* c) {
    MsWellsDev& S = c->wells.ms;
    ms_wells_clear(c);
    S.atomic = false;
    S.have_structure = false;
    S.num_dense = S.num_tree = S.tree_max_seg = S.tree_max_depth = 0;
    S.tree_bytes = 0;
    S.tree_lds_doubles = 0;
    S.h_form.clear();
    dev_free(c, &S.d_tdesc); dev_free(c, &S.d_tint); dev_free(c, &S.d_fac);
    dev_free(c, &S.d_desc); dev_free(c, &S.d_Brows); dev_free(c, &S.d_cell); dev_free(c, &S.d_blkrow); dev_free(c, &S.d_Dcolp); dev_free(c, &S.d_Drows);
    dev_free(c, &S.d_flag); dev_free(c, &S.d_B); dev_free(c, &S.d_C); dev_free(c, &S.d_Dvals); dev_free(c, &S.d_inv);
    S.bytes = 0;
    S.h_Mbp.clear(); S.h_Brows.clear(); S.h_blkp.clear(); S.h_Bcols.clear(); S.h_Dcolp.clear(); S.h_Drows.clear(); S.h_Dnzp.clear();
    S.h_Bvals.clear(); S.h_Cvals.clear(); S.h_Dvals.clear();
}
// A list of a new structure (the stream is idle, the list in force released): the pinned flags, the index arrays, the descriptors and
// the room for the values.  The caller releases what was built if this fails.
int ms_wells_upload_structure(opmhip_ctx* c, const opmhip_ms_wells* ms, const MsWellsList& L, const MsWellsLayout& Y) {
    MsWellsDev& S = c->wells.ms;
    const size_t nw = (size_t)ms->num_ms_wells, nseg = L.nseg, nblk = L.nblk, nnz = L.nnz;
    if (!S.h_flag || S.cap_flag < nw) {
        if (S.h_flag) (void)hipHostFree(S.h_flag);
        S.h_flag = nullptr;
        OPMHIP_HIP(c, hipHostMalloc((void**)&S.h_flag, nw * sizeof(int)));
        S.cap_flag = nw;
    }
    int rc;
    if ((rc = dev_upload(c, &S.d_desc, Y.desc)) || (rc = dev_upload(c, &S.d_Brows, ms->Brows, nseg + nw)) || (rc = dev_upload(c, &S.d_cell, Y.cell)) ||
        (rc = dev_upload(c, &S.d_blkrow, Y.blkrow)) || (rc = dev_upload(c, &S.d_Dcolp, ms->Dcol_pointers, 4 * nseg + nw)) || (rc = dev_upload(c, &S.d_Drows, ms->Drows, nnz)) ||
        (rc = dev_alloc(c, &S.d_flag, nw)) || (rc = dev_alloc(c, &S.d_B, nblk * 12)) || (rc = dev_alloc(c, &S.d_C, nblk * 12)) || (rc = dev_alloc(c, &S.d_Dvals, nnz)) ||
        (rc = dev_alloc(c, &S.d_inv, L.invDoubles)))
        return rc;
    // the tree wells' arrays behind the others, and only where the list has such wells: a dense list allocates what it always did
    if (!Y.tdesc.empty() && ((rc = dev_upload(c, &S.d_tdesc, Y.tdesc)) || (rc = dev_upload(c, &S.d_tint, Y.tint)) || (rc = dev_alloc(c, &S.d_fac, Y.facDoubles)))) return rc;
    S.tree_bytes = sizeof(double) * Y.facDoubles;
    S.bytes = Y.desc.size() * sizeof(MsWellDesc) + Y.tdesc.size() * sizeof(MsTreeDesc) + sizeof(int) * (nseg + nw + 2 * nblk + 4 * nseg + nw + nnz + nw + Y.tint.size()) +
              sizeof(double) * (nblk * 24 + nnz + L.invDoubles) + S.tree_bytes;
    S.atomic = Y.shared;
    S.num_dense = (int)Y.desc.size(); S.num_tree = (int)Y.tdesc.size();
    S.tree_max_seg = Y.treeSeg; S.tree_max_depth = Y.treeDepth;
    S.h_form = L.wform;
    ms_wells_tree_plan(c, Y.tdesc);
    S.have_structure = true;
    S.h_Mbp.assign(ms->Mb_pointers, ms->Mb_pointers + nw + 1); S.h_Brows.assign(ms->Brows, ms->Brows + nseg + nw);
    S.h_blkp.assign(ms->block_pointers, ms->block_pointers + nw + 1); S.h_Bcols.assign(ms->Bcols, ms->Bcols + nblk);
    S.h_Dcolp.assign(ms->Dcol_pointers, ms->Dcol_pointers + 4 * nseg + nw); S.h_Drows.assign(ms->Drows, ms->Drows + nnz);
    S.h_Dnzp.assign(ms->Dnnz_pointers, ms->Dnnz_pointers + nw + 1);
    return OPMHIP_SUCCESS;
}
}  // namespace

namespace opmhip {
// The pivot flags of the last inversion, looked at where the host waits for the stream anyway (the caller has just synchronised, or this
// does): a singular D clears the list and is INVALID_ARGUMENT - the operator is never applied with a broken inverse.
int ms_wells_check(opmhip_ctx* c) {
    MsWellsDev& S = c->wells.ms;
    if (!S.flag_pending) return OPMHIP_SUCCESS;
    OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
    S.flag_pending = false;
    for (int w = 0; w < S.num; ++w)
        if (S.h_flag[w] != 0) {
            const int col = S.h_flag[w] - 1;
            const bool tree = (size_t)w < S.h_form.size() && S.h_form[w] != 0;
            ms_wells_release(c);
            if (tree)
                return fail(c, OPMHIP_INVALID_ARGUMENT, "set_ms_wells: D of multisegment well %d: the 4 x 4 block of segment %d is singular after its children are eliminated (no non-zero finite pivot); "
                            "the tree form pivots inside a segment's block only, the dense form pivots over the whole column and does not have this limit; the list is cleared", w, col);
            return fail(c, OPMHIP_INVALID_ARGUMENT, "set_ms_wells: D of multisegment well %d is singular (no non-zero pivot in column %d of its elimination); the list is cleared", w, col);
        }
    return OPMHIP_SUCCESS;
}
}  // namespace opmhip

extern "C" {

int opmhip_set_ms_wells(opmhip_ctx* c, const opmhip_ms_wells* ms) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        MsWellsDev& S = c->wells.ms;
        if (!ms || ms->num_ms_wells == 0) {   // cleared: the arrays stay for the next list
            OPMHIP_HIP(c, hipSetDevice(c->device));
            if (S.flag_pending) OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
            ms_wells_clear(c);
            S.h_Dvals.clear();   // (a list that comes back is inverted again)
            return OPMHIP_SUCCESS;
        }
        if (!c->pattern_set) return fail(c, OPMHIP_NOT_READY, "set_ms_wells before the pattern is set (the cells are translated to the ILU ordering)");
        if (c->comm.nranks > 1) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_ms_wells: multisegment wells on the device are not supported in decomposed runs");
        const int nw = ms->num_ms_wells;
        if (nw < 0) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_ms_wells: negative well count");
        if (ms->dim != 3 || ms->dim_wells != 4) return fail(c, OPMHIP_INVALID_ARGUMENT, "set_ms_wells: dim = %d, dim_wells = %d; only 3 and 4 are supported", ms->dim, ms->dim_wells);
        if (!ms->Mb_pointers || !ms->Brows || !ms->block_pointers || !ms->Bcols || !ms->Bvals || !ms->Cvals || !ms->Dcol_pointers || !ms->Drows || !ms->Dvals || !ms->Dnnz_pointers)
            return fail(c, OPMHIP_INVALID_ARGUMENT, "set_ms_wells: null array");
        // a refused list leaves none in force: the caller falls back to the callback form
        auto refuse = [&](int rc) { ms_wells_clear(c); S.h_Dvals.clear(); return rc; };
        MsWellsList L;
        std::string msg;
        int rc;
        if ((rc = ms_wells_list_check(*ms, S.form, c->pat.Nb, L, msg))) return refuse(fail(c, rc, "%s", msg.c_str()));
        const size_t nseg = L.nseg, nblk = L.nblk, nnz = L.nnz;
        OPMHIP_HIP(c, hipSetDevice(c->device));
        const bool structure = S.have_structure && record_same(S.h_Mbp, ms->Mb_pointers, (size_t)nw + 1) && record_same(S.h_Brows, ms->Brows, nseg + nw) &&
                               record_same(S.h_blkp, ms->block_pointers, (size_t)nw + 1) && record_same(S.h_Bcols, ms->Bcols, nblk) &&
                               record_same(S.h_Dcolp, ms->Dcol_pointers, 4 * nseg + nw) && record_same(S.h_Drows, ms->Drows, nnz) &&
                               record_same(S.h_Dnzp, ms->Dnnz_pointers, (size_t)nw + 1);
        const bool sB = structure && record_same(S.h_Bvals, ms->Bvals, nblk * 12), sC = structure && record_same(S.h_Cvals, ms->Cvals, nblk * 12);
        const bool sD = structure && record_same(S.h_Dvals, ms->Dvals, nnz);
        if (!(structure && sB && sC && sD)) OPMHIP_HIP(c, hipStreamSynchronize(c->stream));   // earlier kernels on the stream may still read what the copies below replace
        if (!structure) {
            // a new list: the index arrays anew, cells in the internal order, per block its segment row, and whether two blocks meet in a cell
            MsWellsLayout Y;
            if ((rc = ms_wells_list_layout(*ms, S.form, c->pat.Nb, c->pat.toOrder.data(), L, Y, msg))) return refuse(fail(c, rc, "%s", msg.c_str()));
            ms_wells_release(c);
            if ((rc = ms_wells_upload_structure(c, ms, L, Y))) {
                ms_wells_release(c);
                return rc;
            }
        }
        if (!sB && (rc = dev_put_recorded(c, S.d_B, S.h_Bvals, ms->Bvals, nblk * 12))) return refuse(rc);
        if (!sC && (rc = dev_put_recorded(c, S.d_C, S.h_Cvals, ms->Cvals, nblk * 12))) return refuse(rc);
        if (!sD && (rc = dev_put_recorded(c, S.d_Dvals, S.h_Dvals, ms->Dvals, nnz))) return refuse(rc);
        S.num = nw;
        S.maxM = L.maxM;
        if (!sD) {
            launch_ms_wells_factor(c);
            OPMHIP_HIP(c, hipGetLastError());
        }
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_ms_wells_info(opmhip_ctx* c, int info[4]) {
    if (!c || !info) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        int rc;
        if ((rc = ms_wells_check(c))) return rc;
        const MsWellsDev& S = c->wells.ms;
        info[0] = S.num;
        info[1] = S.maxM;
        info[2] = S.num > 0 ? (int)((S.bytes + 1023) / 1024) : 0;
        info[3] = S.factorisations;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_set_ms_wells_form(opmhip_ctx* c, int form) {
    if (!c) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        if (form != OPMHIP_MS_WELLS_DENSE && form != OPMHIP_MS_WELLS_TREE && form != OPMHIP_MS_WELLS_AUTO)
            return fail(c, OPMHIP_INVALID_ARGUMENT, "set_ms_wells_form: form = %d; OPMHIP_MS_WELLS_DENSE (0), _TREE (1) or _AUTO (2)", form);
        MsWellsDev& S = c->wells.ms;
        if (form == S.form) return OPMHIP_SUCCESS;
        if (S.have_structure || S.flag_pending) {   // a list set under the other form is cleared; kernels on the stream may still read its arrays
            OPMHIP_HIP(c, hipSetDevice(c->device));
            OPMHIP_HIP(c, hipStreamSynchronize(c->stream));
        }
        ms_wells_release(c);
        S.form = form;
        return OPMHIP_SUCCESS;
    });
}

int opmhip_get_ms_wells_form_info(opmhip_ctx* c, int info[6]) {
    if (!c || !info) return OPMHIP_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        int rc;
        if ((rc = ms_wells_check(c))) return rc;
        const MsWellsDev& S = c->wells.ms;
        const bool set = S.num > 0;
        info[0] = S.form;
        info[1] = set ? S.num_dense : 0;
        info[2] = set ? S.num_tree : 0;
        info[3] = set ? S.tree_max_seg : 0;
        info[4] = set ? S.tree_max_depth : 0;
        info[5] = set ? (int)((S.tree_bytes + 1023) / 1024) : 0;
        return OPMHIP_SUCCESS;
    });
}

}  // extern "C"
