"""The device-resident multisegment wells at the drop-in boundary, without a GPU: the two symbols are exported, the Python binding's
MsWells mirrors opmhip_ms_wells field by field as a C compiler sees include/opmhip.h, and the struct builder rejects ragged input."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbols_are_declared_and_exported(pkg):
    L = pkg.capi.lib()
    names = pkg.capi.declared_symbols()
    for n in ("opmhip_set_ms_wells", "opmhip_get_ms_wells_info"):
        assert n in names and hasattr(L, n), n
    assert L.opmhip_abi_version() == 11          # additive: no existing struct changed
    capM, capKiB = pkg.capi.ms_wells_caps()
    assert capM % 4 == 0 and capM >= 4 * 33 and 8 * capM * capM <= capKiB * 1024


def test_ms_wells_struct_matches_the_header(pkg, tmp_path):
    fields = [f[0] for f in pkg.capi.MsWells._fields_]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "opmhip.h"', 'int main(void) {', '  printf("ms %zu\\n", sizeof(opmhip_ms_wells));']
    for f in fields:
        lines.append('  printf("ms.%s %%zu\\n", offsetof(opmhip_ms_wells, %s));' % (f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["ms"]) == ctypes.sizeof(pkg.capi.MsWells)
    assert len(out) == 1 + len(fields) == 14
    for f in fields:
        assert int(out["ms." + f]) == getattr(pkg.capi.MsWells, f).offset, f


def test_struct_builder(pkg):
    cells = [[3, 9, 4], [7, 1, 0, 5, 2]]
    wells = [pkg.mswells.tree_well(2, cells[0], seed=1), pkg.mswells.tree_well(4, cells[1], seed=2)]
    ms, keep = pkg.capi.make_ms_wells(wells)
    assert (ms.num_ms_wells, ms.dim, ms.dim_wells) == (2, 3, 4)
    Mbp, Brows, blkp, Bcols, Bv, Cv, Dcp, Dri, Dv, nzp = keep
    assert list(Mbp) == [0, 2, 6] and list(blkp) == [0, 3, 8] and list(Bcols) == cells[0] + cells[1]
    assert len(Brows) == 6 + 2 and Brows[0] == 0 and Brows[2] == 3 and Brows[3] == 0 and Brows[7] == 5     # relative to the well's first block
    assert len(Dcp) == 4 * 6 + 2 and Dcp[8] == nzp[1] and Dcp[9] == 0 and Dcp[-1] == nzp[2] - nzp[1]
    assert len(Bv) == len(Cv) == 12 * 8 and len(Dri) == len(Dv) == nzp[2]
    assert ms.Bcols == Bcols.ctypes.data and ms.Dnnz_pointers == nzp.ctypes.data
    # the dense operators the tests compare against read the same arrays
    B, C, D = pkg.mswells.dense_operators(wells[1], 10)
    assert B.shape == (16, 30) and np.count_nonzero(D) == len(wells[1]["Dvals"]) and np.linalg.matrix_rank(D) == 16
    assert np.array_equal(B[0:4, 21:24], wells[1]["Bvals"].reshape(-1, 4, 3)[0])
    assert pkg.capi.make_ms_wells(None) == (None, []) and pkg.capi.make_ms_wells([]) == (None, [])


@pytest.mark.parametrize("key,change", [("Bvals", lambda a: a[:-1]), ("Cvals", lambda a: a[:-3]), ("Dcolptr", lambda a: a[:-1]), ("Drows", lambda a: a[:-1]),
                                        ("Dvals", lambda a: np.append(a, 1.0)), ("Brows", lambda a: a[::-1]), ("Brows", lambda a: a[:1]),
                                        ("Bcols", lambda a: a[:-1])])
def test_struct_builder_rejects_ragged_input(pkg, key, change):
    w = pkg.mswells.tree_well(3, [5, 1, 8, 2], seed=3)
    w[key] = change(np.asarray(w[key]))
    with pytest.raises(ValueError):
        pkg.capi.make_ms_wells([pkg.mswells.tree_well(2, [0, 4], seed=4), w])
