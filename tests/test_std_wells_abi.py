"""The device-resident standard wells at the drop-in boundary, without a GPU: the symbols are exported, the ABI version is unchanged, the
Python binding's StdWells mirrors opmhip_std_wells field by field as a C compiler sees include/opmhip.h, and the struct builder rejects
ragged input."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("opmhip_set_std_wells", "opmhip_std_wells_begin_iteration", "opmhip_std_wells_apply_residual", "opmhip_std_wells_update", "opmhip_get_std_wells",
           "opmhip_set_std_wells_state", "opmhip_get_std_wells_blocks")


def test_the_symbols_are_declared_and_exported(pkg):
    L = pkg.capi.lib()
    names = pkg.capi.declared_symbols()
    for n in SYMBOLS:
        assert n in names and hasattr(L, n), n
    assert L.opmhip_abi_version() == 11          # additive: no existing struct changed


def test_std_wells_struct_matches_the_header(pkg, tmp_path):
    fields = [f[0] for f in pkg.capi.StdWells._fields_]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "opmhip.h"', 'int main(void) {', '  printf("sw %zu\\n", sizeof(opmhip_std_wells));',
             '  printf("wells %zu\\n", sizeof(opmhip_wells));']
    for f in fields:
        lines.append('  printf("sw.%s %%zu\\n", offsetof(opmhip_std_wells, %s));' % (f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["sw"]) == ctypes.sizeof(pkg.capi.StdWells)
    assert int(out["wells"]) == ctypes.sizeof(pkg.capi.Wells)       # the host list's struct is as it was
    assert len(out) == 2 + len(fields) == 14
    for f in fields:
        assert int(out["sw." + f]) == getattr(pkg.capi.StdWells, f).offset, f


def good():
    return dict(perf_pointers=[0, 3, 4], cell=[5, 6, 7, 5], tw=[1e-12] * 4, dz=[0.0, 2.0, 4.0, 1.0], producer=[1, 0], inj_phase=[0, 2], rate_component=[0, 2],
                rate_target=[1e-3, 2.0], bhp_limit=[1e7, 4e7], control=[0, 1], x=None)


def test_struct_builder(pkg):
    s, keep = pkg.capi.make_std_wells(good())
    assert s.num_wells == 2 and s.x is None and s.cell == keep["cell"].ctypes.data and s.bhp_limit == keep["bhp_limit"].ctypes.data
    assert keep["cell"].dtype == np.int32 and keep["tw"].dtype == np.float64 and list(keep["control"]) == [0, 1]
    s, keep = pkg.capi.make_std_wells(dict(good(), x=np.arange(8.0).reshape(2, 4)))
    assert s.x == keep["x"].ctypes.data and list(keep["x"]) == list(range(8))
    assert pkg.capi.make_std_wells(None) == (None, {})


@pytest.mark.parametrize("key,value", [("cell", [5, 6, 7]), ("tw", [1.0] * 5), ("dz", []), ("producer", [1]), ("control", [0, 1, 0]), ("rate_target", [1.0]),
                                       ("x", [0.0] * 7), ("perf_pointers", [0, 3])])
def test_struct_builder_rejects_ragged_input(pkg, key, value):
    with pytest.raises(ValueError):
        pkg.capi.make_std_wells(dict(good(), **{key: value}))


def test_device_wells_refuse_what_the_abi_cannot_say(pkg):
    """DeviceStandardWells checks its wells before anything goes to the library"""
    W = pkg.wells
    bad = [W.Well("A", [0], [1.0], 0.0, True, ("bhp", 2e7), 1e7)]             # no rate target to return to
    with pytest.raises(ValueError):
        W.DeviceStandardWells(bad, np.zeros(4), model=None)
    bad = [W.Well("B", [0], [1.0], 0.0, False, ("rate", W.GAS, 1.0), 4e7, inj_phase="steam")]
    with pytest.raises(ValueError):
        W.DeviceStandardWells(bad, np.zeros(4), model=None)
