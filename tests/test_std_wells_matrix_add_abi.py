"""The matrix-add form of the resident standard wells is additive to ABI 11: three new entry points, the version as it was; the binding
and the wells class carry the switch."""
import ctypes
import inspect
import re


def test_the_three_symbols_are_exported_and_declared(pkg):
    L = pkg.capi.lib()
    for name in ("opmhip_set_std_wells_matrix_add", "opmhip_std_wells_add_to_matrix", "opmhip_get_std_wells_matrix_add"):
        assert hasattr(L, name) and name in pkg.capi.declared_symbols(), name


def test_the_abi_version_is_still_11(pkg):
    L = pkg.capi.lib()
    L.opmhip_abi_version.restype = ctypes.c_int
    assert L.opmhip_abi_version() == 11
    with open(pkg.capi.HEADER_PATH) as f:
        assert re.search(r"#define\s+OPMHIP_ABI_VERSION\s+11\b", f.read())


def test_the_header_no_longer_lists_the_form_as_not_covered(pkg):
    with open(pkg.capi.HEADER_PATH) as f:
        txt = f.read()
    assert "opmhip_add_well_contributions stays with host lists" not in txt
    entry = txt[txt.index("the matrix-add form of the resident standard wells"):txt.index("int opmhip_set_std_wells_matrix_add")]
    assert "StandardWell_impl.hpp:1688-1712" in entry and "ISTLSolverEbos" in entry


def test_the_python_surface(pkg):
    for name in ("set_std_wells_matrix_add", "std_wells_add_to_matrix", "std_wells_matrix_add_info"):
        assert callable(getattr(pkg.capi.HipModel, name))
    p = inspect.signature(pkg.wells.DeviceStandardWells.__init__).parameters["matrix_add"]
    assert p.default is False                                    # opt-in: a list that does not ask reaches the solver as an operator
