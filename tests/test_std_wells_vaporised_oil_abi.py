"""The vaporised-oil switch of the standard wells is additive to ABI 11: two new entry points, the version and the layout of opmhip_std_wells as they were."""
import ctypes
import re


def test_the_two_symbols_are_exported_and_declared(pkg):
    L = pkg.capi.lib()
    for name in ("opmhip_set_std_wells_vaporised_oil", "opmhip_get_std_wells_solution_rates"):
        assert hasattr(L, name) and name in pkg.capi.declared_symbols(), name


def test_the_abi_version_is_still_11(pkg):
    L = pkg.capi.lib()
    L.opmhip_abi_version.restype = ctypes.c_int
    assert L.opmhip_abi_version() == 11
    with open(pkg.capi.HEADER_PATH) as f:
        assert re.search(r"#define\s+OPMHIP_ABI_VERSION\s+11\b", f.read())


def test_the_layout_of_opmhip_std_wells_is_unchanged(pkg):
    """an int and eleven pointers, as ABI 11 introduced it - in the header and in the binding"""
    with open(pkg.capi.HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    body = re.search(r"typedef struct opmhip_std_wells \{(.*?)\} opmhip_std_wells;", txt, flags=re.S).group(1)
    fields = [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]
    assert fields == ["int num_wells", "const int* perf_pointers", "const int* cell", "const double* tw", "const double* dz", "const int* producer",
                      "const int* inj_phase", "const int* rate_component", "const double* rate_target", "const double* bhp_limit", "const int* control",
                      "const double* x"]
    S = pkg.capi.StdWells
    assert [n for n, _ in S._fields_] == [d.split("*")[-1].split()[-1] for d in fields]
    assert ctypes.sizeof(S) == 8 + 11 * ctypes.sizeof(ctypes.c_void_p) == 96 and S.x.offset == 88
