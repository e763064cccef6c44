"""The further rate limits of the resident wells are additive to ABI 11: two new entry points and one new struct, the version and the layout
of opmhip_std_wells as they were."""
import ctypes
import re

NEW = ("opmhip_set_std_wells_limits", "opmhip_get_std_wells_resv")


def header(pkg):
    with open(pkg.capi.HEADER_PATH) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def fields_of(txt, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
    return [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]


def test_the_new_symbols_are_exported_declared_and_bound(pkg):
    L = pkg.capi.lib()
    if not getattr(L, "_asm_bound", False):
        pkg.capi._bind_assembly(L)
    for name in NEW:
        assert hasattr(L, name) and name in pkg.capi.declared_symbols(), name
    assert len(L.opmhip_set_std_wells_limits.argtypes) == 2 and len(L.opmhip_get_std_wells_resv.argtypes) == 4
    assert L.opmhip_set_std_wells_limits(None, None) == pkg.capi.INVALID_ARGUMENT and L.opmhip_get_std_wells_resv(None, None, None, None) == pkg.capi.INVALID_ARGUMENT


def test_the_new_struct_is_bound_as_declared(pkg):
    txt = header(pkg)
    fields = fields_of(txt, "opmhip_std_wells_limits")
    assert fields == ["const double* oil_rate", "const double* water_rate", "const double* gas_rate", "const double* liquid_rate", "const double* resv_rate",
                      "const int* use_list_target"]
    S = pkg.capi.StdWellsLimits
    assert [n for n, _ in S._fields_] == [d.split("*")[-1].split()[-1] for d in fields] and ctypes.sizeof(S) == 6 * 8
    # an entry left out of the dict is a NULL array
    s, keep = pkg.capi.make_std_wells_limits(dict(liquid_rate=[1.0, 2.0], use_list_target=[1, 0]), 2)
    assert s.oil_rate is None and s.resv_rate is None and s.liquid_rate == keep["liquid_rate"].ctypes.data and s.use_list_target == keep["use_list_target"].ctypes.data
    assert pkg.capi.make_std_wells_limits(None, 2) == (None, {})


def test_the_version_and_the_list_itself_are_unchanged(pkg):
    L = pkg.capi.lib()
    L.opmhip_abi_version.restype = ctypes.c_int
    assert L.opmhip_abi_version() == 11
    with open(pkg.capi.HEADER_PATH) as f:
        raw = f.read()
    assert re.search(r"#define\s+OPMHIP_ABI_VERSION\s+11\b", raw)
    assert "const int* control;            /* per well: 0 rate, 1 bhp */" in raw       # the new modes come through the state call or by switching
    assert ctypes.sizeof(pkg.capi.StdWells) == 96
    assert pkg.wells.CONTROL_CODE == {"rate": 0, "bhp": 1, "thp": 2, "orat": 3, "wrat": 4, "grat": 5, "lrat": 6, "resv": 7}
