"""Group production control of the resident wells is additive to ABI 11: four new entry points and one new struct, the version and the
layout of opmhip_std_wells as they were."""
import ctypes
import re

NEW = {"opmhip_set_std_wells_groups": 2, "opmhip_set_std_wells_guide_rates": 2, "opmhip_set_std_wells_group_targets": 7, "opmhip_get_std_wells_groups": 7}


def header(pkg):
    with open(pkg.capi.HEADER_PATH) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_the_new_symbols_are_exported_declared_and_bound(pkg):
    L = pkg.capi.lib()
    if not getattr(L, "_asm_bound", False):
        pkg.capi._bind_assembly(L)
    for name, nargs in NEW.items():
        assert hasattr(L, name) and name in pkg.capi.declared_symbols(), name
        fn = getattr(L, name)
        assert len(fn.argtypes) == nargs, name
        assert fn(*([None] * nargs)) == pkg.capi.INVALID_ARGUMENT, name       # no context


def test_the_new_struct_is_bound_as_declared(pkg):
    body = re.search(r"typedef struct opmhip_std_wells_groups \{(.*?)\} opmhip_std_wells_groups;", header(pkg), flags=re.S).group(1)
    fields = [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]
    assert fields == ["int num_groups", "const int* well_group", "const double* oil_target", "const double* water_target", "const double* gas_target",
                      "const double* liquid_target", "const double* resv_target", "const int* mode", "const double* guide_rate", "const int* available", "int nupcol"]
    S = pkg.capi.StdWellsGroups
    assert [n for n, _ in S._fields_] == [d.split("*")[-1].split()[-1] for d in fields]
    assert ctypes.sizeof(S) == 8 + 9 * 8 + 8 and S.well_group.offset == 8 and S.nupcol.offset == 80        # the ints padded to the pointers' alignment
    for (n, t), d in zip(S._fields_, fields):
        assert (t is ctypes.c_int) == d.startswith("int "), n
    s, keep = pkg.capi.make_std_wells_groups(dict(num_groups=2, well_group=[0, -1, 1], liquid_target=[1.0, 2.0], guide_rate=[[1.0] * 5] * 3, nupcol=4), 3)
    assert s.num_groups == 2 and s.nupcol == 4 and s.oil_target is None and s.mode is None and s.available is None
    assert s.liquid_target == keep["liquid_target"].ctypes.data and s.well_group == keep["well_group"].ctypes.data and keep["guide_rate"].size == 15
    assert pkg.capi.make_std_wells_groups(None, 3) == (None, {})


def test_the_version_and_the_list_itself_are_unchanged(pkg):
    L = pkg.capi.lib()
    L.opmhip_abi_version.restype = ctypes.c_int
    assert L.opmhip_abi_version() == 11
    with open(pkg.capi.HEADER_PATH) as f:
        raw = f.read()
    assert re.search(r"#define\s+OPMHIP_ABI_VERSION\s+11\b", raw)
    assert ctypes.sizeof(pkg.capi.StdWells) == 96 and ctypes.sizeof(pkg.capi.StdWellsLimits) == 48
    assert pkg.wells.GRUP_CODE == 8 and 8 not in pkg.wells.CONTROL_CODE.values()
