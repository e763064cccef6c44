"""VFP tables and the THP limit are additive to ABI 11: four new entry points and two new structs, the version and the layout of
opmhip_std_wells as they were."""
import ctypes
import re

NEW = ("opmhip_set_vfp_tables", "opmhip_vfp_probe", "opmhip_set_std_wells_thp", "opmhip_get_std_wells_thp")


def header(pkg):
    with open(pkg.capi.HEADER_PATH) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def fields_of(txt, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
    return [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]


def test_the_new_symbols_are_exported_and_declared(pkg):
    L = pkg.capi.lib()
    for name in NEW:
        assert hasattr(L, name) and name in pkg.capi.declared_symbols(), name
    assert L.opmhip_vfp_probe.argtypes is not None and len(L.opmhip_vfp_probe.argtypes) == 11
    assert len(L.opmhip_set_vfp_tables.argtypes) == 2


def test_the_abi_version_is_still_11(pkg):
    L = pkg.capi.lib()
    L.opmhip_abi_version.restype = ctypes.c_int
    assert L.opmhip_abi_version() == 11
    with open(pkg.capi.HEADER_PATH) as f:
        assert re.search(r"#define\s+OPMHIP_ABI_VERSION\s+11\b", f.read())


def test_the_layout_of_opmhip_std_wells_is_unchanged(pkg):
    fields = fields_of(header(pkg), "opmhip_std_wells")
    assert fields == ["int num_wells", "const int* perf_pointers", "const int* cell", "const double* tw", "const double* dz", "const int* producer",
                      "const int* inj_phase", "const int* rate_component", "const double* rate_target", "const double* bhp_limit", "const int* control",
                      "const double* x"]
    S = pkg.capi.StdWells
    assert [n for n, _ in S._fields_] == [d.split("*")[-1].split()[-1] for d in fields]
    assert ctypes.sizeof(S) == 96 and S.x.offset == 88


def test_the_new_structs_are_bound_as_declared(pkg):
    txt = header(pkg)
    for name, S, size in (("opmhip_vfp_tables", pkg.capi.VfpTables, 8 + 11 * 8), ("opmhip_std_wells_thp", pkg.capi.StdWellsThp, 4 * 8)):
        fields = fields_of(txt, name)
        assert [n for n, _ in S._fields_] == [d.split("*")[-1].split()[-1] for d in fields], name
        assert ctypes.sizeof(S) == size, name
    assert fields_of(txt, "opmhip_std_wells_thp") == ["const int* vfp_table", "const double* thp_limit", "const double* alq", "const double* dh"]
    # the control field of opmhip_set_std_wells itself keeps to 0 / 1: THP is reached through the state call or by switching
    with open(pkg.capi.HEADER_PATH) as f:
        raw = f.read()
    assert "const int* control;            /* per well: 0 rate, 1 bhp */" in raw
