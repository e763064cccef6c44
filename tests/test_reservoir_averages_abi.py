"""opmhip_reservoir_averages is additive to ABI 11: one new entry point, the version as it was."""
import ctypes
import re


def test_the_new_symbol_is_exported_declared_and_bound(pkg):
    L = pkg.capi.lib()
    assert hasattr(L, "opmhip_reservoir_averages") and "opmhip_reservoir_averages" in pkg.capi.declared_symbols()
    if not getattr(L, "_asm_bound", False):
        pkg.capi._bind_assembly(L)
    assert len(L.opmhip_reservoir_averages.argtypes) == 2
    assert L.opmhip_reservoir_averages(None, None) == pkg.capi.INVALID_ARGUMENT      # no context: refused before anything is touched
    assert hasattr(pkg.capi.HipModel, "reservoir_averages")


def test_the_abi_version_is_still_11(pkg):
    L = pkg.capi.lib()
    L.opmhip_abi_version.restype = ctypes.c_int
    assert L.opmhip_abi_version() == 11
    with open(pkg.capi.HEADER_PATH) as f:
        txt = f.read()
    assert re.search(r"#define\s+OPMHIP_ABI_VERSION\s+11\b", txt)
    assert re.search(r"int opmhip_reservoir_averages\(opmhip_ctx\* ctx, double\* out\);", txt)
