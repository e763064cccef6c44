"""The tree form of the device-resident multisegment wells at the drop-in boundary, without a GPU: the two new symbols are declared and
exported, the ABI number is unchanged (the entry points are additive), and the cap and form constants are in the header."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbols_are_declared_and_exported(pkg):
    L = pkg.capi.lib()
    names = pkg.capi.declared_symbols()
    for n in ("opmhip_set_ms_wells_form", "opmhip_get_ms_wells_form_info"):
        assert n in names and hasattr(L, n), n
    assert L.opmhip_abi_version() == 11


def test_the_header_keeps_abi_11_and_states_the_cap(pkg):
    with open(os.path.join(ROOT, "include", "opmhip.h")) as f:
        txt = f.read()
    assert re.search(r"#define\s+OPMHIP_ABI_VERSION\s+11\b", txt)
    assert pkg.capi.ms_wells_tree_cap() == 1024 == int(re.search(r"#define\s+OPMHIP_MS_WELLS_TREE_MAX_SEGMENTS\s+(\d+)", txt).group(1))
    for name, value in (("DENSE", 0), ("TREE", 1), ("AUTO", 2)):
        assert int(re.search(r"#define\s+OPMHIP_MS_WELLS_%s\s+(\d+)" % name, txt).group(1)) == value == pkg.capi.MS_WELLS_FORMS[name.lower()]
    # the well's z of 4 doubles per segment stays in LDS under the 64 KiB static limit, and the dense cap is as it was
    assert 4 * 8 * pkg.capi.ms_wells_tree_cap() <= 32 * 1024
    assert pkg.capi.ms_wells_caps() == (256, 32768)
    # each declaration names the reference code it replaces
    for n in ("opmhip_set_ms_wells_form", "opmhip_get_ms_wells_form_info"):
        at = txt.index("int %s(" % n)
        assert "replaces:" in txt[txt.rindex("/*", 0, at):at], n
