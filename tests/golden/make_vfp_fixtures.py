#!/usr/bin/env python3
"""Generates the VFP DATA fixtures from files the reference tree holds.  Run in the build container (needs /root/reference).  Output is
data only - a table as its deck writes it and the expected numbers of the reference's own VFP test - never program text:

  tests/golden/vfpprod2_table.json  <- tests/VFPPROD2: the header (table 32, datum 394, LIQ / WCT / GOR), the five axes and the
                                       7 x 9 x 9 x 1 x 12 BHP values in DECK units (METRIC: Sm3/day, barsa), the unit factors beside
                                       them; values[((((t * nw + w) * ng + g) * na + a) * nf + f)], flo fastest
  tests/golden/vfp_expected.json    <- tests/test_vfpproperties.cpp: the six findInterpData cases (:60-99), the ParseInterpolateLine
                                       table (:574-590, FIELD units) with its 5^5 input grid (:599-613), the four 8-point input axes
                                       (:661-664) and the 4096 values of reference[] (:731-733) of ParseInterpolateRealisticVFPPROD,
                                       max_d_tol / sad_tol (:46-47)

No number is rounded: every token goes through float() and json's repr, which give the same double back.
"""
import json
import os
import re

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NUMBER = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?"


def records(path):
    """the records of the one keyword in the file: lists of tokens (numbers as float, quoted words bare); comments stripped"""
    recs, cur = [], []
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0].strip() == "VFPPROD"
    for line in lines[1:]:
        line = line.split("--")[0]
        while line.strip():
            head, slash, line = line.partition("/")
            for tok in head.split():
                tok = tok.strip("'")
                cur.append(float(tok) if re.fullmatch(NUMBER, tok) else tok)
            if slash:
                recs.append(cur)
                cur = []
    assert not cur
    return recs


def vfpprod2():
    r = records(os.path.join(REF, "tests", "VFPPROD2"))
    head, flo, thp, wfr, gfr, alq = r[:6]
    nf, nt, nw, ng, na = len(flo), len(thp), len(wfr), len(gfr), len(alq)
    values = [None] * (nt * nw * ng * na * nf)
    for rec in r[6:]:
        t, w, g, a = (int(v) - 1 for v in rec[:4])
        assert len(rec) == 4 + nf, rec
        base = (((t * nw + w) * ng + g) * na + a) * nf
        assert values[base] is None
        values[base:base + nf] = rec[4:]
    assert None not in values and len(r) == 6 + nt * nw * ng * na
    out = dict(source="tests/VFPPROD2, deck units as written (METRIC)", kind="VFPPROD", table_num=int(head[0]), datum_depth=head[1],
               flo_type=head[2], wfr_type=head[3], gfr_type=head[4],
               units=dict(system="METRIC", pressure_pa_per_unit=1e5, liquid_rate_divide_by=86400.0, length_m_per_unit=1.0,
                          note="SI = barsa * 1e5, (Sm3/day) / 86400; WCT and GOR (Sm3/Sm3) are ratios"),
               flo_axis=flo, thp_axis=thp, wfr_axis=wfr, gfr_axis=gfr, alq_axis=alq,
               layout="values[((((thp * nwfr + wfr) * ngfr + gfr) * nalq + alq) * nflo + flo)]", values=values)
    path = os.path.join(GOLDEN, "vfpprod2_table.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
    print("wrote", path, (nt, nw, ng, na, nf), os.path.getsize(path))


def expected():
    with open(os.path.join(REF, "tests", "test_vfpproperties.cpp")) as f:
        txt = f.read()
    lines = txt.splitlines()

    def array(name):
        m = re.search(r"double\s+" + name + r"\[\]\s*=\s*\{(.*?)\};", txt, re.S)
        return [float(t) for t in re.findall(NUMBER, m.group(1))]
    tol = {k: float(re.search(r"const double " + k + r" = (" + NUMBER + ");", txt).group(1)) for k in ("max_d_tol", "sad_tol")}
    # findInterpData (:60-99): the axis, the six probes in the order eval0..eval5, their expectations
    sec = "\n".join(lines[59:100])
    axis = [float(t) for t in re.findall(NUMBER, re.search(r"values = \{(.*?)\}", sec).group(1))]
    probe = {n: float(v) for n, v in re.findall(r"double (\w+) = (" + NUMBER + ");", sec)}
    order = re.findall(r"eval(\d) = Opm::detail::findInterpData\((\w+), values\)", sec)
    cases = []
    for k, name in order:
        i0 = int(re.search(r"eval%s\.ind_\[0\], (\d+)" % k, sec).group(1))
        i1 = int(re.search(r"eval%s\.ind_\[1\], (\d+)" % k, sec).group(1))
        fac = float(re.search(r"eval%s\.factor_, (%s)\)" % (k, NUMBER), sec).group(1))
        cases.append(dict(name=name, value=probe[name], i0=i0, i1=i1, factor=fac))
    assert len(cases) == 6
    # ParseInterpolateLine (:574-590): the deck record, FIELD units; (:599-613) the grid
    sec = "\n".join(lines[573:591])
    head = re.search(r"^(\d+) (" + NUMBER + r") (\w+) (\w+) (\w+) THP ' ' FIELD BHP /", sec, re.M)
    axes = [[float(t) for t in re.findall(NUMBER, a)] for a in re.findall(r"^([-+0-9.eE ]+)/ (?:flo|THP|WFR|GFR|ALQ) axis", sec, re.M)]
    rows = [[float(t) for t in re.findall(NUMBER, a)] for a in re.findall(r"^(\d \d \d \d [-+0-9.eE ]+)/", sec, re.M)]
    assert len(axes) == 5 and len(rows) == 2
    grid = "\n".join(lines[598:614])
    steps = {n: float(v) for n, v in re.findall(r"double (\w+) = \w \* (" + NUMBER + ");", grid)}
    line = dict(kind="VFPPROD", table_num=int(head.group(1)), datum_depth=float(head.group(2)), flo_type=head.group(3), wfr_type=head.group(4),
                gfr_type=head.group(5),
                units=dict(system="FIELD", pressure_pa_per_unit=6894.757293168361, length_m_per_unit=0.3048,
                           liquid_rate_m3s_per_unit=0.158987294928 / 86400.0, note="psia, ft, stb/day"),
                flo_axis=axes[0], thp_axis=axes[1], wfr_axis=axes[2], gfr_axis=axes[3], alq_axis=axes[4],
                values=[rows[0][4], rows[1][4]],
                grid=dict(n=int(re.search(r"const int n = (\d+);", grid).group(1)), loop_order=["aqua", "liquid", "vapour", "thp", "alq"],
                          step=steps, note="inputs are SI already (the properties take SI): aqua = w * step, ...; bhp_ref = thp_ref = thp"))
    liq, gor, wct, thp = array("liq"), array("gor"), array("wct"), array("thp")
    m = re.search(r"const double reference\[\] = \{(.*?)\};", txt, re.S)
    ref = [float(t) for t in re.findall(NUMBER, m.group(1))]
    assert len(ref) == 8 ** 4 and len(liq) == len(gor) == len(wct) == len(thp) == 8
    out = dict(source="tests/test_vfpproperties.cpp", max_d_tol=tol["max_d_tol"], sad_tol=tol["sad_tol"],
               find_interp_data=dict(axis=axis, cases=cases), parse_interpolate_line=line,
               realistic=dict(table="vfpprod2_table.json", table_num=32, liq=liq, gor=gor, wct=wct, thp=thp, alq=0.0,
                              loop_order=["thp", "wct", "gor", "liq"],
                              semantics="f_i = -liq * 1.1574074074074073e-05; t_i = thp * 100000.0; aqua = wct * f_i; liquid = f_i - aqua; "
                                        "vapour = gor * liquid; skipped (but counted) where (aqua + liquid) == 0.0 or liquid == 0.0; "
                                        "compared: bhp(32, aqua, liquid, vapour, t_i, 0.0) * 10.0e-6 against reference[i] (barsa)",
                              reference=ref))
    path = os.path.join(GOLDEN, "vfp_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
    print("wrote", path, len(ref), os.path.getsize(path))


if __name__ == "__main__":
    vfpprod2()
    expected()
