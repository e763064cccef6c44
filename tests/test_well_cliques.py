"""grid.with_well_cliques / decks.with_well_cliques: the pattern that also holds a block for every pair of one well's perforated cells,
and the case on it (no GPU)."""
import numpy as np
import pytest


def entries(pat):
    rp, col = pat["rowptr"], pat["col"]
    return [(i, int(col[k])) for i in range(pat["Nb"]) for k in range(rp[i], rp[i + 1])]


LISTS = [[3, 33, 63], [63, 64, 94, 100], [7, 8, 7], [50]]   # a column; one that shares a cell with it; a cell twice; one perforation


def test_symmetric_sorted_idempotent(pkg):
    pat = pkg.grid.cartesian_pattern(6, 5, 4)
    new, old_pos = pkg.grid.with_well_cliques(pat, LISTS)
    e_old, e_new = entries(pat), entries(new)
    rp, col = new["rowptr"], new["col"]
    assert rp.dtype == np.int32 and col.dtype == np.int32 and rp[0] == 0 and rp[-1] == len(col) and new["Nb"] == pat["Nb"]
    for i in range(new["Nb"]):
        assert np.all(np.diff(col[rp[i]:rp[i + 1]]) > 0), i                      # sorted, no duplicate
    s = set(e_new)
    assert len(s) == len(e_new) and all((j, i) in s for i, j in s)               # symmetric
    want = set(e_old) | {(a, b) for cells in LISTS for a in cells for b in cells}
    assert s == want and len(s) > len(e_old)                                     # exactly the stencil and the cliques
    assert (3, 63) in s and (63, 3) in s and (3, 3) in s and (3, 64) not in s    # (pairs of one well only)
    again, pos2 = pkg.grid.with_well_cliques(new, LISTS)                         # idempotent
    assert np.array_equal(again["rowptr"], rp) and np.array_equal(again["col"], col) and np.array_equal(pos2, np.arange(len(col)))
    assert np.array_equal(again["face_dir"], new["face_dir"])


def test_old_entries_keep_their_values_through_old_pos(pkg):
    pat = pkg.grid.cartesian_pattern(6, 5, 4)
    new, old_pos = pkg.grid.with_well_cliques(pat, LISTS)
    e_old, e_new = entries(pat), entries(new)
    assert len(old_pos) == len(e_old) and len(set(old_pos.tolist())) == len(e_old)
    assert [e_new[k] for k in old_pos] == e_old
    assert np.array_equal(new["face_dir"][old_pos], pat["face_dir"])
    fresh = np.ones(len(e_new), bool)
    fresh[old_pos] = False
    assert np.all(new["face_dir"][fresh] == pkg.grid.CLIQUE_FACE) and fresh.sum() == len(e_new) - len(e_old)
    assert (3, 33) in e_old and (3, 63) not in e_old                             # vertical neighbours were there, the cell two layers down was not


def test_a_one_perforation_well_adds_nothing(pkg):
    pat = pkg.grid.cartesian_pattern(6, 5, 4)
    new, old_pos = pkg.grid.with_well_cliques(pat, [[50], [0], [119]])
    assert np.array_equal(new["rowptr"], pat["rowptr"]) and np.array_equal(new["col"], pat["col"]) and np.array_equal(old_pos, np.arange(len(pat["col"])))
    assert np.array_equal(new["face_dir"], pat["face_dir"])
    none, pos = pkg.grid.with_well_cliques(pat, [])
    assert np.array_equal(none["col"], pat["col"]) and np.array_equal(pos, old_pos)
    with pytest.raises(ValueError):
        pkg.grid.with_well_cliques(pat, [[0, 120]])


def test_the_case_on_the_clique_pattern(pkg):
    """trans and thpres 0, area 1.0 on the new entries (the flux divides by the area); everything else as it was"""
    case = pkg.decks.cartesian_case(6, 5, 4, heterogeneous=True)
    case["thpres"] = np.where(case["trans"] > 0.0, 1.0e4, 0.0)

    class W:
        def __init__(self, cells):
            self.cells = np.asarray(cells)
    cq = pkg.decks.with_well_cliques(case, [W(c) for c in LISTS])
    pat, old_pos = pkg.grid.with_well_cliques(dict(Nb=case["Nb"], rowptr=case["rowptr"], col=case["col"]), LISTS)
    assert np.array_equal(cq["rowptr"], pat["rowptr"]) and np.array_equal(cq["col"], pat["col"])
    fresh = np.ones(len(pat["col"]), bool)
    fresh[old_pos] = False
    for key, fill in (("trans", 0.0), ("thpres", 0.0), ("area", 1.0)):
        assert np.array_equal(cq[key][old_pos], case[key]) and np.all(cq[key][fresh] == fill), key
        assert len(cq[key]) == len(pat["col"])
    assert np.all(cq["face_dir"][fresh] == pkg.grid.CLIQUE_FACE)
    for key in ("poro", "volume", "depth", "pv", "meaning", "perm"):
        assert cq[key] is case[key]
    assert len(case["col"]) < len(cq["col"]) and len(case["trans"]) == len(case["col"])       # the case handed in is not changed
    # the per-entry data stay symmetric, as opmhip_set_static asks
    pos = {e: k for k, e in enumerate(entries(pat))}
    tr = np.array([pos[(j, i)] for i, j in entries(pat)])
    for key in ("trans", "area", "thpres"):
        assert np.array_equal(cq[key], cq[key][tr])
    assert np.diff(cq["rowptr"]).max() <= 64
