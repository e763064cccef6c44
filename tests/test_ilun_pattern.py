"""Block ILU(n) (--ilu-fillin-level), the host side: the C ABI exports the new entry points, and the symbolic ILU(n) of csrc/reorder.cpp -
fill rule, level schedule, L/U split, memory guard, distance-2 colouring - built with g++ under AddressSanitizer + UBSan (tests/san/ilun_san.cpp,
the way tests/test_host_logic_sanitized.py builds the rest of reorder.cpp) and compared with the rule restated here in Python: entries of A
have generation 0; row i walks its entries left of the diagonal in ascending column order, fill made earlier in the row included; an entry
(i, k) of generation < n pivots row k, whose entries (k, j), j >= k, of generation < n create a missing (i, j) with generation gen(k, j) + 1.
No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opm-autodiff_amd", "csrc")
LEVEL, JP, GREEDY, LINE, AUTO, D2 = 1, 2, 3, 4, 5, 6
BUDGET = 8   # csrc/internal.hpp: ILUN_BUDGET_FACTOR


def test_library_exports_the_fill_level_calls(pkg):
    L = pkg.capi.lib()
    for name in ("opmhip_set_ilu_fillin_level", "opmhip_get_ilu_info", "opmhip_get_ilu_factors"):
        assert hasattr(L, name), name
        assert name in pkg.capi.declared_symbols()
    assert pkg.capi.REORDER["distance2"] == 6


# ---- patterns ------------------------------------------------------------------------------------------------------------------------
def grid(nx, ny, nz):
    rows = []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                c = i + nx * (j + ny * k)
                r = [c]
                if i > 0: r.append(c - 1)
                if i + 1 < nx: r.append(c + 1)
                if j > 0: r.append(c - nx)
                if j + 1 < ny: r.append(c + nx)
                if k > 0: r.append(c - nx * ny)
                if k + 1 < nz: r.append(c + nx * ny)
                rows.append(set(r))
    return rows


def irregular(nx, ny, nz, seed):
    """a grid with non-neighbour connections along the xy diagonal (triangles with the 7-point couplings) and a well clique"""
    rows = grid(nx, ny, nz)
    rng = np.random.default_rng(seed)
    n = len(rows)
    for c in rng.choice(n, size=max(1, n // 5), replace=False):
        i, j = c % nx, (c // nx) % ny
        if i + 1 < nx and j + 1 < ny:
            d = c + 1 + nx
            rows[c].add(d)
            rows[d].add(c)
    col = int(rng.integers(nx * ny))
    well = [col + nx * ny * k for k in range(nz)]
    for a in well:
        rows[a].update(well)
    return rows


def to_csr(rows):
    rp, cl = [0], []
    for r in rows:
        cl.extend(sorted(r))
        rp.append(len(cl))
    return np.array(rp, np.int32), np.array(cl, np.int32)


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------------
def fill_pattern(rows, n, limit=None):
    """rows: list of sets (ascending elimination order) -> list of dicts col -> generation; None as soon as the rows hold more than
    `limit` entries (the memory guard's question, answered without filling the rest)"""
    F = []
    total = 0
    for i, r in enumerate(rows):
        pat = {j: 0 for j in r}
        k = -1
        while True:
            lower = [j for j in pat if k < j < i]
            if not lower:
                break
            k = min(lower)
            if pat[k] < n:
                for j, g in F[k].items():
                    if j >= k and g < n and j not in pat:
                        pat[j] = g + 1
        F.append(pat)
        total += len(pat)
        if limit is not None and total > limit:
            return None
    return F


def distance2_colours(rows):
    nb = [set(r) for r in rows]
    for i, r in enumerate(rows):
        for j in r:
            nb[j].add(i)
    colour = [-1] * len(rows)
    for i in range(len(rows)):
        taken = set()
        for j in nb[i]:
            for m in nb[j] | {j}:
                if m != i and colour[m] >= 0:
                    taken.add(colour[m])
        c = 0
        while c in taken:
            c += 1
        colour[i] = c
    return colour


# ---- the harness ----------------------------------------------------------------------------------------------------------------------
def parse(path):
    out, lines, p = [], open(path).read().split("\n"), 0

    def vec():
        nonlocal p
        v = [int(x) for x in lines[p].split()]
        p += 1
        return np.array(v[1:], np.int64)
    while p < len(lines) and lines[p].startswith("case"):
        rc = int(lines[p].split()[3])
        p += 1
        if rc != 0:
            out.append({"rc": rc})
            continue
        levels = int(lines[p].split()[1])
        p += 1
        d = {"rc": 0, "levels": levels}
        for k in ("base", "to", "prefix", "lrp", "lcl", "urp", "ucl"):
            d[k] = vec()
        out.append(d)
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("ilun") / "ilun_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D_GLIBCXX_ASSERTIONS", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "san", "ilun_san.cpp"), os.path.join(CSRC, "reorder.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def run(harness, tmp_path, cases):
    """cases: [(rows, kind, n)] -> parsed results; the harness's own checks and the sanitizers must pass"""
    inp, outp = tmp_path / "cases.txt", tmp_path / "out.txt"
    with open(inp, "w") as f:
        for rows, kind, n in cases:
            rp, cl = to_csr(rows)
            f.write("%d %d %d %d\n%s\n%s\n" % (len(rows), len(cl), kind, n, " ".join(map(str, rp)), " ".join(map(str, cl))))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("OPMHIP_TUNING", None)
    r = subprocess.run([harness, str(inp), str(outp)], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    return parse(outp)


def natural_fill_of(res):
    """the harness's filled pattern as a set of (row, column) pairs in natural numbering"""
    to = res["to"]
    fr = np.empty_like(to)
    fr[to] = np.arange(len(to))
    s = set()
    for p in range(len(to)):
        i = int(fr[p])
        s.add((i, i))
        for q in range(res["lrp"][p], res["lrp"][p + 1]):
            s.add((i, int(fr[res["lcl"][q]])))
        for q in range(res["urp"][p], res["urp"][p + 1]):
            s.add((i, int(fr[res["ucl"][q]])))
    return s


def restated_fill(rows, base, n, limit=None):
    """the fill rule in the elimination order `base` (natural row -> position), back in natural numbering; None: more than `limit` entries"""
    N = len(rows)
    ib = np.empty(N, np.int64)
    ib[base] = np.arange(N)
    prow = [{int(base[j]) for j in rows[int(ib[b])]} for b in range(N)]
    F = fill_pattern(prow, n, limit)
    if F is None:
        return None
    return {(int(ib[b]), int(ib[j])) for b in range(N) for j in F[b]}


GRIDS = [(1, 1, 1), (2, 1, 1), (5, 1, 1), (3, 3, 1), (4, 3, 2), (6, 5, 4), (9, 8, 7), (12, 10, 8)]


@pytest.mark.parametrize("n", [1, 2])
def test_fill_matches_the_rule_restated(harness, tmp_path, n):
    cases = []
    grids = GRIDS if n == 1 else GRIDS[:6]
    for g in grids:
        for kind in (LEVEL, JP, GREEDY, LINE, AUTO, D2):
            cases.append((grid(*g), kind, n))
    for seed, g in enumerate([(5, 4, 3), (7, 6, 5)] if n == 1 else [(4, 4, 3)]):
        for kind in (LEVEL, JP, GREEDY, LINE, AUTO, D2):
            cases.append((irregular(*g, seed), kind, n))
    results = run(harness, tmp_path, cases)
    assert len(results) == len(cases)
    for (rows, kind, _), res in zip(cases, results):
        nnzb = sum(len(r) for r in rows)
        if res["rc"] != 0:   # only the memory guard may refuse, and only where the rule's fill is over the budget
            assert res["rc"] == -4, res
            if kind == LEVEL:
                assert len(restated_fill(rows, np.arange(len(rows)), n)) > BUDGET * nnzb
            continue
        if kind == LEVEL:   # the reference's natural-order fill
            assert np.array_equal(res["base"], np.arange(len(rows)))
        assert sorted(res["base"]) == list(range(len(rows)))
        assert natural_fill_of(res) == restated_fill(rows, res["base"], n), (kind, len(rows))
        assert {(i, j) for i, r in enumerate(rows) for j in r} <= natural_fill_of(res)


def test_distance2_colouring_is_the_schedule_of_ilu1(harness, tmp_path):
    shapes = [(1, 1, 1), (3, 3, 1), (6, 5, 4), (10, 9, 8), (20, 20, 20)]
    cases = [(grid(*g), D2, 1) for g in shapes] + [(irregular(6, 6, 5, 3), D2, 1), (grid(10, 9, 8), AUTO, 1)]   # AUTO with n >= 1: distance-2
    for (rows, _, _), res in zip(cases, run(harness, tmp_path, cases)):
        assert res["rc"] == 0
        colour = distance2_colours(rows)
        ncol = max(colour) + 1
        assert res["levels"] == ncol                       # levels equal colours: nothing was renumbered
        prefix = res["prefix"]
        level_of = np.searchsorted(prefix, res["to"], side="right") - 1
        assert np.array_equal(level_of, np.array(colour))  # every row sits in its colour


def test_ilu0_distance2_is_a_valid_ordering(harness, tmp_path):
    cases = [(grid(*g), D2, 0) for g in [(4, 3, 2), (9, 8, 7)]] + [(irregular(5, 4, 3, 1), D2, 0)]
    for res in run(harness, tmp_path, cases):
        assert res["rc"] == 0


def test_memory_guard_refuses_ilu2_on_a_20_cube(harness, tmp_path):
    res = run(harness, tmp_path, [(grid(20, 20, 20), LEVEL, 2), (grid(20, 20, 20), LEVEL, 1)])
    assert res[0]["rc"] == -4            # OPMHIP_INVALID_ARGUMENT: refused, nothing allocated
    assert res[1]["rc"] == 0 and res[1]["levels"] > 20


# ---- the exact-LU limit ---------------------------------------------------------------------------------------------------------------
EXACT_GRIDS = [(6, 5, 1), (4, 3, 2), (5, 4, 3), (8, 6, 1), (1, 1, 30)]   # natural order: the complete fill fits 8 x nnzb


def complete_fill(rows, base):
    """the filled pattern of the complete LU by a plain dense boolean elimination of the pattern taken in the elimination order `base`
    (natural row -> position), back in natural numbering"""
    N = len(rows)
    B = np.zeros((N, N), bool)
    for i, r in enumerate(rows):
        B[base[i], [base[j] for j in r]] = True
    for k in range(N):
        below = k + 1 + np.flatnonzero(B[k + 1:, k])
        B[np.ix_(below, np.arange(k + 1, N))] |= B[k, k + 1:]
    ib = np.empty(N, np.int64)
    ib[base] = np.arange(N)
    return {(int(ib[a]), int(ib[b])) for a, b in zip(*np.nonzero(B))}


def test_fill_level_of_the_size_is_the_complete_lu(harness, tmp_path):
    """n >= Nb: no generation reaches n, so the symbolic pass is the complete symbolic LU - in every ordering whose complete fill fits the
    budget; where it does not, the guard refuses.  The elimination order comes from the same ordering at n = 1 (it does not depend on n)."""
    kinds = (LEVEL, JP, GREEDY, LINE, AUTO, D2)
    cases, shapes = [], []
    for g in EXACT_GRIDS + [(6, 5, 4)]:   # (6, 5, 4): 5818 blocks of complete fill against a budget of 5536 in natural order
        N = g[0] * g[1] * g[2]
        for kind in kinds:
            cases += [(grid(*g), kind, 1), (grid(*g), kind, N), (grid(*g), kind, N + 7)]
            shapes.append(g)
    results = run(harness, tmp_path, cases)
    for q in range(0, len(cases), 3):
        rows, kind, _ = cases[q]
        r1, rN, rM = results[q:q + 3]
        assert r1["rc"] == 0
        full = complete_fill(rows, r1["base"])
        assert full == restated_fill(rows, r1["base"], len(rows))       # the rule restated reaches the same limit
        nnzb = sum(len(r) for r in rows)
        for res in (rN, rM):
            if len(full) > BUDGET * nnzb:
                assert res["rc"] == -4, (kind, len(rows))
                continue
            assert res["rc"] == 0 and np.array_equal(res["base"], r1["base"])
            assert natural_fill_of(res) == full, (kind, len(rows))
        if kind == LEVEL:
            assert (rN["rc"] == 0) == (shapes[q // 3] in EXACT_GRIDS)     # natural order: the complete LU fits the budget, but for (6, 5, 4)
