"""k_conv_pass1 / k_conv_final1 / k_conv_pass2 / k_conv_final2 at their edges, against the numpy statement of
tests/newton_ref.py (math.fsum, np.max).  The residual is the test's own: after one assembly opmhip_upload_system(NULL, b)
writes b into the array the convergence kernels read, so a value can be put at any internal position (opmhip_get_ordering
says where a natural cell lives).  Sizes: one lane, one wave and one workgroup with a lane less, exactly full and a lane
more; 256 full workgroups (one round of the final kernels' loop, exactly), 257 (a second round) and a ragged grid."""
import math
import uuid

import numpy as np
import pytest

import newton_ref
from test_gpu_dd import global_and_parts, run_ranks

pytestmark = pytest.mark.gpu

SIZES = {1: (1, 1, 1), 63: (1, 1, 63), 64: (1, 1, 64), 65: (1, 1, 65), 255: (1, 1, 255), 256: (1, 1, 256), 257: (1, 1, 257),
         65536: (64, 32, 32), 65792: (257, 16, 16), 67240: (41, 41, 40)}
DT, TOL = 86400.0, 1e-2
U = 2.0 ** -52


class Ctx:
    def __init__(self, pkg, n):
        self.pkg, self.Nb = pkg, n
        self.case = case = pkg.decks.cartesian_case(*SIZES[n], state="mixed", heterogeneous=False)
        assert case["Nb"] == n
        self.m = m = pkg.capi.HipModel(case, reorder="graph_coloring_greedy")
        m.set_state(case["pv"], case["meaning"])
        m.assemble(DT, 0, fetch=False)
        self.to, self.fr, _ = m.ordering()
        self.inv_b = m.iq()[:n, 6:9, 0].copy()
        self.pv = float(case["poro"][0] * case["volume"][0])
        assert np.all(case["poro"] * case["volume"] == self.pv)        # every pore volume is the same double
        self.b_avg = self.conv(np.zeros((n, 3)))[6:9].copy()            # the averages depend on the state alone
        self.thr = TOL * self.pv / (DT * self.b_avg)                    # |R| at which a cell's CNV reaches the tolerance

    def positions(self):
        """internal indices where reductions go wrong: ends of the first wave and of the first workgroup, the last cell, the first
        cell of the last workgroup, and the first cell the final kernels meet in their second round"""
        n = self.Nb
        pos = [0, 63, 64, 255, 256, n - 1, (n - 1) // 256 * 256] + ([65536] if n > 65536 else [])
        return sorted(set(p for p in pos if p < n))

    def plant(self, r_internal):
        """r_internal[i] = the residual of the cell at internal index i"""
        b = np.empty((self.Nb, 3))
        b[self.fr] = r_internal
        self.m.upload_system(None, b.reshape(-1))
        return b

    def conv(self, r_internal):
        self.resid = self.plant(r_internal)
        return self.m.convergence(DT, TOL)

    def ref(self, b_avg=None):
        return newton_ref.convergence(self.resid, self.case["poro"], self.case["volume"], self.inv_b, DT, TOL, b_avg=b_avg)


@pytest.fixture(scope="module", params=list(SIZES))
def ctx(pkg, request):
    return Ctx(pkg, request.param)


def depth(n):
    """the depth of the device's summation tree as the kernels are written: 6 shuffle steps, 3 additions over the waves,
    the rounds of the final kernel's loop, 8 halvings"""
    return 6 + 3 + math.ceil(math.ceil(n / 256) / 256) + 8


def test_planted_residual_is_the_one_read(ctx):
    rng = np.random.default_rng(ctx.Nb)
    r = rng.standard_normal((ctx.Nb, 3))
    b = ctx.plant(r)
    assert np.array_equal(ctx.m.get_rhs(), b.reshape(-1))
    assert np.array_equal(b[ctx.fr], r) and np.array_equal(ctx.to[ctx.fr], np.arange(ctx.Nb))


def test_exact_sums(ctx):
    """multiples of 2^-10 below 2^20 with mixed signs: every partial sum is exact in any order, so the sums are numpy's to the bit"""
    n = ctx.Nb
    rng = np.random.default_rng(1000 + n)
    r = rng.integers(-2 ** 29, 2 ** 29, (n, 3)) / 2.0 ** 10
    r[rng.random(n) < 0.5] = 0.0                       # about half the cells hold no residual at all: not violated
    r[n - 1] = (0.0, -3.0, 0.0)
    c = ctx.conv(r)
    ref, violated, dist = ctx.ref(b_avg=c[6:9])
    assert dist.min() >= 1e-9
    assert np.array_equal(c[0:3], r.sum(axis=0)) and np.array_equal(c[0:3], ref[0:3])
    assert np.array_equal(c[3:6], np.abs(r).max(axis=0) / ctx.pv)
    assert c[9] == n * ctx.pv
    k = int(violated.sum())
    assert c[10] == k * ctx.pv and (n == 1 or 0 < k < n)
    assert np.array_equal(c[11:14], c[6:9] * DT * c[3:6]) and np.array_equal(c[14:17], np.abs(c[6:9] * c[0:3]) * DT / c[9])


def test_rounded_sums(ctx):
    """random normal residuals over twelve decades: each sum lies within d 2^-52 sum|x| of fsum, d the depth of the device's tree;
    the factor 2 over the unit roundoff is the margin"""
    n = ctx.Nb
    rng = np.random.default_rng(2000 + n)
    r = rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-6.0, 6.0, (n, 3))
    c = ctx.conv(r)
    ref, _, _ = ctx.ref()
    d = depth(n)
    print(n, d, np.abs(c[0:3] - ref[0:3]) / (U * np.abs(r).sum(axis=0)), np.abs(c[6:9] - ref[6:9]) / (U * ref[6:9]))
    assert np.all(np.abs(c[0:3] - ref[0:3]) <= d * U * np.abs(r).sum(axis=0))
    for ph, e in enumerate(newton_ref.EQ_OF_PHASE):
        assert abs(c[6 + e] - ref[6 + e]) <= d * U * math.fsum(1.0 / ctx.inv_b[:, ph]) / n
    assert abs(c[9] - ref[9]) <= d * U * ref[9]
    assert np.array_equal(c[3:6], ref[3:6])


def test_where_the_maximum_sits(ctx):
    """the largest |R| / pv of each component at a position of its own, every other cell strictly smaller"""
    n = ctx.Nb
    rng = np.random.default_rng(3000 + n)
    pos = ctx.positions()
    for k in range(len(pos)):
        r = rng.uniform(-1.0, 1.0, (n, 3)) * 1e-7
        top = np.array([3.0, -5.0, 7.0]) * (1.0 + 0.125 * k)
        at = [pos[(k + e) % len(pos)] for e in range(3)]
        for e in range(3):
            r[at[e], e] = top[e]
        c = ctx.conv(r)
        assert np.array_equal(c[3:6], np.abs(top) / ctx.pv), (k, at)
        assert np.array_equal(c[11:14], c[6:9] * DT * c[3:6])
        assert np.array_equal(c[3:6], ctx.ref()[0][3:6])


def violated_sets(ctx):
    """(name, internal indices, component or None = all three, sign or None = mixed)"""
    n = ctx.Nb
    idx = np.arange(n)
    sets = [("none", idx[:0], None, None), ("all", idx, None, None)]
    for k, p in enumerate(ctx.positions()):
        sets.append(("one cell at %d" % p, idx[p:p + 1], (2, 0, 1)[k % 3], (-1.0, 1.0)[(k // 3 + k) % 2]))
    blk = 1 if n > 256 else 0
    sets.append(("one whole workgroup", idx[256 * blk:256 * (blk + 1)], None, None))
    sets.append(("every second wave", idx[(idx // 64) % 2 == 1], None, None))
    return sets


def test_the_violated_set(ctx):
    """cnvErrorPv = the pore volume of the cells with |CNV| > tol in any component, decided in numpy from the device's own B_avg;
    a violating entry is 4 times the residual at which CNV meets the tolerance, every other entry a quarter of it"""
    n = ctx.Nb
    rng = np.random.default_rng(4000 + n)
    sets = violated_sets(ctx)
    assert any(s[2] == 2 for s in sets) and any(s[3] == -1.0 for s in sets)      # only the third component; a negative residual
    for name, cells, comp, sign in sets:
        r = 0.25 * ctx.thr[None, :] * np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0)
        if comp is None:
            r[cells] *= 16.0
        else:
            r[cells, comp] = sign * 4.0 * ctx.thr[comp]
        c = ctx.conv(r)
        ref, violated, dist = ctx.ref(b_avg=c[6:9])
        assert dist.min() >= 1e-9 and np.array_equal(c[6:9], ctx.b_avg)
        want = np.zeros(n, bool)
        want[ctx.fr[cells]] = True
        assert np.array_equal(violated, want), name
        assert c[10] == len(cells) * ctx.pv, (name, c[10] / ctx.pv, len(cells))


@pytest.mark.parametrize("what", ["nan", "+inf", "-inf"])
def test_non_finite_residuals(ctx, what):
    """one non-finite entry, in turn at the first cell, the last cell and index 256.  fmax drops a NaN as the reference's
    std::max(maxCoeff, NaN) does (flow/BlackoilModelEbos.hpp:668), so maxCoeff and CNV of that component stay finite and the
    NaN is seen through R_sum and MB alone - which is what newton.py's "NaN residual found!" relies on.  An infinite entry
    shows in both: CNV = +inf, MB = +inf, "Too large residual found!"."""
    n = ctx.Nb
    newton = ctx.pkg.newton
    v = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[what]
    rng = np.random.default_rng(5000 + n)
    r0 = rng.standard_normal((n, 3)) * 1e-6
    base = ctx.conv(r0).copy()
    assert np.all(np.isfinite(base))
    for k, p in enumerate(sorted(set(q for q in (0, n - 1, 256) if q < n))):
        e = (k + n) % 3
        r = r0.copy()
        r[p, e] = v
        c = ctx.conv(r)
        ref, _, _ = ctx.ref(b_avg=c[6:9])
        others = [i for i in range(17) if i not in (e, 3 + e, 10, 11 + e, 14 + e)]
        assert np.array_equal(c[others], base[others]), (p, e)
        with np.errstate(over="ignore"):
            assert c[3 + e] == ref[3 + e] and c[11 + e] == c[6 + e] * DT * c[3 + e]
        assert c[10] == ref[10] == (0.0 if what == "nan" else ctx.pv)        # a NaN compares false: the cell does not count as violated
        if what == "nan":
            # (one cell: nothing is left to take the maximum of, maxCoeff stays at lowest() and B_avg dt lowest() overflows to -inf,
            # in the reference as here)
            assert np.isnan(c[e]) and np.isnan(c[14 + e]) and np.isfinite(c[3 + e]) and (np.isfinite(c[11 + e]) or n == 1)
        else:
            assert c[e] == v and c[3 + e] == np.inf and c[11 + e] == np.inf and c[14 + e] == np.inf
        msg = newton_ref.failure(ref)
        assert msg == ("NaN residual found!" if what == "nan" else "Too large residual found!")
        with pytest.raises(newton.NumericalIssue) as err:
            newton.BlackoilModelHip(ctx.m).get_convergence(DT, 1)
        assert str(err.value) == msg
    ctx.conv(r0)
    assert newton.BlackoilModelHip(ctx.m).get_convergence(DT, 1)[0] in (True, False)      # and no exception without it


def test_two_ranks_return_the_global_numbers(pkg):
    """a two-rank loopback pair, the residual planted per rank: the maximum on rank 1, a violated cell on each rank; every rank
    returns the 17 numbers of the numpy statement over the owned cells of both"""
    world, n = 2, 6
    g, owner, parts = global_and_parts(pkg, n, world, state="mixed", heterogeneous=False)
    group = "v" + uuid.uuid4().hex
    planted = []
    for r in range(world):
        b = np.zeros((parts[r]["Nb"], 3))
        b[5 + 90 * r, (newton_ref.EQ_WATER, newton_ref.EQ_OIL)[r]] = (-0.5, 8.0)[r]     # binary-exact: the sums are exact
        planted.append(b)

    def rank_fn(r):
        c = parts[r]
        m = pkg.capi.HipModel(c, comm=("loopback", world, r, group), reorder="graph_coloring_greedy")
        m.set_state(c["pv"], c["meaning"])
        m.assemble(DT, 0, fetch=False)
        m.upload_system(None, planted[r].reshape(-1))
        return m.convergence(DT, TOL), m.iq()[:c["Nb"], 6:9, 0].copy(), m.get_rhs()

    outs = run_ranks(world, rank_fn)
    for r in range(world):
        assert np.array_equal(outs[r][2], planted[r].reshape(-1))
    own = lambda k: np.concatenate([np.asarray(parts[r][k])[:parts[r]["Nb"]] for r in range(world)])
    N = sum(p["Nb"] for p in parts)
    c = outs[0][0]
    ref, violated, dist = newton_ref.convergence(np.concatenate(planted), own("poro"), own("volume"), np.concatenate([o[1] for o in outs]), DT, TOL, b_avg=c[6:9])
    assert all(np.array_equal(o[0], c) for o in outs)
    pvv = 500.0
    assert np.all(own("poro") * own("volume") == pvv) and dist.min() >= 1e-9 and violated.sum() == 2
    assert np.array_equal(c[0:3], ref[0:3]) and c[newton_ref.EQ_OIL] == 8.0 and c[newton_ref.EQ_WATER] == -0.5
    assert np.array_equal(c[3:6], ref[3:6]) and c[3 + newton_ref.EQ_OIL] == 8.0 / pvv
    assert c[9] == N * pvv and c[10] == 2 * pvv
    d = depth(parts[0]["Nb"]) + 1                     # the ranks' sums are added once more
    assert np.all(np.abs(c[6:9] - ref[6:9]) <= d * U * ref[6:9])
    assert np.array_equal(c[11:14], c[6:9] * DT * c[3:6]) and np.array_equal(c[14:17], np.abs(c[6:9] * c[0:3]) * DT / c[9])
