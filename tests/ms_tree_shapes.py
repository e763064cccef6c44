"""Segment trees for the tests of the multisegment wells' tree form, as parent arrays (parents[i] < i, segment 0 the root: the rooting the
device chooses), and the wells built on them (test infrastructure)."""
import numpy as np


def chain(n):
    return [i - 1 for i in range(n)]


def star(n):
    """one parent with n - 1 children"""
    return [-1] + [0] * (n - 1)


def comb(n, lateral=3):
    """a spine with a lateral chain of `lateral` segments on every spine segment; n a multiple of lateral + 1"""
    g = lateral + 1
    assert n % g == 0
    par = []
    for i in range(n):
        par.append(i - g if i % g == 0 else i - 1)
    par[0] = -1
    return par


def random_tree(n, seed):
    rng = np.random.default_rng(seed)
    return [-1] + [int(rng.integers(0, i)) for i in range(1, n)]


SHAPES = {"chain1": chain(1), "chain2": chain(2), "chain5": chain(5), "chain65": chain(65), "chain130": chain(130), "star71": star(71),
          "comb120": comb(120), "random150": random_tree(150, 7), "random300": random_tree(300, 8)}


def depth(parents):
    lev = []
    for i, p in enumerate(parents):
        lev.append(0 if p < 0 else lev[p] + 1)
    return max(lev) + 1


def well(pkg, parents, cells, seed, offd=0.6):
    """the per-well dict of a well over the tree `parents` that perforates `cells` (spread over the segments in ascending order)"""
    rng = np.random.default_rng(seed)
    Mb = len(parents)
    D = pkg.mswells.D_from_parents(parents, rng, offd)
    nblk = len(cells)
    seg = np.sort(np.arange(nblk) % Mb) if nblk >= Mb else (np.arange(nblk) * Mb) // nblk   # fewer cells than segments: spread over the whole tree
    return pkg.mswells.well_from(D, seg, cells, rng.uniform(-1, 1, (nblk, 4, 3)), rng.uniform(-1, 1, (nblk, 4, 3)))


def scale_rows(pkg, w, rng):
    """rows of D scaled by 10^U(-4, 4), the rows of B with them (z2 is unchanged in exact arithmetic): the construction of
    tests/test_gpu_ms_wells_device.py::test_badly_scaled_rows, in place"""
    Mb = len(w["Brows"]) - 1
    _, _, D = pkg.mswells.dense_operators(w, int(np.max(w["Bcols"])) + 1)
    sc = 10.0 ** rng.uniform(-4, 4, 4 * Mb)
    D = sc[:, None] * D
    w["Dcolptr"], w["Drows"], w["Dvals"] = pkg.mswells.csc(D)
    Bv = w["Bvals"].reshape(-1, 4, 3).copy()
    brow = np.repeat(np.arange(Mb), np.diff(w["Brows"]))
    for blk in range(len(Bv)):
        Bv[blk] *= sc[4 * brow[blk]:4 * brow[blk] + 4, None]
    w["Bvals"] = Bv.reshape(-1)
    return w
