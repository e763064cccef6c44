"""Multisegment wells as the linear solver sees them: the arrays of Opm::MultisegmentWellContribution (B and C in blocked CSR over one
pattern, 4 x 3 blocks; D in scalar CSC over M = 4 Mb well equations), generated for tests and measurements, and the same operators
as dense matrices.  The per-well dict is what capi.make_ms_wells / HipSolver.set_ms_wells take."""
import numpy as np


def csc(D):
    """dense D -> (Dcolptr, Drows, Dvals) of its non-zeros, column by column (what UMFPack takes)"""
    D = np.asarray(D)
    colptr, rows, vals = [0], [], []
    for c in range(D.shape[1]):
        r = np.nonzero(D[:, c])[0]
        rows.append(r)
        vals.append(D[r, c])
        colptr.append(colptr[-1] + len(r))
    return np.array(colptr, np.int32), np.concatenate(rows).astype(np.int32), np.concatenate(vals).astype(np.float64)


def tree_D(Mb, rng, branch=0.2, offd=0.6):
    """D of a well whose segments form a tree (segment i hangs on i - 1, or with probability `branch` on a random earlier one): diagonal
    blocks U(-1, 1) plus +-4 on the diagonal, parent / child blocks offd * U(-1, 1); rows unscaled"""
    D = np.zeros((4 * Mb, 4 * Mb))
    for i in range(Mb):
        blk = rng.uniform(-1, 1, (4, 4))
        blk += np.diag(np.sign(np.diag(blk)) * 4.0)
        D[4 * i:4 * i + 4, 4 * i:4 * i + 4] = blk
        if i > 0:
            p = i - 1 if rng.random() > branch else int(rng.integers(0, i))
            D[4 * i:4 * i + 4, 4 * p:4 * p + 4] = offd * rng.uniform(-1, 1, (4, 4))
            D[4 * p:4 * p + 4, 4 * i:4 * i + 4] = offd * rng.uniform(-1, 1, (4, 4))
    return D


def D_from_parents(parents, rng, offd=0.6):
    """D of a well whose segment i hangs on parents[i] (-1: a root) - any tree or forest, in any numbering; the blocks as tree_D draws
    them: diagonal blocks U(-1, 1) plus +-4 on the diagonal, the two blocks between a segment and its parent offd * U(-1, 1)"""
    Mb = len(parents)
    D = np.zeros((4 * Mb, 4 * Mb))
    for i in range(Mb):
        blk = rng.uniform(-1, 1, (4, 4))
        blk += np.diag(np.sign(np.diag(blk)) * 4.0)
        D[4 * i:4 * i + 4, 4 * i:4 * i + 4] = blk
        p = int(parents[i])
        if p >= 0:
            D[4 * i:4 * i + 4, 4 * p:4 * p + 4] = offd * rng.uniform(-1, 1, (4, 4))
            D[4 * p:4 * p + 4, 4 * i:4 * i + 4] = offd * rng.uniform(-1, 1, (4, 4))
    return D


def _mm_stated(A, B):
    """A @ B with every entry's sum taken over k ascending from 0.0, one rounding per operation (no fused multiply-add)"""
    s = np.zeros((A.shape[0],) + B.shape[1:])
    for k in range(A.shape[1]):
        s = s + (A[:, k:k + 1] * B[k:k + 1] if B.ndim == 2 else A[:, k] * B[k])
    return s


def tree_solve(D, z, parents):
    """D^-1 z by the block elimination over the segment tree that the device's tree form runs (csrc/wells_operator.hip k_ms_wells_tree_factor and
    k_ms_wells_tree_apply), in float64 and in the device's order of operations; the device roots every component at its lowest segment
    number, so `parents` in that rooting gives its bits.
      factor, from the deepest level up:   S_i = D_ii - sum_c E_c D_ci (children c ascending; each product's entries over k ascending
                                           from 0.0), S_i^-1 by wells.invert4_stated (partial pivoting INSIDE the block), E_i = D_pi S_i^-1
      forward, from the deepest level up:  z_p -= E_c z_c over the children of p, ascending
      backward, from the roots down:       x_i = S_i^-1 (z_i - D_ip x_p)
    No row is exchanged across blocks: a singular S_i raises wells.SingularWellEquations although D may be regular."""
    from .wells import invert4_stated
    parents = [int(p) for p in parents]
    Mb = len(parents)
    D = np.asarray(D, float)
    blk = lambda i, j: D[4 * i:4 * i + 4, 4 * j:4 * j + 4]
    level = [-1] * Mb
    for i in range(Mb):
        path = []
        j = i
        while level[j] < 0 and parents[j] >= 0:
            path.append(j)
            j = parents[j]
        if level[j] < 0:
            level[j] = 0
        for q in reversed(path):
            level[q] = level[parents[q]] + 1
    depth = max(level) + 1
    by_level = [[i for i in range(Mb) if level[i] == l] for l in range(depth)]
    children = [[c for c in range(Mb) if parents[c] == i] for i in range(Mb)]
    Sinv, E = [None] * Mb, [None] * Mb
    for l in range(depth - 1, -1, -1):
        for i in by_level[l]:
            S = blk(i, i).copy()
            for c in children[i]:
                S = S - _mm_stated(E[c], blk(c, i))
            Sinv[i] = invert4_stated(S)
            if parents[i] >= 0:
                E[i] = _mm_stated(blk(parents[i], i), Sinv[i])
    x = np.array(z, float).reshape(Mb, 4).copy()
    for l in range(depth - 2, -1, -1):
        for p in by_level[l]:
            for c in children[p]:
                x[p] = x[p] - _mm_stated(E[c], x[c])
    for l in range(depth):
        for i in by_level[l]:
            v = x[i]
            if parents[i] >= 0:
                v = v - _mm_stated(blk(i, parents[i]), x[parents[i]])
            x[i] = _mm_stated(Sinv[i], v)
    return x.reshape(-1)


def well_from(D, seg_of_block, cells, Bvals, Cvals):
    """the per-well dict from D (dense), the segment of each block (ascending), its cell and the block values [nblk, 4, 3] in the reference's
    indexing: Bvals[blk, j, k] multiplies x[cell, k] into well equation j; Cvals[blk, k, j] multiplies z[k] into y[cell, j]"""
    Mb = D.shape[0] // 4
    seg = np.asarray(seg_of_block)
    assert np.all(np.diff(seg) >= 0)
    Brows = np.searchsorted(seg, np.arange(Mb + 1)).astype(np.int32)
    cp, ri, v = csc(D)
    return dict(Brows=Brows, Bcols=np.asarray(cells, np.int32), Bvals=np.asarray(Bvals, np.float64).reshape(-1), Cvals=np.asarray(Cvals, np.float64).reshape(-1),
                Dcolptr=cp, Drows=ri, Dvals=v)


def tree_well(Mb, cells, seed, branch=0.2, offd=0.6):
    """a generated well of Mb segments that perforates `cells` (natural order; spread over the segments in ascending order)"""
    rng = np.random.default_rng(seed)
    D = tree_D(Mb, rng, branch, offd)
    nblk = len(cells)
    seg = np.sort(np.arange(nblk) % Mb) if nblk >= Mb else np.arange(nblk)
    return well_from(D, seg, cells, rng.uniform(-1, 1, (nblk, 4, 3)), rng.uniform(-1, 1, (nblk, 4, 3)))


def dense_operators(well, Nb):
    """(B, C, D): B and C as M x 3 Nb matrices, D as M x M, so that the well's operator is y -= C^T D^-1 B x"""
    Brows = np.asarray(well["Brows"])
    Mb = len(Brows) - 1
    M = 4 * Mb
    Bv = np.asarray(well["Bvals"]).reshape(-1, 4, 3)
    Cv = np.asarray(well["Cvals"]).reshape(-1, 4, 3)
    B, C, D = np.zeros((M, 3 * Nb)), np.zeros((M, 3 * Nb)), np.zeros((M, M))
    for r in range(Mb):
        for blk in range(Brows[r], Brows[r + 1]):
            c = int(well["Bcols"][blk])
            B[4 * r:4 * r + 4, 3 * c:3 * c + 3] += Bv[blk]
            C[4 * r:4 * r + 4, 3 * c:3 * c + 3] += Cv[blk]
    cp = np.asarray(well["Dcolptr"])
    for c in range(M):
        for k in range(cp[c], cp[c + 1]):
            D[int(well["Drows"][k]), c] += well["Dvals"][k]
    return B, C, D
