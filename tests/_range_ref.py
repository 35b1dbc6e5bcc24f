"""The oracle side of the range-search tests: every row of oracle.knn_canonical(metric, x, y, k=n) -- all rows in canonical order,
D = (float) of the fp64 score, NaN scores as pads (I = -1) -- filtered by the predicate on that D (L2: D < radius, IP: D > radius,
radius as float32) and ordered by id within each query.  Returns faiss' (lims, D, I)."""
import numpy as np

IP, L2 = 0, 1


def filter_sorted(metric, Dr, Ir, radius):
    """(lims, D, I) from canonical [nq][n] lists: the rows that satisfy the predicate, ascending id per query"""
    r = np.float32(radius)
    with np.errstate(invalid="ignore"):
        keep = (Ir >= 0) & ((Dr < r) if metric == L2 else (Dr > r))
    nq = Dr.shape[0]
    lims = np.zeros(nq + 1, dtype=np.int64)
    lims[1:] = np.cumsum(keep.sum(axis=1))
    Ds, Is = [], []
    for i in range(nq):
        ids, ds = Ir[i][keep[i]], Dr[i][keep[i]]
        o = np.argsort(ids, kind="stable")
        Is.append(ids[o]); Ds.append(ds[o])
    D = np.concatenate(Ds).astype(np.float32) if nq else np.zeros(0, np.float32)
    I = np.concatenate(Is).astype(np.int64) if nq else np.zeros(0, np.int64)
    return lims, D, I


def range_oracle(metric, x, y, radius):
    from oracle import flat_knn as oracle
    with np.errstate(all="ignore"):
        Dr, Ir = oracle.knn_canonical(metric, x, y, y.shape[0])
    return filter_sorted(metric, Dr, Ir, radius)


def assert_same(got, want, what=""):
    lims, D, I = (np.asarray(a) for a in got)
    lr, Dr, Ir = want
    assert lims.dtype == np.int64 and D.dtype == np.float32 and I.dtype == np.int64, (lims.dtype, D.dtype, I.dtype)
    if not np.array_equal(lims, lr):
        bad = np.flatnonzero(np.diff(lims) != np.diff(lr))
        raise AssertionError("%s: result counts differ at queries %r: got %r want %r" % (what, bad[:4].tolist(), np.diff(lims)[bad[:4]].tolist(),
                                                                                         np.diff(lr)[bad[:4]].tolist()))
    assert np.array_equal(I, Ir), "%s: ids differ at %r" % (what, np.flatnonzero(I != Ir)[:4].tolist())
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32)), "%s: distance bits differ" % what
