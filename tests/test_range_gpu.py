"""range_search on the MI355X against the oracle: every case compares lims, I and the BITS of D with tests/_range_ref.py (all rows of
oracle.knn_canonical filtered by the predicate, ascending id)."""
import numpy as np
import pytest

from _data import bf16_round, gaussian, morgan_like, reaction_fp_like
from _range_ref import IP, L2, assert_same, range_oracle

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


def _index(metric, d):
    import textreact_amd.faiss_compat as faiss
    return faiss.IndexFlatIP(d) if metric == IP else faiss.IndexFlatL2(d)


def _radius_for(metric, x, y, per_query):
    """a radius that gives about `per_query` rows per query, from a search(k) sample (the median k-th distance)"""
    from oracle import flat_knn as oracle
    D, _ = oracle.knn_canonical(metric, x[:64], y, per_query)
    return float(np.median(D[:, -1]))


def _case(kind, seed):
    n, nq = 20_000, 300
    if kind == "gaussian":
        return gaussian(n, 768, seed), gaussian(nq, 768, seed + 1), 0
    if kind == "bf16":
        return bf16_round(gaussian(n, 768, seed)), bf16_round(gaussian(nq, 768, seed + 1)), 0
    if kind == "counts":                       # the fingerprint workload: the int8 form of the scan
        return reaction_fp_like(n, 2048, seed), reaction_fp_like(nq, 2048, seed + 1), 1
    return morgan_like(n, 1024, seed), morgan_like(nq, 1024, seed + 1), 2       # Morgan bits: the fp4 form


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("kind", ["gaussian", "bf16", "counts", "morgan"])
def test_range_search_equals_the_oracle(metric, kind):
    y, x, form = _case(kind, 11)
    idx = _index(metric, y.shape[1])
    idx.add(y)
    for per_query in (10, 100):
        r = _radius_for(metric, x, y, per_query)
        got = idx.range_search(x, r)
        assert_same(got, range_oracle(metric, x, y, r), "%s r=%r" % (kind, r))
        st = idx.last_range_stats()
        assert st["nq"] == 300 and st["n_results"] == got[0][-1], st
        # one radius for all queries: a query of small norm (L2) can have thousands of rows inside it, and those may overflow
        # their lists; a query with at most 1,000 never does
        assert st["n_exact"] <= (np.diff(got[0]) > 1000).sum(), st
        assert st["int8_scan"] == form, st


@pytest.mark.parametrize("metric", [L2, IP])
def test_boundary_ties_are_left_out_and_one_unit_inside_is_kept(metric):
    """integer counts: many rows sit at exactly D == radius; none of them is returned, those one unit inside are"""
    y, x = reaction_fp_like(20_000, 2048, 3), reaction_fp_like(300, 2048, 4)
    y[:300] = x                                                 # (every query has a row at distance 0 / at |x|^2)
    from oracle import flat_knn as oracle
    from _range_ref import filter_sorted
    Dall, Iall = oracle.knn_canonical(metric, x, y, y.shape[0])
    vals, counts = np.unique(Dall[:64, 40:60], return_counts=True)
    r = float(vals[np.argmax(counts)])                         # the most crowded integer score among the 40th-60th places
    idx = _index(metric, 2048)
    idx.add(y)
    got = idx.range_search(x, r)
    assert_same(got, filter_sorted(metric, Dall, Iall, r), "ties r=%r" % r)
    assert (Dall == np.float32(r)).sum() > 100                  # the boundary is crowded ...
    assert not (got[1] == np.float32(r)).any()                  # ... and none of it is returned
    inside = np.float32(r - 1) if metric == L2 else np.float32(r + 1)
    assert (got[1] == inside).sum() == (Dall == inside).sum() > 0      # one unit inside: every such row is


@pytest.mark.parametrize("metric", [L2, IP])
def test_a_radius_that_returns_nothing_and_one_that_returns_everything(metric):
    y, x = gaussian(3000, 64, 5), gaussian(40, 64, 6)
    idx = _index(metric, 64)
    idx.add(y)
    none_r = 0.0 if metric == L2 else 1e30
    lims, D, I = idx.range_search(x, none_r)
    assert lims.tolist() == [0] * 41 and D.shape == (0,) and I.shape == (0,)
    all_r = 1e30 if metric == L2 else -1e30
    got = idx.range_search(x, all_r)
    assert (np.diff(got[0]) == 3000).all()
    assert_same(got, range_oracle(metric, x, y, all_r), "everything")
    # empty index and no queries
    e = _index(metric, 64)
    lims, D, I = e.range_search(x, all_r)
    assert lims.tolist() == [0] * 41 and len(D) == len(I) == 0
    lims, D, I = idx.range_search(x[:0], all_r)
    assert lims.tolist() == [0] and len(D) == 0
    with pytest.raises(AssertionError):
        idx.range_search(gaussian(3, 32, 1), 1.0)               # dimension mismatch, as search
    with pytest.raises(AssertionError):
        idx.range_search(x, float("nan"))


@pytest.mark.parametrize("metric", [L2, IP])
def test_more_rows_inside_than_the_lists_hold_takes_the_exact_path(metric):
    """10,000 near-duplicates of query 0 inside the radius: its lists overflow, the exact fp64 scan answers it"""
    rng = np.random.default_rng(9)
    y = bf16_round(gaussian(20_000, 768, 7))
    x = bf16_round(gaussian(100, 768, 8))
    y[:10_000] = bf16_round(x[0] + 0.01 * rng.standard_normal((10_000, 768)).astype(np.float32))
    idx = _index(metric, 768)
    idx.add(y)
    r = _radius_for(metric, x[1:], y, 30)
    if metric == L2:
        r = max(r, 2.0)                                         # the near-duplicates sit at ~0.08
    want = range_oracle(metric, x, y, r)
    assert want[0][1] - want[0][0] >= 10_000
    got = idx.range_search(x, r)
    assert_same(got, want, "overflow")
    st = idx.last_range_stats()
    assert st["n_exact"] >= 1, st


def _poison(y, x):
    big = np.float32(3.0e38)
    NAN, INF = np.float32(np.nan), np.float32(np.inf)
    y[5, 7] = NAN; y[17, 3] = INF; y[29, 11] = -INF; y[41, :] = NAN; y[53, :] = big; y[54, :] = -big
    y[2000, 0] = NAN; y[2001, -1] = INF
    x[3, 2] = NAN; x[7, 5] = INF; x[11, 9] = -INF; x[13, :] = NAN; x[19, :] = big
    return y, x


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("kind", ["fp32", "integers", "int64_overflow"])
def test_hostile_rows_and_queries(metric, kind):
    """NaN / +-inf components and float32 overflow in rows and queries (tests/test_knn_hostile_gpu.py's values): every query's
    rows and distances are the oracle's; hostile queries take the exact path"""
    if kind == "fp32":
        y, x = gaussian(3000, 64, 1), gaussian(200, 64, 2)
        y, x = _poison(y, x)
    elif kind == "integers":
        y, x = reaction_fp_like(3000, 64, 3), reaction_fp_like(200, 64, 4)
        y, x = _poison(y, x)
    else:                                                       # int64 values whose float32 squares overflow: hostile rows, no NaN
        rng = np.random.default_rng(3)
        y = rng.integers(-10, 11, (3000, 64)).astype(np.int64)
        x = rng.integers(-10, 11, (200, 64)).astype(np.int64)
        y[7, 3] = 2 ** 62; y[9, :] = -(2 ** 40); x[5, 1] = 2 ** 61
    idx = _index(metric, 64)
    for part in np.array_split(y, 3):
        idx.add(part)
    xf, yf = x.astype(np.float32), y.astype(np.float32)
    with np.errstate(all="ignore"):
        r = _radius_for(metric, xf[20:], yf, 40)
    got = idx.range_search(x, r)
    assert_same(got, range_oracle(metric, xf, yf, r), "%s r=%r" % (kind, r))
    if kind != "int64_overflow":
        assert idx.last_range_stats()["n_exact"] >= 5


@pytest.mark.parametrize("metric", [L2, IP])
def test_more_hostile_rows_than_the_index_folds_in(metric):
    y, x = gaussian(4000, 64, 21), gaussian(50, 64, 22)
    y[::3, 0] = np.nan                                          # 1,334 hostile rows > MAX_SPECIAL: every query is exact
    idx = _index(metric, 64)
    idx.add(y)
    with np.errstate(all="ignore"):
        r = _radius_for(metric, x, y, 20)
    got = idx.range_search(x, r)
    assert_same(got, range_oracle(metric, x, y, r), "special overflow")
    assert idx.last_range_stats()["n_exact"] == 50


@pytest.mark.parametrize("metric", [L2, IP])
def test_device_tensors_in_and_out_equal_host_arrays(metric):
    import torch
    y, x = bf16_round(gaussian(20_000, 768, 31)), bf16_round(gaussian(300, 768, 32))
    idx = _index(metric, 768)
    idx.add(torch.from_numpy(y).cuda().bfloat16())
    r = _radius_for(metric, x, y, 50)
    host = idx.range_search(x, r)
    for xd in (torch.from_numpy(x).cuda(), torch.from_numpy(x).cuda().bfloat16()):
        lims, D, I = idx.range_search(xd, r)
        assert lims.is_cuda and D.is_cuda and I.is_cuda and lims.dtype == torch.int64 and D.dtype == torch.float32
        assert_same((lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()), host, "device")
    assert_same(host, range_oracle(metric, x, y, r), "host")


def test_more_queries_than_one_batch():
    """70,000 queries: two blocks of the host entry, appended; the answer does not depend on how the queries are cut"""
    from oracle import flat_knn as oracle
    y = reaction_fp_like(5000, 256, 41)
    x = reaction_fp_like(70_000, 256, 42)
    x[:100] = y[:100]
    idx = _index(L2, 256)
    idx.add(y)
    r = _radius_for(L2, x, y, 20)
    lims, D, I = idx.range_search(x, r)
    assert len(lims) == 70_001 and lims[-1] == len(D) == len(I) > 0
    parts = [idx.range_search(x[a:b], r) for a, b in ((0, 30_000), (30_000, 65_536), (65_536, 70_000))]
    assert np.array_equal(np.concatenate([p[1] for p in parts]).view(np.uint32), D.view(np.uint32))
    assert np.array_equal(np.concatenate([p[2] for p in parts]), I)
    assert np.array_equal(np.diff(lims), np.concatenate([np.diff(p[0]) for p in parts]))
    sel = np.r_[0:16, 65_520:65_552, np.random.default_rng(0).integers(0, 70_000, 16)]
    Dr, Ir = oracle.knn_canonical(L2, x[sel], y, 5000)
    from _range_ref import filter_sorted
    lr, Dw, Iw = filter_sorted(L2, Dr, Ir, r)
    for j, i in enumerate(sel):
        assert I[lims[i]:lims[i + 1]].tolist() == Iw[lr[j]:lr[j + 1]].tolist()
        assert np.array_equal(D[lims[i]:lims[i + 1]].view(np.uint32), Dw[lr[j]:lr[j + 1]].view(np.uint32))


@pytest.mark.parametrize("metric", [L2, IP])
def test_c1_consistency_with_search(metric):
    """C1 size (1,000,000 x 768 bf16, 65,536 queries).  For k = 10 and 256: with the radius at the median k-th D of search(x, k),
    every query's range result holds search's rows that satisfy the predicate, with the same D bits -- all of them, and nothing
    else when it has fewer than k rows; with k or more, no other row of it is better than search's k-th (float D); and 64 sampled
    queries equal the oracle over the full corpus"""
    import torch
    import textreact_amd.faiss_compat as faiss
    from oracle import flat_knn as oracle
    n, d, nq = 1_000_000, 768, 65_536
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    y = torch.randn((n, d), generator=g, device="cuda").bfloat16()
    x = torch.randn((nq, d), generator=g, device="cuda").bfloat16()
    x[:4096] = y[::244][:4096]
    idx = faiss.IndexFlatIP(d) if metric == IP else faiss.IndexFlatL2(d)
    idx.add(y)
    yh = y.float().cpu().numpy()
    sel = np.r_[0:8, 4096:4104, np.random.default_rng(0).integers(0, nq, 48)]
    for k in (10, 256):
        Ds, Is = idx.search(x, k)
        Ds, Is = Ds.cpu().numpy(), Is.cpu().numpy()
        r = float(np.median(Ds[:, -1]))
        lims, D, I = (t.cpu().numpy() for t in idx.range_search(x, r))
        assert idx.last_range_stats()["nq"] == nq
        keep = (Ds < np.float32(r)) if metric == L2 else (Ds > np.float32(r))
        cnt = np.diff(lims)
        full = cnt >= k
        assert (keep[full].all(axis=1)).all()                       # a query with >= k results: search's k all satisfy it
        assert (keep.sum(axis=1)[~full] == cnt[~full]).all()        # fewer: exactly search's rows that satisfy it
        for i in range(nq):                                         # ... and they are the same rows with the same bits
            seg_I, seg_D = I[lims[i]:lims[i + 1]], D[lims[i]:lims[i + 1]]
            assert (np.diff(seg_I) > 0).all(), i                    # ascending id
            m = min(k, len(seg_I))
            pos = np.searchsorted(seg_I, Is[i, :m])
            assert (pos < len(seg_I)).all() and np.array_equal(seg_I[np.minimum(pos, len(seg_I) - 1)], Is[i, :m]), i
            assert np.array_equal(seg_D[pos].view(np.uint32), Ds[i, :m].view(np.uint32)), i
            if len(seg_I) > k:                                      # the rest is not better than search's k-th
                rest = np.delete(seg_D, pos)
                assert ((rest >= Ds[i, k - 1]) if metric == L2 else (rest <= Ds[i, k - 1])).all(), i
        Dr, Ir = oracle.knn_canonical(metric, x[torch.from_numpy(sel).cuda()].float().cpu().numpy(), yh, 4096)
        from _range_ref import filter_sorted
        lr, Dw, Iw = filter_sorted(metric, Dr, Ir, r)
        for j, i in enumerate(sel):
            seg_I, seg_D = I[lims[i]:lims[i + 1]], D[lims[i]:lims[i + 1]]
            if lr[j + 1] - lr[j] < 4096:                            # the oracle's 4,096 best hold every row inside the radius
                assert seg_I.tolist() == Iw[lr[j]:lr[j + 1]].tolist(), (k, i)
                assert np.array_equal(seg_D.view(np.uint32), Dw[lr[j]:lr[j + 1]].view(np.uint32)), (k, i)
            else:                                                   # (a query of small norm, L2): they are all in the answer
                pos = np.searchsorted(seg_I, Iw[lr[j]:lr[j + 1]])
                assert len(seg_I) >= 4096 and np.array_equal(seg_I[np.minimum(pos, len(seg_I) - 1)], Iw[lr[j]:lr[j + 1]]), (k, i)
                assert np.array_equal(seg_D[pos].view(np.uint32), Dw[lr[j]:lr[j + 1]].view(np.uint32)), (k, i)
