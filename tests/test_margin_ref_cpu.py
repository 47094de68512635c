"""The properties of the inputs that tests/test_gpu_margin_matrix.py rests on, for every case that file uses (no GPU).

Lattice cases: the fp32 similarities in two summation orders equal the float64 ones (so any order the kernel uses gives
the same bits), the normalised query survives a round trip through the storage type and the queries through their own
type, and at least 10 % of the queries have a tie at the k-th place (cases with N = k have no (k+1)-th neighbour and are
exempt).  Coarse-grid cases: the fp32 sum of squares is equal in two orders and equal to float64, and in at most 1 % of
the rows taking the (k+1)-th neighbour for the k-th would move the mean by less than the case's bound -- a wrong pick is
visible.  These are conditions on the inputs; seeds are chosen so that they hold."""
import multiprocessing

import numpy as np
import pytest

import margin_ref as mr
import test_gpu_margin_matrix as mm

SAMPLE = 320   # queries of a large case on which the fp32 orders are compared (the rows are drawn alike)


def seq_sum_f32(a, reverse=False):
    """Row sums of a [n, d] float32 array, one fp32 add per element."""
    tot = np.zeros(a.shape[0], np.float32)
    for e in (range(a.shape[1] - 1, -1, -1) if reverse else range(a.shape[1])):
        tot = tot + a[:, e]
    return tot


def lattice_properties(q, db, k, storage, qtype):
    qn, ss = mr.unit_f32(q)
    q64 = q.astype(np.float64)
    assert np.array_equal(ss.astype(np.float64), (q64 * q64).sum(axis=1))
    assert np.array_equal(mr.round_storage(qn, storage), qn)
    assert np.array_equal(mr.round_storage(q, {"f32": storage, "f16": "fp16", "bf16": "bf16"}[qtype]), q)
    assert np.array_equal(mr.round_storage(db, storage), db) and np.abs(db * 64).max() <= 8 and np.array_equal(np.rint(db * 64), db * 64)
    nzq = (q != 0).sum(axis=1)
    assert (nzq == mr.pow4_floor(q.shape[1])).all()
    sub = np.r_[0:min(SAMPLE // 2, q.shape[0]), max(SAMPLE // 2, q.shape[0] - SAMPLE // 2):q.shape[0]]
    exact = mr.lattice_sims(q[sub], db)
    assert np.array_equal(mr.dots_f32(qn[sub], db).astype(np.float64), exact)
    assert np.array_equal(mr.dots_f32(qn[sub], db, reverse=True).astype(np.float64), exact)


@pytest.mark.parametrize("case", list(mm.LATTICE))
def test_lattice_case(case):
    _, n, N, d, k, storage, qtype, order, seed = mm.LATTICE[case]
    q, db = mr.lattice(n, N, d, k, seed, order)
    assert q.shape == (n, d) and db.shape == (N, d) and N >= k
    lattice_properties(q, db, k, storage, qtype)
    if N > k:
        share = mr.kth_tie_share(q, db, k)
        assert share >= 0.10, "%s: only %.3f of the queries tie at the k-th place" % (case, share)
    if order == "repeated":
        _, counts = np.unique(db, axis=0, return_counts=True)
        assert counts.max() == k + 5


def test_lattice_orders_hold_the_same_rows():
    dbs = {o: mr.lattice(9, 1000, 96, 16, 77, o) for o in mr.ORDERS}
    rows = {o: np.unique(dbs[o][1], axis=0, return_counts=True) for o in ("shuffled", "rising", "falling")}
    for o in ("rising", "falling"):
        assert np.array_equal(dbs[o][0], dbs["shuffled"][0])
        assert np.array_equal(rows[o][0], rows["shuffled"][0]) and np.array_equal(rows[o][1], rows["shuffled"][1])
    blocksum = mr.lattice_sims(dbs["rising"][0], dbs["rising"][1])
    assert (blocksum[:, -32:].min(axis=1) > blocksum[:, :32].max(axis=1)).all()     # the similarities do trend upward
    assert np.array_equal(dbs["falling"][1], dbs["rising"][1][::-1])


@pytest.mark.parametrize("case", list(mm.SHARDS) + ["orders"])
def test_lattice_shard_and_order_inputs(case):
    if case == "orders":
        for shape, n, d, k, storage, qtype in ((None, 65, 1024, 16, "fp16", "f32"), (None, 65, 544, 40, "bf16", "f16"),
                                               ("24", 129, 160, 20, "fp16", "bf16"), ("18", 129, 96, 15, "bf16", "f32")):
            for order in ("shuffled", "rising", "falling"):
                q, db = mr.lattice(n, 1000, d, k, 77, order)
                lattice_properties(q, db, k, storage, qtype)
            assert mr.kth_tie_share(q, db, k) >= 0.10
        return
    _, k, order, shards = mm.SHARDS[case]
    n, d, storage, qtype = mm.SHARD_SHAPE[case]
    q, db = mr.lattice(n, sum(shards), d, k, 900 + k, order)
    lattice_properties(q, db, k, storage, qtype)
    assert mr.kth_tie_share(q, db, k) >= 0.10
    assert 0 in shards and shards[0] < k and any(np.cumsum(shards)[:-1] % 32)


@pytest.fixture(scope="module")
def coarse_refs():
    jobs = mm.coarse_jobs()
    pool = multiprocessing.get_context("spawn").Pool(min(len(jobs), 12))
    pending = {key: pool.apply_async(mr.coarse_reference, (job,)) for key, job in jobs.items()}
    yield pending
    pool.terminate()
    pool.join()


@pytest.mark.parametrize("case", list(mm.COARSE))
def test_coarse_case(case, coarse_refs):
    _, d, k, storage, qtype = mm.COARSE[case][:5]
    job = mm.coarse_job(case)
    q, db = mr.coarse_data(job)
    grid = q * 64
    assert np.array_equal(np.rint(grid), grid) and np.abs(grid).max() <= 31
    assert np.array_equal(mr.round_storage(q, {"f32": storage, "f16": "fp16", "bf16": "bf16"}[qtype]), q)
    assert np.array_equal(mr.round_storage(db, storage), db)
    sq = q * q
    ss64 = (q.astype(np.float64) ** 2).sum(axis=1)
    assert np.array_equal(seq_sum_f32(sq).astype(np.float64), ss64) and np.array_equal(seq_sum_f32(sq, True).astype(np.float64), ss64)
    assert np.array_equal(mr.unit_f32(q)[1].astype(np.float64), ss64)
    ref = coarse_refs[mm.job_key(job)].get()
    l64, m64, lseq, mseq = mr.coarse_k(ref, k)
    for name, o, t in (("lists", lseq, l64), ("mean", mseq, m64)):
        _, e_orc, bound = mr.rule(o, o, t)
        print("%s %s: E_orc %.3e bound %.3e" % (case, name, e_orc, bound))
    share = mr.wrong_pick_share(ref, k, bound)
    assert share <= 0.01, "%s: a wrong pick hides under the bound %.3e in %.3f of the rows" % (case, bound, share)


@pytest.mark.parametrize("d", mm.HELPER_DIMS)
def test_helper_inputs(d):
    """The sums of k_unit_rows and k_margin_scores are exact in fp32 in any order on their inputs."""
    x = mm.unit_rows_input(d)
    assert not x[17].any()
    xs, ys, mxy, myx = mm.margin_input(d)
    for a, b in ((x, x), (xs, xs), (ys, ys), (xs, ys)):
        want = (a.astype(np.float64) * b.astype(np.float64)).sum(axis=1)
        assert np.array_equal(seq_sum_f32(a * b).astype(np.float64), want) and np.array_equal(seq_sum_f32(a * b, True).astype(np.float64), want)
    for t in ("fp16", "bf16"):
        assert np.array_equal(mr.round_storage(xs, t), xs) and np.array_equal(mr.round_storage(x, t), x)
    for margin in ("ratio", "distance"):
        t, a, b = mr.margin_f64(xs, ys, mxy, myx, margin)
        mine = mr.margin_f32(xs, ys, mxy, myx, margin)
        assert np.array_equal(np.isfinite(mine), np.isfinite(t))
        assert b[1] == 0 and b[2] == 0 and b[3] < 0 and b[4] < 0 and a[0] == 0 and a[2] == 0 and a[4] < 0
