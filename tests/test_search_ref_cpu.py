"""The id-returning search without a GPU: the feature exists, and the inputs and references of tests/test_gpu_search.py
have the properties its comparisons rest on.

1. libsvx.so exports svx_knn_search and FlatIndex has search / merge_search.
2. Lattice cases: every reference similarity is exact in fp32 (so the GPU's values must equal them as bits), and in
   every case with a (k+1)-th row some queries tie at the k-th place -- the tie rule decides their ids.
3. search_ref.search_exact merged over shards in ascending, reversed and a permuted order equals the one-shot result.
4. Coarse-grid data sets: the share of ambiguous (query, rank) positions -- the only ones exempt from id equality -- is
   at most 1 % per data set and k.  A data set that exceeds the cap gets another seed, not a higher cap."""
import multiprocessing

import numpy as np
import pytest

import margin_ref as mr
import search_ref as sr
import test_gpu_search as gs


def test_feature_exists():
    from svx import _lib
    from svx.postprocess.flat_index import FlatIndex
    lib = _lib.load()
    assert "svx_knn_search" in _lib.EXPORTS and hasattr(lib, "svx_knn_search")
    assert callable(getattr(FlatIndex, "search", None)) and callable(getattr(FlatIndex, "merge_search", None))


def test_search_exact_order():
    sims = np.array([[1.0, 3.0, 3.0, 0.5, 3.0, 1.0], [2.0, 2.0, 2.0, 2.0, 2.0, 2.0]])
    vals, ids = sr.search_exact(sims, 4, id_base=10)
    assert np.array_equal(vals, [[3, 3, 3, 1], [2, 2, 2, 2]]) and np.array_equal(ids, [[11, 12, 14, 10], [10, 11, 12, 13]])
    vals, ids = sr.search_exact(sims[:, :2], 4)
    assert np.array_equal(vals[0], [3, 1, -np.inf, -np.inf]) and np.array_equal(ids[0], [1, 0, -1, -1])
    vals, ids = sr.search_exact(sims[:, :0], 2)
    assert np.isneginf(vals).all() and (ids == -1).all()


def exact_in_fp32(sims):
    return np.array_equal(sims.astype(np.float32).astype(np.float64), sims)


@pytest.mark.parametrize("case", list(gs.LATTICE))
def test_lattice_case(case):
    n, N, d, k, storage, qtype, order, seed = gs.LATTICE[case]
    q, db = mr.lattice(n, N, d, k, seed, order)
    assert N >= k
    sims = mr.lattice_sims(q, db)
    assert exact_in_fp32(sims)
    qn = mr.unit_f32(q)[0]
    assert np.array_equal(mr.round_storage(qn, storage), qn) and np.array_equal(mr.round_storage(db, storage), db)
    assert np.array_equal(mr.round_storage(q, {"f32": storage, "f16": "fp16", "bf16": "bf16"}[qtype]), q)
    assert (case in gs.TIE_CASES) == (N > k)
    if case in gs.TIE_CASES:
        at_k, inside = sr.tie_shares(sims, k)
        print("%s: %.3f of the queries tie at the k-th place, %.3f inside the list" % (case, at_k, inside))
        assert at_k > 0, "%s: no query ties at the k-th place" % case


def test_lattice_cover():
    """The cases the GPU file has to hold."""
    v = list(gs.LATTICE.values())   # (n, N, d, k, storage, query type, order, seed)
    assert {c[6] for c in v} == set(mr.ORDERS)
    assert {1, 15, 16, 17, 24, 25, 63, 64} <= {c[3] for c in v}
    assert {32, 96, 160, 544, 992, 1024} <= {c[2] for c in v}
    assert any(c[1] == c[3] for c in v) and any(c[1] < 32 for c in v) and any(c[1] % 32 for c in v) and any(c[0] == 1 for c in v)
    assert len({(c[4], c[5]) for c in v}) == 6, "every instantiation <storage, query type> has a lattice case"
    assert len({(c[4], c[5]) for c in v if c[0] >= gs.BIG}) == 6, "and one over many workgroups"


@pytest.mark.parametrize("case", list(gs.SHARDS))
def test_shard_case(case):
    n, d, k, storage, qtype, dborder, sizes, id_base = gs.SHARDS[case]
    q, db = mr.lattice(min(n, 400), sum(sizes), d, k, 900 + k, dborder)
    sims = mr.lattice_sims(q, db)
    assert exact_in_fp32(sims) and sr.tie_shares(sims, k)[0] > 0
    assert 0 in sizes and sizes[0] < k and any(np.cumsum(sizes)[:-1] % 32)
    bounds = sr.shard_bounds(sizes)
    m = len(sizes)
    once = sr.search_exact(sims, k, id_base)
    orders = [list(range(m)), list(range(m))[::-1]] + [f(m) for f in gs.SHARD_ORDERS.values()]
    assert gs.SHARD_ORDERS["permuted"](m) not in orders[:2]
    for order in orders:
        states = sr.search_shards(sims, k, bounds, order, id_base)
        assert np.array_equal(states[-1][0], once[0]) and np.array_equal(states[-1][1], once[1]), order
        seen = 0
        for s, st in zip(order, states):
            seen += bounds[s][1] - bounds[s][0]
            assert (st[1][:, min(seen, k):] == -1).all() and (st[1][:, :min(seen, k)] >= id_base).all()


@pytest.fixture(scope="module")
def coarse_refs():
    jobs = gs.coarse_jobs()
    pool = multiprocessing.get_context("spawn").Pool(len(jobs))
    pending = {key: pool.apply_async(sr.coarse_search_reference, (job,)) for key, job in jobs.items()}
    yield pending
    pool.terminate()
    pool.join()


@pytest.mark.parametrize("case", gs.COARSE_SETS)
def test_coarse_ambiguous_share(case, coarse_refs):
    job = gs.mm.coarse_job(case)
    assert len(gs.coarse_jobs()) == len(gs.COARSE_SETS) == 6
    q, db = mr.coarse_data(job)
    for qtype in mr.QTYPES:     # the same rows serve every query type
        assert np.array_equal(mr.round_storage(q, {"f32": job['storage'], "f16": "fp16", "bf16": "bf16"}[qtype]), q)
    ref = coarse_refs[gs.mm.job_key(job)].get()
    assert ref['e'] > 0
    for k in sr.COARSE_KS:
        share = sr.ambiguous_share(ref['S64'], k, ref['e'])
        print("%s k=%d: e %.3e (max |seq - S64| %.3e), ambiguous positions %.4f" % (case, k, ref['e'], ref['e_seq'], share))
        assert share <= sr.AMBIGUOUS_CAP, "%s k=%d: %.4f of the positions are ambiguous" % (case, k, share)
    assert set(gs.COARSE_KS) <= set(sr.COARSE_KS)


def test_lanes_normalisation_on_grid():
    """On coarse-grid rows (sum of squares exact in any order) the kernel-order normalisation equals numpy's."""
    q = mr.coarse_rows(50, 544, 3)
    q[4] = 0
    assert np.array_equal(sr.unit_f32_lanes(q), mr.unit_f32(q)[0])
