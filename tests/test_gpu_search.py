"""FlatIndex.search / merge_search (svx_knn_search, csrc/svx_search.hip) against exact and float64 references, all
through the C ABI.

k_knn_search<BF, QE> has 2 x 3 = 6 instantiations: database storage (fp16 / bf16) x query type (fp32 / fp16 / bf16),
all of one shape (4 waves x 16 query rows = 64 queries per workgroup, every k <= 64).  Cases with n >= 16384 run it over
256 and more workgroups, the last one mostly masked.  The lists continue from an earlier call (`first` = 0: ties
compared by id) in the shard tests.  The LATTICE table names the instantiation every case selects.

(a) test_lattice: LATTICE inputs (margin_ref.py: every similarity exact in fp32).  search returns the values (as float32
    bits) and the ids of search_ref.search_exact, nothing exempt; row by row the values equal the descending sort of
    merge_topk's lists and float32(sum) / float32(k) equals mean_sim, bit for bit.
(b) test_shards: one database cut into shards, handed to merge_search with their id_base in ascending and in a permuted
    order: after every shard the state equals search_exact over the shards seen so far ((-inf, -1) while fewer than k
    rows were seen), the final state equals the one-shot search whatever the order, an id_base above 2^32 comes back.
(c) test_coarse: COARSE-GRID inputs under the rule of search_ref.py: ids distinct and in range, values not increasing,
    |value - S64[id]| <= e, no row that was not returned beats the worst returned one by more than 2e, and the ids
    equal the float64 reference's at every position that is not ambiguous.
(d) test_real_rows: the rows of tests/golden/margin_example.npz searched x in y and y in x at k = 16, same rule.  The
    rows are not on a grid, so the reference normalises them with the fp32 sum of squares in the kernel's own order
    (search_ref.unit_f32_lanes).
(e) test_edges.
No tolerance here is taken from what the kernel produces.  tests/test_search_ref_cpu.py checks, without a GPU, the
properties of the inputs these comparisons rest on."""
import multiprocessing
import os

import numpy as np
import pytest

import margin_ref as mr
import search_ref as sr
import test_gpu_margin_matrix as mm
from test_gpu_margin_matrix import bits, make_index, typed

BIG = mm.BIG   # 16384 queries = 256 workgroups
GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# id: (n, N, d, k, storage, query type, database order, seed)      # selects
LATTICE = {
    # ---- few queries: one or two workgroups
    "h_f32_ragged": (65, 3333, 1024, 16, "fp16", "f32", "shuffled", 1),       # <fp16, F32>, 105 tiles, ragged last tile
    "h_f16_k1": (64, 65, 96, 1, "fp16", "f16", "rising", 5),              # <fp16, F16> k = 1, one row in tile 3
    "h_bf_k15": (63, 49, 160, 15, "fp16", "bf16", "falling", 3),           # <fp16, BF16> second half-tile ragged
    "b_f32_one_query": (1, 33, 32, 15, "bf16", "f32", "rising", 604),            # <bf16, F32> one query, one k-step
    "b_f16_N_eq_k": (65, 16, 512, 16, "bf16", "f16", "shuffled", 5),          # <bf16, F16> N = k = half a tile
    "b_bf_repeated": (64, 241, 544, 16, "bf16", "bf16", "repeated", 6),         # <bf16, BF16> d = 544, every query ties at k
    "h_f32_k64_rising": (65, 3333, 1024, 64, "fp16", "f32", "rising", 14),     # <fp16, F32> replacements in every tile, k = 64
    "h_bf_k63": (64, 65, 544, 63, "fp16", "bf16", "falling", 210),          # <fp16, BF16> k4 = 64 with one +inf slot
    "b_f32_k25_repeated": (65, 256, 160, 25, "bf16", "f32", "repeated", 11),      # <bf16, F32> d = 160
    "b_f16_k24_one_query": (1, 224, 96, 24, "bf16", "f16", "rising", 112),             # <bf16, F16> n = 1, 7 tiles (odd)
    "h_f16_k64_N_eq_k": (63, 64, 1024, 64, "fp16", "f16", "shuffled", 9),        # <fp16, F16> N = k = 64
    "h_f32_d992": (65, 48, 992, 17, "fp16", "f32", "rising", 8),             # <fp16, F32> d = 992
    # ---- n >= 16384: 256 workgroups and more
    "big_h_f32": (BIG, 320, 1024, 16, "fp16", "f32", "rising", 15),        # <fp16, F32> 10 tiles (even)
    "big_h_f16_masked": (BIG + 77, 241, 32, 1, "fp16", "f16", "shuffled", 2),     # <fp16, F16> last workgroup mostly masked
    "big_h_bf": (BIG, 49, 96, 15, "fp16", "bf16", "falling", 17),          # <fp16, BF16>
    "big_b_f32_repeated": (BIG + 77, 241, 160, 16, "bf16", "f32", "repeated", 18),  # <bf16, F32>
    "big_b_f16_N_eq_k": (BIG, 24, 32, 24, "bf16", "f16", "rising", 25),           # <bf16, F16> N = k, less than a tile
    "big_b_bf_d992": (BIG + 77, 241, 992, 20, "bf16", "bf16", "rising", 26),    # <bf16, BF16>
    "big_h_f32_k25": (BIG, 49, 32, 25, "fp16", "f32", "rising", 27),  # <fp16, F32> k = 25 at large n
    # ---- a handful of queries, and k = 64 over many workgroups
    "h_f32_5_queries": (5, 500, 1024, 16, "fp16", "f32", "rising", 28),             # <fp16, F32> 5 of 64 rows
    "b_f16_129_queries": (129, 241, 512, 24, "bf16", "f16", "falling", 29),         # <bf16, F16> second workgroup holds one row
    "h_bf_5_queries": (5, 65, 96, 17, "fp16", "bf16", "repeated", 30),          # <fp16, BF16>
    "big_b_bf_k64": (BIG + 77, 224, 96, 64, "bf16", "bf16", "falling", 46),     # <bf16, BF16> 258 workgroups, k = 64
}
# the cases with a (k+1)-th row: test_search_ref_cpu.py asserts that queries of each tie at the k-th place
TIE_CASES = [c for c, v in LATTICE.items() if v[1] > v[3]]

# id: (n, d, k, storage, query type, order, shard sizes, id_base)
SHARDS = {
    "k16_rising": (333, 544, 16, "fp16", "f32", "rising", [5, 0, 7, 40, 600, 348], 0),            # < k rows after three shards
    "k40_shuffled": (333, 1024, 40, "bf16", "f16", "shuffled", [20, 0, 15, 77, 500, 388], (1 << 33) + 7),  # ids above 2^32
    "k64_repeated": (65, 160, 64, "fp16", "bf16", "repeated", [3, 70, 1, 0, 926], 5),             # k = 64
    "big_k20": (BIG + 77, 96, 20, "fp16", "f16", "rising", [10, 0, 50, 140], 1000),               # 258 workgroups continued
    "k24_bf": (200, 96, 24, "bf16", "bf16", "shuffled", [20, 11, 1, 0, 968], 0),              # k = 24
}
SHARD_ORDERS = {"ascending": lambda m: list(range(m)), "permuted": lambda m: [int(s) for s in np.random.RandomState(7).permutation(m)]}

# The coarse-grid data sets: one per (d, storage), taken from test_gpu_margin_matrix.COARSE (n = 400 queries each);
# every one is searched with every query type at k = 16, 24 and 64.
COARSE_SETS = ("h_f32_96", "h_f32_544", "h_bf_1024", "b_f32_96", "b_f16_544", "b_f32_1024")
COARSE_KS = (16, 24, 64)


def host(state):
    return state[0].cpu().numpy(), state[1].cpu().numpy()


def exact_fails(label, got, want):
    """got, want: (values, ids).  Values as float32 bits, ids exactly."""
    (gs, gi), (ws, wi) = got, want
    ws = ws.astype(np.float32)
    fails = []
    assert gs.dtype == np.float32 and gi.dtype == np.int64 and gs.shape == ws.shape and gi.shape == wi.shape
    bad = np.nonzero((bits(gs) != bits(ws)).any(axis=1))[0]
    if bad.size:
        i = int(bad[0])
        j = int(np.nonzero(bits(gs[i]) != bits(ws[i]))[0][0])
        fails.append("%s: values differ in %d of %d rows; row %d place %d: %.9g, exact %.9g" % (label, bad.size, gs.shape[0], i, j, gs[i, j], ws[i, j]))
    bad = np.nonzero((gi != wi).any(axis=1))[0]
    if bad.size:
        i = int(bad[0])
        j = int(np.nonzero(gi[i] != wi[i])[0][0])
        fails.append("%s: ids differ in %d of %d rows; row %d place %d: %d (%.9g), exact %d (%.9g)"
                     % (label, bad.size, gi.shape[0], i, j, gi[i, j], gs[i, j], wi[i, j], ws[i, j]))
    return fails


# ---- (a) lattice
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(LATTICE))
def test_lattice(case, monkeypatch):
    n, N, d, k, storage, qtype, order, seed = LATTICE[case]
    monkeypatch.delenv("SVX_KNN_SHAPE", raising=False)
    q, db = mr.lattice(n, N, d, k, seed, order)
    want = sr.search_exact(mr.lattice_sims(q, db), k)
    idx = make_index(db, storage)
    qq = typed(q, qtype)
    D, I = idx.search(qq, k)
    assert D.is_cuda and I.is_cuda
    got = host((D, I))
    fails = exact_fails("search", got, want)
    # the values are what the fused entry points keep and average
    topk, _ = idx.merge_topk(qq, k, None)
    lists = mm.sorted_lists(topk)
    if not np.array_equal(bits(lists), bits(got[0])):
        fails.append("search values differ from the sorted lists of merge_topk")
    tot = got[0].astype(np.float64).sum(axis=1)
    assert np.array_equal(tot.astype(np.float32).astype(np.float64), tot)
    mean = idx.mean_sim(qq, k).cpu().numpy()
    if not np.array_equal(bits(tot.astype(np.float32) / np.float32(k)), bits(mean)):
        fails.append("float32(sum of the search values) / k differs from mean_sim")
    assert not fails, "\n".join(fails)


# ---- (b) shards
@pytest.mark.gpu
@pytest.mark.parametrize("order_name", list(SHARD_ORDERS))
@pytest.mark.parametrize("case", list(SHARDS))
def test_shards(case, order_name, monkeypatch):
    from svx.postprocess.flat_index import FlatIndex
    n, d, k, storage, qtype, dborder, sizes, id_base = SHARDS[case]
    monkeypatch.delenv("SVX_KNN_SHAPE", raising=False)
    q, db = mr.lattice(n, sum(sizes), d, k, 900 + k, dborder)
    sims = mr.lattice_sims(q, db)
    qq = typed(q, qtype)
    bounds = sr.shard_bounds(sizes)
    order = SHARD_ORDERS[order_name](len(sizes))
    assert sorted(order) == list(range(len(sizes)))
    wants = sr.search_shards(sims, k, bounds, order, id_base)
    state, seen, fails = None, 0, []
    for s, want in zip(order, wants):
        lo, hi = bounds[s]
        part = FlatIndex(d=d, storage=storage)
        part.add_unit_rows(db[lo:hi])
        assert part.ntotal == hi - lo
        state = part.merge_search(qq, k, state, id_base=id_base + lo)
        seen += hi - lo
        got = host(state)
        if seen < k:
            assert np.isneginf(want[0][:, seen:]).all() and (want[1][:, seen:] == -1).all()
            assert np.isneginf(got[0][:, seen:]).all() and (got[1][:, seen:] == -1).all()
        fails += exact_fails("after shard %d (%d rows seen)" % (s, seen), got, want)
    assert not fails, "\n".join(fails)
    D, I = make_index(db, storage).search(qq, k)
    once = (D.cpu().numpy(), I.cpu().numpy() + id_base)
    assert not exact_fails("one-shot search", once, host(state))
    if id_base >= 1 << 32:
        assert (host(state)[1] >= id_base).all()


# ---- (c) coarse grid
def coarse_jobs():
    return {mm.job_key(mm.coarse_job(c)): mm.coarse_job(c) for c in COARSE_SETS}


@pytest.fixture(scope="module")
def coarse_refs():
    """The float64 matrices and bounds of the coarse data sets, in processes that never touch the GPU (spawn)."""
    jobs = coarse_jobs()
    pool = multiprocessing.get_context("spawn").Pool(len(jobs))
    pending = {key: pool.apply_async(sr.coarse_search_reference, (job,)) for key, job in jobs.items()}
    yield pending
    pool.terminate()
    pool.join()


def rule_fails(label, D, I, S64, e, k):
    """The checks of (c) on one result.  Prints every figure before it is judged."""
    n, N = S64.shape
    fails = []
    srt = np.sort(I, axis=1)
    if not ((I >= 0).all() and (I < N).all() and (srt[:, 1:] != srt[:, :-1]).all()):
        return ["%s: ids out of range or repeated within a row" % label]
    if not (D[:, 1:] <= D[:, :-1]).all():
        fails.append("%s: the values of a row increase" % label)
    at = np.take_along_axis(S64, I, axis=1)
    err = float(np.abs(D.astype(np.float64) - at).max())
    rest = S64.copy()
    np.put_along_axis(rest, I, -np.inf, axis=1)
    missed = float((rest.max(axis=1) - at.min(axis=1)).max()) if N > k else -np.inf
    ref_ids, amb = sr.ambiguous(S64, k, e)
    wrong = (I != ref_ids) & ~amb
    print("%s: e %.3e, max |value - S64[id]| %.3e, best missed row above the worst returned by %.3e (allowed %.3e), "
          "ambiguous positions %.4f, ids differing elsewhere %d" % (label, e, err, missed, 2 * e, amb.mean(), wrong.sum()))
    if not err <= e:
        fails.append("%s: a value is %.3e from the float64 similarity of its id, bound %.3e" % (label, err, e))
    if not missed <= 2 * e:
        fails.append("%s: a row that was not returned is %.3e above the worst returned one, allowed %.3e" % (label, missed, 2 * e))
    if wrong.any():
        i, j = (int(v[0]) for v in np.nonzero(wrong))
        fails.append("%s: %d ids differ from the float64 reference at positions that are not ambiguous; query %d rank %d: %d, reference %d"
                     % (label, wrong.sum(), i, j, I[i, j], ref_ids[i, j]))
    return fails


@pytest.mark.gpu
@pytest.mark.parametrize("k", COARSE_KS)
@pytest.mark.parametrize("qtype", mr.QTYPES)
@pytest.mark.parametrize("case", COARSE_SETS)
def test_coarse(case, qtype, k, coarse_refs, monkeypatch):
    monkeypatch.delenv("SVX_KNN_SHAPE", raising=False)
    job = mm.coarse_job(case)
    ref = coarse_refs[mm.job_key(job)].get()
    q, db = mr.coarse_data(job)
    D, I = make_index(db, job['storage']).search(typed(q, qtype), k)
    fails = rule_fails("%s %s k=%d" % (case, qtype, k), D.cpu().numpy(), I.cpu().numpy(), ref['S64'], ref['e'], k)
    assert not fails, "\n".join(fails)


# ---- (d) real rows
@pytest.mark.gpu
@pytest.mark.parametrize("storage", mr.STORAGES)
@pytest.mark.parametrize("direction", ["x_in_y", "y_in_x"])
def test_real_rows(direction, storage):
    g = np.load(os.path.join(GD, "margin_example.npz"))
    x, y = (g["db_src"], g["db_tgt"]) if direction == "x_in_y" else (g["db_tgt"], g["db_src"])
    assert x.shape == y.shape == (347, 1024) and x.dtype == np.float16
    db = mr.round_storage(y.astype(np.float32), storage)
    ref = sr.rows_search_reference(x.astype(np.float32), db, storage)
    D, I = make_index(db, storage).search(x, 16)
    fails = rule_fails("%s %s" % (direction, storage), D.cpu().numpy(), I.cpu().numpy(), ref['S64'], ref['e'], 16)
    assert not fails, "\n".join(fails)
    share = float(sr.ambiguous(ref['S64'], 16, ref['e'])[1].mean())
    assert share <= sr.AMBIGUOUS_CAP, "ambiguous positions: %.4f" % share


# ---- (e) edges
@pytest.mark.gpu
def test_edges():
    import torch
    from svx import _lib
    q, db = mr.lattice(70, 300, 96, 16, 3, "shuffled")
    q[7] = 0
    sims = mr.lattice_sims(np.where((q != 0).any(axis=1, keepdims=True), q, 1.0), db)
    sims[7] = 0
    idx = make_index(db, "fp16")
    k = 16
    D, I = idx.search(q, k)
    assert D.dtype == torch.float32 and I.dtype == torch.int64 and tuple(D.shape) == tuple(I.shape) == (70, k)
    assert not exact_fails("search with a zero query", host((D, I)), sr.search_exact(sims, k))
    # a zero query: every similarity is 0, the lowest ids win
    state = idx.merge_search(q[7:8], k, None, id_base=1000)
    assert not host(state)[0].any() and np.array_equal(host(state)[1][0], 1000 + np.arange(k))
    # l2: 2 - 2 sim, ascending
    L, I2 = idx.search(q, k, l2=True)
    assert torch.equal(I2, I) and torch.equal(L, 2.0 - 2.0 * D) and bool((L[:, 1:] >= L[:, :-1]).all())
    # no queries
    D0, I0 = idx.search(q[:0], k)
    assert tuple(D0.shape) == tuple(I0.shape) == (0, k) and I0.dtype == torch.int64
    # an empty database: all (-inf, -1); a shard after it fills the lists
    from svx.postprocess.flat_index import FlatIndex
    empty = FlatIndex(d=96, storage="fp16")
    state = empty.merge_search(q, k)
    assert np.isneginf(host(state)[0]).all() and (host(state)[1] == -1).all()
    state = idx.merge_search(q, k, state)
    assert not exact_fails("after an empty first shard", host(state), sr.search_exact(sims, k))
    D1, I1 = empty.search(q, 3)
    assert np.isneginf(D1.cpu().numpy()).all() and (I1.cpu().numpy() == -1).all()
    # argument errors
    with pytest.raises(_lib.SvxError, match=r"supported 1\.\.64"):
        idx.search(q, 65)
    with pytest.raises(_lib.SvxError, match="multiple of 32"):
        FlatIndex(d=40, storage="fp16").search(np.zeros((3, 40), np.float32), 4)
    good = idx.merge_search(q, k)
    for bad in ((good[0][:, :8].contiguous(), good[1][:, :8].contiguous()), (good[0], good[1].to(torch.int32)),
                (good[0].double(), good[1]), (good[0][:5], good[1][:5])):
        with pytest.raises(ValueError, match="state"):
            idx.merge_search(q, k, bad)
