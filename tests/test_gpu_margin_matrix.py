"""Every instantiation of the margin-scoring kernels (csrc/svx_margin.hip) against exact and float64 references.

k_knn_mean<BF, QE, RPW, NW, KREG> has 2 x 3 x 3 x 2 = 36 instantiations: database storage (fp16 / bf16) x query type
(fp32 / fp16 / bf16) x shape (RPW, NW) in {(1,4), (2,4), (1,8)} x top-k lists in registers (k <= 16) or in LDS.
launch_knn_rpw picks (2,4) at n >= 16384 and (1,4) below, SVX_KNN_SHAPE = 14 / 18 / 24 forces a shape, and a forced
or default (2,4) / (1,8) whose LDS lists do not fit beside the tiles (k >= 25) falls back to (1,4).

(a) test_lattice: every instantiation on LATTICE inputs (margin_ref.py: exact arithmetic) -- the kept lists of
    FlatIndex.merge_topk equal the true k largest similarities bit for bit (both sides sorted), the means of
    FlatIndex.mean_sim and merge_topk equal float32(sum) / float32(k) bit for bit.  test_lattice_orders_agree: the
    shuffled, rising and falling orders of one database leave the same lists.
(b) test_lattice_shards: the database handed over shard by shard (shards smaller than k: -inf in the lists and a mean
    of -inf until k rows have been seen; an empty shard; a rising database cut in the middle of a tile): exact after
    every shard, and the final lists equal the one-shot lists.
(c) test_coarse: COARSE-GRID real-valued inputs under stage_check's rule E_gpu <= max(2 E_orc, 4 * 2^-24 max|f64|), for
    the sorted kept lists and for the means: E_gpu against the float64 chain, E_orc = the error of the
    sequential-fp32 restatement on the same rows.
(d) test_unit_rows: svx_unit_rows equals round_storage(x * inv) bit for bit, no share of mismatches allowed.
(e) test_margin_scores: svx_margin_scores within bounds that follow from the kernel's operation count, edge rows
    (zero row, mean of 0, negative mean) equal to numpy's own result, inf / nan included.
No tolerance here is taken from what the kernels produce.  tests/test_margin_ref_cpu.py checks, without a GPU, the
properties of the inputs these comparisons rest on.  profiles/margin_matrix_kernels.txt is the kernel trace of this file.

    python tests/test_gpu_margin_matrix.py --dump FILE     (on the GPU box)
writes one JSON line per coarse-grid case with E_gpu, E_orc, their ratio and the bound, for the lists and the means
(profiles/margin_errors.jsonl)."""
import ctypes
import json
import multiprocessing
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # hand-run: the paths conftest.py sets up for pytest
    import os
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_root, "speech-vecalign_amd"), os.path.join(_root, "oracle"), os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, _p)

import margin_ref as mr

BIG = 16384   # launch_knn_rpw: n >= 128 * 128 selects the (2,4) shape

# id: (SVX_KNN_SHAPE or None, n, N, d, k, storage, query type, database order, seed)      # selects
LATTICE = {
    # ---- default dispatch, n < 16384: shape (1,4)
    "s14_h_f32_reg": (None, 65, 3333, 1024, 16, "fp16", "f32", "shuffled", 1),      # <fp16, F32, 1, 4, reg>, 105 tiles, ragged
    "s14_h_f16_reg": (None, 64, 65, 96, 1, "fp16", "f16", "rising", 5),             # <fp16, F16, 1, 4, reg> k = 1, one row in tile 3
    "s14_h_bf_reg": (None, 63, 49, 160, 15, "fp16", "bf16", "falling", 3),          # <fp16, BF16, 1, 4, reg> second half-tile ragged
    "s14_b_f32_reg": (None, 1, 33, 32, 15, "bf16", "f32", "rising", 604),           # <bf16, F32, 1, 4, reg> one query, one k-step
    "s14_b_f16_reg": (None, 65, 16, 512, 16, "bf16", "f16", "shuffled", 5),         # <bf16, F16, 1, 4, reg> N = k = half a tile
    "s14_b_bf_reg": (None, 64, 241, 544, 16, "bf16", "bf16", "repeated", 6),        # <bf16, BF16, 1, 4, reg> d = 544: second row half partly zero source
    "s14_b_f16_reg_rise": (None, 64, 3333, 512, 16, "bf16", "f16", "rising", 7),    # knn_insert with most lanes pending in every tile
    "s14_h_f32_lds": (None, 65, 48, 992, 17, "fp16", "f32", "rising", 8),           # <fp16, F32, 1, 4, lds> first k past the registers, d = 992
    "s14_h_f16_lds": (None, 63, 64, 1024, 64, "fp16", "f16", "shuffled", 9),        # <fp16, F16, 1, 4, lds> N = k = 64
    "s14_h_bf_lds": (None, 64, 65, 544, 63, "fp16", "bf16", "falling", 210),       # <fp16, BF16, 1, 4, lds> k4 = 64 with one +inf slot
    "s14_b_f32_lds": (None, 65, 256, 160, 25, "bf16", "f32", "repeated", 11),       # <bf16, F32, 1, 4, lds> d = 160: lanes of the first half past d
    "s14_b_f16_lds": (None, 1, 224, 96, 24, "bf16", "f16", "rising", 112),         # <bf16, F16, 1, 4, lds> 7 tiles (odd: ends on tile0)
    "s14_b_bf_lds": (None, 64, 32, 32, 24, "bf16", "bf16", "falling", 13),          # <bf16, BF16, 1, 4, lds> exactly one tile
    "s14_h_f32_lds_rise": (None, 65, 3333, 1024, 64, "fp16", "f32", "rising", 14),  # the LDS replace loop on most columns of every tile
    # ---- default dispatch, n >= 16384: shape (2,4); k <= 24 fits beside the tiles
    "s24_h_f32_reg": (None, BIG, 320, 1024, 16, "fp16", "f32", "rising", 15),       # <fp16, F32, 2, 4, reg> 10 tiles (even)
    "s24_h_f16_reg": (None, BIG + 77, 241, 32, 1, "fp16", "f16", "shuffled", 2),    # <fp16, F16, 2, 4, reg> last workgroup mostly masked
    "s24_h_bf_reg": (None, BIG, 49, 96, 15, "fp16", "bf16", "falling", 17),         # <fp16, BF16, 2, 4, reg>
    "s24_b_f32_reg": (None, BIG + 77, 241, 160, 16, "bf16", "f32", "repeated", 18),  # <bf16, F32, 2, 4, reg>
    "s24_b_f16_reg": (None, BIG, 64, 32, 16, "bf16", "f16", "rising", 19),          # <bf16, F16, 2, 4, reg>
    "s24_b_bf_reg": (None, BIG + 77, 65, 96, 15, "bf16", "bf16", "shuffled", 20),   # <bf16, BF16, 2, 4, reg>
    "s24_h_f32_lds": (None, BIG, 224, 544, 24, "fp16", "f32", "rising", 21),        # <fp16, F32, 2, 4, lds> k = 24: the last k that fits (2,4)
    "s24_h_f16_lds": (None, BIG + 77, 48, 32, 17, "fp16", "f16", "falling", 22),    # <fp16, F16, 2, 4, lds> owner-lane walk with RPW = 2
    "s24_h_bf_lds": (None, BIG, 65, 96, 24, "fp16", "bf16", "shuffled", 23),        # <fp16, BF16, 2, 4, lds>
    "s24_b_f32_lds": (None, BIG + 77, 256, 160, 17, "bf16", "f32", "repeated", 24),  # <bf16, F32, 2, 4, lds>
    "s24_b_f16_lds": (None, BIG, 24, 32, 24, "bf16", "f16", "rising", 25),          # <bf16, F16, 2, 4, lds> N = k
    "s24_b_bf_lds": (None, BIG + 77, 241, 992, 20, "bf16", "bf16", "rising", 26),   # <bf16, BF16, 2, 4, lds>
    "s24_k25_falls_back": (None, BIG, 49, 32, 25, "fp16", "f32", "rising", 27),     # k = 25 does not fit (2,4): (1,4) lds at large n
    # ---- SVX_KNN_SHAPE=24 with few queries: most query rows of the workgroup masked
    "f24_n5_reg": ("24", 5, 500, 1024, 16, "fp16", "f32", "rising", 28),            # <fp16, F32, 2, 4, reg> 5 of 128 rows
    "f24_n129_lds": ("24", 129, 241, 512, 24, "bf16", "f16", "falling", 29),        # <bf16, F16, 2, 4, lds> second workgroup holds one row
    "f24_n5_lds": ("24", 5, 65, 96, 17, "fp16", "bf16", "repeated", 30),            # <fp16, BF16, 2, 4, lds>
    "f24_n129_reg": ("24", 129, 33, 160, 15, "bf16", "bf16", "shuffled", 31),       # <bf16, BF16, 2, 4, reg>
    # ---- SVX_KNN_SHAPE=18: shape (1,8), 8 pieces per wave and tile
    "f18_h_f32_reg": ("18", 129, 3333, 1024, 16, "fp16", "f32", "rising", 32),      # <fp16, F32, 1, 8, reg>
    "f18_h_f16_reg": ("18", 65, 33, 32, 1, "fp16", "f16", "falling", 533),         # <fp16, F16, 1, 8, reg>
    "f18_h_bf_reg": ("18", 200, 49, 544, 15, "fp16", "bf16", "shuffled", 34),       # <fp16, BF16, 1, 8, reg>
    "f18_b_f32_reg": ("18", 128, 241, 992, 16, "bf16", "f32", "repeated", 35),      # <bf16, F32, 1, 8, reg>
    "f18_b_f16_reg": ("18", 1, 64, 96, 16, "bf16", "f16", "rising", 336),          # <bf16, F16, 1, 8, reg>
    "f18_b_bf_reg": ("18", 127, 65, 160, 15, "bf16", "bf16", "falling", 37),        # <bf16, BF16, 1, 8, reg>
    "f18_h_f32_lds": ("18", 129, 3333, 1024, 24, "fp16", "f32", "rising", 38),      # <fp16, F32, 1, 8, lds>
    "f18_h_f16_lds": ("18", 65, 48, 32, 17, "fp16", "f16", "shuffled", 39),         # <fp16, F16, 1, 8, lds>
    "f18_h_bf_lds": ("18", 200, 224, 544, 24, "fp16", "bf16", "falling", 40),       # <fp16, BF16, 1, 8, lds>
    "f18_b_f32_lds": ("18", 128, 256, 992, 17, "bf16", "f32", "repeated", 41),      # <bf16, F32, 1, 8, lds>
    "f18_b_f16_lds": ("18", 1, 65, 96, 24, "bf16", "f16", "rising", 42),            # <bf16, F16, 1, 8, lds>
    "f18_b_bf_lds": ("18", 127, 24, 160, 24, "bf16", "bf16", "shuffled", 43),       # <bf16, BF16, 1, 8, lds> N = k
    "f18_k64_falls_back": ("18", 129, 300, 512, 64, "fp16", "f16", "rising", 44),   # k = 64 does not fit (1,8): (1,4) lds
    # ---- SVX_KNN_SHAPE=14 at n >= 16384: the small shape over 257 workgroups
    "f14_big_reg": ("14", BIG, 65, 32, 16, "fp16", "f32", "rising", 45),            # <fp16, F32, 1, 4, reg>
    "f14_big_lds": ("14", BIG + 77, 224, 96, 64, "bf16", "bf16", "falling", 46),    # <bf16, BF16, 1, 4, lds>
}

# id: (SVX_KNN_SHAPE or None, k, order, shard sizes)       # selects
SHARDS = {
    "reg_rising": (None, 16, "rising", [5, 0, 7, 40, 600, 348]),        # < k rows after three shards; cuts inside tiles; (1,4) reg
    "lds_rising": (None, 40, "rising", [20, 0, 15, 77, 500, 388]),      # (1,4) lds, lists start as -inf / st_in
    "reg_shuffled_18": ("18", 15, "shuffled", [3, 11, 1, 0, 985]),      # (1,8) reg: exactly k rows after the third shard
    "lds_big_k20": (None, 20, "rising", [10, 0, 50, 140]),              # n >= 16384, k = 20: (2,4) lds continued from st_in
}
SHARD_SHAPE = {"reg_rising": (333, 544, "fp16", "f32"), "lds_rising": (333, 1024, "bf16", "f16"),
               "reg_shuffled_18": (200, 96, "bf16", "bf16"), "lds_big_k20": (BIG + 77, 96, "fp16", "f16")}   # n, d, storage, query type

CN = 400     # queries of every coarse-grid case
COMMON = 0.5
# The database is small where k is large and the common component goes with k <= 24, so that the k-th and the (k+1)-th
# neighbour stay further apart than the bound on a mean (tests/test_margin_ref_cpu.py asserts it per case); seeds are
# chosen for that condition alone, on the CPU.
# id: (SVX_KNN_SHAPE, d, k, storage, query type, common component, N, seed)      # selects
COARSE = {
    "h_f32_96": ("24", 96, 16, "fp16", "f32", 0.0, 1000, 7096),          # <fp16, F32, 2, 4, reg>
    "h_f32_544": ("18", 544, 24, "fp16", "f32", COMMON, 1000, 8244),     # <fp16, F32, 1, 8, lds>
    "h_f32_1024": ("14", 1024, 64, "fp16", "f32", 0.0, 200, 8124),       # <fp16, F32, 1, 4, lds>
    "h_f16_96": ("24", 96, 24, "fp16", "f16", COMMON, 1000, 7096),       # <fp16, F16, 2, 4, lds>
    "h_f16_544": ("14", 544, 64, "fp16", "f16", 0.0, 200, 7644),         # <fp16, F16, 1, 4, lds>
    "h_f16_1024": ("18", 1024, 16, "fp16", "f16", COMMON, 1000, 8024),   # <fp16, F16, 1, 8, reg>
    "h_bf_96": ("14", 96, 64, "fp16", "bf16", 0.0, 200, 7096),           # <fp16, BF16, 1, 4, lds>
    "h_bf_544": ("14", 544, 16, "fp16", "bf16", 0.0, 1000, 7544),        # <fp16, BF16, 1, 4, reg>
    "h_bf_1024": ("24", 1024, 24, "fp16", "bf16", 0.0, 1000, 8124),      # <fp16, BF16, 2, 4, lds>
    "b_f32_96": ("18", 96, 24, "bf16", "f32", 0.0, 1000, 7096),          # <bf16, F32, 1, 8, lds>
    "b_f32_544": ("14", 544, 64, "bf16", "f32", 0.0, 200, 7544),         # <bf16, F32, 1, 4, lds>
    "b_f32_1024": ("24", 1024, 16, "bf16", "f32", COMMON, 1000, 8024),   # <bf16, F32, 2, 4, reg>
    "b_f16_96": ("18", 96, 16, "bf16", "f16", 0.0, 1000, 7096),          # <bf16, F16, 1, 8, reg>
    "b_f16_544": ("24", 544, 24, "bf16", "f16", 0.0, 1000, 7544),        # <bf16, F16, 2, 4, lds>
    "b_f16_1024": ("14", 1024, 64, "bf16", "f16", 0.0, 200, 8024),       # <bf16, F16, 1, 4, lds>
    "b_bf_96": ("14", 96, 64, "bf16", "bf16", 0.0, 200, 7096),           # <bf16, BF16, 1, 4, lds>
    "b_bf_544": ("24", 544, 16, "bf16", "bf16", COMMON, 1000, 7544),     # <bf16, BF16, 2, 4, reg>
    "b_bf_1024": ("18", 1024, 24, "bf16", "bf16", COMMON, 1000, 9124),   # <bf16, BF16, 1, 8, lds>
}
HELPER_DIMS = (32, 96, 544, 1024)


def coarse_job(case):
    _, d, _, storage, _, common, N, seed = COARSE[case]
    return dict(n=CN, N=N, d=d, storage=storage, common=common, seed=seed)


def job_key(job):
    return tuple(sorted(job.items()))


def coarse_jobs():
    """The distinct data sets of COARSE (several cases share one: the reference does not depend on k, shape or query type)."""
    return {job_key(coarse_job(c)): coarse_job(c) for c in COARSE}


# ---------------------------------------------------------------------------------------------------- GPU side
def typed(x, qtype):
    """float32 rows whose values are exact in `qtype` -> what FlatIndex takes for that type."""
    if qtype == "f32":
        return x
    if qtype == "f16":
        h = x.astype(np.float16)
        assert np.array_equal(h.astype(np.float32), x)
        return h
    import torch
    b = torch.from_numpy(x).to(torch.bfloat16)
    assert torch.equal(b.float(), torch.from_numpy(x))
    return b


def make_index(db, storage):
    from svx.postprocess.flat_index import FlatIndex
    idx = FlatIndex(d=db.shape[1], storage=storage)
    idx.add_unit_rows(db)
    if db.shape[0]:
        assert np.array_equal(idx.rows.float().cpu().numpy(), db)   # stored as they are
    return idx


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def sorted_lists(topk):
    return -np.sort(-topk.cpu().numpy(), axis=1)


def exact_fails(label, lists, mean, want_lists, want_mean):
    fails = []
    bad = np.nonzero((bits(lists) != bits(want_lists)).any(axis=1))[0]
    if bad.size:
        i = int(bad[0])
        j = int(np.nonzero(bits(lists[i]) != bits(want_lists[i]))[0][0])
        fails.append("%s: kept lists differ in %d of %d rows; row %d place %d: %.9g, exact %.9g"
                     % (label, bad.size, lists.shape[0], i, j, lists[i, j], want_lists[i, j]))
    bad = np.nonzero(bits(mean) != bits(want_mean))[0]
    if bad.size:
        i = int(bad[0])
        fails.append("%s: means differ in %d of %d rows; row %d: %.9g, exact %.9g" % (label, bad.size, mean.shape[0], i, mean[i], want_mean[i]))
    return fails


def run_lattice(q, db, k, storage, qtype):
    """-> failure texts of one search of `db`: mean_sim and a first merge_topk against the exact lists and means."""
    want_lists, want_mean = mr.lattice_ref(q, db, k)
    idx = make_index(db, storage)
    qq = typed(q, qtype)
    mean = idx.mean_sim(qq, k).cpu().numpy()
    topk, mean2 = idx.merge_topk(qq, k, None, want_mean=True)
    lists = sorted_lists(topk)
    fails = exact_fails("merge_topk", lists, mean2.cpu().numpy(), want_lists, want_mean)
    fails += exact_fails("mean_sim", want_lists, mean, want_lists, want_mean)
    return fails, lists


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(LATTICE))
def test_lattice(case, monkeypatch):
    shape, n, N, d, k, storage, qtype, order, seed = LATTICE[case]
    if shape is None:
        monkeypatch.delenv("SVX_KNN_SHAPE", raising=False)
    else:
        monkeypatch.setenv("SVX_KNN_SHAPE", shape)
    q, db = mr.lattice(n, N, d, k, seed, order)
    fails, _ = run_lattice(q, db, k, storage, qtype)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,n,d,k,storage,qtype", [(None, 65, 1024, 16, "fp16", "f32"), (None, 65, 544, 40, "bf16", "f16"),
                                                       ("24", 129, 160, 20, "fp16", "bf16"), ("18", 129, 96, 15, "bf16", "f32")])
def test_lattice_orders_agree(shape, n, d, k, storage, qtype, monkeypatch):
    """The shuffled, rising and falling orders of one database: each exact, and the same sorted lists."""
    if shape is None:
        monkeypatch.delenv("SVX_KNN_SHAPE", raising=False)
    else:
        monkeypatch.setenv("SVX_KNN_SHAPE", shape)
    kept = {}
    for order in ("shuffled", "rising", "falling"):
        q, db = mr.lattice(n, 1000, d, k, 77, order)
        fails, kept[order] = run_lattice(q, db, k, storage, qtype)
        assert not fails, order + ": " + "\n".join(fails)
    assert np.array_equal(bits(kept["rising"]), bits(kept["shuffled"])) and np.array_equal(bits(kept["falling"]), bits(kept["shuffled"]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(SHARDS))
def test_lattice_shards(case, monkeypatch):
    from svx.postprocess.flat_index import FlatIndex
    shape, k, order, shards = SHARDS[case]
    n, d, storage, qtype = SHARD_SHAPE[case]
    if shape is None:
        monkeypatch.delenv("SVX_KNN_SHAPE", raising=False)
    else:
        monkeypatch.setenv("SVX_KNN_SHAPE", shape)
    q, db = mr.lattice(n, sum(shards), d, k, 900 + k, order)
    qq = typed(q, qtype)
    topk, lo, fails = None, 0, []
    for m in shards:
        part = FlatIndex(d=d, storage=storage)
        part.add_unit_rows(db[lo:lo + m])
        assert part.ntotal == m
        topk, mean = part.merge_topk(qq, k, topk, want_mean=True)
        lo += m
        want_lists, want_mean = mr.lattice_ref(q, db[:lo], k)
        if lo < k:
            assert np.isneginf(want_lists[:, lo:]).all() and np.isneginf(want_mean).all()
        fails += exact_fails("after %d rows" % lo, sorted_lists(topk), mean.cpu().numpy(), want_lists, want_mean)
    assert not fails, "\n".join(fails)
    once, once_mean = make_index(db, storage).merge_topk(qq, k, None, want_mean=True)
    assert np.array_equal(bits(sorted_lists(once)), bits(sorted_lists(topk)))
    assert np.array_equal(bits(once_mean.cpu().numpy()), bits(mean.cpu().numpy()))


# ---- (c) coarse-grid family
@pytest.fixture(scope="module")
def coarse_refs():
    """The float64 chain and the sequential-fp32 restatement of every coarse data set, in processes that never touch
    the GPU (spawn), started before the first case asks."""
    jobs = coarse_jobs()
    pool = multiprocessing.get_context("spawn").Pool(min(len(jobs), 12))
    pending = {key: pool.apply_async(mr.coarse_reference, (job,)) for key, job in jobs.items()}
    yield pending
    pool.terminate()
    pool.join()


def run_coarse(case, ref, records=None):
    """-> failure texts (SVX_KNN_SHAPE is set by the caller).  records (optional list) receives one dict per quantity."""
    shape, d, k, storage, qtype = COARSE[case][:5]
    job = coarse_job(case)
    q, db = mr.coarse_data(job)
    l64, m64, lseq, mseq = mr.coarse_k(ref, k)
    idx = make_index(db, storage)
    qq = typed(q, qtype)
    mean = idx.mean_sim(qq, k).cpu().numpy()
    topk, mean2 = idx.merge_topk(qq, k, None, want_mean=True)
    fails = []
    for name, g, o, t in (("lists", sorted_lists(topk), lseq, l64), ("mean", mean, mseq, m64), ("merge mean", mean2.cpu().numpy(), mseq, m64)):
        e_gpu, e_orc, bound = mr.rule(g, o, t)
        print("%s %s: E_gpu %.3e E_orc %.3e bound %.3e" % (case, name, e_gpu, e_orc, bound))
        if records is not None:
            records.append(dict(case=case, what=name, d=d, k=k, storage=storage, qtype=qtype, shape=shape, E_gpu=float("%.3e" % e_gpu),
                                E_orc=float("%.3e" % e_orc), ratio=round(e_gpu / e_orc, 2) if e_orc > 0 else None, bound=float("%.3e" % bound)))
        if not e_gpu <= bound:
            fails.append("%s %s: E_gpu %.3e > max(2 E_orc = %.3e, floor %.3e)" % (case, name, e_gpu, 2 * e_orc, 4 * mr.U * float(np.abs(t).max())))
    return fails


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(COARSE))
def test_coarse(case, coarse_refs, monkeypatch):
    monkeypatch.setenv("SVX_KNN_SHAPE", COARSE[case][0])
    fails = run_coarse(case, coarse_refs[job_key(coarse_job(case))].get())
    assert not fails, "\n".join(fails)


# ---- (d) svx_unit_rows
def unit_rows_input(d):
    x = mr.coarse_rows(301, d, 40 + d, common=1.4 if d == 544 else 0.0, useed=d)
    x[17] = 0
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("storage", mr.STORAGES)
@pytest.mark.parametrize("intype", mr.QTYPES)
def test_unit_rows(intype, storage):
    """Coarse-grid rows (exact sum of squares in any order) and one zero row: round_storage(x * inv) bit for bit."""
    from svx.postprocess.flat_index import FlatIndex
    for d in HELPER_DIMS:
        x = unit_rows_input(d)
        idx = FlatIndex(d=d, storage=storage)
        idx.add(typed(x, intype))
        got = idx.rows.float().cpu().numpy()
        want = mr.unit_rows_ref(x, storage)
        assert not got[17].any()
        diff = bits(got) != bits(want)
        assert not diff.any(), "d = %d: %d of %d elements differ from round_storage(x * inv)" % (d, diff.sum(), diff.size)


# ---- (e) svx_margin_scores
def margin_input(d):
    """-> x, y [403, d] coarse-grid rows, mean_xy, mean_yx [403]; rows 0 .. 4 are the edge rows."""
    n = 403
    x, y = mr.coarse_rows(n, d, 60 + d, 1.4, d), mr.coarse_rows(n, d, 61 + d, 1.4, d)
    rng = np.random.default_rng(d)
    mxy, myx = rng.uniform(0.2, 0.9, n).astype(np.float32), rng.uniform(0.2, 0.9, n).astype(np.float32)
    x[0] = 0                                                          # a zero x row: a = 0
    mxy[1], myx[1] = np.float32(0.375), np.float32(-0.375)            # mean_xy + mean_yx = 0
    x[2], mxy[2], myx[2] = 0, np.float32(0.25), np.float32(-0.25)     # both: 0 / 0
    mxy[3], myx[3] = np.float32(-0.5), np.float32(0.125)              # a negative mean
    y[4] = -y[4]                                                      # a negative mean under a negative cosine
    mxy[4], myx[4] = np.float32(-0.25), np.float32(-0.0625)
    return x, y, mxy, myx


def gpu_margin_scores(x, y, mxy, myx, margin):
    from svx import _lib
    from svx.postprocess.flat_index import _torch_dtype_code, to_device_rows
    from svx.postprocess.score_align import MARGINS
    ctx = _lib.context(None)
    t = ctx.torch
    xd, yd = to_device_rows(ctx, x), to_device_rows(ctx, y)
    assert xd.dtype == yd.dtype
    a, b = t.from_numpy(mxy).to(ctx.tdev), t.from_numpy(myx).to(ctx.tdev)
    out = t.empty((xd.shape[0],), dtype=t.float32, device=ctx.tdev)
    ctx.check(ctx.lib.svx_margin_scores(ctx.h, ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(yd.data_ptr()), _torch_dtype_code(t, xd.dtype),
                                        int(xd.shape[0]), int(xd.shape[1]), ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()),
                                        MARGINS[margin], ctypes.c_void_p(out.data_ptr())))
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("margin", ["ratio", "distance"])
@pytest.mark.parametrize("dtype", mr.QTYPES)
def test_margin_scores(dtype, margin):
    """k_margin_scores on coarse-grid x and y: sxx, syy and sxy are exact in fp32 (integer multiples of 2^-12 below
    2^24 of them), so the error against float64 comes from the kernel's last operations only, each within u = 2^-24
    relative: ix, iy (a square root and a division each), the two products of a, the sum of b, the final operation.
    distance: |error| <= 2u A with A = |a| + |b| + |a - b| (the subtraction may be contracted into an fma);
    ratio: relative error <= 5u.  Rows 0 .. 4 are the edge rows, compared with numpy's own fp32 result."""
    u = mr.U
    for d in HELPER_DIMS:
        x, y, mxy, myx = margin_input(d)
        n = x.shape[0]
        got = gpu_margin_scores(typed(x, dtype), typed(y, dtype), mxy, myx, margin)
        t, a, b = mr.margin_f64(x, y, mxy, myx, margin)
        mine = mr.margin_f32(x, y, mxy, myx, margin)
        # rows whose exact result is not finite, and the zero rows (a = 0 on both sides): numpy's own result
        fin = np.isfinite(t)
        assert fin[3] and fin[4] and (~fin).sum() == (2 if margin == "ratio" else 0)
        for i in sorted({0, 2} | set(np.nonzero(~fin)[0].tolist())):
            assert np.array_equal(got[i:i + 1], mine[i:i + 1], equal_nan=True), "d = %d row %d: %r, numpy %r" % (d, i, got[i], mine[i])
        err = np.abs(got[fin].astype(np.float64) - t[fin])
        if margin == "distance":
            lim = 2 * u * (np.abs(a) + np.abs(b) + np.abs(a - b))[fin]
        else:
            lim = 5 * u * np.abs(t[fin])
        worst = float((err / np.where(lim > 0, lim, 1.0)).max())
        print("margin_scores %s %s d = %d: worst error / bound %.3f" % (dtype, margin, d, worst))
        assert (err <= lim).all(), "d = %d: %d rows past the bound, worst error / bound %.3f" % (d, int((err > lim).sum()), worst)


def main():
    import argparse
    import os
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", required=True)
    a = ap.parse_args()
    jobs = coarse_jobs()
    pool = multiprocessing.get_context("spawn").Pool(min(len(jobs), 12))
    bad, worst = 0, (0.0, "")
    try:
        pending = {key: pool.apply_async(mr.coarse_reference, (job,)) for key, job in jobs.items()}
        with open(a.dump, "w") as f:
            for case in COARSE:
                records = []
                os.environ["SVX_KNN_SHAPE"] = COARSE[case][0]
                fails = run_coarse(case, pending[job_key(coarse_job(case))].get(), records)
                for r in records:
                    f.write(json.dumps(r, separators=(",", ":")) + "\n")
                    if r['bound'] > 0 and r['E_gpu'] / r['bound'] > worst[0]:
                        worst = (r['E_gpu'] / r['bound'], "%s %s: E_gpu %.2e E_orc %.2e" % (case, r['what'], r['E_gpu'], r['E_orc']))
                bad += len(fails)
                for t in fails:
                    print("  " + t, flush=True)
    finally:
        pool.terminate()
        pool.join()
    print("worst E_gpu / bound %.2f (%s)" % worst)
    print("margin matrix, coarse grid: %d cases, %d failures" % (len(COARSE), bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
