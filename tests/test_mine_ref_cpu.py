"""The references of tests/mine_ref.py against one another, svx_mine_greedy through ctypes, and the properties of the
inputs that tests/test_gpu_mine.py rests on.  No GPU.

1. The fp32 contract (a) equals the literal LASER loops (c) on small random lists and on lists built to tie: duplicate
   (similarity, mean) candidates, equal best scores forward and backward, (-inf, -1) tails, ids out of range; the
   retrieval step of svx.postprocess.mine (select_pairs, run on CPU tensors) equals both.
2. svx_mine_greedy equals (c)'s greedy pass on random candidate lists with repeated rows and equal scores; n_cand = 0; an
   index out of range returns -SVX_ERR_ARG.
3. tests/golden/margin_example.npz at k = 16, from the float64 reference (b): for ratio and distance at least 3 % of the
   rows have a margin best that is not the nearest neighbour (measured 6.3 % and 5.2 %), so a kernel that ignored the
   gathered mean would be caught; the share of rows whose two best float64 scores lie within twice the comparison bound
   of margin_ref.rule ((a) against (b)) stays under search_ref.AMBIGUOUS_CAP.  The lattice cases of the GPU test: the
   similarities of BOTH search directions are exact in fp32 in any order of accumulation."""
import ctypes
import os

import numpy as np
import pytest

import margin_ref as mr
import mine_ref as ref
import search_ref as sr
from svx.postprocess import mine

assert tuple(mine.MARGINS) == ref.MARGINS and tuple(mine.RETRIEVALS) == ref.RETRIEVALS   # the names the package takes

GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 16

# (n, N, d, k, storage, query type, database order, seed): the lattice cases of test_gpu_mine.py
LATTICE = {
    "h_f16_65x333": (65, 333, 1024, 16, "fp16", "f16", "shuffled", 71),
    "b_bf_repeated": (64, 241, 544, 16, "bf16", "bf16", "repeated", 6),
    "h_f16_square_k15": (333, 333, 96, 15, "fp16", "f16", "rising", 73),
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lattice_sides(case):
    """-> (x rows [n, d] = the normalised lattice queries, y rows [N, d] = the lattice database, both exact in the storage
    type; S_xy [n, N] and S_yx [N, n] float64: the similarities the two searches compute)."""
    n, N, d, k, storage, qtype, order, seed = LATTICE[case]
    q, db = mr.lattice(n, N, d, k, seed, order)
    x = (q.astype(np.float64) / np.sqrt((q.astype(np.float64) ** 2).sum(axis=1))[:, None]).astype(np.float32)
    assert np.array_equal(mr.round_storage(x, storage), x) and np.array_equal(mr.round_storage(db, storage), db)
    S_xy = mr.lattice_sims(x, db)
    # y in x: the search normalises the database rows as queries, in fp32 and in its own order, and rounds them to storage
    yq = mr.round_storage(sr.unit_f32_lanes(db), storage)
    S_yx = yq.astype(np.float64) @ x.astype(np.float64).T
    return x, db, yq, S_xy, S_yx


# ---- 1. (a) against (c)
def tiny_cases():
    rs = np.random.RandomState(5)
    out = {}
    for name, (n, k, n_db, id_base) in {"random": (9, 5, 12, 0), "k1": (6, 1, 6, 3), "based": (7, 4, 9, (1 << 33) + 7)}.items():
        sims = -np.sort(-rs.rand(n, k).astype(np.float32), axis=1)
        ids = np.stack([rs.permutation(n_db)[:k] for _ in range(n)]).astype(np.int64) + id_base
        out[name] = (sims, ids, rs.rand(n).astype(np.float32) + np.float32(0.2), rs.rand(n_db).astype(np.float32) + np.float32(0.2), id_base)
    # duplicate (similarity, mean) candidates: every score of a row ties
    sims = np.full((4, 6), 0.5, np.float32)
    ids = np.stack([np.roll(np.arange(6), s) for s in range(4)]).astype(np.int64)
    out["all_tie"] = (sims, ids, np.full(4, 0.25, np.float32), np.full(6, 0.75, np.float32), 0)
    # tails and ids out of range, a row without a candidate
    sims = np.float32([[0.9, 0.8, -np.inf], [0.7, 0.6, 0.5], [-np.inf] * 3, [0.4, 0.4, 0.4]])
    ids = np.int64([[2, 0, -1], [7, -5, 1], [-1, -1, -1], [9, 3, 3]])
    out["tails"] = (sims, ids, np.float32([0.5, 0.4, 0.3, 0.2]), np.float32([0.3, 0.5, 0.5, 0.25]), 0)
    for d in ref.synthetic_lists(24, 4, 7, 11, seed=3), ref.synthetic_lists(17, 1, 3, 0, seed=4, shift=3):
        out["synthetic_k%d" % d["sims"].shape[1]] = (d["sims"], d["ids"], d["mean_q"], d["mean_db"], 11 if d["sims"].shape[1] == 4 else 0)
    return out


@pytest.mark.parametrize("margin", ref.MARGINS)
@pytest.mark.parametrize("case", list(tiny_cases()))
def test_contract_equals_laser_loops(case, margin):
    sims, ids, mq, md, id_base = tiny_cases()[case]
    scores, best_id, best_score = ref.candidates(sims, ids, mq, md, margin, id_base)
    lscores = ref.laser_score_candidates(sims, ids, mq, md, margin, id_base)
    assert np.array_equal(bits(scores), bits(lscores))
    lid, lscore = ref.laser_best(lscores, ids)
    assert np.array_equal(best_id, lid) and np.array_equal(bits(best_score), bits(lscore))
    # the float64 reference (b) agrees on which candidates are valid
    s64, _, _ = ref.candidates(sims, ids, mq, md, margin, id_base, np.float64)
    assert np.array_equal(np.isfinite(s64), np.isfinite(scores))
    mean = ref.list_means(sims)
    with np.errstate(invalid="ignore"):
        want = np.float32([np.float32(sum((np.float32(v) for v in row[1:]), np.float32(row[0]))) / np.float32(len(row)) for row in sims])
    assert np.array_equal(bits(mean), bits(want))


def mining_cases():
    """(sims_xy, ids_xy, sims_yx, ids_yx): small two-sided problems, some with equal best scores forward and backward."""
    out = {}
    rs = np.random.RandomState(11)
    for name, (nx, ny, k, levels) in {"random": (9, 7, 3, 0), "coarse_ties": (12, 12, 4, 4), "square_ties": (8, 8, 2, 2)}.items():
        S = rs.rand(nx, ny)
        if levels:
            S = np.rint(S * levels) / levels      # few distinct similarities: ties everywhere, also between the directions
        S = S.astype(np.float32)
        out[name] = sr.search_exact(S, k) + sr.search_exact(np.ascontiguousarray(S.T), k)
    # a symmetric problem: every forward candidate has a backward twin with the same score
    S = np.float32([[0.9, 0.5, 0.1], [0.5, 0.9, 0.5], [0.1, 0.5, 0.9]])
    out["symmetric"] = sr.search_exact(S, 2) + sr.search_exact(S.T.copy(), 2)
    return out


@pytest.mark.parametrize("retrieval", ref.RETRIEVALS)
@pytest.mark.parametrize("margin", ref.MARGINS)
@pytest.mark.parametrize("case", list(mining_cases()))
def test_retrievals_equal_laser_loops(case, margin, retrieval):
    import torch
    sims_xy, ids_xy, sims_yx, ids_yx = mining_cases()[case]
    best = ref.mine(sims_xy, ids_xy, sims_yx, ids_yx, margin)
    mean_x, mean_y = ref.list_means(sims_xy), ref.list_means(sims_yx)
    fb, fs = ref.laser_best(ref.laser_score_candidates(sims_xy, ids_xy, mean_x, mean_y, margin), ids_xy)
    bb, bs = ref.laser_best(ref.laser_score_candidates(sims_yx, ids_yx, mean_y, mean_x, margin), ids_yx)
    for got, want in zip(best, (fb, fs, bb, bs)):
        assert np.array_equal(got.view(np.uint32) if got.dtype == np.float32 else got, want.view(np.uint32) if want.dtype == np.float32 else want)
    thresholds = (None, float(np.median(best[1])))
    for threshold in thresholds:
        want = ref.triples_of_list(ref.laser_retrieve(*best, retrieval, threshold))
        assert ref.as_triples(ref.select(*best, retrieval, threshold)) == want
        # the package's retrieval step, on CPU tensors (the greedy pass is native host code)
        got = mine.select_pairs(*(torch.from_numpy(a) for a in best), retrieval=retrieval, threshold=threshold)
        assert got[0].dtype == np.float32 and got[1].dtype == np.int64 and got[2].dtype == np.int64
        assert ref.as_triples(got) == want
    if retrieval == "max":
        kept = ref.laser_retrieve(*best, "max")
        assert len({c[1] for c in kept}) == len(kept) == len({c[2] for c in kept})


def test_unknown_names_raise():
    import torch
    z = torch.zeros(3, dtype=torch.int64), torch.zeros(3), torch.zeros(3, dtype=torch.int64), torch.zeros(3)
    with pytest.raises(ValueError):
        mine.select_pairs(*z, retrieval="union")
    with pytest.raises(ValueError, match="Wrong margin type: cosine"):
        mine.mine_bitexts(None, None, margin="cosine")
    with pytest.raises(ValueError):
        mine.mine_bitexts(None, None, retrieval="union")


# ---- 2. svx_mine_greedy
def greedy_native(order, src, tgt, n_src, n_tgt):
    from svx import _lib
    lib = _lib.load()
    order, src, tgt = (np.ascontiguousarray(a, np.int64) for a in (order, src, tgt))
    out = np.full(order.shape[0] + 1, -7, np.int64)
    kept = lib.svx_mine_greedy(ctypes.c_void_p(order.ctypes.data), order.shape[0], ctypes.c_void_p(src.ctypes.data),
                               ctypes.c_void_p(tgt.ctypes.data), n_src, n_tgt, ctypes.c_void_p(out.ctypes.data))
    assert out[-1] == -7 and (kept < 0 or (out[kept:] == -7).all())
    return kept, out[:max(kept, 0)]


@pytest.mark.parametrize("seed", range(6))
def test_greedy_native(seed):
    rs = np.random.RandomState(seed)
    n_src, n_tgt, n_cand = [(5, 4, 30), (40, 50, 200), (1, 1, 9), (300, 7, 500), (64, 64, 128), (1000, 1000, 3000)][seed]
    src, tgt = rs.randint(n_src, size=n_cand), rs.randint(n_tgt, size=n_cand)     # repeated rows on both sides
    scores = rs.randint(0, 6, size=n_cand).astype(np.float32)                        # equal scores: the stable order decides
    order = np.argsort(-scores, kind="stable")
    kept, out = greedy_native(order, src, tgt, n_src, n_tgt)
    want = ref.greedy(order, src, tgt)
    assert kept == want.shape[0] and np.array_equal(out, want)
    # (c)'s pass on the sorted triples keeps the same pairs in the same order
    cands = sorted(zip(scores, src, tgt), key=lambda c: -c[0])
    seen_s, seen_t, pairs = set(), set(), []
    for _, s, t in cands:
        if s not in seen_s and t not in seen_t:
            seen_s.add(s)
            seen_t.add(t)
            pairs.append((int(s), int(t)))
    assert [(int(src[c]), int(tgt[c])) for c in out] == pairs
    # a permuted (not sorted) order is honoured as given
    perm = rs.permutation(n_cand)
    kept, out = greedy_native(perm, src, tgt, n_src, n_tgt)
    assert np.array_equal(out, ref.greedy(perm, src, tgt))


def test_greedy_native_edges():
    from svx import _lib
    lib = _lib.load()
    assert lib.svx_mine_greedy(None, 0, None, None, 0, 0, None) == 0
    assert greedy_native(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), 5, 5)[0] == 0
    src, tgt = np.int64([0, 1, 2]), np.int64([2, 1, 0])
    assert greedy_native([0, 1, 2], src, tgt, 3, 3)[0] == 3
    err = -_lib.SVX_ERR_ARG
    assert greedy_native([0, 3, 1], src, tgt, 3, 3)[0] == err          # candidate index past n_cand
    assert greedy_native([0, -1, 1], src, tgt, 3, 3)[0] == err
    assert greedy_native([0, 1, 2], src, tgt, 2, 3)[0] == err          # source row past n_src
    assert greedy_native([0, 1, 2], src, tgt, 3, 2)[0] == err          # target row past n_tgt
    assert greedy_native([0, 1, 2], np.int64([0, -1, 2]), tgt, 3, 3)[0] == err
    assert lib.svx_mine_greedy(None, 3, None, None, 3, 3, None) == err
    assert lib.svx_mine_greedy(None, -1, None, None, 3, 3, None) == err


def test_exports():
    from svx import _lib
    lib = _lib.load()
    for name in ("svx_knn_list_means", "svx_margin_candidates", "svx_mine_greedy"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.SVX_MARGIN_ABSOLUTE == 2


# ---- 3. input properties
@pytest.fixture(scope="module")
def example():
    g = np.load(os.path.join(GD, "margin_example.npz"))
    x, y = g["db_src"], g["db_tgt"]
    assert x.shape == y.shape == (347, 1024)
    lists = ref.example_lists_f64(x, y, K)
    # the fp32 lists both references start from
    return tuple(a.astype(np.float32) if a.dtype == np.float64 else a for a in lists)


@pytest.mark.parametrize("margin", ["ratio", "distance"])
def test_example_has_teeth(example, margin):
    sims_xy, ids_xy, sims_yx, ids_yx = example
    n = sims_xy.shape[0]
    report = []
    for name, (s, i, so) in {"forward": (sims_xy, ids_xy, sims_yx), "backward": (sims_yx, ids_yx, sims_xy)}.items():
        mq64, md64 = ref.list_means(s, np.float64), ref.list_means(so, np.float64)
        s64, best64, _ = ref.candidates(s, i, mq64, md64, margin, 0, np.float64)
        s32, best32, _ = ref.candidates(s, i, ref.list_means(s), ref.list_means(so), margin)
        reranked = float((best64 != i[:, 0]).mean())
        identity = float((best64 == np.arange(n)).mean())
        e32, _, bound = mr.rule(s32, s32, s64)
        gap = ref.top_two_gap(s64)
        close = float((gap <= 2 * bound).mean())
        report.append("%s %s: identity %.3f, re-ranked %.3f, fp32 error %.2e, bound %.2e, smallest gap %.2e, rows within 2 x bound %.4f, "
                      "fp32 best differs from float64 in %d rows" % (margin, name, identity, reranked, e32, bound, gap.min(), close, (best32 != best64).sum()))
        print(report[-1])
        assert reranked >= 0.03, report[-1]
        assert close <= sr.AMBIGUOUS_CAP, report[-1]
        assert (best32 != best64).mean() <= close
    fb, _, bb, _ = ref.mine(sims_xy, ids_xy, sims_yx, ids_yx, margin, np.float64)
    inter = int((bb[fb] == np.arange(n)).sum())
    print("%s: %d intersection pairs" % (margin, inter))
    assert 250 <= inter <= n


@pytest.mark.parametrize("case", list(LATTICE))
def test_lattice_both_directions_exact(case):
    n, N, d, k, storage, qtype, order, seed = LATTICE[case]
    x, db, yq, S_xy, S_yx = lattice_sides(case)
    assert n >= k and N >= k
    for S in (S_xy, S_yx):
        assert np.array_equal(S.astype(np.float32).astype(np.float64), S)
    # y in x: every product is a multiple of u = (smallest exponent step of the rounded rows) * 2^-m and the absolute
    # sum of a row's products stays below 2^24 u, so every partial sum is exact in fp32 whatever its order
    m = int(np.log2(mr.pow4_floor(d))) // 2
    nz = np.abs(yq[yq != 0]).astype(np.float64)
    frac_bits = 10 if storage == "fp16" else 7
    u = 2.0 ** (np.floor(np.log2(nz.min())) - frac_bits - m)
    prods = np.abs(yq.astype(np.float64)) @ np.abs(x.astype(np.float64)).T
    assert prods.max() < 2.0 ** 24 * u
    assert np.array_equal(np.rint(S_yx / u) * u, S_yx)
    # ties at the best place exist in both directions: the order of the contract is exercised
    for S in (S_xy, S_yx):
        vals, _ = sr.search_exact(S, k)
        assert (vals[:, 0] == vals[:, 1]).any() if k > 1 else True
