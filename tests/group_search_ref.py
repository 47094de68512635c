"""References for the grouped search (csrc/svx_groupsearch.hip: k_knn_search_groups, FlatIndex.search_groups) and for local
mining (svx/postprocess/mine.py: mine_local).  numpy only; shared by test_group_search_ref_cpu.py (no GPU) and
test_gpu_group_search.py; TEST INFRASTRUCTURE.

A grouped search is a search per group: `search_groups_exact` is search_ref.search_exact applied to every group's block
of the similarity matrix with id_base = db_off[g]; `mine_local_ref` is mine_ref's loops applied per group.

The LATTICE group sets are built from margin_ref.lattice: one query matrix and one database per group (so every
similarity is exact in fp32 and the GPU must return the reference's bits), concatenated."""
import numpy as np

import margin_ref as mr
import mine_ref as mnr
import search_ref as sr

# query rows and database rows per group that every lattice set draws from (k - 1 and k are filled in per set)
Q_COUNTS = (0, 1, 5, 63, 64, 65, 129)
DB_COUNTS = (0, "k-1", "k", 33, 49, 65, 241)

# id: (d, k, storage, query type, database order, seed, [(queries, database rows) per group])
#   "k-1" / "k" stand for k - 1 / k database rows.  Between them the sets cover every query count and every database count
#   above, group starts that are no multiple of the 32-row tile, the five dimensions, the five k, the four orders and the six
#   instantiations (storage x query type).
LATTICE_SETS = {
    "h_f32_d1024_k16": (1024, 16, "fp16", "f32", "shuffled", 11,
                        [(5, 33), (0, 49), (64, "k"), (1, 241), (65, 0), (129, 65), (63, "k-1"), (64, 49)]),
    "h_f16_d96_k1": (96, 1, "fp16", "f16", "rising", 12,
                     [(63, 33), (65, "k"), (1, 49), (0, 0), (129, 241), (5, "k-1"), (64, 65)]),
    "h_bf_d544_k15": (544, 15, "fp16", "bf16", "falling", 13,
                      [(129, 49), (5, "k-1"), (64, 241), (0, 33), (63, 65), (1, "k"), (65, 33)]),
    "b_f32_d32_k24": (32, 24, "bf16", "f32", "repeated", 14,
                      [(1, 33), (65, 49), (63, 241), (5, 65), (129, 33), (64, "k"), (0, "k-1"), (5, 0)]),
    "b_f16_d992_k64": (992, 64, "bf16", "f16", "shuffled", 15,
                       [(64, 65), (5, "k"), (129, 241), (63, "k-1"), (1, 33), (65, 49), (0, 241), (64, 0)]),
    "b_bf_d96_k16": (96, 16, "bf16", "bf16", "rising", 16,
                     [(65, 241), (63, 49), (0, "k"), (129, "k-1"), (1, 65), (5, 33), (64, 33)]),
    "h_f32_d32_k64_falling": (32, 64, "fp16", "f32", "falling", 17,
                              [(5, 241), (64, 65), (63, "k")]),
    "b_f32_d1024_k15_repeated": (1024, 15, "bf16", "f32", "repeated", 18,
                                 [(65, 49), (1, 33), (129, 241)]),
    # one group: plain search
    "single_group": (544, 16, "fp16", "f32", "shuffled", 19, [(129, 241)]),
}
# >= 300 groups of 40 .. 70 queries: more than 256 workgroups, the last workgroup of most groups partly masked
MANY = ("many_groups", 96, 16, "fp16", "f16", "shuffled", 21, 320)


def resolve_counts(groups, k):
    return [(int(nq), k - 1 if N == "k-1" else k if N == "k" else int(N)) for nq, N in groups]


def many_counts(n_groups, seed):
    rs = np.random.RandomState(seed)
    return [(int(a), int(b)) for a, b in zip(rs.randint(40, 71, size=n_groups), rs.randint(17, 50, size=n_groups))]


def offsets(counts):
    """[(queries, database rows)] -> (q_off, db_off) int64 [n_groups + 1]."""
    c = np.asarray(counts, np.int64).reshape(-1, 2)
    return (np.concatenate([[0], np.cumsum(c[:, 0])]).astype(np.int64), np.concatenate([[0], np.cumsum(c[:, 1])]).astype(np.int64))


def _tying_lattice(nq, N, d, k, seed, order):
    """margin_ref.lattice(nq, N, ...) with the first seed from `seed` on for which, when the group has queries and a
    (k+1)-th row, at least one query ties at the k-th place.  -> (q, db, exact similarities)."""
    for s in range(seed, seed + 400):
        q, db = mr.lattice(max(nq, 1), max(N, 1), d, k, s, order)
        q, db = q[:nq], db[:N]
        sims = mr.lattice_sims(q, db) if nq and N else np.zeros((nq, N))
        if not (nq and N > k) or sr.tie_shares(sims, k)[0] > 0:
            return q, db, sims
    raise AssertionError("no seed gives a tie at the k-th place for %s" % ((nq, N, d, k, seed, order),))


def lattice_groups(counts, d, k, seed, order):
    """One margin_ref.lattice per group, concatenated -> (q [n, d], db [N, d], q_off, db_off, [exact similarity matrix of
    every group, float64]).  A group without queries or without database rows still contributes the other side; the
    `repeated` order falls back to `shuffled` for a database of fewer than k + 6 rows.  Every group with queries and a
    (k+1)-th row has a query that ties at the k-th place (the seed of a group is advanced until it has)."""
    qs, dbs, sims = [], [], []
    for g, (nq, N) in enumerate(counts):
        o = "shuffled" if order == "repeated" and N < k + 6 else order
        q, db, s = _tying_lattice(nq, N, d, k, seed + 1009 * g, o)
        qs.append(q)
        dbs.append(db)
        sims.append(s)
    q_off, db_off = offsets(counts)
    return (np.concatenate(qs).astype(np.float32), np.ascontiguousarray(np.concatenate(dbs), np.float32), q_off, db_off, sims)


# database rows per group of the leak case at k = 16: above k (a leaked row must win its place) and k - 1 (every list has an
# empty slot: any leaked row shows)
LEAK_DB_ROWS = (49, 15)


def leak_groups(n_groups, nq, N, d, k, seed):
    """Consecutive groups hold the SAME lattice database rows, `rising` next to `falling`, and the same queries: every row
    just outside a group's range ties with or beats a row inside it.  -> as lattice_groups."""
    q, up, _ = _tying_lattice(nq, N, d, k, seed, "rising")
    dbs = [up if g % 2 == 0 else np.ascontiguousarray(up[::-1]) for g in range(n_groups)]
    sims = [mr.lattice_sims(q, db) for db in dbs]
    q_off, db_off = offsets([(nq, N)] * n_groups)
    return np.concatenate([q] * n_groups), np.concatenate(dbs), q_off, db_off, sims


def search_groups_exact(group_sims, k, db_off):
    """group_sims[g] [n_g, N_g] -> (values [n, k], ids [n, k] int64): search_ref.search_exact per group with
    id_base = db_off[g], the groups' rows one after the other."""
    vals, ids = [], []
    dtype = np.result_type(*[np.asarray(s).dtype for s in group_sims]) if group_sims else np.float64
    for g, s in enumerate(group_sims):
        s = np.asarray(s)
        v, i = sr.search_exact(s.reshape(s.shape[0], -1) if s.size else np.zeros((s.shape[0], 0), dtype), k, int(db_off[g]))
        vals.append(v.astype(dtype))
        ids.append(i)
    if not vals:
        return np.zeros((0, k), dtype), np.zeros((0, k), np.int64)
    return np.concatenate(vals), np.concatenate(ids)


def blocks(S, q_off, db_off):
    """The diagonal blocks of a full similarity matrix S [n, N]."""
    return [S[int(q_off[g]):int(q_off[g + 1]), int(db_off[g]):int(db_off[g + 1])] for g in range(len(q_off) - 1)]


def lattice_pairs(counts, d, k, storage, seed, order):
    """Document pairs on the lattice, as test_mine_ref_cpu.lattice_sides builds one: per pair x = the normalised lattice
    queries and y = the lattice database, both exact in the storage type.  counts: [(source rows, target rows)].
    -> (x [n_x, d], y [n_y, d], x_off, y_off, [S_xy per pair], [S_yx per pair], [yq per pair]); S_xy [n_g, N_g] and
    S_yx [N_g, n_g] are the similarities the two searches compute (y in x: the search normalises the database rows as
    queries, in fp32 and in its own order, and rounds them to storage: yq)."""
    xs, ys, S_xy, S_yx, yqs = [], [], [], [], []
    for g, (n, N) in enumerate(counts):
        q, db = mr.lattice(n, N, d, k, seed + 1009 * g, "shuffled" if order == "repeated" and N < k + 6 else order)
        x = (q.astype(np.float64) / np.sqrt((q.astype(np.float64) ** 2).sum(axis=1))[:, None]).astype(np.float32)
        assert np.array_equal(mr.round_storage(x, storage), x) and np.array_equal(mr.round_storage(db, storage), db)
        yq = mr.round_storage(sr.unit_f32_lanes(db), storage)
        xs.append(x)
        ys.append(db)
        yqs.append(yq)
        S_xy.append(mr.lattice_sims(x, db))
        S_yx.append(yq.astype(np.float64) @ x.astype(np.float64).T)
    x_off, y_off = offsets(counts)
    return np.concatenate(xs), np.concatenate(ys), x_off, y_off, S_xy, S_yx, yqs


def mine_local_ref(S_xy, S_yx, k, margin, retrieval, threshold=None, dtype=np.float32):
    """Local mining by mine_ref's loops, pair after pair: S_xy[g] [n_x, n_y] are the similarities of pair g's source rows
    to its target rows, S_yx[g] [n_y, n_x] those of the other search.  A pair with fewer than k rows on either side is
    left out.  -> (scores, src, tgt, group, number of pairs left out)."""
    parts, small = [], 0
    for g, (A, B) in enumerate(zip(S_xy, S_yx)):
        if A.shape[0] < k or A.shape[1] < k:
            small += 1
            continue
        lists = sr.search_exact(np.asarray(A).astype(dtype), k) + sr.search_exact(np.asarray(B).astype(dtype), k)
        score, src, tgt = mnr.select(*mnr.mine(*lists, margin, dtype), retrieval, threshold)
        parts.append((score, src, tgt, np.full(src.shape, g, np.int64)))
    if not parts:
        return np.zeros(0, dtype), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), small
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4)) + (small,)


def select_global(fwd_best, fwd_score, bwd_best, bwd_score, x_off, y_off, retrieval, threshold=None):
    """mine_local's retrieval step on GLOBAL row numbers: mine_ref.select once over all pairs (one stable sort, one greedy
    pass), then a stable partition by pair -> (scores, src, tgt, group) with rows numbered inside the pair."""
    score, src, tgt = mnr.select(fwd_best, fwd_score, bwd_best, bwd_score, retrieval, threshold)
    group = np.searchsorted(x_off, src, side="right") - 1
    order = np.argsort(group, kind="stable")
    score, src, tgt, group = score[order], src[order], tgt[order], group[order]
    return score, src - x_off[group], tgt - y_off[group], group


def select_per_group(fwd_best, fwd_score, bwd_best, bwd_score, x_off, y_off, retrieval, threshold=None):
    """The same by one mine_ref.select per pair on the pair's own rows."""
    parts = []
    for g in range(len(x_off) - 1):
        xs, xe, ys, ye = int(x_off[g]), int(x_off[g + 1]), int(y_off[g]), int(y_off[g + 1])
        fb = np.where(fwd_best[xs:xe] >= 0, fwd_best[xs:xe] - ys, -1)
        bb = np.where(bwd_best[ys:ye] >= 0, bwd_best[ys:ye] - xs, -1)
        score, src, tgt = mnr.select(fb, fwd_score[xs:xe], bb, bwd_score[ys:ye], retrieval, threshold)
        parts.append((score, src, tgt, np.full(src.shape, g, np.int64)))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


# ------------------------------------------------------------------------------------------------ real rows
# the cuts of tests/golden/example_full (1148 source rows, 1035 target rows): (source row edges, target row edges)
EXAMPLE_CUTS = {
    "one": ([0, 1148], [0, 1035]),
    "two": ([0, 500, 1148], [0, 517, 1035]),
    "three": ([0, 70, 90, 400], [0, 40, 57, 300]),
}


def example_rows(golden_dir):
    import os
    x = np.fromfile(os.path.join(golden_dir, "example_full", "embeds_en.f16"), dtype=np.float16).reshape(-1, 1024)
    y = np.fromfile(os.path.join(golden_dir, "example_full", "embeds_de.f16"), dtype=np.float16).reshape(-1, 1024)
    assert x.shape == (1148, 1024) and y.shape == (1035, 1024)
    return x, y


def example_reference(q, db, storage):
    """search_ref.rows_search_reference's two matrices for q [n, d] fp16 queries and db [N, d] rows as stored, computed once
    for the whole matrix: dict(S64, seq).  A group's bound comes from its own block (`block_bound`)."""
    qs = mr.round_storage(sr.unit_f32_lanes(q.astype(np.float32)), storage)
    return dict(S64=qs.astype(np.float64) @ db.astype(np.float64).T, seq=mr.dots_f32(qs, db))


def block_bound(ref, qs, qe, ds, de):
    """search_ref's bound e = max(2 max|seq - S64|, 4 * 2^-24 max|S64|) over the block [qs, qe) x [ds, de), which is
    what search_ref.rows_search_reference returns for the block's rows (the rule unchanged)."""
    S64, seq = ref["S64"][qs:qe, ds:de], ref["seq"][qs:qe, ds:de]
    return max(2 * float(np.abs(seq.astype(np.float64) - S64).max()), 4 * mr.U * float(np.abs(S64).max()))
