"""References for the id-returning search (csrc/svx_search.hip: k_knn_search, FlatIndex.search / merge_search).  numpy only;
shared by test_search_ref_cpu.py (no GPU) and test_gpu_search.py; TEST INFRASTRUCTURE.

The result of a search is fully determined: a query's k results are the first k entries of the total order
(similarity descending, id ascending) over all rows seen, padded with (-inf, -1).  `search_exact` is that order by
np.lexsort; `search_shards` is the same merged shard by shard, in any order of the shards.

On the LATTICE inputs of margin_ref.py every similarity is exact in fp32, so the GPU must return search_exact's values
(as bits) and ids, nothing exempt.  On the COARSE-GRID inputs the GPU's fp32 similarities differ from the float64 ones by
rounding; `coarse_search_reference` gives the full float64 matrix S64 on the stored operands, and the bound
    e = max(2 max|seq - S64|, 4 * 2^-24 max|S64|)
(stage_check's rule with the sequential-fp32 matrix margin_ref.dots_f32 as the restatement, taken over the whole
matrix: it never depends on what the kernel returns).  A (query, rank) position is AMBIGUOUS when the float64 gap to
the neighbour above or below it is <= 2e (two values that are each off by e may swap); the rank k + 1 neighbour counts
as the neighbour below rank k.  Only ambiguous positions are exempt from id equality, and test_search_ref_cpu.py caps
their share at 1 % per case."""
import numpy as np

import margin_ref as mr

AMBIGUOUS_CAP = 0.01
COARSE_KS = (1, 16, 24, 64)


def search_exact(sims, k, id_base=0):
    """sims [n, N] -> (values [n, k] of sims' dtype, ids [n, k] int64): per row the first k of (similarity descending,
    id = id_base + column ascending), padded with (-inf, -1)."""
    sims = np.asarray(sims)
    n, N = sims.shape
    ids = np.broadcast_to(np.arange(N, dtype=np.int64) + np.int64(id_base), (n, N))
    return merge_exact(None, sims, ids, k)


def merge_exact(state, sims, ids, k):
    """The lists `state` = (values, ids) (None: empty) merged with further rows (sims [n, m], ids [n, m]) -> state."""
    n = sims.shape[0]
    if state is not None:
        keep = state[1] >= 0
        assert np.array_equal(keep, np.isfinite(state[0]))
        sims = np.concatenate([np.where(keep, state[0], -np.inf), sims], axis=1)
        ids = np.concatenate([state[1], ids], axis=1)
    vals = np.full((n, k), -np.inf, sims.dtype)
    out = np.full((n, k), -1, np.int64)
    for i in range(n):
        order = np.lexsort((ids[i], -sims[i]))[:k]
        order = order[np.isfinite(sims[i][order])]
        vals[i, :order.size] = sims[i][order]
        out[i, :order.size] = ids[i][order]
    return vals, out


def shard_bounds(sizes):
    """[5, 0, 7] -> [(0, 5), (5, 5), (5, 12)]: the row ranges of consecutive shards."""
    edges = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    return [(int(edges[i]), int(edges[i + 1])) for i in range(len(sizes))]


def search_shards(sims, k, bounds, order, id_base=0):
    """The shards `bounds` (row ranges) of sims' columns merged in the given order -> list of states, one after every
    shard.  Ids are id_base + column of the whole database."""
    n = sims.shape[0]
    state, states = None, []
    for s in order:
        lo, hi = bounds[s]
        ids = np.broadcast_to(np.arange(lo, hi, dtype=np.int64) + np.int64(id_base), (n, hi - lo))
        state = merge_exact(state, sims[:, lo:hi], ids, k)
        states.append(state)
    return states


def tie_shares(sims, k):
    """-> (share of queries whose k-th and (k+1)-th values are equal, share of queries with two equal values inside
    their list of k).  0 for the first when there is no (k+1)-th row."""
    top = mr.topk_desc(np.asarray(sims, np.float64), k + 1)
    at_k = float((top[:, k - 1] == top[:, k]).mean()) if sims.shape[1] > k else 0.0
    inside = float((top[:, 1:k] == top[:, :k - 1]).any(axis=1).mean()) if k > 1 else 0.0
    return at_k, inside


# ------------------------------------------------------------------------------------------------ coarse grid
def coarse_search_reference(job):
    """job: dict(n, N, d, storage, common, seed) as margin_ref.coarse_data takes it.  -> dict(S64 [n, N] float64 on the
    stored operands, e = the bound above, e_seq = max|seq - S64|).  Runs in a process that never touches the GPU."""
    q, db = mr.coarse_data(job)
    qs = mr.round_storage(mr.unit_f32(q)[0], job['storage'])
    S64 = qs.astype(np.float64) @ db.astype(np.float64).T
    seq = mr.dots_f32(qs, db)
    e_seq = float(np.abs(seq.astype(np.float64) - S64).max())
    e = max(2 * e_seq, 4 * mr.U * float(np.abs(S64).max()))
    return dict(S64=S64, e=e, e_seq=e_seq)


def unit_f32_lanes(x):
    """x * (1 / sqrtf(sum x^2)) in fp32 with the sum of squares in the order of the search kernels: lane group lg of a
    wave adds the squares of elements 32 s + 8 lg + j (s, then j, ascending) one by one, then (p0 + p1) + (p2 + p3).
    For rows whose squares are exact in fp32 (fp16 / bf16 values) a fused multiply-add changes nothing.  Rows that are
    not on a grid get the kernel's own fp32 normalisation this way, bit for bit; a zero row stays zero."""
    x = np.ascontiguousarray(x, np.float32)
    n, d = x.shape
    assert d % 32 == 0
    sq = (x * x).reshape(n, d // 32, 4, 8)
    assert np.array_equal(sq.astype(np.float64), x.astype(np.float64).reshape(sq.shape) ** 2)
    p = np.zeros((n, 4), np.float32)
    for s in range(d // 32):
        for j in range(8):
            p = p + sq[:, s, :, j]
    ss = (p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])
    with np.errstate(divide="ignore"):
        inv = np.where(ss > 0, np.float32(1) / np.sqrt(ss), np.float32(0)).astype(np.float32)
    return x * inv[:, None]


def rows_search_reference(q, db, storage):
    """coarse_search_reference for given rows: q [n, d] float32 queries (values exact in fp16 or bf16), db [N, d] as stored."""
    qs = mr.round_storage(unit_f32_lanes(q), storage)
    S64 = qs.astype(np.float64) @ db.astype(np.float64).T
    seq = mr.dots_f32(qs, db)
    e_seq = float(np.abs(seq.astype(np.float64) - S64).max())
    return dict(S64=S64, e=max(2 * e_seq, 4 * mr.U * float(np.abs(S64).max())), e_seq=e_seq)


def ambiguous(S64, k, e):
    """-> (ids [n, k] of the float64 reference, mask [n, k]: True where the position's float64 gap to the neighbour above
    or below (rank k + 1 included) is <= 2e)."""
    n, N = S64.shape
    vals, ids = search_exact(S64, min(k + 1, N))
    gap = vals[:, :-1] - vals[:, 1:]                      # gap[j] between ranks j and j + 1
    close = gap <= 2 * e
    amb = np.zeros((n, vals.shape[1]), bool)
    amb[:, :-1] |= close
    amb[:, 1:] |= close
    return ids[:, :k], amb[:, :k]


def ambiguous_share(S64, k, e):
    return float(ambiguous(S64, k, e)[1].mean())
