"""Inputs and references for the margin-scoring kernels (csrc/svx_margin.hip): k_knn_mean, k_unit_rows, k_margin_scores.
Shared by test_margin_ref_cpu.py (the properties the GPU checks rest on, no GPU) and test_gpu_margin_matrix.py;
TEST INFRASTRUCTURE.

Two input families.

LATTICE (exact arithmetic).  A query has exactly 4^m non-zero elements (4^m the largest power of 4 <= d), each +-s with
s a power of two per row; database rows are integers in [-8, 8] divided by 64 and are handed to the index as they are
(FlatIndex.add_unit_rows).  Then the fp32 sum of squares 4^m s^2 and 1 / sqrtf of it are exact, the normalised query
(+-2^-m) is exact in fp16 and bf16, every product and every partial sum of a similarity is an integer multiple of
2^-(m+6) below 2^14 of them -- exact in fp32 in any order -- and so is the sum of up to 64 kept values.  The kept lists
of the GPU must therefore equal the true k largest similarities bit for bit (both sides sorted) and the mean must equal
float32(sum) / float32(k) bit for bit.  Half of a query's non-zero coordinates are a block shared by all queries, positive
in every query; the database value on the block grows with the row index of the `rising` order, so the similarities
trend upward there (every tile replaces most of every list), downward in `falling`; `shuffled` is a permutation of the
same rows, `repeated` is `shuffled` with its best row copied to k + 5 places.  Integer similarities tie often, also at
the k-th place.

COARSE GRID (real-valued, no knife-edge rounding).  Query elements are m * 2^-6 with integer |m| <= 31 (a clipped
rounded Gaussian, optionally with a common component): squares and their sum are exact in fp32 in any order, so with
correctly rounded sqrtf and division the normalised, storage-rounded query of the GPU equals numpy's bit for bit.
Database rows are ordinary random unit rows rounded to storage.  References: a float64 chain (stored operands,
float64 products, exact top-k, float64 mean) and a sequential-fp32 restatement (one fp32 accumulate per element, kept
values summed one by one in fp32); the kept lists and the means are judged by stage_check's rule
E_gpu <= max(2 E_orc, 4 * 2^-24 max|f64|)."""
import numpy as np

from oracle import normalize_l2, round_storage

U = 2.0 ** -24
ORDERS = ("shuffled", "rising", "falling", "repeated")
STORAGES = ("fp16", "bf16")
QTYPES = ("f32", "f16", "bf16")


def unit_f32(x):
    """The kernels' normalisation in numpy's fp32 (the oracle's normalize_l2: x * (1 / sqrt(sum x^2)), a zero row stays
    zero).  -> (x * inv, sum x^2).  float32 sqrt and division are correctly rounded in numpy as in the kernels, and the
    sum of squares is exact for both input families, whatever its order."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return normalize_l2(x), np.einsum("ij,ij->i", x, x, dtype=np.float32)


def topk_desc(sims, k):
    """The k largest entries of every row, descending; rows with fewer than k entries are padded with -inf."""
    n, N = sims.shape
    if N > 4 * k:
        sims = np.partition(sims, N - k, axis=1)[:, N - k:]
    out = -np.sort(-sims, axis=1)[:, :k]
    if out.shape[1] < k:
        out = np.concatenate([out, np.full((n, k - out.shape[1]), -np.inf, out.dtype)], axis=1)
    return out


def dots_f32(q, db, reverse=False):
    """<q_i, db_j> with one fp32 multiply and one fp32 add per element, elements in index order (or reversed)."""
    q, db = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(db, np.float32)
    qt, dbt = np.ascontiguousarray(q.T), np.ascontiguousarray(db.T)
    acc = np.zeros((q.shape[0], db.shape[0]), np.float32)
    tmp = np.empty_like(acc)
    order = range(q.shape[1] - 1, -1, -1) if reverse else range(q.shape[1])
    for e in order:
        np.multiply(qt[e][:, None], dbt[e][None, :], out=tmp)
        np.add(acc, tmp, out=acc)
    return acc


# ------------------------------------------------------------------------------------------------ lattice
def pow4_floor(d):
    p = 1
    while p * 4 <= d:
        p *= 4
    return p


def lattice(n, N, d, k, seed, order="shuffled"):
    """-> (queries [n, d], database [N, d]) float32, every value exact in fp16 and bf16.  The three orders `shuffled`,
    `rising`, `falling` of one (n, N, d, seed) hold the same rows; `repeated` needs N >= k + 6."""
    assert order in ORDERS, order
    rs = np.random.RandomState(seed)
    nz = pow4_floor(d)
    B = nz // 2
    perm = rs.permutation(d)
    block, rest = perm[:B], perm[B:]
    pick = np.argsort(rs.rand(n, rest.size), axis=1)[:, :nz - B]      # nz - B further coordinates per query
    s = (np.float32(2.0) ** rs.randint(-3, 4, size=n)).astype(np.float32)
    q = np.zeros((n, d), np.float32)
    q[:, block] = s[:, None]
    q[np.arange(n)[:, None], rest[pick]] = s[:, None] * rs.choice(np.float32([-1, 1]), size=pick.shape)
    # noise of a few units on the other coordinates (its sum over a query has a spread of 5 .. 10 units, so equal
    # similarities are common); the block sum T of row j of the rising order climbs one unit per row where [-8, 8] allows
    A = int(np.clip(np.rint(np.sqrt(100.0 / (nz - B))), 1, 8))
    ints = rs.randint(-A, A + 1, size=(N, d)).astype(np.float32)
    Tmax = min(8 * B, N // 2)
    T = np.rint(np.linspace(-Tmax, Tmax, N))
    base = np.floor(T / B)
    blk = base[:, None] + (np.arange(B)[None, :] < (T - base * B)[:, None])
    # + c on one block coordinate, - c on its neighbour: cancels in every query, spreads the values over [-8, 8]
    room = 8 - np.abs(blk).max(axis=1)
    c = np.floor(rs.rand(N, B // 2) * (room[:, None] + 1))
    blk[:, 0:2 * (B // 2):2] += c
    blk[:, 1:2 * (B // 2):2] -= c
    ints[:, block] = blk
    assert np.abs(ints).max() <= 8
    db = ints / np.float32(64)
    ro = np.random.RandomState([seed, 1])
    shuffle = ro.permutation(N)
    if order == "falling":
        db = db[::-1]
    elif order in ("shuffled", "repeated"):
        db = db[shuffle]
    if order == "repeated":
        assert N >= k + 6, "repeated order: N = %d too small for k = %d" % (N, k)
        best = int(np.nonzero(shuffle == N - 1)[0][0])
        others = np.setdiff1d(np.arange(N), [best])
        db = db.copy()
        db[ro.choice(others, size=k + 5 - 1, replace=False)] = db[best]
    return q, np.ascontiguousarray(db)


def lattice_sims(q, db):
    """Exact similarities (float64; every value is exact in fp32 as well)."""
    q64 = q.astype(np.float64)
    qn = q64 / np.sqrt((q64 * q64).sum(axis=1))[:, None]
    return qn @ db.astype(np.float64).T


def lattice_ref(q, db, k):
    """-> (kept lists [n, k] float32 descending, -inf where the database has fewer than k rows; mean [n] float32)"""
    top = topk_desc(lattice_sims(q, db), k)
    lists = top.astype(np.float32)
    assert np.array_equal(lists.astype(np.float64), top)
    tot = top.sum(axis=1)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(tot.astype(np.float32).astype(np.float64), tot)
    return lists, (tot.astype(np.float32) / np.float32(k)).astype(np.float32)


def kth_tie_share(q, db, k):
    """Share of queries whose k-th and (k+1)-th largest similarities are equal (0 when N == k)."""
    if db.shape[0] <= k:
        return 0.0
    top = topk_desc(lattice_sims(q, db), k + 1)
    return float((top[:, k - 1] == top[:, k]).mean())


# ------------------------------------------------------------------------------------------------ coarse grid
def _common_dir(d, useed):
    u = np.random.default_rng([int(useed), 0xC0FFEE]).standard_normal(d)
    return u / np.sqrt((u * u).sum())


def coarse_rows(n, d, seed, common=0.0, useed=0, sigma=10.0):
    """[n, d] float32 rows m * 2^-6, integer |m| <= 31.  common: as synth.make_pair(common=), every row gets
    common * |row| * u added before the rounding, u = the unit direction of `useed`."""
    g = np.random.default_rng(seed).standard_normal((n, d))
    if common:
        g = g + common * np.sqrt((g * g).sum(axis=1, keepdims=True)) * _common_dir(d, useed)
    return (np.clip(np.rint(g * sigma), -31, 31) / 64.0).astype(np.float32)


def coarse_db(N, d, seed, storage, common=0.0, useed=0):
    """[N, d] float32: random unit rows rounded to `storage` (handed over with add_unit_rows)."""
    g = np.random.default_rng(seed).standard_normal((N, d))
    if common:
        g = g + common * np.sqrt((g * g).sum(axis=1, keepdims=True)) * _common_dir(d, useed)
    g /= np.sqrt((g * g).sum(axis=1, keepdims=True))
    return round_storage(g.astype(np.float32), storage)


KTOP = 65   # kept per row by coarse_reference: k <= 64 and the (k+1)-th neighbour


def coarse_data(job):
    q = coarse_rows(job['n'], job['d'], job['seed'], job['common'], job['seed'])
    db = coarse_db(job['N'], job['d'], job['seed'] + 1, job['storage'], job['common'], job['seed'])
    return q, db


def coarse_reference(job):
    """job: dict(n, N, d, storage, common, seed).  -> dict(f64 = the 65 largest float64 similarities per query,
    descending; seq = the same of the sequential-fp32 restatement).  Runs in a process that never touches the GPU."""
    q, db = coarse_data(job)
    assert db.shape[0] >= KTOP
    qs = round_storage(unit_f32(q)[0], job['storage'])
    f64 = topk_desc(qs.astype(np.float64) @ db.astype(np.float64).T, KTOP)
    seq = topk_desc(dots_f32(qs, db), KTOP)
    return dict(f64=f64, seq=seq)


def coarse_k(ref, k):
    """-> (lists64 [n, k], mean64 [n], seq lists [n, k] float32, seq mean [n] float32) for one k of a coarse_reference."""
    l64 = ref['f64'][:, :k]
    ls = np.ascontiguousarray(ref['seq'][:, :k], np.float32)
    tot = np.zeros(ls.shape[0], np.float32)
    for j in range(k):
        tot = tot + ls[:, j]
    return l64, l64.sum(axis=1) / k, ls, (tot / np.float32(k)).astype(np.float32)


def rule(gpu, orc, f64):
    """stage_check's rule.  -> (E_gpu, E_orc, bound)"""
    from stage_check import stage_error
    e_gpu, e_orc, bound, _ = stage_error(gpu, orc, f64)
    return e_gpu, e_orc, bound


def wrong_pick_share(ref, k, bound):
    """Share of queries for which taking the (k+1)-th neighbour for the k-th moves the mean by less than `bound`."""
    return float(((ref['f64'][:, k - 1] - ref['f64'][:, k]) / k < bound).mean())


# ------------------------------------------------------------------------------------------------ helper kernels
def unit_rows_ref(x, storage):
    """k_unit_rows: round_storage(x * inv), bit for bit on coarse-grid rows."""
    return round_storage(unit_f32(x)[0], storage)


def margin_f64(x, y, mxy, myx, margin):
    """-> (score, a, b) in float64 from the fp32 inputs: a = <x/|x|, y/|y|>, b = (mxy + myx) / 2 (zero rows: a = 0)."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    sxx, syy, sxy = (x * x).sum(axis=1), (y * y).sum(axis=1), (x * y).sum(axis=1)
    a = sxy / np.sqrt(np.where(sxx > 0, sxx, 1.0)) / np.sqrt(np.where(syy > 0, syy, 1.0))
    b = (mxy.astype(np.float64) + myx.astype(np.float64)) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return (a / b if margin == "ratio" else a - b), a, b


def margin_f32(x, y, mxy, myx, margin):
    """numpy's own fp32 result of the reference's formula (score_align.py:151-160), inf / nan included."""
    xn, yn = unit_f32(x)[0], unit_f32(y)[0]
    a = np.einsum("ij,ij->i", xn, yn, dtype=np.float32)
    b = (mxy.astype(np.float32) + myx.astype(np.float32)) / np.float32(2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (a / b if margin == "ratio" else a - b).astype(np.float32)
