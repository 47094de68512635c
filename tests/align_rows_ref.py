"""svx_alignment_rows (include/svx.h) restated in numpy, and the synthetic descriptor batches its tests run on.
Shared by test_align_rows_cpu.py (no GPU) and test_gpu_align_rows.py; TEST INFRASTRUCTURE.

A batch is a list of pairs, each a dict: v0 [k0, n, d], v1 [k1, m, d] (stored arrays, see DTYPES), align [n + m + 2, 4]
int32 rows (x_start, x_len, y_start, y_len), scores [n + m + 2] float64, info [2] int32.  Nothing here runs the aligner:
the rows are drawn at random, one by one, because the entry point judges every row on its own.

Candidate values are margin_ref.coarse_rows data (m * 2^-6, |m| <= 31): exact in float32, float16 and bfloat16, and
unit_rows_ref is bit-exact on them, so every output is compared bit for bit."""
import numpy as np

from margin_ref import coarse_rows, unit_rows_ref

DTYPES = ("f32", "f16", "bf16")   # stored as float32 / float16 / uint16 (bfloat16 bit patterns)
FILL = 0xA5                        # byte pattern of untouched output memory


# ------------------------------------------------------------------------------------------------ storage
def store(a32, dtype):
    """float32 values that are exact in `dtype` -> the stored array."""
    a32 = np.ascontiguousarray(a32, np.float32)
    if dtype == "f32":
        return a32
    if dtype == "f16":
        out = a32.astype(np.float16)
        assert np.array_equal(out.astype(np.float32), a32)
        return out
    assert dtype == "bf16", dtype
    u = a32.view(np.uint32)
    assert not (u & 0xFFFF).any()
    return (u >> 16).astype(np.uint16)


def to_f32(a, dtype):
    if dtype == "bf16":
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a.astype(np.float32)


def bits(a):
    """Any stored array -> its bit patterns (uint16 / uint32)."""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def storage_bits(a32, storage):
    """float32 values already rounded to `storage` (fp16 | bf16) -> uint16 bit patterns."""
    if storage == "fp16":
        return a32.astype(np.float16).view(np.uint16)
    return (np.ascontiguousarray(a32, np.float32).view(np.uint32) >> 16).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ the contract
def kept_rows(pair, max_score):
    """Row numbers of one pair that the keep rule of include/svx.h keeps, ascending."""
    k0, n = pair["v0"].shape[:2]
    k1, m = pair["v1"].shape[:2]
    n_align, status = int(pair["info"][0]), int(pair["info"][1])
    if status != 0:
        return np.zeros(0, np.int64)
    r = np.arange(max(0, min(n_align, n + m + 2)))
    a = pair["align"][:len(r)].astype(np.int64)
    xs, xl, ys, yl = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    ok = (xl >= 1) & (xl <= k0) & (yl >= 1) & (yl <= k1) & (xs >= 0) & (xs + xl <= n) & (ys >= 0) & (ys + yl <= m)
    with np.errstate(invalid="ignore"):
        ok &= pair["scores"][:len(r)] <= np.float64(max_score)   # NaN fails
    return r[ok]


def reference(batch, max_score, storage=None):
    """-> dict(count, src [count, 2] int32, x_rows / y_rows [count, d] bit patterns, x_unit / y_unit [count, d] uint16 bit
    patterns or None): kept rows numbered in (pair ascending, row ascending) order."""
    dtype = batch["dtype"]
    src, xr, yr = [], [], []
    for p, pair in enumerate(batch["pairs"]):
        for r in kept_rows(pair, max_score):
            xs, xl, ys, yl = (int(v) for v in pair["align"][r])
            src.append((p, int(r)))
            xr.append(pair["v0"][xl - 1, xs + xl - 1])
            yr.append(pair["v1"][yl - 1, ys + yl - 1])
    d = batch["d"]
    empty = np.zeros((0, d), batch["pairs"][0]["v0"].dtype)
    x = np.stack(xr) if xr else empty
    y = np.stack(yr) if yr else empty
    out = dict(count=len(src), src=np.asarray(src, np.int32).reshape(-1, 2), x_rows=bits(x), y_rows=bits(y), x_unit=None, y_unit=None)
    if storage is not None:
        out["x_unit"] = storage_bits(unit_rows_ref(to_f32(x, dtype), storage), storage) if len(src) else np.zeros((0, d), np.uint16)
        out["y_unit"] = storage_bits(unit_rows_ref(to_f32(y, dtype), storage), storage) if len(src) else np.zeros((0, d), np.uint16)
    return out


# ------------------------------------------------------------------------------------------------ generator
# pair kinds: ("rows", R[, n, m]) a pair whose info[0] = R drawn rows; "all_del" ten deletions; "zero_info" info[0] = 0 over rows that
# would be kept; "failed" info[1] != 0 over out-of-range garbage
START_MIDDLE_END = [("all_del", "zero_info", "failed"), ("zero_info", "failed", "all_del"), ("failed", "all_del", "zero_info")]


def chunk_edge_spec(rotation=0):
    """Rows per pair 0, 1, 255, 256, 257, 513 (the chunk edge and the carry), with a pair that keeps nothing at the start,
    in the middle and at the end."""
    a, b, c = START_MIDDLE_END[rotation]
    return [a, ("rows", 255), ("rows", 1), ("rows", 0), b, ("rows", 256), ("rows", 257), ("rows", 513), c]


def make_batch(spec, d, dtype, seed, max_score, k0=3, k1=2, zero_rows=3):
    """Descriptors and candidate tensors for `spec`.  About half of the non-deletion rows score above `max_score`; five of
    them carry the scores max_score, the next double above it, NaN, +inf and -0.0; the largest pair holds the edge rows
    x_len = k0 with y_len = k1 at x_start = 0, and x_start + x_len = n."""
    rs = np.random.RandomState(seed)
    pairs = []
    for i, kind in enumerate(spec):
        R = kind[1] if isinstance(kind, tuple) else 10
        if isinstance(kind, tuple) and len(kind) == 4:
            n, m = kind[2:]
        else:
            n = max(6, (R + 1) // 2)
            m = n + (i % 3)                              # ragged
        cap = n + m + 2
        assert R <= cap
        v0 = coarse_rows(k0 * n, d, [seed, i, 0]).reshape(k0, n, d)
        v1 = coarse_rows(k1 * m, d, [seed, i, 1]).reshape(k1, m, d)
        for v in (v0, v1):
            for _ in range(zero_rows):
                v[rs.randint(v.shape[0]), rs.randint(v.shape[1])] = 0.0
        align = np.zeros((cap, 4), np.int32)
        scores = rs.uniform(0.0, 2.0 * max_score if max_score > 0 else 1.0, size=cap)
        xl = rs.randint(1, k0 + 1, size=cap)
        yl = rs.randint(1, k1 + 1, size=cap)
        align[:, 1], align[:, 3] = xl, yl
        align[:, 0] = (rs.rand(cap) * (n - xl + 1)).astype(np.int32)
        align[:, 2] = (rs.rand(cap) * (m - yl + 1)).astype(np.int32)
        info = np.array([R, 0], np.int32)
        if kind == "all_del":
            side = rs.rand(cap) < 0.5
            align[side, 1] = 0
            align[~side, 3] = 0
        elif kind == "zero_info":
            info[0] = 0
        elif kind == "failed":
            info[:] = (cap, 4)                           # SVX_ERR_TRACEBACK
            align[:, 0], align[:, 2] = 1 << 30, -(1 << 30)
            align[::2, 1] = 1 << 30
            scores[:] = 0.0
        else:
            what = rs.rand(cap)
            align[what < 0.15, 1] = 0                    # deletions
            align[(what >= 0.15) & (what < 0.25), 3] = 0
            align[(what >= 0.25) & (what < 0.28), 1] = k0 + 1          # wider than a candidate
            bad = (what >= 0.28) & (what < 0.31)                       # off the end / before the start
            align[bad, 0] = np.where(rs.rand(int(bad.sum())) < 0.5, n - align[bad, 1] + 1, -1)
        pairs.append(dict(v0=store(v0, dtype), v1=store(v1, dtype), align=align, scores=scores, info=info))
    # ---- edge rows in the largest pair (kept: scores below the threshold)
    big = max((i for i, k in enumerate(spec) if isinstance(k, tuple)), key=lambda i: spec[i][1])
    P = pairs[big]
    n, m = P["v0"].shape[1], P["v1"].shape[1]
    assert spec[big][1] >= 2
    P["align"][0] = (0, k0, 0, k1)
    P["align"][1] = (n - k0, k0, m - 1, 1)
    P["scores"][:2] = (max_score / 2, max_score / 4)
    # ---- the special scores, on rows that every other clause of the rule keeps
    cands = []
    for i, pair in enumerate(pairs):
        if isinstance(spec[i], tuple):
            cands += [(i, int(r)) for r in kept_rows(dict(pair, scores=np.zeros_like(pair["scores"])), 0.0) if not (i == big and r < 2)]
    specials = (max_score, np.nextafter(max_score, np.inf), np.nan, np.inf, -0.0)
    assert len(cands) >= len(specials), "batch too small for the special scores"
    for (i, r), s in zip([cands[j] for j in rs.choice(len(cands), size=len(specials), replace=False)], specials):
        pairs[i]["scores"][r] = s
    return dict(pairs=pairs, d=d, dtype=dtype, spec=spec, max_score=max_score)


def stats(batch):
    """-> (non-deletion rows of the pairs that succeeded, kept rows, rows exactly at the threshold, rows one ulp above)."""
    T = batch["max_score"]
    nondel = kept = at = above = 0
    for pair in batch["pairs"]:
        if pair["info"][1] != 0:
            continue
        R = int(pair["info"][0])
        a, s = pair["align"][:R], pair["scores"][:R]
        live = (a[:, 1] >= 1) & (a[:, 3] >= 1)
        nondel += int(live.sum())
        kept += len(kept_rows(pair, T))
        at += int((s[live] == T).sum())
        above += int((s[live] == np.nextafter(T, np.inf)).sum())
    return nondel, kept, at, above


MAX_SCORE = 0.7000004999999999   # filters.cost_limit(0.7)

# every batch the GPU tests run: name -> (spec, d, dtype, k0, k1)
def cases():
    out = {}
    for d in (32, 96, 1024):
        for dt in DTYPES:
            out["edges-d%d-%s" % (d, dt)] = (chunk_edge_spec(0), d, dt, 3, 2)
    for d in (8, 2048):
        for dt in DTYPES:
            out["raw-d%d-%s" % (d, dt)] = (chunk_edge_spec(0), d, dt, 3, 2)
    for rot in (1, 2):
        out["rotation%d" % rot] = (chunk_edge_spec(rot), 32, "f16", 4, 4)
    out["one-pair"] = ([("rows", 300)], 32, "f32", 3, 2)
    out["tiny-pairs"] = ([("rows", 14 if i % 5 else 9, 6, 6) for i in range(1500)], 32, "bf16", 3, 2)
    return out


def build(name):
    spec, d, dt, k0, k1 = cases()[name]
    seed = sorted(cases()).index(name) + 100
    return make_batch(spec, d, dt, seed, MAX_SCORE, k0=k0, k1=k1)
