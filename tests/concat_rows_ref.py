"""svx_concat_rows (include/svx.h) restated in numpy / plain Python, and the synthetic descriptor batches its tests run on.
Shared by test_concat_rows_cpu.py (no GPU) and test_gpu_concat_rows.py; TEST INFRASTRUCTURE.

A batch is a list of pairs, each a dict like align_rows_ref's (v0, v1, align, scores, info) plus f0 [n, 2] and f1 [m, 2] int32
(start, end) sample positions.  Pairs are monotone alignment lists like a DP's output (with the planted exceptions below);
candidate values are margin_ref.coarse_rows data, exact in all three dtypes, so every output is compared bit for bit.

Parameters are a dict: max_score, max_num_align, sample_rate, max_sil, max_dur, both_sides, min_frames."""
import numpy as np

from align_rows_ref import DTYPES, FILL, MAX_SCORE, bits, storage_bits, store, to_f32   # noqa: F401  (re-exported)
from margin_ref import coarse_rows, unit_rows_ref

RATE = 16000
PARAMS = dict(max_score=MAX_SCORE, max_num_align=3, sample_rate=RATE, max_sil=1.0, max_dur=20.0, both_sides=1, min_frames=RATE)
D_MAX = int(PARAMS["max_dur"] * RATE)    # 320000 samples: a span of exactly this joins
G_MAX = int(PARAMS["max_sil"] * RATE)    # 16000 samples: a gap of exactly this joins


def params(**kw):
    return dict(PARAMS, **kw)


# ------------------------------------------------------------------------------------------------ the contract
def base_rows(pair, max_score):
    """Row numbers of one pair that are base rows, ascending (no width limit)."""
    n, m = pair["v0"].shape[1], pair["v1"].shape[1]
    n_align, status = int(pair["info"][0]), int(pair["info"][1])
    if status != 0:
        return []
    out = []
    for r in range(max(0, min(n_align, n + m + 2))):
        xs, xl, ys, yl = (int(v) for v in pair["align"][r])
        if xl < 1 or yl < 1 or xs < 0 or ys < 0 or xs + xl > n or ys + yl > m:
            continue
        if not (float(pair["scores"][r]) <= float(max_score)):   # NaN fails
            continue
        out.append(r)
    return out


def walk(pair, prm):
    """-> (outputs, events).  outputs: (c_i, c_ie, e + 1, x_start, x_len, y_start, y_len) of every (i, e) the joining rule
    emits, in (i, e) order, before the duration filter.  events: (c_i, e, what, slack) per join attempted, what in "joined",
    "dur_src", "dur_tgt", "disconnected", "sil", "end" (no next base row in the pair), "max" (max_num_align reached while the
    next row would have been connected); slack = (samples under max_dur on the source, samples under max_sil at the tighter
    gap) for what the checks got to see."""
    a = pair["align"].astype(np.int64)
    F0, F1 = pair.get("f0"), pair.get("f1")
    rate, both = prm["sample_rate"], prm["both_sides"]
    c = base_rows(pair, prm["max_score"])
    outs, events = [], []
    for i, f in enumerate(c):
        xs, ys = int(a[f, 0]), int(a[f, 2])
        outs.append((f, f, 1, xs, int(a[f, 1]), ys, int(a[f, 3])))
        for e in range(1, prm["max_num_align"] + 1):
            if i + e >= len(c):
                events.append((f, e, "end", None))
                break
            nx, l = c[i + e], c[i + e - 1]
            connected = a[nx, 0] == a[l, 0] + a[l, 1] and a[nx, 2] == a[l, 2] + a[l, 3]
            if e == prm["max_num_align"]:
                if connected:
                    events.append((f, e, "max", None))
                break
            dx = int(F0[a[nx, 0] + a[nx, 1] - 1, 1]) - int(F0[xs, 0])
            dy = int(F1[a[nx, 2] + a[nx, 3] - 1, 1]) - int(F1[ys, 0])
            if dx / rate > prm["max_dur"]:
                events.append((f, e, "dur_src", (D_MAX - dx, None)))
                break
            if both and dy / rate > prm["max_dur"]:
                events.append((f, e, "dur_tgt", (D_MAX - dx, None)))
                break
            if not connected:
                events.append((f, e, "disconnected", None))
                break
            gx = int(F0[a[nx, 0], 0]) - int(F0[a[l, 0] + a[l, 1] - 1, 1])
            gy = int(F1[a[nx, 2], 0]) - int(F1[a[l, 2] + a[l, 3] - 1, 1])
            if gx / rate > prm["max_sil"] or gy / rate > prm["max_sil"]:
                events.append((f, e, "sil", (D_MAX - dx, G_MAX - max(gx, gy))))
                break
            events.append((f, e, "joined", (D_MAX - dx, G_MAX - max(gx, gy), D_MAX - dy)))
            outs.append((f, nx, e + 1, xs, int(a[nx, 0] + a[nx, 1]) - xs, ys, int(a[nx, 2] + a[nx, 3]) - ys))
    return outs, events


def durations(pair, o):
    """Span of output `o` in samples on the two sides."""
    F0, F1 = pair["f0"], pair["f1"]
    return int(F0[o[3] + o[4] - 1, 1]) - int(F0[o[3], 0]), int(F1[o[5] + o[6] - 1, 1]) - int(F1[o[5], 0])


def chain_outputs(pair, prm):
    """-> [(output, fits)] of one pair after the duration filter, in (i, e) order: the lines of the reference's files."""
    k0, k1 = pair["v0"].shape[0], pair["v1"].shape[0]
    out = []
    for o in walk(pair, prm)[0]:
        if prm["min_frames"] > 0:
            dx, dy = durations(pair, o)
            if not (prm["min_frames"] <= dx and prm["min_frames"] <= dy):
                continue
        out.append((o, o[4] <= k0 and o[6] <= k1))
    return out


def pair_outputs(pair, prm):
    """-> (fitting outputs, wide outputs) of one pair."""
    outs = chain_outputs(pair, prm)
    return [o for o, fits in outs if fits], [o for o, fits in outs if not fits]


def reference(batch, prm, storage=None):
    """-> dict(count, wide, meta [count, 8] int32, x_rows / y_rows [count, d] bit patterns, x_unit / y_unit [count, d] uint16 bit
    patterns or None): fitting outputs numbered in (pair, i, e) order."""
    dtype, d = batch["dtype"], batch["d"]
    meta, xr, yr, wide = [], [], [], 0
    for p, pair in enumerate(batch["pairs"]):
        fit, w = pair_outputs(pair, prm)
        wide += len(w)
        for o in fit:
            meta.append((p,) + o)
            xr.append(pair["v0"][o[4] - 1, o[3] + o[4] - 1])
            yr.append(pair["v1"][o[6] - 1, o[5] + o[6] - 1])
    empty = np.zeros((0, d), batch["pairs"][0]["v0"].dtype if batch["pairs"] else np.float32)
    x = np.stack(xr) if xr else empty
    y = np.stack(yr) if yr else empty
    out = dict(count=len(meta), wide=wide, meta=np.asarray(meta, np.int32).reshape(-1, 8), x_rows=bits(x), y_rows=bits(y), x_unit=None, y_unit=None)
    if storage is not None:
        out["x_unit"] = storage_bits(unit_rows_ref(to_f32(x, dtype), storage), storage) if len(meta) else np.zeros((0, d), np.uint16)
        out["y_unit"] = storage_bits(unit_rows_ref(to_f32(y, dtype), storage), storage) if len(meta) else np.zeros((0, d), np.uint16)
    return out


def as_lists(pair):
    """The pair as the text tools see it: ([(src ids, tgt ids, cost)] of the rows info[0] announces, src frames, tgt frames)."""
    R = int(pair["info"][0])
    rows = [(list(range(r[0], r[0] + r[1])), list(range(r[2], r[2] + r[3])), float(s)) for r, s in zip(pair["align"][:R].tolist(), pair["scores"][:R])]
    return rows, [tuple(v) for v in pair["f0"].tolist()], [tuple(v) for v in pair["f1"].tolist()]


# ------------------------------------------------------------------------------------------------ generator
TYPES = [(1, 1)] * 12 + [(2, 1), (1, 2), (1, 0), (0, 1)]   # mostly 1-1, so runs form; deletions in between break them


def frames_for(rs, n):
    """n segments of 0.3 .. 4 s; most gaps are below half a second, one in seven is 1 .. 2 s (over max_sil)."""
    dur = rs.randint(int(0.3 * RATE), 4 * RATE, size=n)
    gap = np.where(rs.rand(n) < 1 / 7, rs.randint(RATE + 1, 2 * RATE, size=n), rs.randint(0, RATE // 2, size=n))
    start = np.cumsum(gap + np.concatenate([[0], dur[:-1]]))
    return np.stack([start, start + dur], axis=1).astype(np.int32)


def monotone_rows(rs, R, x0=0, y0=0):
    """R alignment rows that walk the lattice from (x0, y0) like a DP's output -> (rows, n, m)."""
    rows, x, y = [], x0, y0
    for _ in range(R):
        xl, yl = TYPES[rs.randint(len(TYPES))]
        rows.append((x, xl, y, yl))
        x, y = x + xl, y + yl
    return np.asarray(rows, np.int32).reshape(-1, 4), x, y


def finish_pair(seed, i, d, dtype, k0, k1, n, m, rows, scores, info, f0, f1, zero_rows=2):
    """Candidate tensors and padded arrays for one pair whose first rows are `rows`."""
    rs = np.random.RandomState([seed, i, 7])
    cap = n + m + 2
    assert len(rows) <= cap, (len(rows), cap)
    v0 = coarse_rows(k0 * n, d, [seed, i, 0]).reshape(k0, n, d)
    v1 = coarse_rows(k1 * m, d, [seed, i, 1]).reshape(k1, m, d)
    for v in (v0, v1):
        for _ in range(zero_rows if v.shape[1] else 0):
            v[rs.randint(v.shape[0]), rs.randint(v.shape[1])] = 0.0
    align = np.zeros((cap, 4), np.int32)
    align[:len(rows)] = rows
    align[len(rows):] = (0, 1, 0, 1)               # what lies behind info[0] would be a base row: it must not be read as one
    sc = np.zeros(cap)
    sc[:len(rows)] = scores
    return dict(v0=store(v0, dtype), v1=store(v1, dtype), align=align, scores=sc, info=np.asarray(info, np.int32), f0=f0, f1=f1)


def random_pair(seed, i, R, d, dtype, k0, k1, kind="rows", start=(0, 0)):
    rs = np.random.RandomState([seed, i, 3])
    lead = []
    if start != (0, 0):   # deletions up to `start`, so that the first base row begins where the pair before ended
        lead = [(x, 1, 0, 0) for x in range(start[0])] + [(start[0], 0, y, 1) for y in range(start[1])]
    rows, n, m = monotone_rows(rs, R, *start)
    rows = np.concatenate([np.asarray(lead, np.int32).reshape(-1, 4), rows])
    n, m = max(n, 6), max(m, 6 + i % 3)
    scores = np.where(rs.rand(len(rows)) < 0.12, MAX_SCORE * 1.5, rs.uniform(0.0, MAX_SCORE, size=len(rows)))   # over-threshold rows
    info = [len(rows), 0]
    if kind == "all_del":
        side = rs.rand(len(rows)) < 0.5
        rows[side, 1], rows[~side, 3] = 0, 0
    elif kind == "zero_info":
        info = [0, 0]
    elif kind == "failed":
        info = [n + m + 2, 4]                        # SVX_ERR_TRACEBACK
        rows[:, 0], rows[:, 2] = 1 << 30, -(1 << 30)
        rows[::2, 1] = 1 << 30
        scores[:] = 0.0
    pair = finish_pair(seed, i, d, dtype, k0, k1, n, m, rows, scores, info, frames_for(rs, n), frames_for(rs, m))
    if kind == "failed":
        pair["align"][:] = pair["align"][0] if len(rows) else (1 << 30, 1 << 30, -(1 << 30), 1)
    return pair


def gap_pair(seed, i, d, dtype, k0, k1, hole=300):
    """Two connected base rows with `hole` rows in between that are no base rows (x_len = y_len = 0), then a normal tail."""
    rs = np.random.RandomState([seed, i, 4])
    tail, n, m = monotone_rows(rs, 20, 2, 2)
    rows = np.concatenate([[(0, 1, 0, 1)], np.tile([(1, 0, 1, 0)], (hole, 1)), [(1, 1, 1, 1)], tail]).astype(np.int32)
    n = m = max(n, m, (len(rows) + 1) // 2)
    f = np.stack([np.arange(n) * (2 * RATE), np.arange(n) * (2 * RATE) + RATE + RATE // 2], axis=1).astype(np.int32)   # 1.5 s, 0.5 s gaps
    return finish_pair(seed, i, d, dtype, k0, k1, n, m, rows, rs.uniform(0, MAX_SCORE, size=len(rows)), [len(rows), 0], f, f.copy())


def equality_pair(seed, i, d, dtype, k0, k1):
    """1-1 rows over hand-made frames, groups far apart (3 s) so that only the rows of a group can join:
      A  span exactly max_dur on both sides (joins)           B  one sample more on the source (does not)
      C  gap exactly max_sil (joins)                          D  one sample more (does not)
      E  alone, exactly min_frames long on both sides (kept)  F  alone, one sample less on the source (dropped)
      H  source inside max_dur, target one sample over: joins only with both_sides = 0
      K  three short 1-1 rows: 3 x 3 at e = 2;  (2-1)(1-1)(1-1): 4 x 3 at e = 2, one wider than k0 = 3."""
    far = 3 * RATE
    s, t, rows = [], [], []
    at = [0, 0]          # running sample position per side
    def seg(side, dur, gap):
        lst = (s, t)[side]
        start = at[side] + gap
        lst.append((start, start + dur))
        at[side] = start + dur
    def both(dur, gap):
        seg(0, dur, gap), seg(1, dur, gap)
    def one_to_one():
        rows.append((len(s) - 1, 1, len(t) - 1, 1))
    # A
    both(100000, far); one_to_one(); both(D_MAX - 100000 - 1000, 1000); one_to_one()
    # B
    both(100000, far); one_to_one(); seg(0, D_MAX - 100000 - 1000 + 1, 1000); seg(1, D_MAX - 100000 - 1000, 1000); one_to_one()
    # C
    both(2 * RATE, far); one_to_one(); both(2 * RATE, G_MAX); one_to_one()
    # D
    both(2 * RATE, far); one_to_one(); seg(0, 2 * RATE, G_MAX + 1); seg(1, 2 * RATE, G_MAX); one_to_one()
    # E, F
    both(RATE, far); one_to_one()
    seg(0, RATE - 1, far); seg(1, RATE, far); one_to_one()
    # H
    both(100000, far); one_to_one(); seg(0, D_MAX - 100000 - 1000, 1000); seg(1, D_MAX - 100000 - 1000 + 1, 1000); one_to_one()
    # K: three 1-1 rows, then (2-1)(1-1)(1-1)
    both(2 * RATE, far); one_to_one()
    for _ in range(2):
        both(2 * RATE, 100); one_to_one()
    seg(0, 2 * RATE, far); seg(0, 2 * RATE, 100); seg(1, 4 * RATE + 100, far)
    rows.append((len(s) - 2, 2, len(t) - 1, 1))
    for _ in range(2):
        both(2 * RATE, 100); one_to_one()
    n, m = len(s), len(t)
    rows = np.asarray(rows, np.int32)
    f0, f1 = np.asarray(s, np.int32), np.asarray(t, np.int32)
    return finish_pair(seed, i, d, dtype, k0, k1, n, m, rows, np.full(len(rows), MAX_SCORE / 2), [len(rows), 0], f0, f1)


def make_batch(spec, d, dtype, seed, k0=3, k1=3):
    """spec entries: ("rows", R) a random monotone pair of R rows; ("after", R) the same behind deletions that place its first base row where
    the pair before ended (numerically connected across the pair edge); "gap", "equal" the planted pairs above; "all_del",
    "zero_info", "failed" pairs that have no base rows."""
    pairs = []
    for i, kind in enumerate(spec):
        if kind == "gap":
            pairs.append(gap_pair(seed, i, d, dtype, k0, k1))
        elif kind == "equal":
            pairs.append(equality_pair(seed, i, d, dtype, k0, k1))
        elif isinstance(kind, tuple) and kind[0] == "after":
            prev = pairs[-1]
            last = prev["align"][base_rows(prev, MAX_SCORE)[-1]]
            pairs.append(random_pair(seed, i, kind[1], d, dtype, k0, k1, start=(int(last[0] + last[1]), int(last[2] + last[3]))))
        elif isinstance(kind, tuple):
            pairs.append(random_pair(seed, i, kind[1], d, dtype, k0, k1))
        else:
            pairs.append(random_pair(seed, i, 10, d, dtype, k0, k1, kind=kind))
    return dict(pairs=pairs, d=d, dtype=dtype, spec=spec, k=(k0, k1))


def classes(batch, prm):
    """How often each planted situation occurs in `batch` under `prm` (the CPU test asserts that none is zero)."""
    c = dict.fromkeys(("joined", "deletion_between", "over_threshold", "chunk_edge", "far_apart", "pair_edge", "longer_than_max",
                       "dur_exact", "dur_one_more", "sil_exact", "sil_one_more", "min_exact", "min_one_less", "src_ok_tgt_over",
                       "fits_exactly", "one_wider", "wide", "dropped_by_duration", "no_base_rows", "disconnected"), 0)
    k0, k1 = batch["k"]
    prev_last = None
    for pair in batch["pairs"]:
        base = base_rows(pair, prm["max_score"])
        R = int(pair["info"][0]) if pair["info"][1] == 0 else 0
        a = pair["align"]
        if not base:
            c["no_base_rows"] += 1
            prev_last = None
            continue
        live = (a[:R, 1] >= 1) & (a[:R, 3] >= 1)
        c["over_threshold"] += int((pair["scores"][:R][live] > prm["max_score"]).sum())
        if prev_last is not None and a[base[0], 0] == prev_last[0] and a[base[0], 2] == prev_last[1]:
            c["pair_edge"] += 1
        prev_last = (int(a[base[-1], 0] + a[base[-1], 1]), int(a[base[-1], 2] + a[base[-1], 3]))
        outs, events = walk(pair, prm)
        for f, e, what, slack in events:
            if what == "joined":
                c["joined"] += 1
                c["dur_exact"] += slack[0] == 0
                c["sil_exact"] += slack[1] == 0
            c["longer_than_max"] += what == "max"
            c["disconnected"] += what == "disconnected"
            c["dur_one_more"] += what == "dur_src" and slack[0] == -1
            c["sil_one_more"] += what == "sil" and slack[1] == -1
        c["src_ok_tgt_over"] += sum(1 for f, e, what, slack in walk(pair, dict(prm, both_sides=1))[1] if what == "dur_tgt")
        for o in outs:
            if o[2] > 1:
                c["chunk_edge"] += o[0] // 256 != o[1] // 256
                c["far_apart"] += o[1] - o[0] > 256
                c["deletion_between"] += o[1] - o[0] >= o[2]
                c["fits_exactly"] += o[4] == k0 and o[6] == k1
                c["one_wider"] += (o[4] == k0 + 1 and o[6] <= k1) or (o[6] == k1 + 1 and o[4] <= k0)
            dx, dy = durations(pair, o)
            c["min_exact"] += min(dx, dy) == prm["min_frames"]
            c["min_one_less"] += min(dx, dy) == prm["min_frames"] - 1
            c["dropped_by_duration"] += prm["min_frames"] > 0 and min(dx, dy) < prm["min_frames"]
        c["wide"] += len(pair_outputs(pair, prm)[1])
    return {k: int(v) for k, v in c.items()}


# every batch the GPU tests run: name -> (spec, d, dtype, k0, k1)
START_MIDDLE_END = [("all_del", "zero_info", "failed"), ("zero_info", "failed", "all_del"), ("failed", "all_del", "zero_info")]


def edge_spec(rotation=0):
    """Pairs of 0, 1, 255, 256, 257, 513 and 1100 rows, the planted pairs, a pair numerically connected to the one before it,
    and a pair without base rows at the start, in the middle and at the end."""
    a, b, c = START_MIDDLE_END[rotation]
    return [a, ("rows", 255), ("rows", 1), ("rows", 0), "equal", ("after", 40), b, ("rows", 256), ("rows", 257), "gap", ("rows", 513),
            ("rows", 1100), c]


def cases():
    out = {}
    for d in (32, 96, 1024):
        for dt in DTYPES:
            out["edges-d%d-%s" % (d, dt)] = (edge_spec(0), d, dt, 3, 3)
    for d in (8, 2048):
        for dt in DTYPES:
            out["raw-d%d-%s" % (d, dt)] = (edge_spec(0), d, dt, 3, 3)
    for rot in (1, 2):
        out["rotation%d" % rot] = (edge_spec(rot), 32, "f16", 4, 2)
    out["one-pair"] = ([("rows", 300)], 32, "f32", 3, 2)
    out["tiny-pairs"] = ([("rows", 14 if i % 5 else 9) for i in range(1500)], 32, "bf16", 3, 2)
    out["no-rows"] = (["all_del", "zero_info", "failed", ("rows", 0)], 32, "f16", 3, 3)
    return out


def build(name):
    spec, d, dt, k0, k1 = cases()[name]
    seed = sorted(cases()).index(name) + 300
    return make_batch(spec, d, dt, seed, k0=k0, k1=k1)
