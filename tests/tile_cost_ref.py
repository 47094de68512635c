"""Value-level check of the wide-band tile sweep (csrc/svx_tiles.hip) against float64; TEST INFRASTRUCTURE (numpy).

The sweep makes its costs on the matrix cores and consumes them on the spot: the level view of a wide search has no
a_b_costs.  It does hold, on every lattice node of the band, the float64 sum a_b_csum, the back-pointer and
new_b_offset, and the reference recurrence is csum[node] = csum[pred] + (double) cost_fp32.  So for a general node
whose back-pointer names type t = (xo, yo)

        c^ = csum[x, y] - csum[x - xo, y - yo]

is the fp32 cost the sweep used for t at that cell, up to one float64 rounding of the sum.  check_view() states two
checks on a set of node tables (the GPU's level view, or the oracle's own tables), both on the tables' OWN sums at the
predecessors, so that no error accumulates along paths.  `cost` [T][A][B] is indexed like the reference's a_b_costs
(dp_ref._candidate: the cost cell of node (a, b) is [t, a - 2, b]):

  1. winner costs      E[t] = max |c^ - cost[t]| over the general nodes with a finite sum whose back-pointer is t;
                       E[t] <= bound[t].
  2. one-step optimum  want = min over all candidates of csum[pred] + step (cost[t] for a type, the tables' del_penalty
                       for the two deletions; the reference's candidate order, first strictly smaller), t* its winner,
                       s the tables' winner:  -bound[s] <= csum - want <= bound[t*], a deletion has bound 0, and the
                       finite pattern is that of want.

The bound is the rule of stage_check.py applied per type plane, nothing fitted to the kernel:

        bound[t] = max(2 E_orc[t], 4 * 2^-24 * max |c64[t]|) + 4 * 2^-52 * max |csum|
        E_orc[t] = max |oracle make_sparse_costs[t] - c64[t]|      over the finite cells of the band

with c64 = stage_ref.band_costs(norm1(v0), norm1(v1), n0, n1, path, b_offset, types, W) (here: costs_from_dots of
band_dots, the same expression; test_tile_costs_cpu.py pins the two to each other bit for bit).  It is per type, not
global, because family T puts the types on different scales on purpose.

Inputs.  On ordinary data most off-path nodes are won by a deletion or a small type, and the planes of the larger
types are never seen.  So every case runs two families through the same check:

  family N  make_pair(..., deletions=8) as it is and with common=1.4, normalisers computed by the pipeline (c64 on the
            float64 normalisers of stage_ref.norms on the oracle's draws);
  family T  one pair per probed type t = (xo, yo) in one call, the same embeddings each, caller-supplied normalisers
            that are constant per layer: n0[xo-1][:] = n1[yo-1][:] = BIG (64 up to 15 types, 1024 above), every other
            layer 1.  Type t becomes cheap and wins often; its bound is on its own scale.

The CPU side of a case (oracle costs for E_orc, float64 dots, the oracle's own DP tables and the checks on them) runs
in a spawn pool of processes that never touch the GPU (RefFarm)."""
import multiprocessing
import os

import numpy as np

import dp_ref
import stage_ref
from fuzz_gpu_vs_oracle import store_round
from synth import alignment_types, make_pair

U32, U64 = 2.0 ** -24, 2.0 ** -52
FRAC, SAMPLE, NSAMP = 0.2, 20000, 100
MIN_WINS = 100          # a probed type must win at this many general nodes (min_wins: less on small lattices)
MIN_TYPES_N = 5         # family N: this many types must do so
COMMON = 1.4
TILE = 32               # csrc/svx_tiles.hip: TL


# ------------------------------------------------------------------------------------------ the two checks
def band_grid(new_b_offset, B, size0, size1, A):
    """Nodes of the band: (a [A+2][1], xx, yy [A+2][B], general-node mask) as dp_ref._diagonal has them."""
    bout = np.asarray(new_b_offset, np.int64)
    a = np.arange(A + 2, dtype=np.int64)[:, None]
    yy = bout[:, None] + np.arange(B, dtype=np.int64)[None, :]
    xx = a - yy
    bx = (xx == 0) & (0 <= yy) & (yy <= size1)
    by = ~bx & (yy == 0) & (0 <= xx) & (xx <= size0)
    gen = ~bx & ~by & (1 <= xx) & (xx <= size0) & (1 <= yy) & (yy <= size1) & (a >= 2) & (a - 2 < A)
    return a, xx, yy, gen


def check_view(view, cost, types, bound, label, worst_cells=3):
    """The two checks of the module docstring on one set of node tables.
    view: a_b_csum [A+2][B] f64, a_b_xp, a_b_yp, new_b_offset, del_penalty, size0, size1 (a level view or the oracle's
    tables); cost [T][A][B] float64, inf outside the documents; bound [T] WITHOUT the float64 term, which is added
    here from the view's own sums.
    -> (records, fails): one record per type with E, wins, bound, the worst ratio of check 2 charged to that type
    (c2) and the number of nodes over it (c2_over); fails are texts that name the worst cells with their tile."""
    csum = np.asarray(view['a_b_csum'], np.float64)
    xp, yp = np.asarray(view['a_b_xp'], np.int64), np.asarray(view['a_b_yp'], np.int64)
    bout = np.asarray(view['new_b_offset'], np.int64)
    size0, size1, pen = int(view['size0']), int(view['size1']), float(view['del_penalty'])
    T, A, B = cost.shape
    assert csum.shape == (A + 2, B) and len(types) == T
    mv = [(int(x), int(y)) for x, y in types] + [(0, 1), (1, 0)]
    a, xx, yy, gen = band_grid(bout, B, size0, size1, A)
    fin = gen & np.isfinite(csum)
    f64term = 4 * U64 * float(np.abs(csum[fin]).max()) if fin.any() else 0.0
    bnd = np.concatenate([np.asarray(bound, np.float64) + f64term, [0.0, 0.0]])
    fails = []
    # the tables' winner s per node
    code = {m: k for k, m in enumerate(mv)}
    s = np.full(csum.shape, -1, np.int64)
    for m, k in code.items():
        s[(xp == m[0]) & (yp == m[1])] = k
    if (fin & (s < 0)).any():
        fails.append("%s: %d finite general nodes whose back-pointer is no move of the set" % (label, int((fin & (s < 0)).sum())))
    step_rows = np.full((A + 2, B), np.inf)
    best = np.full(csum.shape, np.inf)
    tstar = np.full(csum.shape, -1, np.int64)
    E, wins = np.zeros(T), np.zeros(T + 2, np.int64)
    where = [None] * T
    for t, (xo, yo) in enumerate(mv):
        ap = a - xo - yo
        apc = np.clip(ap, 0, A + 1)
        xpv, ypv = xx - xo, yy - yo
        bpv = ypv - bout[apc]
        ok = gen & (ap >= 0) & (0 <= xpv) & (xpv <= size0) & (0 <= ypv) & (ypv <= size1) & (0 <= bpv) & (bpv < B)
        prev = csum[apc, np.clip(bpv, 0, B - 1)]
        if t < T:
            step_rows[2:] = cost[t]
            step = step_rows
        else:
            step = pen
        with np.errstate(invalid="ignore"):
            tot = np.where(ok, prev + step, np.inf)
        tot = np.where(np.isnan(tot), np.inf, tot)
        take = tot < best
        best = np.where(take, tot, best)
        tstar[take] = t
        mine = fin & (s == t)
        wins[t] = int(mine.sum())
        if (mine & ~ok).any():
            fails.append("%s: move %s wins at %d nodes whose predecessor is outside the band or the lattice" % (label, mv[t], int((mine & ~ok).sum())))
            mine &= ok
        if t < T and mine.any():
            with np.errstate(invalid="ignore"):
                err = np.where(mine, np.abs((csum - prev) - step_rows), 0.0)
            err = np.where(np.isnan(err), np.inf, err)
            E[t] = float(err.max())
            where[t] = np.argsort(err, axis=None)[::-1][:worst_cells]
    want_fin = gen & np.isfinite(best)
    if not np.array_equal(fin, want_fin):
        bad = np.argwhere(fin != want_fin)
        fails.append("%s: finite pattern differs from the one-step optimum's at %d general nodes, first node (x, y) = (%d, %d)"
                     % (label, len(bad), xx[tuple(bad[0])], yy[tuple(bad[0])]))
    both = fin & want_fin & (s >= 0)
    d = np.where(both, csum - np.where(both, best, 0.0), 0.0)
    hi, lo = bnd[np.clip(tstar, 0, T + 1)], bnd[np.clip(s, 0, T + 1)]
    over_hi, over_lo = both & (d > hi), both & (-d > lo)
    records = []
    for t in range(T + 2):
        up, dn = both & (tstar == t) & (d > 0), both & (s == t) & (d < 0)
        top = max(float(d[up].max()) if up.any() else 0.0, float((-d[dn]).max()) if dn.any() else 0.0)
        n_over = int((over_hi & (tstar == t)).sum() + (over_lo & (s == t)).sum())
        rec = dict(type=list(mv[t]), wins=int(wins[t]), c2=top, c2_over=n_over)
        if t < T:
            rec.update(E=float(E[t]), bound=float(bnd[t]))
            if not E[t] <= bnd[t]:
                fails.append("%s type %s: winner costs off by %.3e > bound %.3e at %d nodes; worst %s"
                             % (label, mv[t], E[t], bnd[t], wins[t], describe_cells(where[t], xx, yy, csum.shape)))
        if n_over:
            cells = np.argsort(np.where((over_hi & (tstar == t)) | (over_lo & (s == t)), np.abs(d), 0.0), axis=None)[::-1][:worst_cells]
            fails.append("%s move %s: one-step optimum missed by %.3e (bound %.3e) at %d nodes; worst %s"
                         % (label, mv[t], top, bnd[t], n_over, describe_cells(cells, xx, yy, csum.shape)))
        records.append(rec)
    return records, fails


def describe_cells(flat, xx, yy, shape):
    """Nodes as '(x, y) tile (I, J) + (i, j)': the cost cell of node (x, y) is (x - 1, y - 1), tiles are TILE nodes a side."""
    out = []
    for f in np.asarray(flat).tolist():
        r, c = np.unravel_index(f, shape)
        x, y = int(xx[r, c]), int(yy[r, c])
        out.append("(%d, %d) tile (%d, %d) + (%d, %d)" % (x, y, x // TILE, y // TILE, x % TILE, y % TILE))
    return "; ".join(out)


def bounds(E_orc, cmax):
    """bound[t] without the float64 term: max(2 E_orc[t], 4 * 2^-24 * max |c64[t]|)."""
    return np.maximum(2.0 * np.asarray(E_orc, np.float64), 4 * U32 * np.asarray(cmax, np.float64))


# ------------------------------------------------------------------------------------------ float64 costs
def band_dots(v0n, v1n, searchpath, b_offset, types, W):
    """<v0n[xo-1][xx], v1n[yo-1][yy]> on the band cells in float64 -> ([T][A][B] dots, nan outside the documents,
    xx, yy [A][B]).  Cells and summation as stage_ref.band_costs."""
    path = np.asarray(searchpath, np.int64).reshape(-1, 2)
    boff = np.asarray(b_offset, np.int64)
    A, B = path.shape[0], 2 * int(W)
    aa = path[:, 0] + path[:, 1]
    assert np.array_equal(aa, np.arange(A))
    yy = boff[aa][:, None] + np.arange(B)[None, :]
    xx = aa[:, None] - yy
    ok = (xx >= 0) & (xx < v0n.shape[1]) & (yy >= 0) & (yy < v1n.shape[1])
    xv, yv = xx[ok], yy[ok]
    out = np.full((len(types), A, B), np.nan)
    for t, (xo, yo) in enumerate(types):
        out[t][ok] = np.einsum("id,id->i", v0n[xo - 1][xv], v1n[yo - 1][yv])
    return out, xx, yy


def costs_from_dots(dots, xx, yy, n0, n1, types):
    """stage_ref.band_costs' expression on stored dots: 2 xo yo (1 - dot) / ((1e-6 + n0[xo-1][xx]) + n1[yo-1][yy])."""
    n0, n1 = np.asarray(n0, np.float64), np.asarray(n1, np.float64)
    ok = ~np.isnan(dots[0])
    xv, yv = xx[ok], yy[ok]
    out = np.full(dots.shape, np.inf)
    for t, (xo, yo) in enumerate(types):
        out[t][ok] = (2.0 * xo * yo) * (1.0 - dots[t][ok]) / ((1e-6 + n0[xo - 1][xv]) + n1[yo - 1][yv])
    return out


# ------------------------------------------------------------------------------------------ probes
def probe_norms(t, K0, K1, n, m, big):
    """Family T: constant per layer, BIG on the two layers type t reads, 1 elsewhere -> (n0 [K0][n], n1 [K1][m]) float32."""
    n0, n1 = np.ones((K0, n), np.float32), np.ones((K1, m), np.float32)
    n0[t[0] - 1, :] = big
    n1[t[1] - 1, :] = big
    return n0, n1


def big_of(types):
    return 64.0 if len(types) <= 15 else 1024.0


def probed_types(types, limit=45, at_least=40):
    """Indices of the types family T probes: all of them up to `limit`; above, a fixed subset of >= at_least that holds
    the first and the last type and, for every overlap layer of either side, the first and the last type of the list
    that use it (two per layer wherever two exist), filled up with evenly spaced ones."""
    T = len(types)
    if T <= limit:
        return list(range(T))
    pick = {0, T - 1}
    for side in (0, 1):
        for layer in sorted({ty[side] for ty in types}):
            users = [k for k, ty in enumerate(types) if ty[side] == layer]
            pick.update((users[0], users[-1]))
    k = 0
    spaced = [int(round(i * (T - 1) / (at_least - 1))) for i in range(at_least)]
    while len(pick) < at_least:
        pick.add(spaced[k])
        k += 1
    return sorted(pick)


# ------------------------------------------------------------------------------------------ cases
def _prior5(n, m):
    """Five uneven blocks whose covering width is above 32: the band bends four times."""
    xs = np.cumsum([0, 40, 50, 10, 20, n - 120])
    ys = np.cumsum([0, 37, 45, 25, 10, m - 117])
    return [(list(range(xs[i], xs[i + 1])), list(range(ys[i], ys[i + 1]))) for i in range(5)]


def _case(name, types, sizes, W, store, d, seed, search="straight", probes=None, shape=None):
    return dict(name=name, types=[tuple(t) for t in types], sizes=list(sizes), W=W, store=store, d=d, seed=seed, search=search,
                probes=probes, shape=shape)


# name: (types, sizes, W, seed, the kernel the dispatcher picks)      (svx_tiles.hip: svxl_band_tiles_batch)
_A_SETS = {
    "a5": (alignment_types(5), [(150, 137)], 40, 1, "k_band_tiles<E, 8, 5, 5>"),
    "a6": (alignment_types(6), [(150, 137)], 33, 2, "k_band_tiles<E, 12, 8, 2>"),
    "ms2_custom": ([(1, 1), (1, 2), (2, 1), (9, 1), (1, 9), (3, 3), (2, 9)], [(150, 137)], 40, 3, "k_band_tiles_gen<E, 2, false>"),
    "a7": (alignment_types(7), [(150, 137)], 40, 4, "k_band_tiles_gen<E, 3, false>"),
    "a8": (alignment_types(8), [(150, 137)], 36, 5, "k_band_tiles_gen<E, 4, false>"),
    "a10": (alignment_types(10), [(150, 137)], 48, 6, "k_band_tiles_gen<E, 6, false>"),
    "a12_dense": (alignment_types(12), [(150, 140)], 151, 7, "k_band_tiles_gen<E, 9, false>"),
    "a16_dense": (alignment_types(16), [(120, 118)], 121, 8, "k_band_tiles_gen<E, 17, false>"),
    "m2o20": (None, [(160, 120)], 60, 9, "k_band_tiles_gen<E, 3, false>"),       # int32 back-pointers
    "bigh_100": ([(1, 1), (100, 1), (1, 100), (1, 2), (2, 1)], [(330, 320)], 120, 10, "k_band_tiles_gen<E, 17, true>"),
}
STORES = ("f32", "f16", "bf16")
ELEM = {"f32": "ElemF32", "f16": "ElemF16", "bf16": "ElemBF16"}
B_DIMS = (8, 40, 1016, 1024, 1032, 2048)


def _types_of(name):
    ty = _A_SETS[name][0]
    return dp_ref.many_to_one_types(20) if ty is None else ty


def _cases():
    out = {}
    for name, (_, sizes, W, seed, kern) in _A_SETS.items():
        for st in STORES:
            out["A_%s_%s" % (name, st)] = _case("A_%s_%s" % (name, st), _types_of(name), sizes, W, st, 72, 100 + seed, shape=kern.replace("E,", ELEM[st] + ","))
    for a, kern in ((5, "k_band_tiles<E, 8, 5, 5>"), (7, "k_band_tiles_gen<E, 3, false>")):
        for d in B_DIMS:
            for st in STORES:
                nm = "B_a%d_d%d_%s" % (a, d, st)
                out[nm] = _case(nm, alignment_types(a), [(100, 97)], 40, st, d, 200 + a, shape=kern.replace("E,", ELEM[st] + ","))
    k5 = "k_band_tiles<ElemBF16, 8, 5, 5>"
    t5 = alignment_types(5)
    out["C_20x25_W33"] = _case("C_20x25_W33", t5, [(20, 25)], 33, "bf16", 72, 301, shape=k5)            # smaller than one tile, dense
    out["C_40x300_W45"] = _case("C_40x300_W45", t5, [(40, 300)], 45, "bf16", 72, 302, shape=k5)         # a steep path
    out["C_150x137_W151"] = _case("C_150x137_W151", t5, [(150, 137)], 151, "bf16", 72, 303, shape=k5)   # dense
    out["C_257x250_W33"] = _case("C_257x250_W33", t5, [(257, 250)], 33, "bf16", 72, 304, shape=k5)      # one past a tile multiple
    out["C_batch3"] = _case("C_batch3", t5, [(150, 137), (128, 160), (160, 120)], 40, "bf16", 72, 305, shape=k5)
    out["C_around_wide"] = _case("C_around_wide", t5, [(150, 137)], None, "bf16", 72, 306, search="around_wide", shape=k5)
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return _CASES


def injection_cases():
    """The cases whose family T the injected faults run on; -a 9 (36 types) is CPU-only, no GPU case."""
    c = cases()
    return [c["A_a5_f32"], _case("A_a9_f32", alignment_types(9), [(150, 137)], 40, "f32", 72, 120), c["C_257x250_W33"]]


def case_prior(case, n, m):
    return _prior5(n, m) if case['search'] == "around_wide" else None


def case_width(case):
    if case['W'] is not None:
        return case['W']
    from svx.vecalign.dp_utils import prior_width
    n, m = case['sizes'][0]
    return prior_width(_prior5(n, m), n, m)


def case_pairs(case):
    """-> {'N': [pair, ...], 'T': [pair, ...]}: one dict per pair of the two calls of a case.  Family N: every size as
    iid and as aniso data; family T: one pair per probed type on the iid data, the sizes in turn."""
    types = case['types']
    K0, K1 = max(x for x, _ in types), max(y for _, y in types)
    fam_n, fam_t = [], []
    for i, (n, m) in enumerate(case['sizes']):
        for kind in ("iid", "aniso"):
            fam_n.append(dict(n=n, m=m, K0=K0, K1=K1, kind=kind, data=(i, kind), seed=1000 * case['seed'] + 10 * i + (kind == "aniso"),
                              probe=None))
    probes = case['probes'] if case['probes'] is not None else probed_types(types)
    for k, t in enumerate(probes):
        i = k % len(case['sizes'])
        n, m = case['sizes'][i]
        fam_t.append(dict(n=n, m=m, K0=K0, K1=K1, kind="iid", data=(i, "iid"), seed=1000 * case['seed'] + 100 + k, probe=int(t)))
    return dict(N=fam_n, T=fam_t)


def embeddings(case, size_index, kind):
    """The storage-rounded float32 embeddings of one size of a case."""
    types = case['types']
    K0, K1 = max(x for x, _ in types), max(y for _, y in types)
    n, m = case['sizes'][size_index]
    v0, v1 = make_pair(n, m, max(K0, K1), case['d'], 7000 + 10 * case['seed'] + size_index, deletions=8,
                       common=COMMON if kind == "aniso" else 0.0)
    return (store_round(np.ascontiguousarray(v0[:K0]), case['store']), store_round(np.ascontiguousarray(v1[:K1]), case['store']))


def pair_norms(case, pair):
    """Family T: the probe normalisers; family N: None (computed by the pipeline)."""
    if pair['probe'] is None:
        return None
    return probe_norms(case['types'][pair['probe']], pair['K0'], pair['K1'], pair['n'], pair['m'], big_of(case['types']))


# ------------------------------------------------------------------------------------------ the CPU side
def oracle_pair(orc, case, pair, v0, v1, W, inject=None):
    """The oracle's straight / around search of one pair as dp_ref.straight_stack / around_ref.around_stack run it
    (same draws from RandomState(seed)).  inject(f) may change the costs before the DP.
    -> dict(f [T][A][B] f32, path, b_offset, n0, n1 (the oracle's fp32), view: the tables of its DP as a level view)"""
    n, m = pair['n'], pair['m']
    a, b = v0.copy(), v1.copy()
    orc.make_norm1(a)
    orc.make_norm1(b)
    rs = np.random.RandomState(pair['seed'])
    norms = pair_norms(case, pair)
    if norms is None:
        n0, n1 = orc.compute_norms(a, b, NSAMP, rs), orc.compute_norms(b, a, NSAMP, rs)
    else:
        n0, n1 = norms
    pen, _ = orc.make_del_penalty(a[0], b[0], n0[0], n1[0], SAMPLE, FRAC, rs)
    prior = case_prior(case, n, m)
    path = orc.search_path(prior if prior is not None else [(list(range(n)), list(range(m)))], False, n, m)
    f, bo = orc.make_sparse_costs(a, b, n0, n1, path, case['types'], W)
    if inject is not None:
        f = inject(f)
    csum, xp, yp, bout = orc.sparse_dp(f, bo, case['types'], pen, n, m)
    return dict(f=f, path=np.asarray(path, np.int64).reshape(-1, 2), b_offset=np.asarray(bo, np.int32), n0=n0, n1=n1,
                view=dict(a_b_csum=csum, a_b_xp=xp, a_b_yp=yp, new_b_offset=bout, del_penalty=float(pen), size0=n, size1=m))


def f64_norms(orc, case, pair, v0n, v1n):
    """The normalisers c64 is evaluated on: the probe's (family T), or stage_ref.norms on the oracle's draws."""
    norms = pair_norms(case, pair)
    if norms is not None:
        return norms[0].astype(np.float64), norms[1].astype(np.float64)
    dr = stage_ref.replay_draws(orc, pair['seed'], pair['n'], pair['m'], pair['K0'], pair['K1'], 1 << 30, SAMPLE, NSAMP)[0]
    return stage_ref.norms(v0n, v1n, dr['idx0']), stage_ref.norms(v1n, v0n, dr['idx1'])


def case_reference(name, self_check=True, case=None, keep_data=True):
    """The CPU side of one case -> dict(W, data={(size index, kind): dict(dots, xx, yy, path, b_offset)},
    N=[per pair], T=[per pair]); per pair: n0, n1 (float64, what c64 is evaluated on), E_orc [T], cmax [T], and with
    self_check the records and failures of check_view on the oracle's own tables: against c64 under the bound
    ('orc_records', 'orc_fails'), against the oracle's own fp32 costs under the float64 term alone ('own_fails'), and
    the input conditions on the oracle's back-pointers ('cond_fails').  keep_data=False drops the float64 dots."""
    import oracle as orc
    case = cases()[name] if case is None else case
    W = case_width(case)
    types = case['types']
    out = dict(W=W, data={}, N=[], T=[])
    emb = {}
    for fam, pairs in case_pairs(case).items():
        for pair in pairs:
            key = pair['data']
            if key not in emb:
                emb[key] = embeddings(case, *key)
            v0, v1 = emb[key]
            o = oracle_pair(orc, case, pair, v0, v1, W)
            if key not in out['data']:
                v0n, v1n = stage_ref.norm1(v0), stage_ref.norm1(v1)
                dots, xx, yy = band_dots(v0n, v1n, o['path'], o['b_offset'], types, W)
                out['data'][key] = dict(dots=dots, xx=xx, yy=yy, path=o['path'], b_offset=o['b_offset'], v0n=v0n, v1n=v1n)
            dat = out['data'][key]
            assert np.array_equal(dat['path'], o['path']) and np.array_equal(dat['b_offset'], o['b_offset'])
            n0, n1 = f64_norms(orc, case, pair, dat['v0n'], dat['v1n'])
            c64 = costs_from_dots(dat['dots'], dat['xx'], dat['yy'], n0, n1, types)
            rec = dict(n0=n0, n1=n1, probe=pair['probe'], **pair_errors(o['f'], c64))
            if self_check:
                lab = "%s %s pair %d (oracle)" % (name, fam, len(out[fam]))
                rec['orc_records'], rec['orc_fails'] = check_view(o['view'], c64, types, bounds(rec['E_orc'], rec['cmax']), lab)
                _, rec['own_fails'] = check_view(o['view'], o['f'].astype(np.float64), types, np.zeros(len(types)), lab + " own costs")
                rec['cond_fails'] = win_count_fails(rec['orc_records'], pair, types, lab)
            out[fam].append(rec)
    for dat in out['data'].values():
        del dat['v0n'], dat['v1n']
    if not keep_data:
        out['data'] = {}
    return out


def pair_errors(f, c64):
    """E_orc[t] and max |c64[t]| over the finite cells of the band; the infinite patterns must agree."""
    fin = np.isfinite(c64)
    assert np.array_equal(np.isfinite(f), fin), "the oracle's costs and c64 differ in their infinite cells"
    T = c64.shape[0]
    E, cmax = np.zeros(T), np.zeros(T)
    for t in range(T):
        if fin[t].any():
            E[t] = float(np.abs(f[t][fin[t]].astype(np.float64) - c64[t][fin[t]]).max())
            cmax[t] = float(np.abs(c64[t][fin[t]]).max())
    return dict(E_orc=E, cmax=cmax)


# ------------------------------------------------------------------------------------------ injected errors
INJECTIONS = ("relative_2^-18", "neighbour_layer", "rows_shifted")


def injected(name_or_case, kind):
    """The oracle with one fault put into the target plane of every family-T pair of a case before its DP:
      relative_2^-18   the plane times (1 + 2^-18);
      neighbour_layer  the plane made from the neighbouring overlap layer of the source side (layer xo, or xo - 2 for
                       the last one), normalisers and factor as before;
      rows_shifted     32 rows of the plane in the middle of the band moved by one cell.
    -> [(type, flagged by check 1, flagged by check 2)] per probed type, the bound being the clean oracle's."""
    import oracle as orc
    case = cases()[name_or_case] if isinstance(name_or_case, str) else name_or_case
    W, types = case_width(case), case['types']
    K0 = max(x for x, _ in types)
    out, emb, dat = [], {}, {}
    for pair in case_pairs(case)['T']:
        key = pair['data']
        if key not in emb:
            emb[key] = embeddings(case, *key)
        v0, v1 = emb[key]
        t = pair['probe']
        xo, yo = types[t]
        clean = oracle_pair(orc, case, pair, v0, v1, W)
        if key not in dat:
            v0n, v1n = stage_ref.norm1(v0), stage_ref.norm1(v1)
            dat[key] = band_dots(v0n, v1n, clean['path'], clean['b_offset'], types, W) + (v0n, v1n)
        dots, xx, yy, v0n, v1n = dat[key]
        n0, n1 = f64_norms(orc, case, pair, v0n, v1n)
        c64 = costs_from_dots(dots, xx, yy, n0, n1, types)
        err = pair_errors(clean['f'], c64)

        def inject(f):
            f = f.copy()
            if kind == "relative_2^-18":
                f[t] = (f[t].astype(np.float64) * (1 + 2.0 ** -18)).astype(np.float32)
            elif kind == "neighbour_layer":
                other = xo if xo < K0 else xo - 2
                wrong = v0n.copy()
                wrong[xo - 1] = v0n[other]
                d2, _, _ = band_dots(wrong, v1n, clean['path'], clean['b_offset'], [(xo, yo)], W)
                f[t] = costs_from_dots(d2, xx, yy, n0, n1, [(xo, yo)])[0].astype(np.float32)
            else:
                r0 = f.shape[1] // 2 - 16
                f[t, r0:r0 + 32, 1:] = f[t, r0:r0 + 32, :-1].copy()
            return f
        bad = oracle_pair(orc, case, pair, v0, v1, W, inject=inject)
        recs, _ = check_view(bad['view'], c64, types, bounds(err['E_orc'], err['cmax']), "injected")
        r = recs[t]
        out.append((types[t], bool(r['E'] > r['bound']), any(x['c2_over'] for x in recs)))
    return out


# ------------------------------------------------------------------------------------------ the pool
class RefFarm:
    """case_reference() of many cases in processes that never touch the GPU (spawn), at most 16 of them, a few cases
    ahead of the consumer (the results are large)."""

    def __init__(self, names, ahead=6, self_check=False, keep_data=True):
        self.pool = multiprocessing.get_context("spawn").Pool(max(1, min(16, (os.cpu_count() or 2) - 1)))
        self.names, self.ahead, self.args, self.pending = list(names), ahead, (self_check, None, keep_data), {}

    def _submit(self, name):
        if name not in self.pending:
            self.pending[name] = self.pool.apply_async(case_reference, (name,) + self.args)

    def get(self, name):
        self._submit(name)
        if name in self.names:
            at = self.names.index(name)
            for nxt in self.names[at + 1:at + 1 + self.ahead]:
                self._submit(nxt)
        return self.pending.pop(name).get()

    def close(self):
        self.pool.terminate()
        self.pool.join()


# ------------------------------------------------------------------------------------------ the GPU side
def run_gpu(case, fam):
    """One PreparedBatch call over the pairs of one family of a case -> (PreparedBatch, [level view per pair])."""
    import torch
    from svx.vecalign import dp_utils
    pairs = case_pairs(case)[fam]
    cast = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[case['store']]
    dev = {}
    for p in pairs:
        if p['data'] not in dev:
            v0, v1 = embeddings(case, *p['data'])
            dev[p['data']] = (torch.from_numpy(v0).cuda().to(cast), torch.from_numpy(v1).cuda().to(cast))
    norms = [pair_norms(case, p) for p in pairs]
    kw = {}
    if case['search'] == "around_wide":
        kw['priors'] = [case_prior(case, p['n'], p['m']) for p in pairs]
    pb = dp_utils.PreparedBatch([dev[p['data']] for p in pairs], case['types'], FRAC, case_width(case), 0, SAMPLE, NSAMP,
                                rngs=[np.random.RandomState(p['seed']) for p in pairs],
                                norms=None if fam == "N" else norms, search=case['search'], **kw)
    pb.run()
    pb.results()
    return pb, [pb.level_stack(i, 0) for i in range(len(pairs))]


def check_case_gpu(case, ref, records=None):
    """Both families of a case on the GPU against the case's CPU reference -> list of failure texts."""
    types = case['types']
    fails = []
    for fam in ("N", "T"):
        _, views = run_gpu(case, fam)
        for i, (pair, view, r) in enumerate(zip(case_pairs(case)[fam], views, ref[fam])):
            lab = "%s %s pair %d (%d x %d%s)" % (case['name'], fam, i, pair['n'], pair['m'],
                                                 "" if pair['probe'] is None else ", probe %s" % (types[pair['probe']],))
            dat = ref['data'][pair['data']]
            if 'a_b_costs' in view:
                fails.append("%s: the level view has a_b_costs: not the tile sweep" % lab)
            if not np.array_equal(np.asarray(view['searchpath'], np.int64).reshape(-1, 2), dat['path']) or \
                    not np.array_equal(view['b_offset'], dat['b_offset']):
                fails.append("%s: search path or b_offset differ from the oracle's" % lab)
                continue
            c64 = costs_from_dots(dat['dots'], dat['xx'], dat['yy'], r['n0'], r['n1'], types)
            recs, bad = check_view(view, c64, types, bounds(r['E_orc'], r['cmax']), lab)
            fails += bad
            fails += win_count_fails(recs, pair, types, lab)
            if records is not None:
                for t, rec in enumerate(recs[:len(types)]):
                    if pair['probe'] is None or pair['probe'] == t:
                        records.append(dict(case=case['name'], family=fam, kind=pair['kind'], pair=i, type=rec['type'], wins=rec['wins'],
                                            E_gpu=rec['E'], E_orc=float(r['E_orc'][t]), bound=rec['bound'], c2=rec['c2'], c2_over=rec['c2_over']))
    return fails


def min_wins(n, m):
    """How many general nodes a type must win at for a pair n x m to count as having shown its plane: MIN_WINS = 100
    from 120 a side, the sizes at which that figure was measured on the oracle.  A type's wins lie along the alignment
    path, about one per path position wherever the data favour it, so documents with a shorter side s cannot be asked
    for more than about s of them, whatever the seed (100 x 97 at d >= 1016: 93 .. 99 for the fifth type of family N
    over eight seeds).  Below 120 the figure is 0.8 s, and s / 2 below s = 40, where the lattice of 20 x 25 has 500
    general nodes for ten types.  Taken from the oracle's tables and the sizes, never from the GPU's counts."""
    s = min(n, m)
    return MIN_WINS if s >= 120 else (int(0.8 * s) if s >= 40 else s // 2)


def win_count_fails(recs, pair, types, label):
    """Family T: the probed type wins at >= min_wins general nodes; family N: >= MIN_TYPES_N types do."""
    T, need = len(types), min_wins(pair['n'], pair['m'])
    if pair['probe'] is not None:
        w = recs[pair['probe']]['wins']
        return [] if w >= need else ["%s: the probed type wins at %d general nodes, fewer than %d" % (label, w, need)]
    often = sum(1 for r in recs[:T] if r['wins'] >= need)
    return [] if often >= MIN_TYPES_N else ["%s: %d types win at >= %d general nodes, fewer than %d" % (label, often, need, MIN_TYPES_N)]
