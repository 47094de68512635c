"""Tie-breaking reference for the DP kernels; TEST INFRASTRUCTURE (numpy, no GPU).

The reference (dp_core.pyx:79-141 dense_dp, :269-404 sparse_dp) lets the FIRST STRICTLY SMALLER candidate win: the
alignment types in list order, then the (0,1) deletion, then the (1,0) deletion (dense: the 1-1 step, then (0,1), then
(1,0)).  This module restates the two loops with that rule as a switch -- tie="first" is the reference, tie="last" lets
an equal candidate replace the incumbent -- counts how often a node is decided by a tie (tie_stats), and builds the two
input families on which the kernels' costs are THE SAME BITS as the oracle's, so that everything downstream of them can
be compared bit for bit with nothing excused:

  family P  costs fed to the per-op entry points: float32 dyadic numbers k/8 from a small set, a tenth of them +inf,
            dyadic penalty.  Every float64 sum is exact (a multiple of 1/8 far below 2^53) and ties are the norm.
  family Z  whole documents through svx_align_batch: all embeddings zero, depth-0 normalisers supplied by the caller
            from a small dyadic set.  Every dot product is exactly 0 on both sides, so the cost of type (xo, yo) at
            (x, y) is float(2 xo yo / ((1e-6 + n0[xo-1][x]) + n1[yo-1][y])) and a sampled 1-1 score is
            float(2 / float(n0 + n1)); at levels >= 1 the normalisers of zero rows are exactly 1.

The loops run over diagonals and moves in the reference's order and over the cells of one diagonal as numpy vectors:
every move reaches back at least one diagonal, so the cells of a diagonal do not depend on each other and the result is
that of the scalar loop.  Shared by test_dp_ties_cpu.py and test_gpu_dp_ties.py."""
import numpy as np

from synth import alignment_types

INF = np.inf


def _moves(types):
    return [(int(x), int(y)) for x, y in types] + [(0, 1), (1, 0)]


def _diagonal(a, B, bout, x_in, y_in, A):
    """Cells of node diagonal a: (yy, xx, border x == 0, border y == 0, general)."""
    yy = np.arange(B) + int(bout[a])
    xx = a - yy
    bx = (xx == 0) & (0 <= yy) & (yy <= y_in)
    by = ~bx & (yy == 0) & (0 <= xx) & (xx <= x_in)
    gen = ~bx & ~by & (1 <= xx) & (xx <= x_in) & (1 <= yy) & (yy <= y_in) & (0 <= a - 2 < A)
    return yy, xx, bx, by, gen


def _candidate(t, mv, T, a, yy, xx, gen, costs, bout, csum, pen, x_in, y_in, B, Aout):
    """Move t into the general cells of diagonal a -> (allowed, total) or None when the diagonal it comes from does not exist."""
    xo, yo = mv
    ap = a - xo - yo
    if not 0 <= ap < Aout:
        return None
    xpv, ypv = xx - xo, yy - yo
    bpv = ypv - int(bout[ap])
    ok = gen & (0 <= xpv) & (xpv <= x_in) & (0 <= ypv) & (ypv <= y_in) & (0 <= bpv) & (bpv < B)
    prev = csum[ap, np.clip(bpv, 0, B - 1)]
    step = costs[t, a - 2, :].astype(np.float64) if t < T else pen  # band index of the cost cell = b (b_offset_out[a] = b_offset_in[a-2] + 1)
    with np.errstate(invalid="ignore"):
        return ok, prev + step


def sparse_dp(costs, b_offset_in, types, pen, x_in, y_in, tie="first"):
    """dp_core.pyx:269-404 -> (csum [A+2][B] f64, xp, yp [A+2][B] i32, b_offset_out [A+2] i32)."""
    assert tie in ("first", "last")
    costs = np.asarray(costs, np.float32)
    T, A, B = costs.shape
    mv = _moves(types)
    assert T == len(mv) - 2
    pen = float(pen)
    Aout = A + 2
    bout = np.empty(Aout, np.int32)
    bout[:2] = b_offset_in[0]
    bout[2:] = np.asarray(b_offset_in, np.int32) + 1
    csum = np.full((Aout, B), INF, np.float64)
    xp = np.full((Aout, B), -42, np.int32)
    yp = np.full((Aout, B), -42, np.int32)
    for a in range(Aout):
        yy, xx, bx, by, gen = _diagonal(a, B, bout, x_in, y_in, A)
        best = np.full(B, INF)
        wx = np.full(B, -42, np.int32)
        wy = np.full(B, -42, np.int32)
        if gen.any():
            for t in range(T + 2):
                c = _candidate(t, mv[t], T, a, yy, xx, gen, costs, bout, csum, pen, x_in, y_in, B, Aout)
                if c is None:
                    continue
                ok, tot = c
                take = ok & ((tot < best) if tie == "first" else ((tot <= best) & (tot < INF)))
                best = np.where(take, tot, best)
                wx = np.where(take, mv[t][0], wx).astype(np.int32)
                wy = np.where(take, mv[t][1], wy).astype(np.int32)
        best = np.where(bx, pen * yy, np.where(by, pen * xx, best))
        csum[a] = best
        xp[a] = np.where(bx, 0, np.where(by, 1, wx))
        yp[a] = np.where(bx, 1, np.where(by, 0, wy))
    return csum, xp, yp, bout


def tie_stats(costs, b_offset, types, pen, csum, new_b_offset, x_in=None, y_in=None):
    """How the nodes of one level were decided (x_in, y_in: the document sizes, as given to sparse_dp).  Over the
    reachable nodes (finite csum, borders included), the shares of nodes whose minimum is attained by >= 2 candidates
    ('tied') and, among those, by two alignment types ('type_type'), by a type and a deletion ('type_del'), by the two
    deletions ('del_del').  A node with three tied candidates can count for several kinds.  'nodes' is the count."""
    costs = np.asarray(costs, np.float32)
    T, A, B = costs.shape
    mv = _moves(types)
    Aout = A + 2
    bout = np.asarray(new_b_offset, np.int32)
    assert np.array_equal(bout[2:], np.asarray(b_offset, np.int32) + 1)
    if x_in is None or y_in is None:
        raise ValueError("tie_stats needs the document sizes")
    n = dict(nodes=0, tied=0, type_type=0, type_del=0, del_del=0)
    n["nodes"] = int(np.isfinite(csum).sum())
    for a in range(Aout):
        yy, xx, bx, by, gen = _diagonal(a, B, bout, x_in, y_in, A)
        live = gen & np.isfinite(csum[a])
        if not live.any():
            continue
        ntype = np.zeros(B, np.int64)
        d01 = np.zeros(B, bool)
        d10 = np.zeros(B, bool)
        for t in range(T + 2):
            c = _candidate(t, mv[t], T, a, yy, xx, gen, costs, bout, csum, float(pen), x_in, y_in, B, Aout)
            if c is None:
                continue
            ok, tot = c
            hit = live & ok & (tot == csum[a])
            if t < T:
                ntype += hit
            elif t == T:
                d01 = hit
            else:
                d10 = hit
        nd = d01.astype(np.int64) + d10
        n["tied"] += int((ntype + nd >= 2).sum())
        n["type_type"] += int((ntype >= 2).sum())
        n["type_del"] += int(((ntype >= 1) & (nd >= 1)).sum())
        n["del_del"] += int((nd == 2).sum())
    out = {k: (n[k] / n["nodes"] if n["nodes"] else 0.0) for k in ("tied", "type_type", "type_del", "del_del")}
    out["nodes"] = n["nodes"]
    return out


def dense_dp(cost, pen, tie="first"):
    """dp_core.pyx:79-141 -> (csum [s0+1][s1+1] f64, bp i32).  pen is a C float in the reference's signature."""
    assert tie in ("first", "last")
    cost = np.asarray(cost, np.float32)
    s0, s1 = cost.shape
    penf = np.float32(pen)
    pend = float(penf)
    csum = np.empty((s0 + 1, s1 + 1), np.float64)
    bp = np.empty((s0 + 1, s1 + 1), np.int32)
    for c in range(s1 + 1):
        csum[0, c], bp[0, c] = float(np.float32(c) * penf), 1
    for r in range(s0 + 1):
        csum[r, 0], bp[r, 0] = float(np.float32(r) * penf), 2
    csum[0, 0], bp[0, 0] = 0.0, 4
    less = (lambda x, y: x < y) if tie == "first" else (lambda x, y: x <= y)
    for c in range(1, s1 + 1):
        for r in range(1, s0 + 1):
            best, b = csum[r - 1, c - 1] + float(cost[r - 1, c - 1]), 0
            c1 = csum[r, c - 1] + pend
            if less(c1, best):
                best, b = c1, 1
            c2 = csum[r - 1, c] + pend
            if less(c2, best):
                best, b = c2, 2
            csum[r, c], bp[r, c] = best, b
    return csum, bp


def dense_tie_stats(cost, pen, csum):
    """tie_stats for the dense DP: the 1-1 step plays the alignment type."""
    cost = np.asarray(cost, np.float64)
    pend = float(np.float32(pen))
    s0, s1 = cost.shape
    if s0 == 0 or s1 == 0:
        return dict(nodes=0, tied=0.0, type_type=0.0, type_del=0.0, del_del=0.0)
    with np.errstate(invalid="ignore"):
        c0 = csum[:-1, :-1] + cost == csum[1:, 1:]
        c1 = csum[1:, :-1] + pend == csum[1:, 1:]
        c2 = csum[:-1, 1:] + pend == csum[1:, 1:]
    live = np.isfinite(csum[1:, 1:])
    nodes = int(np.isfinite(csum).sum())
    k = c0.astype(int) + c1 + c2
    return dict(nodes=nodes, tied=float((live & (k >= 2)).sum()) / nodes, type_type=0.0,
                type_del=float((live & c0 & (c1 | c2)).sum()) / nodes, del_del=float((live & c1 & c2).sum()) / nodes)


# ------------------------------------------------------------------------------------------ family P
P_N, P_M = 70, 64   # as test_sparse_dp_any_band_offsets_vs_oracle: a run spans several staged chunks


def take_types(T, reverse=False):
    """T alignment types: alignment_types(a) where it has exactly T, else the first T of the next larger set."""
    a = 2
    while len(alignment_types(a)) < T:
        a += 1
    ty = alignment_types(a)[:T]
    return ty[::-1] if reverse else ty


def band_offsets(rs, A, B, jumps):
    """The monotone and the jumping b_offset of test_sparse_dp_any_band_offsets_vs_oracle."""
    steps = rs.randint(0, 2, A)
    if jumps:
        for k in rs.choice(A, 12, replace=False):
            steps[k] = rs.choice([-2, -1, 2, 3])
        steps[40:60] = rs.randint(0, 2, 20)
    return (np.cumsum(steps) - B // 2).astype(np.int32)


def p_costs(rs, shape, L, mode="rand"):
    """float32 k/8, k < L, a tenth +inf; mode 'equal': every cost 0.5; 'zero': every cost 0."""
    if mode == "equal":
        return np.full(shape, 0.5, np.float32)
    if mode == "zero":
        return np.zeros(shape, np.float32)
    f = (rs.randint(0, L, shape) / 8.0).astype(np.float32)
    f[rs.rand(*shape) < 0.1] = np.inf
    return f


# name, types, B, jumping offsets, L, penalty, cost mode.
# svx_dp.hip picks the fast kernel's instantiation from (T, B):
#   dpf_groups: G = 4 if B <= 16 else 2 if B <= 32 else 1, halved while T < G
#   dpf_tpl:    t = ceil(T / G); TPLT = t if t <= 4 else 6 if t <= 6 else 0 (generic loop)
# so B = 14 with T = 4, 6, 10, 15, 21, 28 gives G = 4 with TPLT = 1, 2, 3, 4, 6, 0; B = 24 with T = 2, 3, 6, 8, 10, 15 gives
# G = 2; B = 40 with T = 1, 2, 3, 4, 6, 10 gives G = 1.  B > 64 leaves the fast kernel: k_sparse_dp<true> while the csum
# ring + tables fit 150 KB of LDS, k_sparse_dp<false> above (B = 2000, steps of 9: ten diagonals of 2000 doubles).
def dpf_groups(T, B):
    G = 4 if B <= 16 else (2 if B <= 32 else 1)
    while G > 1 and T < G:
        G >>= 1
    return G


def dpf_tpl(T, B):
    t = max(1, -(-T // dpf_groups(T, B)))
    return t if t <= 4 else (6 if t <= 6 else 0)


def _p_sparse_cases():
    out = []
    k = 0
    for B, Ts in ((14, (4, 6, 10, 15, 21, 28)), (24, (2, 3, 6, 8, 10, 15)), (40, (1, 2, 3, 4, 6, 10))):
        for T in Ts:
            L = 2 if T <= 4 else (4 if T <= 9 else 8)   # few moves need few cost values for a quarter of the nodes to tie
            pen = (0.375, 0.25)[k % 2]
            out.append(("B%d_T%d" % (B, T), take_types(T), B, k % 2 == 0, L, pen, "rand"))
            k += 1
    out += [
        ("B14_T10_reversed", take_types(10, reverse=True), 14, True, 4, 0.375, "rand"),   # merge keys follow list order, not (xo, yo)
        ("B24_T6_reversed", take_types(6, reverse=True), 24, False, 2, 0.25, "rand"),
        ("B14_T3_two_groups", take_types(3), 14, True, 2, 0.25, "rand"),                   # T < 4: G falls to 2
        ("B14_T10_all_equal", take_types(10), 14, False, 0, 0.0, "equal"),
        ("B14_T10_all_zero", take_types(10), 14, True, 0, 0.0, "zero"),
        ("B24_T8_all_zero", take_types(8), 24, False, 0, 0.0, "zero"),
        ("B40_T6_all_equal", take_types(6), 40, True, 0, 0.0, "equal"),
        ("B96_ring", take_types(10), 96, True, 4, 0.375, "rand"),                          # k_sparse_dp<true>
        ("B96_ring_all_zero", take_types(6), 96, False, 0, 0.0, "zero"),
        ("B2000_noring", [(1, 1), (4, 5), (8, 1), (1, 8), (2, 2)], 2000, True, 4, 0.375, "rand"),   # k_sparse_dp<false>
    ]
    return out


P_SPARSE = _p_sparse_cases()


def p_sparse_inputs(case):
    """-> (costs [T][A][B] f32, b_offset [A] i32, types, pen, N, M)"""
    name, types, B, jumps, L, pen, mode = case
    A = P_N + P_M - 1
    for k in range(1000):   # the first seed whose band holds the end node (N, M), so that the traceback has a path to walk
        rs = np.random.RandomState(1000 + sum(map(ord, name)) + 7919 * k)
        bo = band_offsets(rs, A, B, jumps)
        if 0 <= P_M - (bo[A - 1] + 1) < B and 0 <= -bo[0] < B:
            break
    return p_costs(rs, (len(types), A, B), L, mode), bo, types, pen, P_N, P_M


# name, s0, s1, L, penalty, cost mode
P_DENSE = [
    ("1x1", 1, 1, 0, 0.25, "equal"),                  # 0.5 = two deletions of 0.25
    ("1x9", 1, 9, 0, 0.25, "equal"),
    ("64x64", 64, 64, 3, 0.125, "rand"),
    ("257x250", 257, 250, 2, 0.125, "rand"),
    ("64x64_all_zero", 64, 64, 0, 0.0, "zero"),
    ("64x64_all_equal", 64, 64, 0, 0.25, "equal"),    # 1-1 step = two deletions everywhere
]


def p_dense_inputs(case):
    name, s0, s1, L, pen, mode = case
    rs = np.random.RandomState(2000 + sum(map(ord, name)))
    return p_costs(rs, (s0, s1), L, mode), pen


# ------------------------------------------------------------------------------------------ family Z
FRAC, SAMPLE, NSAMP = 0.2, 20000, 100
LEVELS6 = (0.25, 0.5, 0.75, 1.0, 1.5, 2.0)
LEVELS2 = (0.5, 1.0)


def z_pair(N, M, K0, K1, d, levels, seed):
    """Zero embeddings and depth-0 normalisers drawn from `levels` -> (v0, v1, n0, n1) float32."""
    rs = np.random.RandomState(seed)
    lv = np.asarray(levels, np.float32)
    n0 = lv[rs.randint(0, len(lv), (K0, N))]
    n1 = lv[rs.randint(0, len(lv), (K1, M))]
    return np.zeros((K0, N, d), np.float32), np.zeros((K1, M, d), np.float32), np.ascontiguousarray(n0), np.ascontiguousarray(n1)


def z_cost(xo, yo, n0, n1):
    """The band cost of type (xo, yo) on zero embeddings (dp_core.pyx:229-235), n0 / n1 the two normalisers."""
    return np.float32((2.0 * xo) * yo * 1.0 / ((1e-6 + float(np.float32(n0))) + float(np.float32(n1))))


def z_oracle(orc, v0, v1, n0, n1, types, W, max_full, seed, del_penalties=None):
    return orc.vecalign(v0.copy(), v1.copy(), types, FRAC, W, max_full, SAMPLE, NSAMP, norms0=n0, norms1=n1,
                        rng=np.random.RandomState(seed), del_penalties=del_penalties)


def many_to_one_types(m):
    from svx.vecalign.vecalign import resolve_search_params
    types, sk, tk, _ = resolve_search_params(10, m, 5)
    assert (sk, tk) == (m, 1)
    return types


def straight_stack(orc, v0, v1, types, W, seed, norms=None, pen=None):
    """The oracle's straight search as one stack entry: make_sparse_costs + sparse_dp + sparse_traceback on the
    straight path over the whole documents, depth-0 normalisers (computed, or `norms` = (n0, n1) as supplied by the
    caller) and deletion penalty (estimated, or `pen`)."""
    N, M = v0.shape[1], v1.shape[1]
    a, b = v0.copy(), v1.copy()
    orc.make_norm1(a)
    orc.make_norm1(b)
    rs = np.random.RandomState(seed)
    if norms is None:
        n0, n1 = orc.compute_norms(a, b, 100, rs), orc.compute_norms(b, a, 100, rs)
    else:
        n0, n1 = norms
    est, knob = orc.make_del_penalty(a[0], b[0], n0[0], n1[0], 20000, 0.2, rs)
    path = orc.search_path([(list(range(N)), list(range(M)))], False, N, M)
    f, bo = orc.make_sparse_costs(a, b, n0, n1, path, types, W)
    use = est if pen is None else float(pen)
    csum, xp, yp, bout = orc.sparse_dp(f, bo, types, use, N, M)
    al, sc = orc.sparse_traceback(csum, xp, yp, bout, N, M)
    return dict(a_b_costs=f, b_offset=bo, a_b_csum=csum, a_b_xp=xp, a_b_yp=yp, new_b_offset=bout, final_alignments=al,
                alignment_scores=sc, del_penalty=use, del_penalty_estimated=est, knob_scores=knob, size0=N, size1=M,
                alignment_types=list(types), n0=n0, n1=n1)


def straight_oracle(orc, v0, v1, types, W, seed):
    """make_sparse_costs + sparse_dp + sparse_traceback on the straight path, depth-0 norms and penalty (oracle)."""
    st = straight_stack(orc, v0, v1, types, W, seed)
    return st['final_alignments'], st['alignment_scores']


# Coarse-to-fine cases (test c).  name, [(N, M)], a, W, storage, d, levels, max_size_full_dp, seed, pipeline
Z_FUSED = [
    ("a5_W7_f32_6lv", [(300, 280)], 5, 7, "f32", 32, LEVELS6, 100, 1, False),
    ("a5_W7_f32_6lv_pipeline", [(300, 280)], 5, 7, "f32", 32, LEVELS6, 100, 1, True),
    ("a5_W7_f16_2lv", [(300, 280)], 5, 7, "f16", 32, LEVELS2, 100, 2, False),
    ("a2_W7_bf16_2lv", [(300, 280)], 2, 7, "bf16", 32, LEVELS2, 100, 3, False),
    ("a4_W12_f32_2lv", [(300, 280)], 4, 12, "f32", 32, LEVELS2, 100, 4, False),
    ("a6_W12_f16_6lv", [(300, 280)], 6, 12, "f16", 32, LEVELS6, 100, 5, False),
    ("a9_W20_bf16_2lv", [(300, 280)], 9, 20, "bf16", 32, LEVELS2, 100, 6, False),
    ("a5_W20_f32_3levels", [(300, 280)], 5, 20, "f32", 32, LEVELS2, 60, 7, False),       # 300 x 280 -> 150 x 140 -> 75 x 70: three levels
    ("a5_W7_bf16_d1024", [(300, 280)], 5, 7, "bf16", 1024, LEVELS2, 100, 8, False),      # generation-3 band kernel's epilogue
    ("a5_W7_f32_ragged4", [(300, 280), (211, 333), (120, 97), (402, 399)], 5, 7, "f32", 32, LEVELS2, 100, 9, False),
]

# Straight search (test d).  name, [(N, M)], types, W, storage, d, levels, seed
Z_STRAIGHT = [
    ("narrow_a5_W16", [(200, 190)], alignment_types(5), 16, "f32", 32, LEVELS2, 21),          # band of 32: the band kernels on a straight path
    ("a5_W40", [(300, 280)], alignment_types(5), 40, "f32", 32, LEVELS2, 22),                 # LDS-resident shape, 10 types
    ("a6_W33_bf16", [(330, 310)], alignment_types(6), 33, "bf16", 32, LEVELS6, 23),           # LDS-resident shape, 15 types
    ("a7_W40", [(250, 260)], alignment_types(7), 40, "f32", 32, LEVELS2, 24),                 # general shape, MS = 3
    ("a8_W36_f16", [(240, 230)], alignment_types(8), 36, "f16", 32, LEVELS6, 40),             # MS = 4
    ("a10_W48", [(220, 230)], alignment_types(10), 48, "f32", 32, LEVELS6, 40),               # MS = 6
    ("a12_dense", [(150, 140)], alignment_types(12), 200, "f32", 32, LEVELS2, 27),            # MS = 9
    ("a16_dense", [(120, 118)], alignment_types(16), 200, "f32", 32, LEVELS6, 41),            # MS = 17
    ("ms2_custom", [(260, 250)], [(1, 1), (1, 2), (2, 1), (9, 1), (1, 9), (3, 3), (2, 9)], 40, "f32", 32, LEVELS2, 29),
    ("m2o20_W60", [(330, 120)], None, 60, "f32", 32, LEVELS6, 40),                            # int32 back-pointers
    ("bigh_100", [(330, 320)], [(1, 1), (100, 1), (1, 100), (1, 2), (2, 1)], 120, "f32", 32, LEVELS2, 31),
    ("a10_W60_batch3", [(210, 200), (330, 310), (120, 260)], alignment_types(10), 60, "f32", 32, LEVELS6, 40),
]


def z_straight_types(case):
    return many_to_one_types(20) if case[2] is None else case[2]


def z_fused_pairs(case):
    """-> [(v0, v1, n0, n1, seed)] of a Z_FUSED case."""
    _, sizes, a, W, store, d, levels, max_full, seed, _ = case
    K = max(1, a - 1)
    return [z_pair(N, M, K, K, d, levels, 100 * seed + k) + (100 * seed + k,) for k, (N, M) in enumerate(sizes)]


def z_fused_refs(name, keep_embeddings=False):
    """The oracle's stacks of a Z_FUSED case, one per pair (in a process that never touches the GPU)."""
    import oracle
    case = [c for c in Z_FUSED if c[0] == name][0]
    out = []
    for v0, v1, n0, n1, seed in z_fused_pairs(case[:5] + (min(case[5], 32),) + case[6:]):   # (zero rows: the width changes nothing)
        ref = z_oracle(oracle, v0, v1, n0, n1, alignment_types(case[2]), case[3], case[7], seed)
        if not keep_embeddings:
            for st in ref.values():
                st.pop('v0'), st.pop('v1')
        out.append(ref)
    return out


def z_straight_pairs(case):
    _, sizes, _, W, store, d, levels, seed = case
    types = z_straight_types(case)
    K0, K1 = max(x for x, _ in types), max(y for _, y in types)
    return [z_pair(N, M, K0, K1, d, levels, 100 * seed + k) + (100 * seed + k,) for k, (N, M) in enumerate(sizes)]


def z_straight_refs(name, keep_costs=True):
    """The oracle's straight search of a Z_STRAIGHT case, one stack entry per pair."""
    import oracle
    case = [c for c in Z_STRAIGHT if c[0] == name][0]
    out = []
    for v0, v1, n0, n1, seed in z_straight_pairs(case):
        st = straight_stack(oracle, v0, v1, z_straight_types(case), case[3], seed, norms=(n0, n1))
        if not keep_costs:
            st.pop('a_b_costs')
        out.append(st)
    return out
