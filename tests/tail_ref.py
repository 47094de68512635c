"""Cases for the refinement chain's tail -- sparse traceback, search path, dense traceback -- on inputs that no DP
produced; TEST INFRASTRUCTURE (numpy only, seeded, no GPU).  Shared by test_tail_ref_cpu.py, test_gpu_tail.py and
tests/golden/make_golden.py (which records what the REAL reference returns on the success cases, tail_records.json).
The expected value everywhere is the CPU oracle; the reference is never fed a failure case (with a (0,0) back-pointer
it does not terminate).

What the kernels dispatch on, restated from speech-vecalign_amd/csrc/svx_dp.hip (default SVX_TB_WIN_KB = 20):

  tb_chunk(B, wide)  (svx_dp.hip:679-684):  c = (20480 / (B * (wide ? 2 : 1) + 4)) & ~15; a window of c diagonals is
      used when c >= 64, else 0.  wide = int32 xp / yp (16-bit pairs in LDS), not wide = packed bytes.
  svxl_sparse_traceback, the per-op entry (svx_dp.hip:1432-1446):  always int32: chunk = tb_chunk(B, true), no corridor.
      B <= 158 -> tb_walk<2> (chunk 2560 at B = 2, 640 at 14, 240 at 40, 64 at 158);  B >= 159 -> tb_walk<0>
      (the choice of the walk: svx_dp.hip:870-873).
  svxl_sparse_traceback_batch, the fused path (svx_dp.hip:1448-1463):  packed = every step <= 15 (svx_api.hip,
      `bp.packable`).  packed:  B <= 316 -> tb_walk<1> (chunk 64 at 316);  else B > 320 (TB_COR_W, svx_dp.hip:676) and
      B % 16 == 0 -> tb_walk<3>, corridor windows of TB_COR_CHUNK = 64 diagonals x 320 columns;  else tb_walk<0>.
      int32: as the per-op entry.
  corridor origin (sparse_traceback_block, svx_dp.hip:830-835 and :846-852):  c0 = clamp((b - 160) & ~15, 0, B - 320),
      b = the walk's column at the end node for the topmost window, and for window j - 1 the column of the node the walk
      stands on when it enters window j.
  sp_lds_rows (svx_dp.hip:1465-1472; sp_smem_bytes(r) = 16 r + 32, :1018):  search_path_block takes n_align <= rows
      (:1107), rows = max_rows when 16 max_rows + 32 <= 150 KB, else 9597; above it one thread runs search_path_thread.
"""
import zlib

import numpy as np

TB_WIN_BYTES = 20 * 1024
TB_COR_CHUNK, TB_COR_W = 64, 320
SP_LDS_LIMIT = 150 * 1024
SP_LDS_ROWS = SP_LDS_LIMIT // 16 - 3   # 9597
EXTEND_TEXT = 'asked to extend alignments but already bigger than requested'


def tb_chunk(B, wide):
    c = (TB_WIN_BYTES // (B * (2 if wide else 1) + 4)) & ~15
    return c if c >= 64 else 0


def tb_mode(B, packed):
    """-> (MODE of tb_walk, diagonals per window, corridor columns) for a band of B cells."""
    chunk = tb_chunk(B, not packed)
    if chunk > 0:
        return (1 if packed else 2), chunk, 0
    if packed and B > TB_COR_W and B % 16 == 0:
        return 3, TB_COR_CHUNK, TB_COR_W
    return 0, 0, 0


def sp_lds_rows(max_rows):
    return max_rows if 16 * max_rows + 32 <= SP_LDS_LIMIT else SP_LDS_ROWS


def sp_form(n_align, size0, size1):
    """'block' | 'thread': which form k_search_path runs for the per-op entry (max_rows = size0 + size1 + 2)."""
    return 'block' if n_align <= sp_lds_rows(size0 + size1 + 2) else 'thread'


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


# ------------------------------------------------------------------------------------------ A: sparse traceback
POOL = [(1, 0), (0, 1), (1, 1), (1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (1, 3)]
FAT_POOL = [(1, 0), (0, 1), (1, 1), (2, 3), (4, 4), (5, 2)]   # four diagonals a row: 257 rows cross a 640-diagonal window


def steps_to(rs, diag, pool=POOL):
    """Backward steps (px, py) whose diagonal lengths sum to exactly `diag`."""
    out, left = [], diag
    while left > 0:
        c = [s for s in pool if s[0] + s[1] <= left]
        out.append(c[rs.randint(len(c))])
        left -= sum(out[-1])
    return out


def steps_n(rs, n, pool=POOL):
    return [pool[rs.randint(len(pool))] for _ in range(n)]


def walk_nodes(steps):
    N, M = sum(s[0] for s in steps), sum(s[1] for s in steps)
    nodes = [(N, M)]
    for px, py in steps:
        nodes.append((nodes[-1][0] - px, nodes[-1][1] - py))
    assert nodes[-1] == (0, 0)
    return nodes


NEIGHBOURS = ((0, -1), (0, 1), (-1, 0), (1, 0))   # (diagonal, column) offsets of the mutant reads


def tb_tables(steps, B, a_out, seed):
    """-> dict(csum, xp, yp, boff, N, M, nodes, cols): a table in which the backward walk `steps` from (N, M) to (0, 0) is
    written and everything else is garbage (-42 in about 30 %, else -1..3); b_offset_out arbitrary int32 (not monotone,
    a few at the ends of the int32 range) except that every walk node lies in the band, some at column 0 and some at
    B - 1; csum i.i.d. normal, so about half of the score differences are negative.
    The filling discriminates: the four cells next to a walk node (same diagonal +-1 column, same column +-1 diagonal)
    never hold that node's step."""
    rs = np.random.RandomState(seed)
    nodes = walk_nodes(steps)
    N, M = nodes[0]
    assert a_out >= N + M + 1 and B >= 2
    boff = rs.randint(-3 * B - 7, M + 3 * B + 8, a_out).astype(np.int64)
    k = 1 + a_out // 50
    boff[rs.randint(0, a_out, k)] = rs.choice([2 ** 31 - 1, -2 ** 31, 2 ** 31 - 2, -2 ** 31 + 1], k)
    cols, prev = [], None
    for i, (x, y) in enumerate(nodes):
        st = steps[i] if i < len(steps) else None
        u = rs.rand()
        c = 0 if u < 0.15 else (B - 1 if u < 0.3 else int(rs.randint(B)))
        if prev is not None and prev[0] == x + y + 1 and prev[1] == c and prev[2] == st:
            c = (c + 1) % B   # (a neighbouring walk cell with the same step would hide a read of the wrong diagonal)
        cols.append(c)
        boff[x + y] = y - c
        prev = (x + y, c, st)
    g = rs.randint(-1, 4, (2, a_out, B))
    g[rs.rand(2, a_out, B) < 0.3] = -42
    xp, yp = g[0].astype(np.int32), g[1].astype(np.int32)
    cells = set()
    for (x, y), c, (px, py) in zip(nodes, cols, steps):
        xp[x + y, c], yp[x + y, c] = px, py
        cells.add((x + y, c))
    for (x, y), c, (px, py) in zip(nodes, cols, steps):
        for da, db in NEIGHBOURS:
            a, b = x + y + da, c + db
            if 0 <= a < a_out and 0 <= b < B and (a, b) not in cells and (xp[a, b], yp[a, b]) == (px, py):
                xp[a, b] = yp[a, b] = -42
    csum = rs.standard_normal((a_out, B))
    return dict(csum=csum, xp=xp, yp=yp, boff=boff.astype(np.int32), N=N, M=M, nodes=nodes, cols=cols, steps=list(steps), B=B)


def py_walk(t, mutate=None):
    """The reference's walk (dp_utils.py:105-131) restated with Python integers and explicit range checks, spans only.
    mutate = (row, da, db): at that row the back-pointers are read da diagonals / db columns off.  Raises on any failure."""
    xp, yp, boff, B = t['xp'], t['yp'], t['boff'], t['B']
    a_out = xp.shape[0]
    xx, yy, rows = t['N'], t['M'], []
    while True:
        aa = xx + yy
        if not 0 <= aa < a_out:
            raise Exception('traceback bug')
        bb = yy - int(boff[aa])
        if not 0 <= bb < B:
            raise Exception('traceback bug')
        if xx == 0 and yy == 0:
            return rows
        if xx < 0 or yy < 0 or len(rows) > t['N'] + t['M']:
            raise Exception('traceback bug')
        ra, rb = aa, bb
        if mutate is not None and mutate[0] == len(rows):
            ra, rb = aa + mutate[1], bb + mutate[2]
            if not (0 <= ra < a_out and 0 <= rb < B):
                raise Exception('traceback bug')
        px, py = int(xp[ra, rb]), int(yp[ra, rb])
        if px < 0 or py < 0 or (px == 0 and py == 0):
            raise Exception('traceback bug')
        rows.append((xx - px, px, yy - py, py))
        xx, yy = xx - px, yy - py


def rows_to_alignments(rows):
    return [(list(range(r[0], r[0] + r[1])), list(range(r[2], r[2] + r[3]))) for r in rows]


FLUSH_ROWS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257)
LDS_B, GLOBAL_B = (2, 14, 40, 158), (159, 160, 400)


def _tb_ok_specs():
    """name -> (B, steps, a_out).  Steps are at most 100 a side (the library's limit), 100 included."""
    out = {}

    def add(name, B, steps, extra):
        assert name not in out
        out[name] = (B, steps, sum(map(sum, steps)) + 1 + extra)
    # 1. every mode and chunk size; a_out = 2 * chunk + r: the topmost window is full, one diagonal long, one short
    for B in LDS_B:
        chunk = tb_chunk(B, True)
        for r in (0, 1, chunk - 1):
            name = "win_B%d_r%d" % (B, r)
            add(name, B, steps_to(np.random.RandomState(_seed(name)), 2 * chunk + r - 1), 0)
    for B in GLOBAL_B:
        name = "global_B%d" % B
        add(name, B, steps_to(np.random.RandomState(_seed(name)), 257), 2)
    # 2. the 64-row flush in the lanes
    for B in (14, 158):
        for n in FLUSH_ROWS:
            name = "rows%d_B%d" % (n, B)
            add(name, B, steps_n(np.random.RandomState(_seed(name)), n, FAT_POOL if B == 14 else POOL), n % 3)
    # 3. all deletions: n = N + M = cap - 2 > 512 (the in-place move shifts by two rows over several 256-row rounds)
    for B in (14, 158):
        name = "alldel_B%d" % B
        st = [(1, 0)] * 300 + [(0, 1)] * 300
        np.random.RandomState(_seed(name)).shuffle(st)
        add(name, B, [tuple(s) for s in st], 2)
    # 4. steps that skip whole windows (chunk 64 at B = 158)
    add("skip_B158", 158, [(1, 1)] * 5 + [(100, 100)] + [(1, 1)] * 70 + [(100, 1)] + [(1, 2)] * 30 + [(1, 100)] + [(2, 1)] * 20
        + [(100, 100)] + [(1, 0), (0, 1)] * 10, 2)
    add("skip_first_B158", 158, [(100, 100)] + [(1, 1)] * 40 + [(1, 100)] + [(1, 1)] * 3, 0)
    # 5. degenerate sizes
    for B in (14, 160):
        add("empty_a1_B%d" % B, B, [], 0)
        add("empty_a3_B%d" % B, B, [], 2)
        for extra in (0, 2):
            add("zeroN_x%d_B%d" % (extra, B), B, [(0, 1)] * 7, extra)
            add("zeroM_x%d_B%d" % (extra, B), B, [(1, 0)] * 7, extra)
    return out


TB_OK = _tb_ok_specs()


def tb_ok_case(name):
    B, steps, a_out = TB_OK[name]
    return tb_tables(steps, B, a_out, _seed(name))


# 6. failures.  Three windows at B = 14 (chunk 640); the same tables at B = 160 walk global memory.
FAIL_A_OUT = 2 * 640 + 100
FAIL_KINDS_AT = ('node_left', 'node_right', 'm42', 'zero', 'px_gt', 'py_gt')
FAIL_WHERE = ('last', 'middle', 'first')
TB_FAIL = ([(k, None, B) for B in (14, 160) for k in ('end_left', 'end_right', 'origin_1', 'origin_mB')]
           + [(k, w, B) for B in (14, 160) for k in FAIL_KINDS_AT for w in FAIL_WHERE])


def tb_fail_id(spec):
    return "%s_%s_B%d" % (spec[0], spec[1] or "x", spec[2])


def tb_fail_case(spec):
    """A success table with one thing wrong -> the dict of tb_tables plus 'bad' = index of the offending walk node."""
    kind, where, B = spec
    rs = np.random.RandomState(_seed(tb_fail_id(spec)))
    D = FAIL_A_OUT - 1
    if kind == 'px_gt':      # a thin walk: x stays <= 3 in every window, so that px = x + 1 is an ordinary small step
        steps = [(0, 1)] * (D - 6) + [(1, 1)] * 3
    elif kind == 'py_gt':
        steps = [(1, 0)] * (D - 6) + [(1, 1)] * 3
    else:
        steps = steps_to(rs, D)
    if kind in ('px_gt', 'py_gt'):
        rs.shuffle(steps)
        steps = [tuple(s) for s in steps]
    t = tb_tables(steps, B, FAIL_A_OUT, _seed(tb_fail_id(spec)) ^ 0x5A5A)
    nodes, cols, N, M = t['nodes'], t['cols'], t['N'], t['M']
    centre = {'last': 2 * 640 + 50, 'middle': 640 + 320, 'first': 320, None: 0}[where]
    i = min(range(1, len(steps)), key=lambda k: abs(sum(nodes[k]) - centre))
    x, y = nodes[i]
    a, c = x + y, cols[i]
    if where is not None:
        lo = {'last': 1280, 'middle': 640, 'first': 1}[where]
        assert lo <= a < lo + 640
    if kind == 'end_left':
        t['boff'][N + M], i = M + 1, 0
    elif kind == 'end_right':
        t['boff'][N + M], i = M - B, 0
    elif kind == 'origin_1':
        t['boff'][0], i = 1, len(steps)
    elif kind == 'origin_mB':
        t['boff'][0], i = -B, len(steps)
    elif kind == 'node_left':
        t['boff'][a] = y + 1
    elif kind == 'node_right':
        t['boff'][a] = y - B
    elif kind == 'm42':
        t['xp'][a, c] = t['yp'][a, c] = -42
    elif kind == 'zero':
        t['xp'][a, c] = t['yp'][a, c] = 0
    elif kind == 'px_gt':
        t['xp'][a, c] = x + 1
    elif kind == 'py_gt':
        t['yp'][a, c] = y + 1
    t['bad'] = i
    return t


def window_boundary_inside_block(t, chunk):
    """Does the walk enter a new window at a row number that is no multiple of 64?"""
    if chunk <= 0:
        return False
    nodes = t['nodes']
    for r in range(1, len(t['steps'])):
        if sum(nodes[r]) // chunk != sum(nodes[r - 1]) // chunk and r % 64 != 0:
            return True
    return False


# ------------------------------------------------------------------------------------------ B: search path
def random_alignment(rs, n, del_share, blocks, del_ends=False):
    """n monotone alignment rows ([x ids], [y ids]).  del_share of them are deletions of either side (runs mix both
    sides); with `blocks` a seventh of the others are many-to-many up to 40 x 40, half of those with equal widths or
    1 : 3 (append_slant then has a rint tie at every other point)."""
    out, x, y = [], 0, 0
    for i in range(n):
        if rs.rand() < del_share or (del_ends and i in (0, 1, n - 2, n - 1)):
            if rs.rand() < 0.5:
                out.append(([x], []))
                x += 1
            else:
                out.append(([], [y]))
                y += 1
            continue
        p = q = 1
        if blocks and rs.rand() < 1.0 / 7:
            u = rs.rand()
            if u < 0.25:
                p = q = int(rs.randint(2, 41))
            elif u < 0.5:
                p = int(rs.randint(1, 14))
                q = 3 * p
                if rs.rand() < 0.5:
                    p, q = q, p
            else:
                p, q = int(rs.randint(1, 41)), int(rs.randint(1, 41))
        out.append((list(range(x, x + p)), list(range(y, y + q))))
        x, y = x + p, y + q
    return out


def up_max(alignments):
    """(xmax, ymax) of extend_alignments (dp_utils.py:234-240) after upsample_alignment: the largest index, or 0."""
    X = sum(len(a) for a, _ in alignments)
    Y = sum(len(b) for _, b in alignments)
    return max(2 * X - 1, 0), max(2 * Y - 1, 0)


SP_ROWS, SP_SHARES = (0, 1, 2, 50, 400), (0.0, 0.5, 1.0)
SP_EXTRA = ((0, 0), (1, 0), (0, 1), (1, 1), (0, 37), (23, 0), (9, 14))   # all three branches of extend_alignments
SP_GRID = [(n, s, b) for n in SP_ROWS for s in SP_SHARES for b in (False, True)]


def sp_id(g):
    return "n%d_del%g_%s" % (g[0], g[1], "blocks" if g[2] else "plain")


def sp_alignment(g):
    n, share, blocks = g
    rs = np.random.RandomState(_seed(sp_id(g)))
    return random_alignment(rs, n, share, blocks, del_ends=(n >= 50 and share == 0.5))


def sp_calls(al):
    """[(label, upsample, size0, size1)] of one alignment: as it is, and up-sampled with every extension."""
    xm, ym = up_max(al)
    X, Y = sum(len(a) for a, _ in al), sum(len(b) for _, b in al)   # (sizes the path buffers are made for)
    return [("same", False, X, Y)] + [("up_%d_%d" % e, True, xm + e[0], ym + e[1]) for e in SP_EXTRA]


def sp_long(rows):
    """A `rows`-row alignment of 1-1 rows and deletions whose last two rows are 1-1 (so that the points of the first
    rows - 1 rows do not depend on the last one)."""
    rs = np.random.RandomState(9598)
    al = random_alignment(rs, rows - 2, 0.3, False)
    x = sum(len(a) for a, _ in al)
    y = sum(len(b) for _, b in al)
    return al + [([x], [y]), ([x + 1], [y + 1])]


def ref_search_path(R, al, upsample, size0, size1):
    """The reference chain (R = its dp_utils module).  Only for success cases."""
    al = [(list(a), list(b)) for a, b in al]
    if upsample:
        al = R.upsample_alignment(al)
        R.extend_alignments(al, size0, size1)
    return R.alignment_to_search_path(al)


# ------------------------------------------------------------------------------------------ C: dense traceback
def dense_table(shape, seed):
    """-> (bp [s0+1][s1+1] int32, nodes): a random lattice walk from (s0, s1) to (0, 0) written as codes 0 / 1 / 2 into
    garbage (0, 1, 2, 3, -1, 7, 4), 4 at the origin."""
    rs = np.random.RandomState(seed)
    s0, s1 = shape[0] - 1, shape[1] - 1
    bp = rs.choice([0, 1, 2, 3, -1, 7, 4], size=shape).astype(np.int32)
    bp[0, 0] = 4
    x, y, nodes = s0, s1, []
    while (x, y) != (0, 0):
        ok = [b for b in (0, 1, 2) if not (x == 0 and b in (0, 2)) and not (y == 0 and b in (0, 1))]
        b = ok[rs.randint(len(ok))]
        bp[x, y] = b
        nodes.append((x, y))
        x, y = x - (b != 1), y - (b != 2)
    return bp, nodes


DENSE_OK = {"1x1": (1, 1), "1x9": (1, 9), "9x1": (9, 1), "40x37": (40, 37), "2x2": (2, 2)}
DENSE_BAD_VALUES = (3, -1, 7, 4)
DENSE_FAIL = ([("value", v, w) for v in DENSE_BAD_VALUES for w in ("first", "middle", "last")]
              + [("border", b, e) for b, e in ((0, "x0"), (2, "x0"), (0, "y0"), (1, "y0"))])


def dense_ok_case(name):
    return dense_table(DENSE_OK[name], _seed("dense" + name))[0]


def dense_fail_case(spec):
    kind, v, where = spec
    for k in range(1000):   # a walk that reaches the border asked for away from the origin
        bp, nodes = dense_table((40, 37), _seed("dense%r" % (spec,)) + k)
        if kind == "value":
            x, y = nodes[{"first": 0, "middle": len(nodes) // 2, "last": len(nodes) - 1}[where]]
            break
        hit = [(x, y) for x, y in nodes if (x == 0 and y > 1 if where == "x0" else y == 0 and x > 1)]
        if hit:
            x, y = hit[0]
            break
    bp = bp.copy()
    bp[x, y] = v
    return bp, (x, y)


# ------------------------------------------------------------------------------------------ D: shifted pairs
def shifted_pair(S, J, K0, K1, d, seed, noise=0.5):
    """source = J unrelated rows then S shared rows; target = the noisy copy of the shared rows then J unrelated rows;
    layers as synth.make_pair.  The optimum under straight search: about J source deletions, the shared run at distance
    J from the straight path, about J target deletions."""
    rng = np.random.default_rng(seed)
    shared = rng.standard_normal((S, d)).astype(np.float32)
    src = np.concatenate([rng.standard_normal((J, d)).astype(np.float32), shared])
    tgt = np.concatenate([shared + noise * rng.standard_normal((S, d)).astype(np.float32), rng.standard_normal((J, d)).astype(np.float32)])

    def layers(b, K):
        n = b.shape[0]
        out = np.zeros((K, n, d), np.float32)
        cs = np.concatenate([np.zeros((1, d), np.float32), np.cumsum(b.astype(np.float64), axis=0).astype(np.float32)])
        for k in range(K):
            if n > k:
                out[k, k:] = cs[k + 1:n + 1] - cs[:n - k]
        return out
    return layers(src, K0), layers(tgt, K1)


TYPES5 = [(x, y) for x in range(1, 5) for y in range(1, 5) if x + y <= 5]   # synth.alignment_types(5)
TYPES20 = [(1, 1), (1, 2), (2, 1), (20, 1)]
# W -> (types, S, J, data seed, seed of the random draws, mirrored).  J < W, about 0.75 W; N + M = 2 (S + J) crosses >= 8
# windows of 64 diagonals.  The walk's band column runs from W (on the straight path) J / 2 columns down and back; with the
# two documents swapped ("mirrored") it runs up instead, which is what moves the corridor at B = 336, where the only
# origins are 0 (column < 176) and 16.  The (20, 1) type swallows runs of unrelated source rows that would otherwise be
# deletions, hence the larger J there.  Seeds chosen on the CPU (test_tail_ref_cpu.py states the conditions).
SHIFTED = {
    158: (TYPES5, 400, 118, 1, 11, False),
    159: (TYPES5, 400, 119, 2, 12, False),
    160: (TYPES5, 400, 120, 3, 13, False),
    161: (TYPES5, 400, 121, 4, 14, False),
    168: (TYPES5, 400, 126, 5, 15, True),
    400: (TYPES5, 500, 300, 6, 16, False),
    79: (TYPES20, 192, 66, 21, 17, False),
    80: (TYPES20, 192, 66, 21, 17, False),
}
SHIFTED_D = 32


def shifted_case(W):
    types, S, J, seed, rseed, mirror = SHIFTED[W]
    K0, K1 = max(x for x, _ in types), max(y for _, y in types)
    if mirror:
        v1, v0 = shifted_pair(S, J, K1, K0, SHIFTED_D, seed)
    else:
        v0, v1 = shifted_pair(S, J, K0, K1, SHIFTED_D, seed)
    return v0, v1, types, rseed


def shifted_mode(W):
    types = SHIFTED[W][0]
    return tb_mode(2 * W, max(max(t) for t in types) <= 15)


def alignment_nodes(alignments):
    """Walk nodes of an alignment in traceback order: (N, M) first, (0, 0) last."""
    x = sum(len(a) for a, _ in alignments)
    y = sum(len(b) for _, b in alignments)
    nodes = [(x, y)]
    for a, b in reversed(alignments):
        x, y = x - len(a), y - len(b)
        nodes.append((x, y))
    return nodes


def simulate_corridor(nodes, boff, B):
    """sparse_traceback_block's corridor rule on a walk -> (window origins in the order they are set, number of reads
    outside their window).  nodes: traceback order; boff = new_b_offset [a_out]."""
    a_out = len(boff)
    nwin = (a_out + TB_COR_CHUNK - 1) // TB_COR_CHUNK

    def origin(node):
        b = node[1] - int(boff[sum(node)])
        return min(max((b - TB_COR_W // 2) & ~15, 0), B - TB_COR_W)
    c0 = {nwin - 1: origin(nodes[0])}
    k, outside = 0, 0   # nodes[k]: where the walk stands
    for j in range(nwin - 1, -1, -1):
        if j > 0:
            c0[j - 1] = origin(nodes[k])
        lo = j * TB_COR_CHUNK
        while k < len(nodes) - 1 and sum(nodes[k]) >= lo:
            b = nodes[k][1] - int(boff[sum(nodes[k])])
            outside += not c0[j] <= b < c0[j] + TB_COR_W
            k += 1
    assert k == len(nodes) - 1
    return [c0[j] for j in range(nwin - 1, -1, -1)], outside
