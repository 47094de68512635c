"""The per-op entries of include/svx.h (the drop-in for dp_core.pyx and the numpy hot spots of dp_utils.py) at every
row width and dispatch edge, through their public Python mirrors (svx.vecalign.dp_core / dp_utils), so the ctypes
prototypes are covered too.

These entries launch kernels of their own (svx_rows.hip "per-op (plain pointer) kernels", svxl_score_path,
svxl_band_costs, svxl_dense_costs, svxl_dense_dp, svxl_del_penalty), not the fused pipeline's; test_gpu_ops.py runs
them at d = 64 only.  Every continuous case here compares, on float32 inputs,
  (a) the CPU oracle's function of the same name, and
  (b) the float64 restatement of stage_ref.py (norm1, downsample, norms, dense_costs, score_path, band_costs)
by the rule of stage_check.py, with no number of its own:
        E_gpu <= max(2 * E_orc, 4 * 2^-24 * max |f64|),
integer outputs (b_offset) and the pattern of infinite cells bit for bit.  Each case runs on make_pair data as it is
("iid") and with common=1.4 ("aniso").  tests/test_op_ref_cpu.py guards the reference side of every case below on the
CPU (it imports the tables of this file).

Which case selects which instantiation (read off nch_f32 / choose_variant and make_plan of svx_band.hip, which
tests/test_op_ref_cpu.py restates; profiles/op_matrix_kernels.txt is the kernel trace of this file, checked against
this table):

    d = 8, 256            NCH 1 (one 16-byte piece; every lane of the only chunk full)
    d = 264, 512          NCH 2 (first lanes of the second chunk; both chunks full)
    d = 520, 1024         NCH 4
    d = 1032, 2048        NCH 8          of k_norm1_plain, k_pairsum_plain, k_subnorm_plain, k_sample_mean_plain,
                                         k_rownorms_plain and k_score_path<ElemF32, NCH>
    compute_norms "rows33000" (d = 8)    k_rownorms_plain's grid-stride loop (more than 8192 workgroups of 4 rows)
    score_path n = 70001 (d = 8, 264)    k_score_path's grid-stride loop (more than 16384 workgroups of 4 rows)

    band set      types                      layers   k_band_costs2_op<ElemF32, ROWS, NSLOT, UPW, S>, passes
    t1            [(1, 1)]                   1 + 1    64, 2, 1, 4     1
    rep           [(1, 1)] * 3               1 + 1    32, 8, 5, 3     1  (more than one type on two layers needs a repeated
                                                                         type; the oracle, like dp_core.pyx, loops over
                                                                         the list and accepts it)
    m21           [(1, 1), (2, 1)]           2 + 1    32, 8, 5, 3     1
    t3, t4, t5    alignment_types(3 .. 5)    .. 4 + 4 32, 8, 5, 3     1  (t5: all 8 slots, all 10 types of a pass)
    t6            alignment_types(6)         5 + 5    32, 12, 8, 3    1
    t7            alignment_types(7), 21     6 + 6    32, 20, 8, 2    2  (broken by the 16 types of a pass)
    t10           alignment_types(10), 45    9 + 9    32, 20, 8, 2    3  (type limit)
    t11           alignment_types(11), 55    10 + 10  32, 20, 8, 2    4  (type limit; 20 layers in all)
    diag12        [(i, i) for i in 1 .. 12]  12 + 12  32, 20, 8, 2    2  (broken by the 20 slots of a pass: 10 + 2 types)
    straight      alignment_types(4), 40 x 150 docs, a straight path: part of the band lies outside the lattice
    len135, len136     alignment_types(4) on 70 x 64, 70 x 65: with t4 (70 x 66, 137 points) the path is one short of,
                       equal to and one over 8 chunks of lim + 1 = 17 points (32 rows, W = 9 and 40)
    len146 .. len148   [(1, 1)] on 80 x 65 .. 67: the same around 3 chunks of 49 points (64 rows, W = 9 and 40)
  every set at d = 264 (sixteen 64-byte k-slabs and a 32-byte tail); t1, t4 and t7 also at d = 8, 1024, 2048;
  W = 3, 9, 40 (B = 6, 18, 80: below one 16-cell band chunk, just above one, five chunks).  The entry's [T][A][B] layout
  always leaves through the kernel's cell-by-cell write-out (the 16-byte one is the pipeline layout's).
    dense_dp s0 = 2729 / 2730            ring of 3 (s0 + 1) doubles below / above 64 KiB (hipFuncSetAttribute branch)
    dense_dp s0 = 6399 / 6400            the largest ring / refused

    python tests/test_gpu_op_matrix.py --dump FILE     (on the GPU box)
writes one JSON line per (op, case, data kind) with E_gpu, E_orc, the bound and the array size
(profiles/op_errors.jsonl); no assertion refers to those values."""
import contextlib
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # hand-run: the paths conftest.py sets up for pytest
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_root, "speech-vecalign_amd"), os.path.join(_root, "oracle"), os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, _p)

import stage_ref
from stage_check import U, stage_error
from synth import alignment_types, make_pair

COMMON = 1.4
KINDS = ("iid", "aniso")
WIDTHS = (8, 256, 264, 512, 520, 1024, 1032, 2048)      # the row kernels: every NCH, full and partly filled
DENSE_WIDTHS = (8, 264, 1024, 2048)
DENSE_SHAPES = ((1, 1), (1, 130), (63, 65), (64, 64), (65, 129), (130, 1))
DENSE_OFFSETS = ((0, 0), (2, 0), (1, 2))                 # K = 3: (0, 0), (K - 1, 0), (1, 2)
NORM1_ROWS = ((1, 1), (3, 21), (1, 64), (1, 65), (3, 43))   # (K, n): 1, 63, 64, 65, 129 rows
DOWN_N = (2, 3, 64, 65, 66, 67, 129, 130)                # h = 1, 1, 32, 32, 33, 33, 64, 65
DOWN_K = (1, 3)
NORMS_CASES = (  # name, K0, n0, K1, n1, num_samples   (S = ceil(num_samples / K1) per layer)
    ("k1_1", 3, 70, 1, 61, 100), ("k1_3", 3, 70, 3, 61, 100), ("k1_4", 3, 70, 4, 61, 100), ("one_sample", 3, 70, 3, 61, 1),
    ("n1_1", 3, 70, 3, 1, 100), ("n0_1", 3, 1, 3, 61, 100))
NORMS_BIG = ("rows33000", 3, 11000, 3, 61, 100)          # d = 8 only: past 8192 workgroups of 4 rows
SCORE_N = (1, 3, 4, 5, 4099)
SCORE_BIG, SCORE_BIG_WIDTHS = 70001, (8, 264)            # past 16384 workgroups of 4 rows
SHRUNK_ROWS = 300                                        # what the CPU guard puts in place of the two largest counts
BAND_W = (3, 9, 40)
R64, R32_8, R32_12, R32_20 = (64, 2, 1, 4), (32, 8, 5, 3), (32, 12, 8, 3), (32, 20, 8, 2)
BAND_SETS = {  # name: (types, (n, m) with a straight path or None for the 70 x 66 pair, (ROWS, NSLOT, UPW, S), passes)
    "t1": ([(1, 1)], None, R64, 1),
    "rep": ([(1, 1)] * 3, None, R32_8, 1),
    "m21": ([(1, 1), (2, 1)], None, R32_8, 1),
    "t3": (alignment_types(3), None, R32_8, 1),
    "t4": (alignment_types(4), None, R32_8, 1),
    "t5": (alignment_types(5), None, R32_8, 1),
    "t6": (alignment_types(6), None, R32_12, 1),
    "t7": (alignment_types(7), None, R32_20, 2),
    "t10": (alignment_types(10), None, R32_20, 3),
    "t11": (alignment_types(11), None, R32_20, 4),
    "diag12": ([(i, i) for i in range(1, 13)], None, R32_20, 2),
    "straight": (alignment_types(4), (40, 150), R32_8, 1),
    "len135": (alignment_types(4), (70, 64), R32_8, 1),
    "len136": (alignment_types(4), (70, 65), R32_8, 1),
    "len146": ([(1, 1)], (80, 65), R64, 1),
    "len147": ([(1, 1)], (80, 66), R64, 1),
    "len148": ([(1, 1)], (80, 67), R64, 1),
}
BAND_KEYS = [(s, 264) for s in BAND_SETS] + [(s, d) for d in (8, 1024, 2048) for s in ("t1", "t4", "t7")]
DP_SHAPES = ((2729, 5), (2730, 5), (6399, 3), (5, 7000))

CONTINUOUS_OPS = ("make_norm1", "downsample_vectors", "compute_norms", "score_path", "make_dense_costs", "make_sparse_costs")
KEYS = {"make_norm1": WIDTHS, "downsample_vectors": WIDTHS, "compute_norms": WIDTHS, "score_path": WIDTHS,
        "make_dense_costs": DENSE_WIDTHS, "make_sparse_costs": BAND_KEYS}
UNITS = [(op, key, kind) for op in CONTINUOUS_OPS for key in KEYS[op] for kind in KINDS]


def _oracle():
    import oracle
    oracle.lib()
    return oracle


def _seed(*parts):
    """A seed that depends on the case alone (no hash(): it differs from process to process)."""
    return sum((i + 1) * 7919 * (p if isinstance(p, int) else sum(map(ord, p))) for i, p in enumerate(parts)) % 1000003


def _pair(n, m, K, d, seed, kind, normed=True):
    """make_pair's float32 layers, normalised by the oracle (what every op but make_norm1 is fed)."""
    v0, v1 = make_pair(n, m, K, d, seed, common=COMMON if kind == "aniso" else 0.0)
    if normed:
        orc = _oracle()
        orc.make_norm1(v0)
        orc.make_norm1(v1)
    return v0, v1


def _norms(v0, v1, seed):
    orc = _oracle()
    rs = np.random.RandomState(seed)
    return orc.compute_norms(v0, v1, 100, rs), orc.compute_norms(v1, v0, 100, rs)


# ------------------------------------------------------------------------------------------------ the cases
# cases_<op>(key, kind, shrink) yields (case name, inputs); ref_<op>(inputs) -> (oracle, float64) on the CPU;
# gpu_<op>(inputs, oracle result) -> the mirror's result (AssertionError for what must be bit-exact).
def cases_norm1(d, kind, shrink=False):
    for K, n in NORM1_ROWS:
        v = _pair(n, n, K, d, _seed("norm1", d, K * n), kind, normed=False)[0]
        if n >= 21:   # a zero row and a row of norm 1e-6: the + 1e-5 of the denominator decides
            v[0, 5] = 0.0
            v[0, 7] *= np.float32(1e-6 / np.sqrt((v[0, 7].astype(np.float64) ** 2).sum()))
        yield "rows%d" % (K * n), dict(v=v)


def ref_norm1(a):
    o = a['v'].copy()
    _oracle().make_norm1(o)
    return o, stage_ref.norm1(a['v'])


def gpu_norm1(a, ref):
    import torch
    from svx.vecalign import dp_utils
    got = a['v'].copy()
    dp_utils.make_norm1(got)
    # the same call on a device tensor with one guard row behind it: rows past the tensor stay untouched
    K, n, d = a['v'].shape
    guard = np.random.RandomState(K * n + d).rand(d).astype(np.float32)
    buf = torch.from_numpy(np.concatenate([a['v'].reshape(K * n, d), guard[None]])).cuda()
    view = buf[:K * n].view(K, n, d)
    assert view.data_ptr() == buf.data_ptr()
    dp_utils.make_norm1(view)
    back = buf.cpu().numpy()
    assert np.array_equal(back[K * n].view(np.uint32), guard.view(np.uint32)), "make_norm1 wrote past the last row"
    assert np.array_equal(back[:K * n].view(np.uint32), got.reshape(K * n, d).view(np.uint32)), "device-tensor call differs from the numpy call"
    return got


def cases_downsample(d, kind, shrink=False):
    for K in DOWN_K:
        for n in DOWN_N:
            yield "K%d_n%d" % (K, n), dict(v=_pair(n, n, K, d, _seed("down", d, K, n), kind)[0])


def ref_downsample(a):
    # h = 1 (n = 2, 3): the mean is the only pair sum, so oracle and float64 give the zero row and the rule's bound is 0
    return _oracle().downsample_vectors(a['v']), stage_ref.downsample(a['v'])


def gpu_downsample(a, ref):
    from svx.vecalign import dp_utils
    return dp_utils.downsample_vectors(a['v'])


def cases_norms(d, kind, shrink=False):
    table = NORMS_CASES + ((NORMS_BIG,) if d == 8 else ())
    for name, K0, n0, K1, n1, ns in table:
        if shrink and name == NORMS_BIG[0]:
            n0 = SHRUNK_ROWS // K0
        v0, v1 = _pair(n0, n1, max(K0, K1), d, _seed("norms", d, name), kind)
        yield name, dict(v0=np.ascontiguousarray(v0[:K0]), v1=np.ascontiguousarray(v1[:K1]), ns=ns, seed=_seed("draw", d, name))


def ref_norms(a):
    orc = _oracle()
    idx = orc.sample_norm_indices(a['v1'].shape[1], a['v1'].shape[0], a['ns'], np.random.RandomState(a['seed']))
    a['idx'] = idx
    return orc.compute_norms(a['v0'], a['v1'], a['ns'], np.random.RandomState(a['seed'])), stage_ref.norms(a['v0'], a['v1'], idx)


@contextlib.contextmanager
def recorded_choice():
    """np.random.choice, recording what it hands out (compute_norms draws from numpy's global stream)."""
    drawn, real = [], np.random.choice

    def choice(*args, **kw):
        r = real(*args, **kw)
        drawn.append(np.array(r))
        return r
    np.random.choice = choice
    try:
        yield drawn
    finally:
        np.random.choice = real


def gpu_norms(a, ref):
    from svx.vecalign import dp_utils
    np.random.seed(a['seed'])
    with recorded_choice() as drawn:
        got = dp_utils.compute_norms(a['v0'], a['v1'], a['ns'])
    assert len(drawn) == len(a['idx']) and all(np.array_equal(x, y) for x, y in zip(drawn, a['idx'])), \
        "the replayed indices are not the ones the wrapper drew"
    return got


def cases_score(d, kind, shrink=False):
    N, M = 70, 61
    v0, v1 = _pair(N, M, 1, d, _seed("score", d), kind)
    n0, n1 = _norms(v0, v1, _seed("score-norms", d))
    assert float(n0.min() + n1.min()) > 0.1   # no epsilon in this formula: normalisers stay away from zero
    for n in SCORE_N + ((SCORE_BIG,) if d in SCORE_BIG_WIDTHS else ()):
        name = "n%d" % n
        if shrink and n == SCORE_BIG:
            n = SHRUNK_ROWS
        rs = np.random.RandomState(_seed("score-idx", d, n))
        xs = np.concatenate([[-1, 0, N - 1, -N], rs.randint(-N, N, n)])[:n].astype(np.int32)
        ys = np.concatenate([[M - 1, -M, 0, -1], rs.randint(-M, M, n)])[:n].astype(np.int32)
        yield name, dict(xs=xs, ys=ys, n0=n0[0], n1=n1[0], v0=v0[0], v1=v1[0])


def ref_score(a):
    out = np.empty(len(a['xs']), np.float32)
    # the oracle indexes with C pointers: it gets the wrapped indices; the float64 side wraps by numpy's own indexing
    _oracle().score_path(np.mod(a['xs'], a['v0'].shape[0]).astype(np.int32), np.mod(a['ys'], a['v1'].shape[0]).astype(np.int32),
                         a['n0'], a['n1'], a['v0'], a['v1'], out)
    return out, stage_ref.score_path(a['xs'], a['ys'], a['n0'], a['n1'], a['v0'], a['v1'])


def gpu_score(a, ref):
    from svx.vecalign import dp_core
    out = np.full(len(a['xs']), np.nan, np.float32)
    dp_core.score_path(a['xs'], a['ys'], a['n0'], a['n1'], a['v0'], a['v1'], out)
    return out


def cases_dense(d, kind, shrink=False):
    for s0, s1 in DENSE_SHAPES:
        v0, v1 = _pair(s0, s1, 3, d, _seed("dense", d, s0, s1), kind)
        n0, n1 = _norms(v0, v1, _seed("dense-norms", d, s0, s1))
        for o0, o1 in DENSE_OFFSETS:
            yield "%dx%d_off%d%d" % (s0, s1, o0, o1), dict(v0=v0, v1=v1, n0=n0, n1=n1, o0=o0, o1=o1)


def ref_dense(a):
    return (_oracle().make_dense_costs(a['v0'], a['v1'], a['n0'], a['n1'], a['o0'], a['o1']),
            stage_ref.dense_costs(a['v0'], a['v1'], a['n0'], a['n1'], a['o0'], a['o1']))


def gpu_dense(a, ref):
    from svx.vecalign import dp_core
    return dp_core.make_dense_costs(a['v0'], a['v1'], a['n0'], a['n1'], a['o0'], a['o1'])


def straight_path(n, m):
    """The unit-step lattice path from (0, 0) to (n, m) closest to the straight line."""
    A = n + m + 1
    xs = [(a * n + (A - 1) // 2) // (A - 1) for a in range(A)]
    return [(x, a - x) for a, x in enumerate(xs)]


def cases_band(key, kind, shrink=False):
    orc = _oracle()
    name, d = key
    types, size = BAND_SETS[name][:2]
    n, m = size or (70, 66)
    K = max(max(x, y) for x, y in types)
    v0, v1 = _pair(n, m, K, d, _seed("band", name, d), kind)
    n0, n1 = _norms(v0, v1, _seed("band-norms", name, d))
    if size:
        path = straight_path(n, m)
    else:   # the search path of the oracle's dense alignment, as test_gpu_ops.test_sparse_ops_other_bands_vs_oracle builds it
        al = orc.dense_traceback(orc.dense_dp(orc.make_dense_costs(v0, v1, n0, n1), 0.4)[1])
        path = orc.search_path(al, False, n, m)
    assert len(path) == n + m + 1
    for W in BAND_W:
        yield "W%d" % W, dict(v0=v0, v1=v1, n0=n0, n1=n1, path=path, types=types, W=W)


def ref_band(a):
    fo, bo = _oracle().make_sparse_costs(a['v0'], a['v1'], a['n0'], a['n1'], a['path'], a['types'], a['W'])
    a['boff'] = bo
    return fo, stage_ref.band_costs(a['v0'], a['v1'], a['n0'], a['n1'], a['path'], bo, a['types'], a['W'])


def gpu_band(a, ref):
    from svx.vecalign import dp_core
    fg, bg = dp_core.make_sparse_costs(a['v0'], a['v1'], a['n0'], a['n1'], a['path'], a['types'], a['W'])
    assert np.array_equal(bg, a['boff']), "b_offset differs from the oracle's"
    return fg


OPS = {"make_norm1": (cases_norm1, ref_norm1, gpu_norm1), "downsample_vectors": (cases_downsample, ref_downsample, gpu_downsample),
       "compute_norms": (cases_norms, ref_norms, gpu_norms), "score_path": (cases_score, ref_score, gpu_score),
       "make_dense_costs": (cases_dense, ref_dense, gpu_dense), "make_sparse_costs": (cases_band, ref_band, gpu_band)}


def key_name(key):
    return "d%d" % key if isinstance(key, int) else "%s_d%d" % key


def key_dim(key):
    return key if isinstance(key, int) else key[1]


def judge(label, got, orc, f64):
    """The rule of the module docstring.  -> (failure text or None, record or None)"""
    got, orc = np.asarray(got), np.asarray(orc)
    if got.shape != f64.shape or orc.shape != f64.shape:
        return "%s: shapes gpu %s oracle %s f64 %s" % (label, got.shape, orc.shape, f64.shape), None
    if got.dtype != np.float32:
        return "%s: result dtype %s" % (label, got.dtype), None
    if not (np.array_equal(np.isinf(got), np.isinf(orc)) and np.array_equal(np.signbit(got[np.isinf(got)]), np.signbit(orc[np.isinf(orc)]))
            and np.array_equal(np.isfinite(got), np.isfinite(f64))):
        return "%s: the pattern of infinite cells differs from the oracle's" % label, None
    e_gpu, e_orc, bound, n = stage_error(got, orc, f64)
    rec = dict(E_gpu=e_gpu, E_orc=e_orc, bound=bound, size=n)
    if not e_gpu <= bound:
        fin = np.isfinite(f64)
        return ("%s: E_gpu %.3e > max(2 E_orc = %.3e, floor 4 * 2^-24 max|f64| = %.3e) over %d values"
                % (label, e_gpu, 2 * e_orc, 4 * U * float(np.abs(f64[fin]).max()), n)), rec
    return None, rec


def run_unit(op, key, kind, records=None):
    """Every case of one (op, key, data kind) on the GPU.  -> list of failure texts"""
    cases, ref, gpu = OPS[op]
    fails = []
    for name, a in cases(key, kind):
        label = "%s %s %s %s" % (op, key_name(key), name, kind)
        o, t = ref(a)
        try:
            g = gpu(a, o)
        except AssertionError as e:
            fails.append("%s: %s" % (label, e))
            continue
        text, rec = judge(label, g, o, t)
        if text:
            fails.append(text)
        if rec is not None and records is not None:
            records.append(dict(op=op, case="%s_%s" % (key_name(key), name), kind=kind, **rec))
    return fails


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.gpu
@pytest.mark.parametrize("op,key,kind", UNITS, ids=["%s-%s-%s" % (o, key_name(k), kd) for o, k, kd in UNITS])
def test_op_matrix(op, key, kind):
    fails = run_unit(op, key, kind)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_downsample_short_inputs():
    """n = 0 and n = 1 have no row pair: the empty shape [K, 0, d] comes back and the entry returns before it reserves
    scratch or launches anything (svx_downsample: h <= 0).  n = 0 hands the entry an empty device tensor, whose address
    is null; before this test it was refused as a null argument."""
    from svx import _lib
    from svx.vecalign import dp_utils
    ctx = _lib.context()
    dp_utils.downsample_vectors(np.ones((1, 2, 8), np.float32))
    before = ctx.lib.svx_scratch_bytes(ctx.h)
    for K in DOWN_K:
        for n in (0, 1):
            want = _oracle().downsample_vectors(np.ones((K, n, 2048), np.float32))
            got = dp_utils.downsample_vectors(np.ones((K, n, 2048), np.float32))
            assert got.shape == want.shape == (K, 0, 2048) and got.dtype == np.float32
    assert ctx.lib.svx_scratch_bytes(ctx.h) == before


DIAG_REFUSED, DIAG_ACCEPTED = 81, 80   # [(i, i) for i in 1 .. k]: two new slots per type, 10 types per 20-slot pass


def diag_types(k):
    return [(i, i) for i in range(1, k + 1)]


@pytest.mark.gpu
def test_band_pass_limit_is_refused():
    """The per-op entry takes what the fused path takes: up to eight passes of the 20-slot shape.  81 types on 81 layers
    per side need nine and are refused before anything is launched; the 80-type list needs eight, is accepted and is
    judged by the rule of this file -- on the same context, right after the refusal."""
    from svx import _lib
    from svx.vecalign import dp_core
    v0, v1 = _pair(20, 22, DIAG_REFUSED, 8, 5, "iid")
    n0, n1 = _norms(v0, v1, 6)
    path = straight_path(20, 22)
    with pytest.raises(_lib.SvxError, match=r"band costs: no kernel shape for 81 alignment types"):
        dp_core.make_sparse_costs(v0, v1, n0, n1, path, diag_types(DIAG_REFUSED), 3)
    a = dict(v0=v0, v1=v1, n0=n0, n1=n1, path=path, types=diag_types(DIAG_ACCEPTED), W=3)
    o, t = ref_band(a)
    text, _ = judge("make_sparse_costs diag80", gpu_band(a, o), o, t)
    assert text is None, text


@pytest.mark.gpu
@pytest.mark.parametrize("W", BAND_W)
def test_band_empty_type_list(W):
    """T = 0: the [0][A][B] cost array has no address; the kernel still validates the path and writes b_offset."""
    from svx.vecalign import dp_core
    v0, v1 = _pair(70, 66, 1, 8, 7, "iid")
    n0, n1 = _norms(v0, v1, 8)
    path = straight_path(70, 66)
    fo, bo = _oracle().make_sparse_costs(v0, v1, n0, n1, path, [], W)
    fg, bg = dp_core.make_sparse_costs(v0, v1, n0, n1, path, [], W)
    assert fg.shape == fo.shape == (0, len(path), 2 * W) and fg.dtype == np.float32
    assert bg.dtype == np.int32 and np.array_equal(bg, bo) and np.array_equal(bo, np.array(path)[:, 1] - W)


@pytest.mark.gpu
@pytest.mark.parametrize("s0,s1", DP_SHAPES)
def test_dense_dp_lds_edges(s0, s1):
    """The ring of 3 (s0 + 1) doubles: 65520 bytes at s0 = 2729 (a plain launch), 65544 at 2730 (the launch first raises
    the kernel's dynamic-LDS limit), 153600 = 150 KiB at 6399 (the largest the entry takes); (5, 7000) is the long side
    on the other axis.  csum and the back-pointers are the oracle's bit for bit."""
    from svx.vecalign import dp_core
    cost = np.random.RandomState(s0 + s1).rand(s0, s1).astype(np.float32)
    csum_o, bp_o = _oracle().dense_dp(cost, 0.37)
    csum_g, bp_g = dp_core.dense_dp(cost, 0.37)
    assert bp_g.dtype == np.int32 and csum_g.dtype == np.float64
    assert np.array_equal(bp_g, bp_o)
    assert np.array_equal(csum_g.view(np.uint64), csum_o.view(np.uint64))


@pytest.mark.gpu
def test_dense_dp_refuses_6400_rows():
    from svx import _lib
    from svx.vecalign import dp_core
    with pytest.raises(_lib.SvxError, match="max 6399"):
        dp_core.dense_dp(np.zeros((6400, 3), np.float32), 0.1)
    assert np.array_equal(dp_core.dense_dp(np.zeros((2, 3), np.float32), 0.0)[1], _oracle().dense_dp(np.zeros((2, 3), np.float32), 0.0)[1])


KNOB_FRACS = (0.0, 0.05, 0.2, 1.0)


def knob_sets():
    """name -> float32 sample set (DeletionKnob(s, 0, max(s)))."""
    out = {}
    for n in (1, 2, 255, 256, 257, 1000003):   # 256 threads sweep the samples: below, at and above one pass, and many
        rs = np.random.RandomState(n)
        out["n%d" % n] = (rs.rand(n) ** 2 * 1.7 + 0.01).astype(np.float32)
    out["all_equal"] = np.full(1000, 0.625, np.float32)
    out["all_zero"] = np.zeros(1000, np.float32)           # res_min >= res_max: the range becomes [0, 1e-4]
    neg = (np.random.RandomState(3).rand(5000) * 2.0).astype(np.float32)
    neg[::7] = -neg[::7] - np.float32(0.01)                # samples below res_min = 0 are outside the histogram
    out["negative"] = neg
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n1", "n2", "n255", "n256", "n257", "n1000003", "all_equal", "all_zero", "negative"])
def test_deletion_knob(name):
    """svx_del_penalty equals the oracle's DeletionKnob exactly.  The all-zero set is the reference's res_min >= res_max
    branch (dp_utils.py:55-57): its range end is the double 0 + 1e-4, which frac = 1.0 returns as it is (before this
    test the kernel returned float32(1e-4) = 9.999999747e-05 there)."""
    from svx.vecalign import dp_utils
    s = knob_sets()[name]
    for frac in KNOB_FRACS:
        want = _oracle().del_penalty_from_scores(s, 0, max(s), frac)
        got = dp_utils.DeletionKnob(s, 0, max(s)).percentile_frac_to_del_penalty(frac)
        assert got == want, (name, frac, got, want)


@pytest.mark.gpu
def test_bad_dimension_is_refused_by_every_op():
    """d = 12 (no multiple of 8) and d = 2056 (above SVX_MAX_DIM) are refused by each of the six continuous ops with the
    `embedding dimension` text, and the context serves a valid call afterwards."""
    from svx import _lib
    from svx.vecalign import dp_core, dp_utils
    for d in (12, 2056):
        v = np.ones((2, 6, d), np.float32)
        n = np.ones((2, 6), np.float32)
        idx = np.arange(4, dtype=np.int32)
        out = np.zeros(4, np.float32)
        calls = (lambda: dp_utils.make_norm1(v.copy()),
                 lambda: dp_utils.downsample_vectors(v),
                 lambda: dp_utils.compute_norms(v, v, 10),
                 lambda: dp_core.score_path(idx, idx, n[0], n[0], v[0], v[0], out),
                 lambda: dp_core.make_dense_costs(v, v, n, n),
                 lambda: dp_core.make_sparse_costs(v, v, n, n, straight_path(6, 6), [(1, 1)], 3))
        for call in calls:
            with pytest.raises(_lib.SvxError, match="embedding dimension %d" % d):
                call()
            ok = np.full((1, 3, 8), 2.0, np.float32)
            dp_utils.make_norm1(ok)
            want = np.full((1, 3, 8), 2.0, np.float32)
            _oracle().make_norm1(want)
            assert np.abs(ok - want).max() < 1e-6


# ------------------------------------------------------------------------------------------------ dump mode
def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", required=True)
    a = ap.parse_args()
    bad, worst = 0, {}
    with open(a.dump, "w") as f:
        for op, key, kind in UNITS:
            records = []
            fails = run_unit(op, key, kind, records)
            for r in records:
                f.write(json.dumps(dict(r, E_gpu=float("%.3e" % r['E_gpu']), E_orc=float("%.3e" % r['E_orc']), bound=float("%.3e" % r['bound'])),
                                   separators=(",", ":")) + "\n")
                ratio = r['E_gpu'] / r['bound'] if r['bound'] > 0 else (0.0 if r['E_gpu'] == 0 else float("inf"))
                if ratio >= worst.get(op, (-1.0, ""))[0]:
                    worst[op] = (ratio, "%s %s: E_gpu %.2e E_orc %.2e bound %.2e" % (r['case'], r['kind'], r['E_gpu'], r['E_orc'], r['bound']))
            f.flush()
            bad += len(fails)
            print("%s %s %s: %d records, %d failures" % (op, key_name(key), kind, len(records), len(fails)), flush=True)
            for t in fails:
                print("  " + t, flush=True)
    for op, (ratio, where) in worst.items():
        print("%s: worst E_gpu / bound %.3f (%s)" % (op, ratio, where))
    print("op matrix: %d units, %d failures" % (len(UNITS), bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
