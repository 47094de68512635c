"""The reference side of tests/test_gpu_op_matrix.py, on the CPU: a broken oracle call or float64 restatement must not
make the GPU test vacuous.  The cases are the GPU file's own tables (one list, imported); the two largest row counts
(compute_norms over 33000 rows, score_path over 70001 samples) run with a few hundred rows here.

  1. The oracle agrees with the float64 restatement: E_orc <= 64 * 2^-24 * sqrt(d) * max|f64|.  This is the loose
     sanity bound as stated, kept and not tightened: the sequential-sum bound (d * 2^-24 per dot product, divided by
     the cost's denominator) is LARGER than it at every d >= 64 for these denominators, so it would check less; the
     statistical sqrt(d) form is what an fp32 chain over d terms shows in practice.  It bounds the reference, not a kernel.
  2. stage_ref.dense_costs(..., offset0, offset1) is, on offsets (0, 0), the function it was before it took offsets.
  3. For every continuous case the rule's bound max(2 E_orc, floor) is at most 1e-4 * max|f64|, so the rule cannot pass
     a kernel that drops a 16-byte piece or a whole chunk of a row.  Shown once per op (d = 264 and 2048, both data
     kinds): the oracle run on inputs whose rows lost their last four floats violates the rule.  No kernel is involved."""
import numpy as np
import pytest

import stage_ref
import test_gpu_op_matrix as m
from stage_check import U, stage_error

CPU_UNITS = [(op, key, kind) for op, key, kind in m.UNITS]


@pytest.mark.parametrize("op,key,kind", CPU_UNITS, ids=["%s-%s-%s" % (o, m.key_name(k), kd) for o, k, kd in CPU_UNITS])
def test_reference_side_of_every_case(op, key, kind):
    cases, ref, _ = m.OPS[op]
    d, seen = m.key_dim(key), 0
    for name, a in cases(key, kind, shrink=True):
        o, t = ref(a)
        label = "%s %s %s %s" % (op, m.key_name(key), name, kind)
        assert o.dtype == np.float32 and o.shape == t.shape and t.dtype == np.float64, label
        assert np.array_equal(np.isfinite(o), np.isfinite(t)) and not np.isnan(t).any(), label
        e_same, e_orc, bound, n = stage_error(o, o, t)
        assert e_same == e_orc and n > 0, label
        top = float(np.abs(t[np.isfinite(t)]).max())
        assert e_orc <= 64 * U * np.sqrt(d) * top, (label, e_orc, top)
        assert bound <= 1e-4 * top, (label, bound, top)
        if op == "make_dense_costs" and (a['o0'], a['o1']) == (0, 0):
            v0, v1 = a['v0'].astype(np.float64), a['v1'].astype(np.float64)
            old = 2.0 * (1.0 - np.matmul(v0[0], v1[0].T)) / ((1e-6 + a['n0'].astype(np.float64)[0][:, None]) + a['n1'].astype(np.float64)[0][None, :])
            assert np.array_equal(t, old) and np.array_equal(t, stage_ref.dense_costs(a['v0'], a['v1'], a['n0'], a['n1'])), label
        if op == "downsample_vectors" and a['v'].shape[1] // 2 == 1:   # h = 1: the mean is the only row
            assert not o.any() and not t.any(), label
        seen += 1
    assert seen >= 3


def test_case_tables_cover_what_the_matrix_promises():
    assert set(m.WIDTHS) == {8, 256, 264, 512, 520, 1024, 1032, 2048}
    assert sorted(K * n for K, n in m.NORM1_ROWS) == [1, 63, 64, 65, 129]
    assert sorted({n // 2 for n in m.DOWN_N}) == [1, 32, 33, 64, 65]
    assert m.NORMS_BIG[1] * m.NORMS_BIG[2] == 33000 and m.NORMS_BIG[1] * m.NORMS_BIG[2] > 4 * 8192
    assert m.SCORE_BIG > 4 * 16384
    assert {(s, d) for s, d in m.BAND_KEYS if d == 264} == {(s, 264) for s in m.BAND_SETS}
    assert {m.BAND_SETS[s][2] for s, _ in m.BAND_KEYS} == {m.R64, m.R32_8, m.R32_12, m.R32_20}
    assert len(m.alignment_types(11)) == 55
    assert len(m.alignment_types(10)) == 45 and len(m.alignment_types(7)) == 21
    for s0, _ in m.DP_SHAPES[:2]:
        assert (3 * (s0 + 1) * 8 > 64 * 1024) == (s0 == 2730)
    assert 3 * 6400 * 8 == 150 * 1024


SHAPES = (m.R64, m.R32_8, m.R32_12, m.R32_20)   # choose_variant's options, in its order
MAXPASS, WAVES = 8, 4                            # B2_MAXPASS, B2_WAVES


def make_plan(types, tpp, nslot_max):
    """svx_band.hip make_plan: consecutive types are packed into a pass while they fit its type and slot limits.
    -> [(types in the pass, slots in use, what ended it: 'types' / 'slots' / 'end')] or None past MAXPASS passes."""
    passes, t = [], 0
    while t < len(types):
        if len(passes) >= MAXPASS:
            return None
        xs, ys, nt, why = set(), set(), 0, 'end'
        while t < len(types):
            if nt >= tpp:
                why = 'types'
                break
            x, y = types[t]
            if len(xs | {x}) + len(ys | {y}) > nslot_max:
                why = 'slots'
                break
            xs.add(x)
            ys.add(y)
            nt += 1
            t += 1
        if nt == 0:
            return None
        passes.append((nt, len(xs) + len(ys), why))
    return passes


def choose_variant(types):
    """svx_band.hip choose_variant -> ((ROWS, NSLOT, UPW, S), passes of make_plan) or None: the first shape that takes the
    set in one pass, else whatever plan the last shape has."""
    kx, ky = max([0] + [x for x, _ in types]), max([0] + [y for _, y in types])
    for i, shape in enumerate(SHAPES):
        rows, nslot, upw, _ = shape
        tpp = WAVES * upw // (rows // 16)
        if i < len(SHAPES) - 1 and (kx + ky > nslot or len(types) > tpp):
            continue
        plan = make_plan(types, tpp, nslot)
        if plan is not None:
            return shape, plan
    return None


def test_band_sets_select_the_shapes_the_table_names():
    seen = set()
    for name, (types, _, shape, npass) in m.BAND_SETS.items():
        got = choose_variant(types)
        assert got is not None and got[0] == shape and len(got[1]) == npass, (name, got)
        seen.add(shape)
    assert seen == set(SHAPES)
    ends = {name: [why for _, _, why in choose_variant(m.BAND_SETS[name][0])[1]] for name in ("t7", "t10", "t11", "diag12")}
    assert ends["t7"] == ['types', 'end'] and ends["t10"] == ['types', 'types', 'end'] and ends["t11"] == ['types'] * 3 + ['end']
    assert ends["diag12"] == ['slots', 'end']
    assert choose_variant([]) == (m.R64, [])       # T = 0: the first shape, no pass


def test_band_path_lengths_sit_on_the_chunk_edges():
    """Fixed chunks of lim + 1 = ROWS - min(2 W, 16) + 1 path points: the 32-row and the 64-row shape each see a path one
    short of, equal to and one over a whole number of chunks (at W = 9 and 40, where a workgroup has 16 band cells)."""
    for names, rows in ((("len135", "len136", "t4"), 32), (("len146", "len147", "len148"), 64)):
        rest = []
        for name in names:
            types, size, shape, _ = m.BAND_SETS[name]
            n, mm = size or (70, 66)
            assert shape[0] == rows
            rest.append((n + mm + 1) % (rows - 16 + 1))
        assert rest == [rows - 16, 0, 1], (names, rest)


def test_pass_limit_edge():
    assert choose_variant(m.diag_types(m.DIAG_REFUSED)) is None
    shape, plan = choose_variant(m.diag_types(m.DIAG_ACCEPTED))
    assert shape == m.R32_20 and [p[:2] for p in plan] == [(10, 20)] * 8


def test_every_set_of_the_retired_kernel_has_a_plan():
    """What the first band-cost kernel took -- at most 18 overlap layers in all, at most 128 types -- is always planned:
    no pass over <= 18 layers can run out of the 20 slots, so passes end at 16 types only and ceil(T / 16) <= 8."""
    rs = np.random.RandomState(18)
    sets = []
    for kx in range(1, 18):
        ky = 18 - kx
        grid = [(x, y) for x in range(1, kx + 1) for y in range(1, ky + 1)]
        worst = (grid * (128 // len(grid) + 1))[:128]           # every layer of both sides, the most types
        sets += [worst, worst[::-1], [(kx, ky)] * 128]
        for _ in range(20):
            n = int(rs.randint(1, 129))
            sets.append([(int(rs.randint(1, kx + 1)), int(rs.randint(1, ky + 1))) for _ in range(n)])
    for types in sets:
        got = choose_variant(types)
        assert got is not None, types
        plan = got[1]
        assert sum(nt for nt, _, _ in plan) == len(types) and len(plan) <= MAXPASS
        if got[0] == m.R32_20:
            assert all(why != 'slots' for _, _, why in plan) and len(plan) == -(-len(types) // 16)


def _drop_last_piece(a, keys):
    b = dict(a)
    for k in keys:
        v = a[k].copy()
        v[..., -4:] = 0.0
        b[k] = v
    return b


ROW_INPUTS = {"make_norm1": ("v",), "downsample_vectors": ("v",), "compute_norms": ("v0", "v1"), "score_path": ("v0", "v1"),
              "make_dense_costs": ("v0", "v1"), "make_sparse_costs": ("v0", "v1")}


@pytest.mark.parametrize("kind", m.KINDS)
@pytest.mark.parametrize("d", [264, 2048])
@pytest.mark.parametrize("op", m.CONTINUOUS_OPS)
def test_rule_catches_a_dropped_piece(op, d, kind):
    """A kernel that skipped the last 16-byte piece of every row computes what the oracle computes on rows whose last
    four floats are zero; against the float64 value of the intact rows that breaks the rule in every case whose result
    depends on that piece at all."""
    cases, ref, _ = m.OPS[op]
    key = d if op != "make_sparse_costs" else ("t4", d if d == 264 else 2048)
    seen = 0
    for name, a in cases(key, kind, shrink=True):
        o, t = ref(a)
        broken, t_broken = ref(_drop_last_piece(a, ROW_INPUTS[op]))
        if np.array_equal(t_broken, t):   # the piece does not reach the result: all-zero layers, downsample's h = 1
            continue
        e_bad, e_orc, bound, _ = stage_error(broken, o, t)
        assert e_bad > bound, (op, name, kind, e_bad, bound)
        seen += 1
    assert seen >= 3
