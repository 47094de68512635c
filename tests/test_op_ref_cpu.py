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
    assert {m.BAND_SETS[s][3] for s, _ in m.BAND_KEYS} == {(6, 4), (6, 2), (12, 2), (8, 1), (14, 1), (3, 2), (2, 1), (6, 1)}
    assert len(m.alignment_types(10)) == 45 and len(m.alignment_types(7)) == 21
    for s0, _ in m.DP_SHAPES[:2]:
        assert (3 * (s0 + 1) * 8 > 64 * 1024) == (s0 == 2730)
    assert 3 * 6400 * 8 == 150 * 1024


def band_plan(types, sw_max=4):
    """svx_costs.hip band_plan / BAND_DISPATCH restated for what decides the instantiation of these sets: staging pieces
    per thread, the slab widths' layer / type limits (the LDS limits bind later than those for every set here)."""
    kx, ky, T = max(x for x, _ in types), max(y for _, y in types), len(types)
    for sw in (4, 2, 1):
        if sw > sw_max:
            continue
        npt = -(-(kx + ky) * 48 * 8 * sw // 512)
        if sw == 4 and (T > 2 or kx + ky > 2):
            continue
        if sw == 2 and npt > 12:
            continue
        if npt > 14:
            return None
        if sw == 4:
            return 6, 4
        if sw == 2:
            return (3 if npt <= 3 else 6 if npt <= 6 else 12), 2
        return (2 if npt <= 2 else 6 if npt <= 6 else 8 if npt <= 8 else 14), 1


def test_band_sets_select_the_instantiations_the_table_names():
    for name, (types, sw, _, inst) in m.BAND_SETS.items():
        assert band_plan(types, int(sw) if sw else 4) == inst, name
    assert band_plan(m.alignment_types(11)) is None


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
