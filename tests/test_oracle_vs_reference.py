"""Pins the oracle: every intermediate of the oracle's vecalign() equals the REAL reference's,
bit for bit, on seeded inputs.  The reference's results are recorded in tests/golden/reference_records.json
(as sha256 digests of the values the assertions compare; tests/golden/make_golden.py records)."""
import json
import os

import numpy as np
import pytest

from cases import STACK_CASES, STACK_KEYS, digest
from synth import alignment_types, make_pair

RECORDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_records.json")


def records():
    with open(RECORDS) as f:
        return json.load(f)


@pytest.mark.parametrize("N,M,K,d,a,kw", STACK_CASES)
def test_stack_bit_exact(orc, N, M, K, d, a, kw):
    ref = records()["stack"][repr((N, M, K, d, a, kw))]
    v0, v1 = make_pair(N, M, K, d, 1, zero_rows=kw.get("zero_rows", 0))
    types = [tuple(t) for t in records()["types"][str(a)][0]]
    assert types == alignment_types(a)
    W = kw.get("W", int(np.ceil((a - 1) / 2.0)) + 5)
    mf = kw.get("max_full", 300)
    np.random.seed(3)
    so = orc.vecalign(v0.copy(), v1.copy(), types, 0.2, W, mf, 20000, 100)
    assert sorted(str(dep) for dep in so) == sorted(ref)
    for dep in so:
        for key in STACK_KEYS:
            if key not in ref[str(dep)]:
                continue
            assert key in so[dep], (dep, key)
            assert digest(so[dep][key], key) == ref[str(dep)][key], (dep, key)


def test_rng_draw_order_matches_reference():
    """svx.vecalign.dp_utils.draw_indices consumes numpy's global stream exactly like the reference."""
    from svx.vecalign import dp_utils
    ref = records()["rng_draws"]
    np.random.seed(9)
    ni, ki = dp_utils.draw_indices(1100, 1000, 4, 4, 300, 20000, 100)
    flat = np.concatenate([ni, ki]).astype(np.int32)
    assert flat.size == ref["count"]
    assert digest(flat) == ref["sha256"]
