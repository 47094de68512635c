"""tile_cost_ref.py without a GPU: the two checks pass on the oracle's own tables, the inputs of every case show the
planes they are meant to show, and the checks can fail -- each of three faults put into one cost plane of the oracle
before its DP is flagged for every probed type.  The CPU side of a case runs in tile_cost_ref.RefFarm (spawn pool)."""
import multiprocessing
import os

import numpy as np
import pytest

import stage_ref
import tile_cost_ref as tc
from synth import alignment_types

CASES = list(tc.cases())
INJECTED = [(c['name'], k) for c in tc.injection_cases() for k in tc.INJECTIONS]


@pytest.fixture(scope="module")
def farm():
    f = tc.RefFarm(CASES, ahead=16, self_check=True, keep_data=False)
    yield f
    f.close()


@pytest.fixture(scope="module")
def injections():
    pool = multiprocessing.get_context("spawn").Pool(max(1, min(len(INJECTED), 16, (os.cpu_count() or 2) - 1)))
    by_name = {c['name']: c for c in tc.injection_cases()}
    jobs = {(n, k): pool.apply_async(tc.injected, (by_name[n], k)) for n, k in INJECTED}
    yield jobs
    pool.terminate()
    pool.join()


def test_costs_from_dots_is_band_costs(orc):
    """c64 as the checks evaluate it (stored dots, then the cost expression) is stage_ref.band_costs bit for bit."""
    case = tc.cases()["A_a5_bf16"]
    pair = tc.case_pairs(case)['N'][1]
    v0, v1 = tc.embeddings(case, *pair['data'])
    o = tc.oracle_pair(orc, case, pair, v0, v1, case['W'])
    v0n, v1n = stage_ref.norm1(v0), stage_ref.norm1(v1)
    n0, n1 = tc.f64_norms(orc, case, pair, v0n, v1n)
    dots, xx, yy = tc.band_dots(v0n, v1n, o['path'], o['b_offset'], case['types'], case['W'])
    want = stage_ref.band_costs(v0n, v1n, n0, n1, o['path'], o['b_offset'], case['types'], case['W'])
    assert np.array_equal(tc.costs_from_dots(dots, xx, yy, n0, n1, case['types']), want)
    # the oracle's normalisers are the float64 ones within a few fp32 ulps: the draws were replayed in its order
    assert np.abs(o['n0'] - n0).max() < 1e-6 and np.abs(o['n1'] - n1).max() < 1e-6


@pytest.mark.parametrize("name", CASES)
def test_oracle_tables_and_input_conditions(farm, name):
    """On the oracle's own tables: c^ is the oracle's fp32 cost within the float64 term and its DP is one-step optimal
    on its own costs with no allowance; both checks pass against c64 under bound[t]; and the case shows what it is meant
    to show -- in every family-T pair the probed type wins at >= min_wins general nodes, in family N five types do."""
    ref = farm.get(name)
    case = tc.cases()[name]
    assert len(ref['N']) == 2 * len(case['sizes']) and len(ref['T']) == len(tc.probed_types(case['types']))
    fails = [f for fam in ("N", "T") for r in ref[fam] for f in r['own_fails'] + r['orc_fails'] + r['cond_fails']]
    assert not fails, "\n".join(fails[:20])
    for r in ref['T']:   # E on the oracle's tables is E_orc restricted to the winners
        rec = r['orc_records'][r['probe']]
        assert rec['E'] <= r['E_orc'][r['probe']] + (rec['bound'] - tc.bounds(r['E_orc'], r['cmax'])[r['probe']])


@pytest.mark.parametrize("name,kind", INJECTED)
def test_injected_faults_are_flagged(injections, name, kind):
    """A relative error of 2^-18, the neighbouring overlap layer, and 32 rows shifted by one cell, each in the probed
    plane alone: check 1 or check 2 is over its bound for every probed type."""
    out = injections[(name, kind)].get()
    assert len(out) >= 10
    missed = [t for t, c1, c2 in out if not (c1 or c2)]
    assert not missed, "%s / %s: not flagged for types %s" % (name, kind, missed)


def test_probed_subsets():
    for a in (12, 16):
        types = alignment_types(a)
        pick = tc.probed_types(types)
        assert 40 <= len(pick) < len(types) and pick[0] == 0 and pick[-1] == len(types) - 1 and pick == sorted(set(pick))
        for side in (0, 1):
            for layer in range(1, a):
                users = [k for k, ty in enumerate(types) if ty[side] == layer]
                assert len([k for k in pick if k in users]) >= min(2, len(users))
    assert tc.probed_types(alignment_types(10)) == list(range(45))


def test_case_table_covers_every_instantiation():
    """9 shapes x 3 storages: the kernel each case expects, and the kernel trace of the GPU module
    (profiles/tile_costs_kernels.txt) holds exactly these, two launches per case (family N, family T)."""
    import collections
    want = collections.Counter()
    for c in tc.cases().values():
        want[c['shape']] += 2
    assert len(want) == 27
    got = {}
    with open(os.path.join(os.path.dirname(__file__), "..", "profiles", "tile_costs_kernels.txt")) as f:
        for line in f:
            if not line.startswith("#") and "k_band_tiles" in line:
                calls, kernel = line.split(None, 1)
                got[kernel.strip()] = int(calls)
    assert got == dict(want)
    from dp_ref import many_to_one_types
    assert max(x for x, _ in many_to_one_types(20)) > 15      # int32 back-pointers
