"""Every template instantiation the dispatchers can choose at d = 256 .. 2048, stage by stage.

Each case is ONE svx_align_batch call over three ragged pairs (3-4 pyramid levels with max_size_full_dp = 300, odd
lengths on the way down); every level of every pair (PreparedBatch.level_stack) is compared with
  (a) the oracle's stack: discrete results exact, the DP kernels exact on the GPU's own costs (stage_check.check_discrete),
  (b) the float64 chain on the oracle's discrete choices: E_gpu <= max(2 E_orc, 4 * 2^-24 max|f64|) for every continuous
      stage (stage_check.check_continuous; the rule and its reasons are in stage_check's docstring).
Each case runs on make_pair data as it is ("iid": mean cosine ~ 0) and with a common component ("aniso": mean cosine
~ 0.66 at level 0, where the oracle's own sequential fp32 chain is furthest from the truth).

The "selects" column names what the dispatch code picks for the case (svx_rows.hip pyramid / knob dispatch,
svx_band.hip band_version + shapes, svx_costs.hip); profiles/stage_matrix_kernels.txt is the kernel trace of this
file, checked against it.

    python tests/test_gpu_stage_matrix.py --dump FILE     (on the GPU box)
writes one JSON line per (case, data kind, stage) with, per depth, E_gpu, E_orc, their ratio and the array size of the
pair that comes closest to its bound (lists indexed like `depth`), and prints the worst ratio per stage, for the cases below plus the second storage type of the rows that pytest
runs with one (profiles/stage_errors.jsonl)."""
import json
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # hand-run: the paths conftest.py sets up for pytest
    import os
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_root, "speech-vecalign_amd"), os.path.join(_root, "oracle"), os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, _p)

import stage_check as sc
from synth import alignment_types

SIZES = ((1201, 1153), (2497, 2305), (613, 2111))
COMMON = 1.4   # mean cosine 1.96 / 2.96 = 0.66


def _asym():
    return [(x, y) for x, y in alignment_types(5) if x <= 4 and y <= 2]


# id: (storage, d, K0, K1, types, W, extra make_pair keywords)      # selects
CASES = {
    "bench_bf16_1024": ("bf16", 1024, 4, 4, alignment_types(5), 7, {}),   # pyramid FULL NCH 2, band v3 NK 32, knob 16-bit NCH 2
    "bench_f16_1024": ("f16", 1024, 4, 4, alignment_types(5), 7, {}),
    "bf16_512": ("bf16", 512, 4, 4, alignment_types(5), 7, {}),           # FULL NCH 1, band v3 NK 16
    "bf16_256": ("bf16", 256, 4, 4, alignment_types(5), 7, {}),           # partial NCH 1, band v3 NK 8
    "f16_256": ("f16", 256, 4, 4, alignment_types(5), 7, {}),             # band v3 NK 8, f16
    "f16_512": ("f16", 512, 4, 4, alignment_types(5), 7, {}),             # band v3 NK 16, f16
    "bf16_2048": ("bf16", 2048, 2, 2, alignment_types(3), 6, {}),         # FULL NCH 4, band v2 (d outside v3)
    "bf16_1016": ("bf16", 1016, 4, 4, alignment_types(5), 7, {}),         # last piece partly outside the row, v3 refused (d % 32)
    "bf16_1032": ("bf16", 1032, 4, 4, alignment_types(5), 7, {}),         # NCH bump to 4
    "bf16_520": ("bf16", 520, 4, 4, alignment_types(5), 7, {}),
    "f32_256": ("f32", 256, 4, 4, alignment_types(5), 7, {}),             # FULL NCH 1, level-0 band v2 fp32
    "f32_512": ("f32", 512, 4, 4, alignment_types(5), 7, {}),             # FULL NCH 2
    "f32_1024": ("f32", 1024, 4, 4, alignment_types(5), 7, {}),           # FULL NCH 4
    "f32_2048": ("f32", 2048, 4, 4, alignment_types(5), 7, {}),           # FULL NCH 8
    "f32_264": ("f32", 264, 2, 2, alignment_types(3), 6, {}),             # partial lanes at each NCH
    "f32_1032": ("f32", 1032, 2, 2, alignment_types(3), 6, {}),
    "f32_8": ("f32", 8, 2, 2, alignment_types(3), 6, {}),                 # one 16-byte piece
    "asym_bf16_1024": ("bf16", 1024, 4, 2, _asym(), 7, {}),               # v3 plan with short wt_n rows
    "types15_bf16_1024": ("bf16", 1024, 5, 5, alignment_types(6), 8, {}),  # 15 types, 5 layers: v3 refused -> v2 nslot 12
    "types36_bf16_1024": ("bf16", 1024, 8, 8, alignment_types(9), 9, {}),  # 36 types -> v2 nslot 20, several passes
    "onetype_f32_1024": ("f32", 1024, 1, 1, alignment_types(2), 3, {}),   # one type: v2 {64, 2, 1, 4} at level 0 too
    "zero_rows_bf16_1024": ("bf16", 1024, 4, 4, alignment_types(5), 7, {"zero_rows": 6}),   # PAD candidates: stage values only
    "deletions_bf16_1024": ("bf16", 1024, 4, 4, alignment_types(5), 7, {"deletions": 40}),
}
DUMP_ONLY = {
    "f16_2048": ("f16", 2048, 2, 2, alignment_types(3), 6, {}),
}
KINDS = ("iid", "aniso")
SINGLE_KIND = {"zero_rows_bf16_1024": "aniso", "deletions_bf16_1024": "iid"}
PARAMS = [(c, k) for c in CASES for k in KINDS if SINGLE_KIND.get(c, k) == k]


def jobs_of(case, kind, table=None):
    store, d, k0, k1, types, W, extra = (table or CASES)[case]
    base = 1000 * (sorted({**CASES, **DUMP_ONLY}).index(case) + 1)
    return [dict(n=n, m=m, k0=k0, k1=k1, d=d, store=store, types=types, W=W, params=sc.params(),
                 data_seed=base + i, seed=base + 500 + i, common=COMMON if kind == "aniso" else 0.0, **extra)
            for i, (n, m) in enumerate(SIZES)]


def run_case(orc, pool, case, kind, records=None, table=None):
    jobs = jobs_of(case, kind, table)
    _, res, stacks = sc.run_gpu(jobs)
    refs = pool.get((case, kind), jobs)
    fails = []
    for i, (ref, f64) in enumerate(refs):
        label = "%s/%s pair %d (%d x %d)" % (case, kind, i, jobs[i]['n'], jobs[i]['m'])
        mine = [] if records is not None else None
        fails += sc.check_continuous(stacks[i], ref, f64, label, mine)
        for r in mine or []:
            records.append(dict(r, pair=i))
        fails += sc.check_discrete(orc, stacks[i], res[i], ref, label, spans="zero_rows" not in jobs[i])
    return fails


@pytest.fixture(scope="module")
def pool():
    p = sc.RefPool(sc.pool_workers())
    p.plan([((c, k), jobs_of(c, k)) for c, k in PARAMS])
    yield p
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case,kind", PARAMS)
def test_stage_matrix(orc, pool, case, kind):
    fails = run_case(orc, pool, case, kind)
    assert not fails, "\n".join(fails)


def main():
    import argparse
    import oracle
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", required=True)
    a = ap.parse_args()
    table = {**CASES, **DUMP_ONLY}
    todo = [(c, k) for c in table for k in KINDS if SINGLE_KIND.get(c, k) == k]
    pool = sc.RefPool(sc.pool_workers())
    pool.plan([((c, k), jobs_of(c, k, table)) for c, k in todo])
    bad, summary = 0, {}
    try:
        with open(a.dump, "w") as f:
            for case, kind in todo:
                records = []
                fails = run_case(oracle, pool, case, kind, records, table)
                worst = {}   # per (stage, depth): the pair closest to its bound
                for r in records:
                    k = (r['stage'], r['depth'])
                    if k not in worst or r['E_gpu'] * worst[k]['bound'] > worst[k]['E_gpu'] * r['bound']:
                        worst[k] = r
                for stage in sc.CONTINUOUS:
                    rs = [worst[k] for k in sorted(worst) if k[0] == stage]
                    f.write(json.dumps(dict(case=case, kind=kind, stage=stage, depth=[r['depth'] for r in rs],
                                            E_gpu=[float("%.2e" % r['E_gpu']) for r in rs], E_orc=[float("%.2e" % r['E_orc']) for r in rs],
                                            ratio=[round(r['E_gpu'] / r['E_orc'], 2) if r['E_orc'] > 0 else None for r in rs],
                                            size=[r['size'] for r in rs]), separators=(",", ":")) + "\n")
                    for r in rs:
                        top = summary.setdefault(stage, [(0.0, ""), (0.0, "")])
                        where = "%s/%s pair %d depth %d: E_gpu %.2e E_orc %.2e" % (case, kind, r['pair'], r['depth'], r['E_gpu'], r['E_orc'])
                        if r['E_orc'] > 0 and r['E_gpu'] / r['E_orc'] > top[0][0]:
                            top[0] = (r['E_gpu'] / r['E_orc'], where)
                        if r['bound'] > 0 and r['E_gpu'] / r['bound'] > top[1][0]:
                            top[1] = (r['E_gpu'] / r['bound'], where)
                f.flush()
                bad += len(fails)
                print("%s/%s: %d stage records, %d failures" % (case, kind, len(worst), len(fails)), flush=True)
                for t in fails:
                    print("  " + t, flush=True)
    finally:
        pool.close()
    for stage, (by_ratio, by_bound) in summary.items():
        print("%s: worst E_gpu / E_orc %.2f (%s); worst E_gpu / bound %.2f (%s)" % ((stage,) + by_ratio + by_bound))
    print("stage matrix: %d cases, %d failures" % (len(todo), bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
