"""The tile sweep's cost planes against float64 (tests/tile_cost_ref.py): the wide straight search, the dense mode and
SVX_SEARCH_AROUND_WIDE make their costs on the matrix cores and keep none, so the costs are recovered from the level
view's float64 node sums, c^ = csum[x, y] - csum[pred], and checked per type plane: winner costs and one-step
optimality under bound[t] = max(2 E_orc[t], 4 * 2^-24 max |c64[t]|) + 4 * 2^-52 max |csum|.  Every case runs family N
(natural data, iid and with a common component; the pipeline's normalisers) and family T (one pair per probed type with
that type made cheap by caller-supplied normalisers) as one PreparedBatch call each, and asserts on the GPU's own
back-pointers that the probed planes were seen (tile_cost_ref.min_wins).

  A  every instantiation of the dispatcher (svxl_band_tiles_batch), 9 shapes x fp32 / fp16 / bf16, at d = 72 (a slab
     tail in all three storages); the kernel each case selects is in tile_cost_ref._A_SETS, and
     profiles/tile_costs_kernels.txt is the kernel trace of this file, checked against it;
  B  row widths 8 .. 2048 on the LDS-resident shape 0 and on the general shape MS 3;
  C  geometry: a lattice below one tile, a steep path, dense, tile corners, a batch of three sizes, a bent band around
     a block prior.

    python tests/test_gpu_tile_costs.py --dump FILE     (on the GPU box)
writes one JSON line per (case, family) with lists indexed like `type` -- family T: every probed type, from the
probe's own pair; family N: every type that wins anywhere, from the pair (iid / aniso, every size) closest to that
type's bound -- holding E_gpu, E_orc, bound and the win count, and the number of nodes over the one-step optimum's
bound (profiles/tile_cost_errors.jsonl; the per-type lines are grouped so that the file stays readable in a diff)."""
import json
import sys

import pytest

if __name__ == "__main__":   # hand-run: the paths conftest.py sets up for pytest
    import os
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_root, "speech-vecalign_amd"), os.path.join(_root, "oracle"), os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, _p)

import tile_cost_ref as tc

CASES = list(tc.cases())


@pytest.fixture(scope="module")
def farm():
    f = tc.RefFarm(CASES)
    yield f
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_tile_costs(farm, name):
    fails = tc.check_case_gpu(tc.cases()[name], farm.get(name))
    assert not fails, "\n".join(fails[:30])


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", required=True)
    ap.add_argument("--only", default="", help="comma-separated prefixes of case names")
    a = ap.parse_args()
    todo = [c for c in CASES if not a.only or any(c.startswith(p) for p in a.only.split(","))]
    farm = tc.RefFarm(todo)
    bad, worst = 0, (0.0, "")
    try:
        with open(a.dump, "w") as f:
            for name in todo:
                records = []
                fails = tc.check_case_gpu(tc.cases()[name], farm.get(name), records)
                over = {fam: sum(r['c2_over'] for r in records if r['family'] == fam) for fam in ("N", "T")}
                keep = {}   # family N: per type the pair closest to its bound (most wins among pairs that show no cost)
                for r in records:
                    k = (r['family'], tuple(r['type'])) if r['family'] == "N" else (r['family'], r['pair'])
                    if k not in keep or (r['E_gpu'] * keep[k]['bound'], r['wins']) > (keep[k]['E_gpu'] * r['bound'], keep[k]['wins']):
                        keep[k] = r
                records = [r for r in keep.values() if r['family'] == "T" or r['wins'] > 0]
                for fam in ("N", "T"):
                    rs = [r for r in records if r['family'] == fam]
                    line = dict(case=name, family=fam, type=[r['type'] for r in rs], wins=[r['wins'] for r in rs], c2_over=over[fam])
                    for k in ("E_gpu", "E_orc", "bound"):
                        line[k] = [float("%.2e" % r[k]) for r in rs]
                    f.write(json.dumps(line, separators=(",", ":")) + "\n")
                for r in records:
                    if r['bound'] > 0 and r['E_gpu'] / r['bound'] > worst[0]:
                        worst = (r['E_gpu'] / r['bound'], "%s family %s %s pair %d type %s: E_gpu %.2e E_orc %.2e bound %.2e at %d nodes"
                                 % (name, r['family'], r['kind'], r['pair'], tuple(r['type']), r['E_gpu'], r['E_orc'], r['bound'], r['wins']))
                f.flush()
                bad += len(fails)
                top = max((r['E_gpu'] / r['bound'] for r in records if r['bound'] > 0), default=0.0)
                print("%s: %d records, worst E_gpu / bound %.2f, %d failures" % (name, len(records), top, len(fails)), flush=True)
                for t in fails[:30]:
                    print("  " + t, flush=True)
    finally:
        farm.close()
    print("worst E_gpu / bound %.2f (%s)" % worst)
    print("tile costs: %d cases, %d failures" % (len(todo), bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
