"""Band-edge contact and band doubling on the CPU oracle (tests/contact_ref.py): the facts svx_band_contact and
svx_align_widen are built on, and what they are held to on the GPU (tests/test_gpu_contact.py, test_gpu_widen.py)."""
import ctypes

import numpy as np
import pytest

from around_ref import block_deletion_pair, true_pairs_found
from contact_ref import INT32_MAX, contact, contact_of_stack, end_csum, widen_chain
from dp_ref import straight_stack
from synth import alignment_types, make_pair

TYPES5 = alignment_types(5)


@pytest.fixture(scope="module")
def chains(orc):
    """Per seed 0..2 of block_deletion_pair: (src, doubling chain from the straight band W = 7, coarse-to-fine stack)."""
    out = []
    for seed in range(3):
        v0, v1, src = block_deletion_pair(seed=seed)
        stacks, report = widen_chain(orc, v0, v1, TYPES5, 7, 11)
        c2f = orc.vecalign(v0.copy(), v1.copy(), TYPES5, 0.2, 7, 100, 20000, 100, rng=np.random.RandomState(11))
        out.append((v0, v1, src, stacks, report, c2f))
    return out


def test_doubling_from_the_straight_band(chains):
    """W = 7 -> 14 -> 28: touching nodes 20 / 26 / 40, then 13 / 21 / 5, then none; 55 true pairs in round 0."""
    want_touch = [(20, 13, 0), (26, 21, 0), (40, 5, 0)]
    want_found = [(55, 126, 174), (55, 134, 171), (55, 126, 171)]
    for (v0, v1, src, stacks, report, c2f), touch, found in zip(chains, want_touch, want_found):
        assert [st['a_b_csum'].shape[1] for st in stacks] == [14, 28, 56]
        assert tuple(contact_of_stack(st)[0] for st in stacks) == touch
        assert tuple(true_pairs_found(st['final_alignments'], src) for st in stacks) == found
        assert report == (2, 28, touch[0], 0)
        last = contact_of_stack(stacks[-1])
        assert last[1] == 0 and last[2] > 0 and last[3] == len(stacks[-1]['final_alignments']) + 1


def test_final_spans_are_coarse_to_fine_s(chains):
    for v0, v1, src, stacks, report, c2f in chains:
        assert stacks[-1]['final_alignments'] == c2f[0]['final_alignments']


def test_end_node_cost_never_rises(chains):
    """The new band contains the old path, so the total cost of the returned path cannot rise from round to round."""
    for v0, v1, src, stacks, report, c2f in chains:
        cs = [end_csum(st) for st in stacks]
        assert all(np.isfinite(cs)) and all(b <= a for a, b in zip(cs, cs[1:])) and cs[-1] < cs[0]
    assert [round(end_csum(st), 3) for st in chains[0][3]] == [191.216, 142.688, 118.578]


def test_one_round_from_w20_runs_the_wide_band(orc, chains):
    """W = 20 touches 10 / 7 / 8 nodes; one round at W = 40 (80 cells: the tile sweep on the GPU) clears the edge."""
    for (v0, v1, src, _, _, c2f), touch0 in zip(chains, (10, 7, 8)):
        stacks, report = widen_chain(orc, v0, v1, TYPES5, 20, 11)
        assert report == (1, 40, touch0, 0) and len(stacks) == 2
        assert stacks[-1]['final_alignments'] == c2f[0]['final_alignments']


def test_width_cap_and_round_limit(orc, chains):
    v0, v1 = chains[0][0], chains[0][1]
    assert widen_chain(orc, v0, v1, TYPES5, 7, 11, max_width_over2=14)[1] == (1, 14, 20, 13)
    assert widen_chain(orc, v0, v1, TYPES5, 7, 11, max_rounds=1)[1] == (1, 14, 20, 13)
    assert widen_chain(orc, v0, v1, TYPES5, 7, 11, max_rounds=0)[1] == (0, 7, 20, 20)
    assert widen_chain(orc, v0, v1, TYPES5, 7, 11, max_width_over2=20)[1][:2] == (2, 20)   # 14, then the cap


def test_guard_two_counts_more_than_guard_zero(orc, chains):
    for (v0, v1, src, stacks, _, _), want in zip(chains, (59, 92, 103)):
        g0, g2 = contact_of_stack(stacks[0], 0), contact_of_stack(stacks[0], 2)
        assert g2[0] == want and g2[0] > g0[0] and g2[1] >= g0[1] and g2[2:] == g0[2:]
        assert contact_of_stack(stacks[-1], 2)[0] == 0


def test_healthy_searches_do_not_touch(orc):
    """Six clean pairs: coarse-to-fine (W = 7) keeps 5 cells of clearance, the straight search (W = 16) 10 or 11."""
    for seed in range(6):
        v0, v1 = make_pair(300, 280, 4, 32, seed, deletions=10)
        c2f = orc.vecalign(v0.copy(), v1.copy(), TYPES5, 0.2, 7, 100, 20000, 100, rng=np.random.RandomState(seed))
        got = contact_of_stack(c2f[0])
        assert got[:3] == (0, 0, 5) and got[3] == len(c2f[0]['final_alignments']) + 1
        got = contact_of_stack(straight_stack(orc, v0, v1, TYPES5, 16, seed))
        assert got[:2] == (0, 0) and got[2] in (10, 11)


def test_borders_never_count():
    """A path that hugs a document border: the band's cells beyond the border are no lattice nodes, so that side is not
    real; the other side is 3 cells away.  A band wider than the lattice has no real side at all."""
    n, m, B = 6, 5, 4
    rows = np.array([[i, 1, 0, 0] for i in range(n)] + [[n, 0, j, 1] for j in range(m)])   # along y = 0, then along x = n
    bout = np.zeros(n + m + 3, np.int32)
    bout[n:] = np.arange(m + 3)                     # the band starts on the path: b = 0 everywhere
    got = contact(rows, bout, B, n, m)
    assert got == (0, 0, 3, n + m + 1)
    assert contact(rows, bout, B, n, m, guard=3)[0] > 0
    wide = np.full(n + m + 3, -2, np.int32)
    assert contact(rows, wide, 2 * (n + m), n, m) == (0, 0, INT32_MAX, n + m + 1)
    assert contact(np.zeros((0, 4), np.int64), wide, 2 * (n + m), n, m) == (0, 0, INT32_MAX, 1)


def hand_made(touching, B=6):
    """1-1 rows far from both borders whose node i + 1 touches the low edge iff touching[i]: new_b_offset puts it at b = 0
    or at b = 2.  (Node 0, the origin, has no lattice node beside it on its diagonal: it never touches.)"""
    k = len(touching)
    rows = np.array([[0, 101, 0, 101]] + [[100 + i, 1, 100 + i, 1] for i in range(1, k)])
    size = 400
    bout = np.zeros(2 * size + 3, np.int32)
    for i, t in enumerate(touching):
        bout[2 * (101 + i)] = (101 + i) - (0 if t else 2)
    return rows, bout, B, size, size


@pytest.mark.parametrize("touching, want", [
    ([1, 1, 1, 0, 0, 0, 0], (3, 3)),               # a run at the start
    ([0, 0, 0, 0, 1, 1], (2, 2)),                  # at the end
    ([0, 1, 1, 0, 1, 1, 1, 0, 1], (6, 3)),         # split runs: the longest wins
    ([1, 1, 0, 1, 1], (4, 2)),                     # split over two of the same length
    ([1, 1, 1, 1, 1], (5, 5)),                     # all touching
    ([0, 0, 0], (0, 0)),
])
def test_longest_run(touching, want):
    rows, bout, B, s0, s1 = hand_made(touching)
    got = contact(rows, bout, B, s0, s1)
    assert got[:2] == want and got[3] == len(touching) + 1
    assert got[2] == (0 if any(touching) else 2)
    assert contact(rows, bout, B, s0, s1, guard=2)[:2] == (len(touching), len(touching))


def test_library_exports_the_entries():
    """Fails on a build without the feature, with no GPU."""
    from svx import _lib
    lib = _lib.load()
    assert hasattr(lib, "svx_band_contact") and hasattr(lib, "svx_align_widen")
    assert {"svx_band_contact", "svx_align_widen"} <= set(_lib.EXPORTS)
    assert ctypes.sizeof(_lib.WidenParams) == 16
    assert [f[0] for f in _lib.WidenParams._fields_] == ["guard", "max_width_over2", "max_rounds", "reserved"]
