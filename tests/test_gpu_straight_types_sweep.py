"""24-case slice of the randomised sweep of tests/fuzz_straight_types.py: straight search with -a 7..16 and
--many_to_one 9..100 (the general tile shape), bands of 33 cells up to the dense mode, all three storage types,
deletions and zero rows, against the oracle's straight path.  Exact ties and penalty knife-edges are counted apart."""
import pytest

pytestmark = pytest.mark.gpu


def test_straight_types_sweep_slice():
    from fuzz_straight_types import run
    bad, _, _ = run(24, seed=2026, max_size=200)
    assert bad == 0
