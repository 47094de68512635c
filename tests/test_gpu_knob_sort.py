"""svx_knob_sort on the GPU (include/svx.h): the counting sort of the sampled (x, y) pairs by source row, the device code
that svx_align_batch runs per (pair, level).  Every case checks four properties, all exact:

  * kstart is the exclusive prefix sum of bincount(clamp(kx), n), and kstart[n] == kn;
  * korder is a permutation of 0..kn-1;
  * clamp(kx[korder[p]]) is non-decreasing and agrees with kstart;
  * kys[p] == clamp(ky[korder[p]]).

The order inside one source row is unspecified (it is the arrival order of the LDS atomics), so korder is never compared
with a reference permutation.  The scatter is staged in LDS while (n + 1 + kn) * 4 bytes fit SVX_KNOB_SORT_STAGE_LDS and
goes straight to memory above that; the last two shapes sit on the two sides of that edge."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def stage_edge(kn):
    """The largest n whose cnt[n + 1] + ord[kn] still fit the staging LDS."""
    from svx import _lib
    return _lib.SVX_KNOB_SORT_STAGE_LDS // 4 - 1 - kn


# (kn, n, m, what)
SHAPES = [
    (20000, 4096, 4096, "workload"),
    (20000, 3, 5, "thousands_per_row"),
    (100, 600, 600, "mostly_empty_rows"),
    (1, 1, 1, "smallest"),
    (255, 256, 256, "below_thread_count"),
    (257, 256, 256, "above_thread_count"),
    (20000, 100, 100, "one_row_holds_all"),
    (20000, "last_staged", 64, "last_staged_n"),
    (20000, "first_direct", 64, "first_direct_n"),
]


def resolve(kn, n, m):
    if n == "last_staged":
        n = stage_edge(kn)
    elif n == "first_direct":
        n = stage_edge(kn) + 1
    return kn, n, m


def draw(kn, n, m, what, out_of_range, seed):
    rng = np.random.RandomState(seed)
    if what == "one_row_holds_all":
        kx = np.full(kn, 37, np.int32)
    else:
        kx = rng.randint(0, n, size=kn).astype(np.int32)
    ky = rng.randint(0, m, size=kn).astype(np.int32)
    if out_of_range:
        # indices outside [0, n) / [0, m) on both sides: -1, n, n + 5 (a fifth of the samples, at least one of each
        # where the list is long enough)
        for arr, size in ((kx, n), (ky, m)):
            bad = np.array([-1, size, size + 5], np.int32)
            at = rng.permutation(kn)[:max(min(kn, 3), kn // 5)]
            arr[at] = bad[np.arange(len(at)) % 3]
    return kx, ky


def run_sort(kx, ky, n, m):
    import torch
    from svx import _lib
    from svx.vecalign.dp_utils import _p
    ctx = _lib.context()
    kn = len(kx)
    dkx, dky = torch.from_numpy(kx).to(ctx.tdev), torch.from_numpy(ky).to(ctx.tdev)
    korder = torch.full((kn,), -7, dtype=torch.int32, device=ctx.tdev)
    kys = torch.full((kn,), -7, dtype=torch.int32, device=ctx.tdev)
    kstart = torch.full((n + 1,), -7, dtype=torch.int32, device=ctx.tdev)
    ctx.check(ctx.lib.svx_knob_sort(ctx.h, _p(dkx), _p(dky), kn, n, m, _p(korder), _p(kys), _p(kstart)))
    ctx.sync()
    return korder.cpu().numpy(), kys.cpu().numpy(), kstart.cpu().numpy()


def check(kx, ky, n, m, korder, kys, kstart):
    kn = len(kx)
    cx, cy = np.clip(kx, 0, n - 1), np.clip(ky, 0, m - 1)
    want = np.zeros(n + 1, np.int64)
    want[1:] = np.cumsum(np.bincount(cx, minlength=n))
    assert np.array_equal(kstart, want), "kstart is not the exclusive prefix sum of the row counts"
    assert kstart[n] == kn
    assert np.array_equal(np.sort(korder), np.arange(kn)), "korder is not a permutation of 0..kn-1"
    rows = cx[korder]
    assert np.all(np.diff(rows) >= 0), "source rows along korder decrease somewhere"
    # position p belongs to the row whose [kstart[x], kstart[x + 1]) holds it
    assert np.array_equal(rows, np.searchsorted(want, np.arange(kn), side="right") - 1), "korder disagrees with kstart"
    assert np.array_equal(kys, cy[korder]), "kys is not the clamped ky of korder"


@pytest.mark.parametrize("out_of_range", [False, True], ids=["in_range", "out_of_range"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[3] for s in SHAPES])
def test_knob_sort(shape, out_of_range):
    kn, n, m = resolve(*shape[:3])
    kx, ky = draw(kn, n, m, shape[3], out_of_range, seed=1234 + kn + n)
    check(kx, ky, n, m, *run_sort(kx, ky, n, m))


def test_stage_edge_is_the_documented_one():
    """The two edge shapes really sit on the two sides of the rule of include/svx.h, and both histograms fit."""
    from svx import _lib
    n = stage_edge(20000)
    assert (n + 1 + 20000) * 4 <= _lib.SVX_KNOB_SORT_STAGE_LDS < (n + 2 + 20000) * 4
    assert (n + 2) * 4 <= 150 * 1024
