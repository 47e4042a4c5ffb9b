"""distributed.SetsPlan on hand-made sample counts, no GPU: the ranks' item ranges are contiguous and cover the whole,
every rank's sample_base is the prefix sum at its first item, and no share exceeds the ideal by as much as one item — the
bound the plan's rule gives: a range ends at the FIRST boundary at which the samples reach its target, so the boundary
before it lies below the target, and the range began at or above its own."""
import numpy as np
import pytest

from edgegraph3d_amd.distributed import SetsPlan

CASES = {
    "plain": [5, 3, 8, 1, 1, 9, 4, 4, 2, 7, 6, 3],
    "zeros_inside": [0, 0, 4, 0, 7, 0, 0, 3, 0, 5, 0],
    "zeros_at_the_ends": [0, 0, 0, 6, 2, 2, 0, 0],
    "one_giant_item": [1, 2, 1, 1000, 1, 2, 1],
    "giant_first": [500, 1, 1, 1, 1],
    "giant_last": [1, 1, 1, 1, 500],
    "all_zero": [0, 0, 0, 0, 0],
    "single_item": [17],
    "no_items": [],
    "equal": [4] * 16,
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("world", [1, 2, 3, 4, 7, 16])
def test_ranges_cover_bases_are_prefix_sums_shares_are_within_one_item(name, world):
    counts = np.asarray(CASES[name], np.int64)
    n, total = len(counts), int(counts.sum())
    prefix = np.concatenate([[0], np.cumsum(counts)])
    plans = [SetsPlan(counts, world, r) for r in range(world)]
    ranges = plans[0].ranges()
    assert len(ranges) == world
    at = 0
    for r, (b, e, base) in enumerate(ranges):
        assert b == at and b <= e <= n, (name, world, r)           # contiguous, in item order
        assert (b, e) == plans[r].item_range() and base == plans[r].sample_base()   # every rank computes the same split
        assert base == int(prefix[b])
        assert plans[r].n_samples() == int(prefix[e] - prefix[b])
        at = e
    assert at == n                                                  # ... and they cover the whole
    if world > n:
        assert sum(1 for b, e, _ in ranges if e == b) >= world - n  # more ranks than items: the surplus ranks are empty
    shares = [int(prefix[e] - prefix[b]) for b, e, _ in ranges]
    assert sum(shares) == total
    biggest = int(counts.max()) if n else 0
    assert max(shares) * world < total + biggest * world or total == 0, (name, world, shares)   # share < ideal + one item
    if name == "one_giant_item" and world >= 2:
        # the giant is one item: it cannot be cut, and nothing else is piled on the rank that takes it beyond its share
        owner = next(r for r, (b, e, _) in enumerate(ranges) if b <= 3 < e)
        assert shares[owner] <= 1000 + 4
    if name == "all_zero":
        sizes = [e - b for b, e, _ in ranges]
        assert max(sizes) - min(sizes) <= 1                         # nothing to balance by: evenly by items


def test_bad_arguments_are_refused():
    for world, rank in ((0, 0), (2, 2), (2, -1)):
        with pytest.raises(ValueError):
            SetsPlan([1, 2], world, rank)
    with pytest.raises(ValueError):
        SetsPlan([1, -2], 2, 0)
