"""The numpy truth of the bit tile's tests (tests/exact_truth_bits.py) held to the oracle's b1 distances, so that it cannot drift from
the pinned arithmetic, and the data held to the tie conditions that make the tests worth running: no GPU."""
import numpy as np
import pytest

from oracle import oraclebind
from tests import exact_truth_bits as bits

# the share of queries with equal distances at ranks k and k + 1 (n = 5003, 300 queries, k = 10), as computed when the data were chosen
STATED = {(8, "hamming"): 0.99, (72, "hamming"): 0.88, (128, "hamming"): 0.90, (136, "hamming"): 0.87, (1024, "hamming"): 0.65,
          (8, "tanimoto"): 0.99, (72, "tanimoto"): 0.53, (128, "tanimoto"): 0.32, (136, "tanimoto"): 0.32, (1024, "tanimoto"): 0.05}


@pytest.mark.parametrize("metric", bits.METRICS)
@pytest.mark.parametrize("ndim", [8, 72, 136])
def test_the_truth_carries_the_oracles_bits(metric, ndim):
    rows, queries = bits.data(ndim)
    truth = bits.truth(metric, ndim)
    rng = np.random.default_rng(ndim)
    pairs = [(int(q), int(r)) for q, r in zip(rng.integers(0, len(queries), 40), rng.integers(0, len(rows), 40))]
    if ndim == 8:  # … and the pairs that divide 0 by 0, or by little
        empty = np.flatnonzero(~rows.any(axis=1))
        pairs += [(len(queries) - 1, int(empty[0])), (len(queries) - 1, int(np.flatnonzero(rows.any(axis=1))[0])), (0, int(empty[-1]))]
    for q, r in pairs:
        want = np.float32(oraclebind.distance(queries[q], rows[r], metric, "b1", ndim))
        got = truth.exact[q, r]
        assert (np.isnan(want) and np.isnan(got)) or want.view(np.uint32) == got.view(np.uint32), (metric, ndim, q, r, want, got)


@pytest.mark.parametrize("ndim", [8, 72, 128, 136, 1024])
def test_ties_at_rank_k_are_the_rule_for_hamming(ndim):
    share = bits.truth("hamming", ndim).tie_share(bits.K)
    print(f"hamming, {ndim} dimensions: {share:.2f} of the queries tie at ranks k, k + 1 (stated: {STATED[ndim, 'hamming']})")
    assert share >= 0.6, "below this share a wrong tie order could go unseen"


@pytest.mark.parametrize("metric", ["tanimoto", "sorensen"])
@pytest.mark.parametrize("ndim", [8, 72, 128, 136])
def test_ties_at_rank_k_are_frequent_for_the_quotients(metric, ndim):
    share = bits.truth(metric, ndim).tie_share(bits.K)
    print(f"{metric}, {ndim} dimensions: {share:.2f} of the queries tie at ranks k, k + 1 (stated: {STATED[ndim, 'tanimoto']})")
    assert share >= 0.25, "below this share a wrong tie order could go unseen"


def test_the_short_rows_bring_empty_sets_and_nan_distances():
    rows, queries = bits.data(8)
    assert int((~rows.any(axis=1)).sum()) == 25 and not queries[-1].any()
    for metric in ("tanimoto", "sorensen"):
        truth = bits.truth(metric, 8)
        assert int(np.isnan(truth.exact[-1]).sum()) == 25 and not np.isnan(truth.exact[:-1][queries[:-1].any(axis=1)]).any()
        first = truth.order(bits.K)[-1]
        assert np.isnan(truth.exact[-1, first]).all() and np.all(np.diff(first) < 0), "NaN first, the later slot first among them"
    assert not np.isnan(bits.truth("hamming", 8).exact).any()


def test_the_order_is_nan_first_then_distance_then_the_later_slot():
    rows = np.array([[0b1000_0000], [0], [0b1100_0000], [0], [0b1000_0000]], dtype=np.uint8)
    queries = np.array([[0], [0b1000_0000]], dtype=np.uint8)
    truth = bits.BitsTruth("tanimoto", rows, queries)
    assert truth.order(5)[0].tolist() == [3, 1, 4, 2, 0]  # 0 / 0 twice, then 1 − 0 / n three times
    assert truth.order(5)[1].tolist() == [4, 0, 2, 3, 1]  # 0, 0, 0.5, 1, 1
    assert bits.BitsTruth("tanimoto", rows, queries, allowed=[True, False, True, True, False]).order(5)[0].tolist() == [3, 2, 0]
    hamming = bits.BitsTruth("hamming", rows, queries)
    assert hamming.exact[1].tolist() == [0.0, 1.0, 1.0, 1.0, 0.0] and hamming.order(2)[1].tolist() == [4, 0]
    keys = truth.order(3)
    truth.check(keys, truth.exact[np.arange(2)[:, None], keys], np.array([3, 3]), 3)
    with pytest.raises(AssertionError):
        truth.check(keys[:, ::-1], truth.exact[np.arange(2)[:, None], keys[:, ::-1]], np.array([3, 3]), 3)
