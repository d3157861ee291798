"""CPU: the compiled reference against the oracle over the edge inputs of tests/distance_edges.py — the values
`util.make_vectors` never produces (i8 beyond ±100, non-finite and subnormal components, degenerate rows for the closing
arithmetic) at row lengths that put the tail of the kernels' row loop at each of its edges. The oracle is what the GPU tests
hold the kernels to, so this is what holds the oracle to the real reference there."""
import numpy as np
import pytest

from tests import distance_edges as edges
from tests import util

LANES = (0, 1, 2, 8)


def test_the_table_reaches_every_tail_of_the_row_loop():
    """The dimensions are derived from `row_geometry`, not guessed: every (G, chunks per lane) the table promises is what the
    engine's geometry gives for the smallest and the largest ragged row of that many chunks, in every storage kind."""
    for dtype in edges.FLOATS + ("i8", "b1"):
        pc = edges.per_chunk(dtype)
        reached = {edges.geometry_of(dtype, ndim) for ndim in edges.dimensions(dtype)}
        for chunks, want in list(edges.SHORT_ROWS.items()) + list(edges.LONG_ROWS.items()):
            for ndim in ((chunks - 1) * pc + 1, max(1, chunks * pc - 1)):
                assert ndim in edges.dimensions(dtype)
                assert edges.geometry_of(dtype, ndim) == want, (dtype, ndim)
                assert ndim == 1 or pc <= 2 or ndim % pc, "zero padding must fall inside the last chunk"
        # G ≤ 2, 4 loads in flight: whole rounds and a tail of 1 and 3 · G = 8, 8 in flight: tails of 1, 2 and 7, one and two whole rounds
        assert {(1, 1), (2, 1), (2, 3), (2, 4), (8, 2), (8, 7), (8, 8), (8, 9), (8, 17)} <= reached
        assert max(edges.bytes_per_vector(dtype, ndim) for ndim in edges.dimensions(dtype)) <= 2064
    assert edges.row_geometry(96) == (2, 6) and edges.row_geometry(1536) == (8, 96) and edges.row_geometry(96, forced=8) == (8, 8)


@pytest.mark.parametrize("metric,dtype", edges.PAIRS)
def test_reference_and_oracle_agree_on_edge_inputs(reference, metric, dtype):
    """Same result class (finite, +inf, -inf, NaN) on every case, in the reference's loop order and in the kernels' layouts of
    1, 2 and 8 lanes; finite values bit-equal for the exact pairs and cos/i8, within the stated float tolerance otherwise."""
    from oracle import oraclebind
    exact = util.exact_pair(metric, dtype) or (dtype == "i8" and metric == "cos")
    tolerance = util.tolerance(dtype)
    wrong, count = [], 0
    for name, _, _, ndim, a, b in edges.cases(metric, dtype):
        count += 1
        want = np.float32(reference.distance(a, b, metric, dtype, ndim))
        model = None
        if dtype == "i8" and metric in ("ip", "pearson"):
            x, y = a.astype(np.int64), b.astype(np.int64)
            if ndim > edges.I8_EXACT_WITH_MINUS_128:  # only rows whose f32 sums stay exact in ANY order are in the table up here
                assert not name.startswith("constant")
                assert max(np.abs(x * y).sum(), (x * x).sum(), (y * y).sum()) < 2 ** 24, (name, ndim)
            model = edges.i8_model(metric, a, b)
            if metric == "ip":
                assert model.view(np.uint32) == want.view(np.uint32), (name, ndim, model, want)
            elif not abs(float(model) - float(want)) <= tolerance * max(1.0, abs(float(want))):
                wrong.append((name, ndim, "model", float(model), float(want)))
        for lanes in LANES:
            got = np.float32(oraclebind.distance(a, b, metric, dtype, ndim, lanes))
            if edges.result_class(got) != edges.result_class(want):
                wrong.append((name, ndim, lanes, float(got), float(want)))
            elif not np.isfinite(want):
                continue
            elif exact:
                if got.view(np.uint32) != want.view(np.uint32):
                    wrong.append((name, ndim, lanes, float(got), float(want)))
            elif not abs(float(got) - float(want)) <= tolerance * max(1.0, abs(float(want))):
                wrong.append((name, ndim, lanes, float(got), float(want)))
    assert count > 0
    assert not wrong, f"{len(wrong)} of {count} cases × {len(LANES)} layouts differ (name, ndim, lanes, oracle, reference): {wrong[:12]}"


def test_the_findings_the_table_was_built_around(reference):
    """What the reference does at these edges, pinned so that the table keeps exercising it."""
    from oracle import oraclebind
    empty = np.zeros(16, dtype=np.uint8)
    for metric in ("tanimoto", "sorensen"):  # two empty sets: 0 / 0
        assert np.isnan(reference.distance(empty, empty, metric, "b1", 128))
        assert np.isnan(oraclebind.distance(empty, empty, metric, "b1", 128))
    high = np.full(1041, 127, dtype=np.int8)  # cos of a row with itself, one ulp below zero
    assert reference.distance(high, high, "cos", "i8", 1041) == oraclebind.distance(high, high, "cos", "i8", 1041) == -np.float32(2.0 ** -23)
    # divergence over f64 runs in f32: the largest finite double narrows to +inf and the distance is NaN, where f64 arithmetic
    # stays finite or infinite; a constant against a ramp, d = 40, gives the f32 sums of the reference, not 210.41275 rounded once
    big = np.full(3, 0.25)
    big[0] = np.finfo(np.float64).max
    assert np.isnan(reference.distance(big, np.full(3, 0.25), "divergence", "f64", 3))
    for lanes in LANES:
        assert np.isnan(oraclebind.distance(big, np.full(3, 0.25), "divergence", "f64", 3, lanes))
    constant, ramp = np.full(40, 1.0), np.arange(1, 41, dtype=np.float64)
    want = np.float32(reference.distance(constant, ramp, "divergence", "f64", 40))
    assert abs(float(want) - float(np.float32(oraclebind.distance(constant, ramp, "divergence", "f64", 40, 0)))) <= 4 * np.spacing(want)
