"""No GPU: the f8 (OCP e4m3fn) casts of csrc/casts.hpp against a codec in plain numpy — a table of the 256 values, and "the nearest
finite code, ties to the even code, ±448 beyond it, a NaN → 0x7F, the sign kept"; tests/test_gpu_exact_f8.py borrows it — and f8's pairs."""
import numpy as np
import pytest

import usearch_amd
from usearch_amd.index import test_exact_tiled_pair as tiled_pair

CODES = np.arange(256)
DECODE = np.where(CODES & 0x78, (1 + (CODES & 7) / 8) * 2.0 ** ((CODES >> 3 & 15) - 7.0), (CODES & 7) / 8 * 2.0 ** -6) * np.where(CODES & 0x80, -1, 1)
DECODE[[0x7F, 0xFF]] = np.nan
FINITE = np.array(sorted((c for c in range(256) if c & 0x7F != 0x7F), key=lambda c: (DECODE[c], -(c >> 7))), dtype=np.uint8)  # by value, −0 before +0


def encode(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    size = np.minimum(np.abs(x), 448.0)
    above = np.clip(np.searchsorted(DECODE[:0x7F], size), 1, 0x7E)  # the first code at or above |x|, and the one below it
    below = above - 1
    with np.errstate(invalid="ignore"):  # (a NaN has no neighbours)
        down, up = size - DECODE[below], DECODE[above] - size
    code = np.where((down < up) | ((down == up) & (below % 2 == 0)), below, above)
    return (np.where(np.isnan(x), 0x7F, code) | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def test_every_f16_pattern():  # every midpoint, both saturation edges, ±∞, the NaNs with their signs, −0, the subnormals
    x = np.arange(65536, dtype=np.uint16).view(np.float16)
    assert np.array_equal(usearch_amd.cast(x, "f16", "f8", len(x)), encode(x))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_midpoints_their_neighbours_and_the_ends(dtype):
    # the 253 midpoints, the two neighbours of each in the source kind (what a cast that rounds twice gets wrong), ±448, ±∞, past 448
    kind = {"f32": np.float32, "f64": np.float64}[dtype]
    values = DECODE[FINITE]
    middles = ((values[1:] + values[:-1]) / 2).astype(kind)
    assert len(middles) == 253 and np.array_equal(middles.astype(np.float64), (values[1:] + values[:-1]) / 2)
    ends = np.array([448, -448, np.inf, -np.inf], dtype=kind)
    x = np.concatenate([middles, np.nextafter(middles, kind(np.inf)), np.nextafter(middles, kind(-np.inf)), ends, np.nextafter(ends[:2], ends[2:])])
    got = usearch_amd.cast(x, dtype, "f8", len(x))
    assert np.array_equal(got, encode(x)) and list(got[-6:]) == [0x7E, 0xFE, 0x7E, 0xFE, 0x7E, 0xFE]


@pytest.mark.parametrize("dtype", ["f32", "f16", "f64"])
def test_decoding_is_exact_and_comes_back(dtype):
    kind = usearch_amd.index.NUMPY_DTYPES[dtype]
    wide = usearch_amd.cast(FINITE, "f8", dtype, len(FINITE)).view(kind)
    assert np.array_equal(wide.astype(np.float64), DECODE[FINITE]) and np.array_equal(np.signbit(wide), FINITE >> 7 == 1)
    assert np.array_equal(usearch_amd.cast(wide, dtype, "f8", len(FINITE)), FINITE) and np.isnan(usearch_amd.cast(np.array([0x7F, 0xFF], dtype=np.uint8), "f8", dtype, 2).view(kind)).all()


@pytest.mark.parametrize("metric", ["cos", "ip", "l2sq"])
def test_f8_has_a_tiled_kernel_for_every_result_count_a_list_holds(metric):
    assert all(tiled_pair(metric, "f8", wanted) for wanted in range(1, 65))
    assert not tiled_pair(metric, "f8", 0) and not tiled_pair(metric, "f8", 65)
