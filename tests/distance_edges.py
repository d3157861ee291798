"""Edge inputs of the distance arithmetic, shared by the CPU test (reference against oracle) and the GPU test (kernels
against both). No GPU dependency. `cases(metric, dtype)` yields `(name, metric, dtype, ndim, a, b)`: `a` plays the query, `b`
the stored row, both in the storage kind. The part of a name before the first `@` or `/` is its VALUE CLASS.

Dimensions come from `row_geometry` (usearch_amd/csrc/engine.hip), restated in `row_geometry` below: the tail of
`measure_rows` depends on chunks per lane against the unroll depth (4 deep for G ≤ 2, 8 deep for G = 8).

Every input is built so that its result does not depend on the order of summation:
  · the ordinary components are multiples of 1/8 in [-2, 2] — every sum of ip, cos, l2sq and pearson over at most 2.2 k of them
    is exact in f32, whatever the order;
  · a special value sits in ONE component of a pair, so a sum holds at most one overflowing term and never inf - inf across
    terms (ip/f32 of two rows that are large everywhere is NaN in one order and -inf in another: no such pair is here);
  · a partner of the largest finite value is 0.5 or the value itself, never a number that puts a product next to the overflow
    threshold, where a fused and an unfused multiply-add land on different sides of it."""
from __future__ import annotations

import numpy as np

from tests import util

FLOATS = ("bf16", "f16", "f32", "f64")
ITEM_BYTES = {"f64": 8, "f32": 4, "f16": 2, "bf16": 2, "i8": 1}
# pearson/f64 is not in the table: the reference computes it in f32, oracle and kernels still in double
PAIRS = ([(m, d) for m in ("ip", "cos", "l2sq", "pearson") for d in FLOATS + ("i8",) if (m, d) != ("pearson", "f64")]
         + [("divergence", d) for d in FLOATS] + [("haversine", "f32"), ("haversine", "f64")]
         + [(m, "b1") for m in ("hamming", "tanimoto", "jaccard", "sorensen")])
# the (metric, scalar) pairs with a build for G = 4, which `row_geometry` never picks (common.hpp `all_kernel_builds`)
G4_PAIRS = {(m, d) for m in ("ip", "cos", "l2sq") for d in ("f32", "f16", "bf16", "i8")} | {("hamming", "b1")}
I8_EXACT_WITH_MINUS_128 = 1024  # 128² · 1024 = 2²⁴: beyond it the f32 sums of ip / pearson over i8 stop being exact


def bytes_per_vector(dtype: str, ndim: int) -> int:
    return (ndim + 7) // 8 if dtype == "b1" else ndim * ITEM_BYTES[dtype]


def per_chunk(dtype: str) -> int:
    """Scalars (bits for b1) in one 16-byte chunk."""
    return 128 if dtype == "b1" else 16 // ITEM_BYTES[dtype]


def _pow2_ceil(x: int) -> int:
    return 1 << max(0, (x - 1).bit_length())


def row_geometry(nbytes: int, forced: int = 0):
    """→ (lanes per row G, 16-byte chunks read per row); `forced` = USEARCH_AMD_LANES."""
    raw_chunks = max(1, (nbytes + 15) // 16)
    lanes = min(8, _pow2_ceil(raw_chunks))
    if raw_chunks <= 8:
        lanes = min(2, lanes)
    if forced in (1, 2, 4, 8):
        lanes = min(forced, _pow2_ceil(raw_chunks))
    return lanes, (nbytes + 16 * lanes - 1) // (16 * lanes) * lanes


# Whole 16-byte chunks of a row → (G, chunks per lane). Rows of ≤ 128 bytes run G ≤ 2 with 4 loads in flight: 1 chunk (G = 1) and 2
# chunks (G = 2) are 1 per lane, 5 are 3 per lane, 7 are 4 per lane. 5 per lane is out of reach there (2 · 4 · 16 = 128 bytes is the
# longest such row), so the largest reachable row stands in for it: 8 whole chunks, the only one without any padding.
SHORT_ROWS = {1: (1, 1), 2: (2, 1), 5: (2, 3), 7: (2, 4), 8: (2, 4)}
# Longer rows run G = 8 with 8 loads in flight: 1, 7, 8, 9 and 17 chunks per lane.
LONG_ROWS = {9: (8, 2), 49: (8, 7), 57: (8, 8), 65: (8, 9), 129: (8, 17)}
# (9 chunks are 2 per lane once padded to a multiple of G: the shortest row G = 8 ever sees. 1 per lane under G = 8 is a row of 8
# chunks or fewer, which only a forced USEARCH_AMD_LANES = 8 produces: the GPU test forces it on the short rows above.)


def dimensions(dtype: str):
    """For every chunk count above, the smallest ndim that reaches it (one scalar in the last chunk) and the largest that is no
    multiple of the scalars per chunk (one scalar short of full): zero padding inside the last chunk both times, and a stray low
    bit pattern in the last byte of a b1 row. Plus the full 128-byte row. At most 129 chunks = 2 064 bytes."""
    pc = per_chunk(dtype)
    out = set()
    for chunks in list(SHORT_ROWS) + list(LONG_ROWS):
        out.add((chunks - 1) * pc + 1)
        out.add(max(1, chunks * pc - 1))
    out.add(8 * pc)
    return sorted(out)


def geometry_of(dtype: str, ndim: int):
    """→ (G, chunks per lane) the engine picks for such rows."""
    lanes, chunks = row_geometry(bytes_per_vector(dtype, ndim))
    return lanes, chunks // lanes


def value_class(name: str) -> str:
    return name.split("@")[0].split("/")[0]


def encode(x: np.ndarray, dtype: str) -> np.ndarray:
    """float64 intent → storage kind; every value placed here is representable, so nothing rounds but the ordinary ones."""
    if dtype == "bf16":
        return util.to_bf16(np.asarray(x, dtype=np.float64).astype(np.float32))
    return np.asarray(x, dtype=np.float64).astype(util.NP_DTYPE[dtype])


# smallest subnormal, smallest normal, largest finite of each storage kind (all exact in float64)
LIMITS = {
    "f64": (5e-324, 2.0 ** -1022, float(np.finfo(np.float64).max)),
    "f32": (2.0 ** -149, 2.0 ** -126, float(np.finfo(np.float32).max)),
    "f16": (2.0 ** -24, 2.0 ** -14, 65504.0),
    "bf16": (2.0 ** -133, 2.0 ** -126, (2.0 - 2.0 ** -7) * 2.0 ** 127),
}


def _grid(ndim: int, seed: int) -> np.ndarray:
    """Multiples of 1/8 in [-2, 2], none of them zero."""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 17, ndim) / 8.0
    return x * rng.choice([-1.0, 1.0], ndim)


def _positions(ndim: int):
    """A component of the first chunk and one of the last (ragged) chunk."""
    return [("first", 0)] if ndim == 1 else [("first", 0), ("last", ndim - 1)]


def _specials(dtype: str):
    """(class, value in a, value in b) placed in one component of an ordinary pair."""
    sub, tiny, big = LIMITS[dtype]
    inf, nan = float("inf"), float("nan")
    return [
        ("negative-zero", -0.0, -0.0), ("negative-zero", -0.0, 1.0),
        ("subnormal", sub, sub), ("subnormal", sub, -sub), ("subnormal", sub, big),
        ("smallest-normal", tiny, tiny), ("smallest-normal", tiny, big),
        ("largest-finite", big, 0.5), ("largest-finite", 0.5, big), ("largest-finite", big, big), ("largest-finite", big, -big),
        ("plus-inf", inf, 0.5), ("plus-inf", 0.5, inf), ("plus-inf", inf, inf),
        ("minus-inf", -inf, 0.5), ("minus-inf", 0.5, -inf),
        ("nan", nan, 0.5), ("nan", 0.5, nan),
    ]


def _float_cases(metric: str, dtype: str, ndim: int):
    a, b = _grid(ndim, 11 + ndim), _grid(ndim, 12 + ndim)
    zero = np.zeros(ndim)
    yield "zeros/one-side-b", a, zero
    yield "zeros/one-side-a", zero, b
    yield "zeros/both", zero, zero
    yield "negative-zero/all", -zero, -zero
    yield "negative-zero/against-ordinary", a, -zero
    # pearson's denominator 0: n·Σa² = (Σa)² for a constant row, exactly (1.5² · 2064² < 2²⁴), fused or not
    ramp = (np.arange(ndim) % 17) / 8.0
    yield "constant/against-ramp", np.full(ndim, 1.5), ramp
    yield "constant/ramp-against-it", ramp, np.full(ndim, 1.5)
    yield "constant/both", np.full(ndim, 1.5), np.full(ndim, -0.25)
    sub, tiny, _ = LIMITS[dtype]
    yield "subnormal/all", np.full(ndim, sub), np.full(ndim, sub)  # every product underflows in f32: cos sees two zero norms
    yield "smallest-normal/all", np.full(ndim, tiny), np.full(ndim, -tiny)
    for where, at in _positions(ndim):
        for name, x, y in _specials(dtype):
            p, q = a.copy(), b.copy()
            p[at], q[at] = x, y
            yield f"{name}@{where}", p, q
        if dtype != "f16":  # a - b = 1e-20 in one component, equal elsewhere: the squared distance is an f32 subnormal (1e-40)
            p, q = a.copy(), a.copy()
            p[at], q[at] = 1e-20, 0.0
            yield f"subnormal-result@{where}", p, q


def _divergence_cases(dtype: str, ndim: int):
    h = util.make_vectors(2, ndim, "f64", seed=21 + ndim, clustered=False, metric="divergence")
    a, b = h[0], h[1]
    zero, uniform = np.zeros(ndim), np.full(ndim, 1.0 / ndim)
    yield "identical/histograms", a, a
    yield "ordinary/histograms", a, b
    yield "zeros/one-side-b", a, zero
    yield "zeros/one-side-a", zero, b
    yield "zeros/both", zero, zero
    yield "negative-zero/all", -zero, -zero
    holes_a, holes_b = a.copy(), b.copy()
    holes_a[::3] = 0.0   # exact zeros: on one side, on the other, on both
    holes_b[1::3] = 0.0
    holes_b[::6] = 0.0
    yield "zeros/in-histogram", holes_a, holes_b
    sub, tiny, big = LIMITS[dtype]
    inf, nan = float("inf"), float("nan")
    specials = [("negative-zero", -0.0, 0.5), ("subnormal", sub, sub), ("subnormal", sub, 0.5), ("subnormal", 0.0, sub),
                ("smallest-normal", tiny, tiny), ("smallest-normal", tiny, 0.5),
                ("largest-finite", big, 0.5), ("largest-finite", 0.5, big), ("largest-finite", big, big),
                ("plus-inf", inf, 0.5), ("plus-inf", 0.5, inf), ("minus-inf", -inf, 0.5), ("nan", nan, 0.5), ("nan", 0.5, nan)]
    if dtype == "f64":  # inside f64, outside f32: the reference narrows every element to float
        specials += [("beyond-f32", 1e30, 1e30), ("beyond-f32", 1e-30, 1e-30), ("beyond-f32", 1e30, 1e-30), ("beyond-f32", 1e-30, 0.5)]
        yield "beyond-f32/all-1e-30", a * 1e-30, b * 1e-30
        yield "beyond-f32/all-1e30", a * 1e30, b * 1e30
        yield "beyond-f32/constant-against-ramp-1e30", np.full(ndim, 1e30), (np.arange(ndim) + 1.0) * 1e30
    for where, at in _positions(ndim):
        hot = zero.copy()
        hot[at] = 1.0
        yield f"one-hot@{where}", hot, uniform
        yield f"one-hot@{where}/stored", uniform, hot
        for name, x, y in specials:
            p, q = a.copy(), b.copy()
            p[at], q[at] = x, y
            yield f"{name}@{where}", p, q


def full_range_i8(n: int, ndim: int, seed: int) -> np.ndarray:
    """int8 rows over the whole range, -128 included (`make_vectors` stops at ±100)."""
    return np.random.default_rng(seed).integers(-128, 128, (n, ndim)).astype(np.int8)


def _i8_cases(metric: str, ndim: int, constants: bool):
    a, b = full_range_i8(2, ndim, 31 + ndim)
    zero = np.zeros(ndim, dtype=np.int8)
    yield "full-range/random", a, b
    yield "zeros/one-side-b", a, zero
    yield "zeros/one-side-a", zero, b
    yield "zeros/both", zero, zero
    for where, at in _positions(ndim):
        for x, y in ((-128, -128), (-128, 127), (127, 127), (127, -128)):
            p, q = a.copy(), b.copy()
            p[at], q[at] = x, y
            yield f"full-range/{x}-against-{y}@{where}", p, q
    if constants:
        high, low = np.full(ndim, 127, dtype=np.int8), np.full(ndim, -128, dtype=np.int8)
        yield "constant/all-127", high, high
        yield "constant/all-minus-128", low, low
        yield "constant/minus-128-against-127", low, high
        yield "constant/127-against-random", high, b
        yield "constant/random-against-minus-128", a, low


def i8_constants_allowed(metric: str, ndim: int) -> bool:
    """cos and l2sq sum in int32 (exact to 2³¹). ip and pearson sum in f32: a constant row of -128 keeps them exact to d = 1 024,
    beyond which the compiled reference and any other order drift apart (d = 4 096, all 127, ip: 4.6e-5 relative) and pearson of two
    constant rows flips between 0 and 2. pearson's closing `n·Σa² - (Σa)²` must also cancel exactly whether the compiler fuses it
    or not, which it does when n is a power of two (both products are then exact)."""
    if metric in ("cos", "l2sq"):
        return True
    if metric == "ip":
        return ndim <= I8_EXACT_WITH_MINUS_128
    return ndim <= I8_EXACT_WITH_MINUS_128 and ndim & (ndim - 1) == 0


def _b1_cases(ndim: int):
    nbytes = (ndim + 7) // 8
    rng = np.random.default_rng(41 + ndim)
    a, b = rng.integers(0, 256, (2, nbytes), dtype=np.uint8)  # the stray low bits of the last byte are set at random …
    empty, full = np.zeros(nbytes, dtype=np.uint8), np.full(nbytes, 255, dtype=np.uint8)  # … and all of them in `full`
    stray = empty.copy()
    stray[-1] = (1 << (8 * nbytes - ndim)) - 1  # nothing but the bits beyond ndim: the reference counts whole bytes
    yield "ordinary/random", a, b
    yield "empty/both", empty, empty  # tanimoto, sorensen: 0 / 0 = NaN in the reference
    yield "empty/against-full", empty, full
    yield "empty/full-against-it", full, empty
    yield "empty/against-random", empty, b
    yield "full/both", full, full
    yield "full/against-random", full, b
    if ndim % 8:
        yield "stray-bits/alone", stray, stray
        yield "stray-bits/against-empty", stray, empty
        yield "stray-bits/against-random", stray, b


def _haversine_cases():
    nan, inf = float("nan"), float("inf")
    yield "same-point/ordinary", (48.2, 16.37), (48.2, 16.37)
    yield "same-point/origin", (0.0, 0.0), (0.0, 0.0)
    yield "same-point/negative-zero", (-0.0, -0.0), (0.0, 0.0)
    yield "ordinary/two-cities", (48.2, 16.37), (-33.87, 151.21)
    yield "poles/north-to-south", (90.0, 0.0), (-90.0, 0.0)
    yield "poles/south-to-north", (-90.0, 45.0), (90.0, 45.0)
    yield "poles/same-pole-other-longitude", (90.0, 0.0), (90.0, 120.0)
    yield "antipodes/equator", (0.0, 0.0), (0.0, 180.0)
    yield "antipodes/equator-west", (0.0, -90.0), (0.0, 90.0)
    yield "antimeridian/across", (10.0, 179.9999), (10.0, -179.9999)
    yield "antimeridian/across-equator", (0.0, -179.9999), (0.0, 179.9999)
    yield "out-of-range/both", (1e6, 1e6), (-1e6, 3e5)
    yield "out-of-range/one", (1e6, -1e6), (12.5, 45.25)
    yield "nan/latitude", (nan, 10.0), (20.0, 30.0)
    yield "nan/stored-longitude", (5.0, 10.0), (20.0, nan)
    yield "plus-inf/latitude", (inf, 10.0), (20.0, 30.0)


def cases(metric: str, dtype: str):
    """Every edge case of one (metric, scalar) pair."""
    if metric == "haversine":
        for name, a, b in _haversine_cases():
            yield name, metric, dtype, 2, encode(np.array(a), dtype), encode(np.array(b), dtype)
        return
    ndims = dimensions(dtype)
    if dtype == "i8":
        # every value class at d = 16, 1 024 (the exactness bound of the f32 sums) and 2 048; cos at 1 041, where all 127 gives -1.19e-7
        ndims = sorted(set(ndims) | {16, 1024, 2048} | ({1041} if metric == "cos" else set()))
    for ndim in ndims:
        if dtype == "b1":
            found = _b1_cases(ndim)
        elif dtype == "i8":
            found = _i8_cases(metric, ndim, i8_constants_allowed(metric, ndim))
        elif metric == "divergence":
            found = ((name, encode(a, dtype), encode(b, dtype)) for name, a, b in _divergence_cases(dtype, ndim))
        else:
            found = ((name, encode(a, dtype), encode(b, dtype)) for name, a, b in _float_cases(metric, dtype, ndim))
        for name, a, b in found:
            yield name, metric, dtype, ndim, a, b


def result_class(x: float) -> str:
    """finite, +inf, -inf or nan (a NaN's sign and payload are not compared: the reference's differ between builds)."""
    if np.isnan(x):
        return "nan"
    if np.isinf(x):
        return "+inf" if x > 0 else "-inf"
    return "finite"


def i8_model(metric: str, a: np.ndarray, b: np.ndarray) -> np.float32:
    """ip and pearson over i8 from the five sums in int64, closed with the reference's formulas in float32
    (metric_ip_gt 1309-1326, metric_pearson_gt 1511-1550): what the reference computes while its f32 sums stay exact."""
    x, y = a.astype(np.int64), b.astype(np.int64)
    f = np.float32
    ab, a2, b2, sa, sb = (f(int(v)) for v in ((x * y).sum(), (x * x).sum(), (y * y).sum(), x.sum(), y.sum()))
    if metric == "ip":
        return f(1) - ab
    n = f(len(a))
    if len(a) <= 1:
        return f(0)
    with np.errstate(all="ignore"):
        denominator = (n * a2 - sa * sa) * (n * b2 - sb * sb)
        if denominator == 0:
            return f(0)
        return f(1) - (n * ab - sa * sb) / np.sqrt(denominator)
