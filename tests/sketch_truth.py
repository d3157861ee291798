"""A plain float64 truth of the sketch (usearch_amd/csrc/sketch.hpp) in numpy, for the tests that hold the device's records, the
host twins and the walk's prune counters to it. Nothing of the library is imported here: stored rows, the stored directions D (the
transposed [dimensions][64] f32 array) and 128-byte records come in as arrays.

For a stored row b:  b̂ = b / ‖b‖,  c = D b̂,  r = ‖b̂ − Dᵀĉ‖ with ĉ the 62 halves the record stores, and δ = ‖D Dᵀ − I‖_F over the stored
columns. A record is SOUND when its ρ ≥ r, and TIGHT when ρ is no more than `sketch_residual` can make of r:

    ρ = f32(√(1 − 2ĉ·c + (1 + δ)‖ĉ‖² + 1e-9)) · 1.000001f + 1e-30f                                    (sketch.hpp)
    r² = 1 − 2ĉ·c + ĉᵀ(D Dᵀ)ĉ ≥ 1 − 2ĉ·c + (1 − δ)‖ĉ‖²   ⇒   the radicand ≤ r² + 2δ‖ĉ‖² + 1e-9
    the narrowing of the root and the f32 product each round by at most 1 + 2⁻²⁴

so ρ ≤ √(r² + 2δ‖ĉ‖² + 1e-9) · 1.000001 · (1 + 2⁻²³) + 1e-30."""
from __future__ import annotations

import numpy as np

RANK, COLUMNS, RECORD_BYTES = 62, 64, 128
NORM_RANGE = (2.0 ** -100, 2.0 ** 100)  # `sketch_norm_in_range`: Σb² outside it is never pruned


def widen(rows: np.ndarray, dtype: str) -> np.ndarray:
    """Stored rows (f32, f16, or bf16 bit patterns as uint16; or their bytes) → float64, exactly."""
    rows = np.ascontiguousarray(rows)
    if rows.dtype == np.uint8:
        rows = rows.view({"f32": np.float32, "f16": np.float16, "bf16": np.uint16}[dtype])
    if dtype == "bf16":
        return (rows.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return rows.astype(np.float64)


def decode_records(records: np.ndarray):
    """The record layout: halves 0 … 61 in bytes 0 … 123, f32 ρ in bytes 124 … 127 → (ĉ float64 [n, 62], ρ float64 [n])."""
    records = np.ascontiguousarray(records, dtype=np.uint8)
    assert records.ndim == 2 and records.shape[1] == RECORD_BYTES
    halves = np.ascontiguousarray(records[:, :2 * RANK]).view(np.float16).astype(np.float64)
    rho = np.ascontiguousarray(records[:, 2 * RANK:]).view(np.float32)[:, 0].astype(np.float64)
    return halves, rho


def gram_defect(directions: np.ndarray) -> float:
    """δ = ‖D Dᵀ − I‖_F over the stored columns (those that are not all zero), in float64. The products of two f32 values are exact in
    float64; they are summed one after the other in dimension order (numpy's cumulative sum), the entries in row order — the
    plainest order there is, and one that leaves no room for a 1e-12 disagreement over which float64 sum is meant: every diagonal
    entry is 1 + O(1e-8), so the ORDER of 777 additions alone moves δ by 1e-8 of itself."""
    d = np.ascontiguousarray(directions, dtype=np.float32).astype(np.float64)
    stored = np.flatnonzero(np.any(d != 0.0, axis=0))
    assert len(stored) == 0 or (stored[-1] == len(stored) - 1 and len(stored) <= RANK), "the stored columns come first, 62 at most"
    d = d[:, :len(stored)]
    if not len(stored):
        return 0.0
    gram = np.cumsum(d[:, :, None] * d[:, None, :], axis=0)[-1] - np.eye(len(stored))
    return float(np.sqrt(np.cumsum((gram * gram).ravel())[-1]))


def rank_of(directions: np.ndarray) -> int:
    return int(np.any(np.asarray(directions) != 0.0, axis=0).sum())


def ordinary_rows(rows64: np.ndarray) -> np.ndarray:
    """Rows the sketch may prune at all: finite, with Σb² inside `sketch_norm_in_range` (the rest is listed under NEVER PRUNED)."""
    with np.errstate(over="ignore", invalid="ignore"):
        n2 = (rows64.astype(np.longdouble) ** 2).sum(axis=1)
    return np.isfinite(rows64).all(axis=1) & (n2 >= NORM_RANGE[0]) & (n2 <= NORM_RANGE[1])


def truth(rows64: np.ndarray, directions: np.ndarray, records: np.ndarray) -> dict:
    """→ for every row: `c` float64 [n, 64] = D b̂, `r` = ‖b̂ − Dᵀĉ‖ against the STORED halves, `c2` = ‖ĉ‖², and `ordinary`; rows that are
    not ordinary hold NaN. `delta`: the gram defect."""
    d = np.ascontiguousarray(directions, dtype=np.float32).astype(np.float64)
    ordinary = ordinary_rows(rows64)
    halves, _ = decode_records(records)
    n = len(rows64)
    c, r, c2 = np.full((n, COLUMNS), np.nan), np.full(n, np.nan), np.full(n, np.nan)
    b = rows64[ordinary]
    norms = np.sqrt((b.astype(np.longdouble) ** 2).sum(axis=1))
    unit = (b.astype(np.longdouble) / norms[:, None]).astype(np.float64)
    c[ordinary] = unit @ d
    stored = halves[ordinary]
    r[ordinary] = np.sqrt(((unit - stored @ d[:, :RANK].T).astype(np.longdouble) ** 2).sum(axis=1)).astype(np.float64)
    c2[ordinary] = (stored ** 2).sum(axis=1)
    return {"c": c, "r": r, "c2": c2, "ordinary": ordinary, "delta": gram_defect(directions)}


def cos_distance(a64: np.ndarray, b64: np.ndarray) -> np.ndarray:
    """The true 1 − a·b / (‖a‖ ‖b‖) of query a against every row of b (norms in long double)."""
    a, b = a64.astype(np.longdouble), b64.astype(np.longdouble)
    return np.asarray(1 - (b @ a) / (np.sqrt((a * a).sum()) * np.sqrt((b * b).sum(axis=1))), dtype=np.float64)


def ceiling(r: np.ndarray, c2: np.ndarray, delta: float) -> np.ndarray:
    """The most `sketch_residual` can make of r (see the module's head)."""
    return np.sqrt(r * r + 2.0 * delta * c2 + 1e-9) * 1.000001 * (1.0 + 2.0 ** -23) + 1e-30


def f16_neighbours(x: np.ndarray):
    """The two f16 values that enclose x (equal where x is one)."""
    with np.errstate(over="ignore"):
        nearest = x.astype(np.float16)
    wide = nearest.astype(np.float64)
    below = np.where(wide > x, np.nextafter(nearest, np.float16(-np.inf)), nearest)
    above = np.where(wide < x, np.nextafter(nearest, np.float16(np.inf)), nearest)
    return below.astype(np.float64), above.astype(np.float64)


def check_records(rows64: np.ndarray, directions: np.ndarray, reported_defect: float, records: np.ndarray, never=(), duplicates=(),
                  what: str = "") -> dict:
    """Every assertion a set of records must pass against the truth; → the figures worth printing."""
    facts = truth(rows64, directions, records)
    halves, rho = decode_records(records)
    ordinary, r, delta = facts["ordinary"], facts["r"], facts["delta"]
    for row in never:
        assert not ordinary[row], f"{what}: row {row} was meant as a row that is never pruned"
    # never pruned: ρ = +∞ and 124 zero bytes (an ordinary row may join them only through a coefficient f16 cannot hold: none here)
    infinite = np.isposinf(rho)
    assert np.array_equal(infinite, ~ordinary), f"{what}: ρ = +inf on rows {np.flatnonzero(infinite != ~ordinary)[:8]} against the rule"
    assert not np.asarray(records)[~ordinary, :2 * RANK].any(), f"{what}: a row that is never pruned carries coefficients"
    assert np.isfinite(rho[ordinary]).all() and (rho[ordinary] > 0).all()
    # the gram defect the records were made with
    assert abs(reported_defect - delta) <= 1e-12 * delta, f"{what}: gram defect {reported_defect!r} against the truth's {delta!r}"
    # sound: no tolerance (the builder's 1e-9 under the root is worth ≥ 3e-10 on ρ; numpy's error here is ~1e-13)
    shortfall = float(np.max(r[ordinary] - rho[ordinary]))
    # tight
    over = float(np.max(rho[ordinary] / ceiling(r[ordinary], facts["c2"][ordinary], delta)))
    # coefficients: each stored half is one of the two f16 neighbours of the true c_j; columns 62 and 63 are not stored at all
    below, above = f16_neighbours(facts["c"][ordinary][:, :RANK])
    stored = halves[ordinary]
    off = (stored != below) & (stored != above)
    figures = {"rows": int(ordinary.sum()), "never": int((~ordinary).sum()), "r_minus_rho": shortfall, "rho_over_ceiling": over,
               "coefficients_off": int(off.sum()), "delta": delta, "rank": rank_of(directions),
               "median_r": float(np.median(r[ordinary])), "median_rho": float(np.median(rho[ordinary]))}
    print(f"{what}: {figures}")
    assert shortfall <= 0.0, f"{what}: ρ below the true residual by {shortfall:.3g} (row {np.flatnonzero(ordinary)[np.argmax(r[ordinary] - rho[ordinary])]})"
    assert over <= 1.0, f"{what}: ρ is {over:.9f} of the most the closing arithmetic can make of the true residual"
    assert not off.any(), f"{what}: {int(off.sum())} coefficients are no f16 neighbour of the true ones, first at {np.argwhere(off)[0]}"
    assert not stored[:, figures["rank"]:].any(), f"{what}: coefficients on directions that do not exist"
    for copy, original in duplicates:
        assert np.array_equal(records[copy], records[original]), f"{what}: rows {copy} and {original} are equal, their records are not"
    return figures


def differences(a: np.ndarray, b: np.ndarray) -> dict:
    """Two sets of records compared bit for bit → how many records differ, and in what: coefficients (how many halves, the largest
    step in units of the last place), ρ (the largest step in ulps of f32)."""
    a, b = np.ascontiguousarray(a, dtype=np.uint8), np.ascontiguousarray(b, dtype=np.uint8)
    assert a.shape == b.shape
    ha, hb = (np.ascontiguousarray(x[:, :2 * RANK]).view(np.int16).astype(np.int64) for x in (a, b))
    ra, rb = (np.ascontiguousarray(x[:, 2 * RANK:]).view(np.int32)[:, 0].astype(np.int64) for x in (a, b))
    return {"records": int((a != b).any(axis=1).sum()), "halves": int((ha != hb).sum()),
            "largest_half_step": int(np.abs(ha - hb).max(initial=0)), "rho": int((ra != rb).sum()),
            "largest_rho_step": int(np.abs(ra - rb).max(initial=0))}


def prune_counts(trace, bounds: np.ndarray):
    """The model of the walk's prune decision (usearch_amd/csrc/kernels.hpp, `search_one`), for one query. `trace`: the oracle's
    segments of the query's level-0 walk (oracle/oraclebind.py `search_traced` with tiles of 64 cells), each (top was full, radius,
    first segment of its hop, fresh slots in list order); `bounds[slot]`: the lower bound of the query's distance to that member, or
    None / all −inf for a query that walks without the sketch → (tested, pruned).

    What the kernel does, restated (line numbers of kernels.hpp):
      · a hop takes its list one TILE of 64 cells at a time (1829-1832: `cell = tile + lane`); the probe of the visited set names the
        tile's fresh neighbours (2021-2029), they are measured, and committed in list order (2145-) BEFORE the next tile is looked at:
        so a list of more than 64 cells (connectivity 40: 80 cells) tests its second tile against the state the first tile's commits
        left — `top.size` and `radius` are read per tile, not per hop;
      · the sketch is asked only when `sketch_on && top.size == ef` at that point (2057); then every fresh candidate of the tile is
        tested, `sketch_tested += count` (2119), whether its record came beside the probe (1968: tile 0 of a list of ≤ 32 cells) or behind it;
      · a candidate is pruned iff `bound >= radius` with the radius of the tile's start (2117: `!(bound >= radius)` survives, so a NaN
        bound prunes nothing), `sketch_pruned += count − kept` (2119);
      · a query whose Σa² is out of range has `sketch_on` false (1412) and counts nothing."""
    tested = pruned = 0
    if bounds is None:
        return 0, 0
    for full, radius, _, fresh in trace:
        if not full or not len(fresh):
            continue
        tested += len(fresh)
        pruned += int(np.count_nonzero(bounds[fresh] >= np.float32(radius)))
    return tested, pruned
