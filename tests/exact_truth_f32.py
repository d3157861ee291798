"""The f64 ground truth of tests/exact_truth.py for f32 rows on the matrix units (`v_mfma_f32_32x32x2_f32`, csrc/exact_tiled.hip):
the same truth, the same data generator and the same checker — `check`, `order`, `decided`, `edge_slots`, `assert_decides` are used
as they are — with the bound re-derived for f32 products and WITHOUT the one assertion of `Truth.__init__` that f32 cannot meet: that
the bound stay below the suite's float tolerance, `util.tolerance("f32")·max(1, |d|)` = 1e-5·max(1, |d|).

THE CONTRACT. The f32 tiled route is f32 arithmetic in the matrix unit's summation order. It is not bit-equal to the wave-per-query
kernel and it is not promised within 1e-5 of anything: every distance lies within the derived bound below of the f64 distance of the
row it names — the rule the 16-bit kinds live under. On the planted data of tests/test_gpu_exact_f32.py the worst-case bound exceeds
1e-5·max(1, |d|) by up to 1.4 × (cos, 64-d) and 4.4 × (ip, 50-d) — and by 18 × for l2sq at 96-d, which the truth covers although the
engine has no tiled kernel for l2sq over f32 (that refusal is pinned by tests/test_gpu_exact.py): the 1e-5 cannot be promised by derivation. What
the hardware does is recorded in tests/test_gpu_exact_f32.py, as a share of the bound and as a share of 1e-5·max(1, |d|).

THE BOUND, per (query a, row b), term by term as in tests/exact_truth.py. u = 2⁻²⁴, γ = (ndim + 16)·u.
  · Σab. The products are no longer exact (f32 × f32 has 48 bits), but the matrix unit's step is a fused multiply-add: the chain
    s ← fl(s + aᵢbᵢ) rounds ONCE per term, so a sum of ndim terms from a zero accumulator makes ndim roundings, each of at most u
    times a partial sum that Σ|aᵢbᵢ| bounds: |error| ≤ ndim·u·Σ|aᵢbᵢ| (first order; in any order — only the order is the kernel's
    own). Exact products gave (ndim − 1); the extra unit comes out of γ's sixteen spare ones.
  · Σa², Σb² (`row_norms_kernel<scalar_f32_k>`: a lane takes every 64th element by fmaf, then six shuffle-adds): ⌈ndim/64⌉ roundings
    of the chain — one per fmaf, the square not rounded on its own — and six of the adds: ≤ (ndim/64 + 7)·u·Σx² each.
  · ip (1 − Σab): one more rounding, u·|1 − Σab| ≤ u·(1 + Σ|aᵢbᵢ|). In all (ndim + 1)·u·Σ|aᵢbᵢ| + u, which is ≤ γ·Σ|aᵢbᵢ| exactly
    when 15·Σ|aᵢbᵢ| ≥ 1 — Σ|aᵢbᵢ| ≥ 1/15 is asserted, as `Truth` asserts it.                                 bound = γ·Σ|aᵢbᵢ|
  · l2sq (Σa² + Σb² − 2Σab, two roundings of at most u·(Σa² + Σb²) and u·d ≤ u·(Σa² + Σb² + 2Σ|aᵢbᵢ|)):
    (ndim/64 + 9)·u·(Σa² + Σb²) + (2·ndim + 2)·u·Σ|aᵢbᵢ|, below γ on both terms.               bound = γ·(Σa² + Σb² + 2Σ|aᵢbᵢ|)
  · cos (1 − Σab / (√Σa²·√Σb²)): Σ|aᵢbᵢ| ≤ √Σa²·√Σb² (Cauchy-Schwarz), so the sum's error is ≤ ndim·u of the quotient's scale; the
    norms add (ndim/64 + 7)·u (half of it per root, two roots); the two roots, their product, the division and the subtraction a
    rounding each (quotient ≤ 1): (ndim + ndim/64 + 12)·u < 2γ, stated as the 16-bit kinds state it.                  bound = 3γ
  · no fused fold: the wide kernel's fold with the thresholds inside the sums is f16-only. f32 takes the general fold, whose pruning
    test (cos: Σab·rsq(Σb²) against (1 − bound − 1e-5)·√Σa²; ip, l2sq: the closed distance against the bound itself, `≤`) drops
    nothing whose closed distance could enter a list: it costs no accuracy, only — if it were wrong — completeness, which `check`
    holds every query to.
The bound is derived, not measured.

THE DATA. `plant` is the generator of tests/exact_truth.py with "f32" for the kind: `narrow` rounds the f64 constructions to f32, so
every scalar keeps a full 24-bit mantissa — a kernel that narrowed its operands to 16 bits on the way (2⁻¹¹ or 2⁻⁸ per scalar where
the bound allows a few hundred 2⁻²⁴ in all) fails soundness on every case. Decided means what it means there: each of the first k gaps
at least `DECIDED_GAP_IN_BOUNDS` = 8 bounds wide; the cap is `DECIDED_SHARE` = 80 % of the queries, every edge row covered.
"""
from __future__ import annotations

import numpy as np

from tests import exact_truth
from tests.exact_truth import DECIDED_GAP_IN_BOUNDS, DECIDED_SHARE, UNIT, edge_slots, widen  # noqa: F401 (one import for the tests)


class Truth(exact_truth.Truth):
    """`exact_truth.Truth` for f32 rows: the same fields — `exact`, `bound`, `distances`, `allowed`, `allowed_count`, `metric`,
    `dtype`, `ndim` — under the bound derived above, without the assertion that the bound stay below 1e-5·max(1, |d|)."""

    def __init__(self, metric: str, dtype: str, rows: np.ndarray, queries: np.ndarray, allowed=None):
        assert dtype == "f32"
        self.metric, self.dtype = metric, dtype
        r, q = widen(rows, dtype), widen(queries, dtype)
        self.ndim = ndim = r.shape[1]
        self.allowed = np.ones(len(r), dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
        ab, r2, q2 = q @ r.T, (r * r).sum(1), (q * q).sum(1)
        gamma = (ndim + 16) * UNIT
        if metric == "ip":
            d = 1.0 - ab
            absolute = np.abs(q) @ np.abs(r).T
            bound = gamma * absolute
            assert absolute.min() >= 1.0 / 15, "γ's spare units must cover the closing subtraction"
        elif metric == "l2sq":
            d = np.maximum(q2[:, None] + r2[None, :] - 2.0 * ab, 0.0)
            bound = gamma * (q2[:, None] + r2[None, :] + 2.0 * (np.abs(q) @ np.abs(r).T))
        else:
            assert metric == "cos"
            with np.errstate(divide="ignore", invalid="ignore"):
                d = 1.0 - ab / (np.sqrt(q2)[:, None] * np.sqrt(r2)[None, :])
            zero_q, zero_r = (q2 == 0)[:, None], (r2 == 0)[None, :]
            d = np.where(zero_q & zero_r, 0.0, np.where(zero_q | zero_r, 1.0, d))
            bound = np.full_like(d, 3.0 * gamma)
        self.exact = d  # of every row, allowed or not (soundness is checked against the row a key names)
        self.bound = bound
        self.distances = np.where(self.allowed[None, :], d, np.inf)
        self.allowed_count = int(self.allowed.sum())


class Case(exact_truth.Case):
    """`exact_truth.Case` whose truths are the f32 `Truth` above."""

    def truth(self, allowed=None, count=None) -> Truth:
        key = (None if allowed is None else np.asarray(allowed, dtype=bool).tobytes(), count)
        if key not in self._truths:
            self._truths[key] = Truth(self.metric, self.dtype, self.rows, self.queries[:count], allowed)
        return self._truths[key]


def plant(metric: str, ndim: int, rows: int, queries: int, rungs: int, seed: int, **options) -> Case:
    """`exact_truth.plant` for f32 (`edges`, `usable`, `copies`, `near_ties` as there): the existing generator, run with this module's
    `Case` in the place of its own for the duration of the call — it builds its cases, and through them its truths, by that name."""
    theirs = exact_truth.Case
    exact_truth.Case = Case
    try:
        return exact_truth.plant(metric, "f32", ndim, rows, queries, rungs, seed, **options)
    finally:
        exact_truth.Case = theirs
