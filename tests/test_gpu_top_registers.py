"""GPU: `top_gt` — the result buffer as the search kernels hold it — driven directly, one wave per layout: 1, 2, 4, 8 and 16 cells per
lane in registers, each with and without the frontier flags, and the scratch-memory layout in LDS and in device memory
(`global_ak = true`). A script of inserts under the traversal's acceptance rule (and, on the flagged layouts, of closed inserts and of
`first_open` + `close`) is replayed on the device and on the plain-Python model of tests/container_model.py; after EVERY operation the
accepted flag, the size and the radius bits must agree, and at the end every cell, padding included.

The truth: on scripts without NaN (±inf, ±0, subnormals, FLT_MAX and heavy ties among them) and on NaN-only scripts it is the
reference's `sorted_buffer_gt` with `std::lower_bound` (`lower_bound_insert`); where NaN meets numbers the reference's binary search has
no path-independent answer and the device follows its own rule, the same in every layout: NaN first (`nan_first_insert`, DESIGN.md
§4a). The two rules agree wherever the first applies (tests/test_container_model.py).

Limits per layout E: 1, E−1, E, E+1, 32·E, 64·E−1, 64·E (a drop on a lane boundary and off one, the radius in the last cell of a lane
and elsewhere, the full capacity), 608 for E = 16; 1, 63, 64, 65, 200 and 1 100 in scratch memory (the insert's 64-cell tiles). A
script is 3·limit + 64 operations long: the buffer fills, then every further insert is a replacement or a refusal.
"""
import numpy as np
import pytest

from tests import container_model as model

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
CLOSED = 0x80000000
INF_BITS = 0x7F800000
SPECIALS = np.array([np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, 3.4028235e38, -3.4028235e38, 1.0, -1.0], dtype=np.float32)
VALUE_SETS = ("two levels", "eight levels", "distinct", "specials", "nan only", "5% nan", "30% nan")


def limits_of(epl):
    if epl == 0:
        return [1, 63, 64, 65, 200, 1100]
    limits = {1, epl - 1, epl, epl + 1, 32 * epl, 64 * epl - 1, 64 * epl} | ({608} if epl == 16 else set())
    return sorted(limit for limit in limits if 0 < limit <= 64 * epl)


def values_of(name, count, rng):
    if name == "two levels":
        return rng.integers(0, 2, size=count).astype(np.float32) * 0.5 - 1.0
    if name == "eight levels":
        return rng.integers(0, 8, size=count).astype(np.float32) * 0.5 - 1.0
    if name == "distinct":
        return rng.permutation(count).astype(np.float32) * 0.25 - 3.0
    if name == "specials":
        return SPECIALS[rng.integers(0, len(SPECIALS), size=count)]
    if name == "nan only":
        return np.full(count, np.nan, dtype=np.float32)
    values = rng.integers(0, 8, size=count).astype(np.float32) * 0.5 - 1.0
    values[rng.random(count) < (0.05 if name == "5% nan" else 0.30)] = np.nan
    return values


def bits_of(x):
    return int(np.float32(x).view(np.uint32))


def replay(epl, flags, global_memory, limit, name, seed):
    """One script on the device and on the model; asserts every record and every cell."""
    from usearch_amd import index as ua
    rng = np.random.default_rng(seed)
    count = 3 * limit + 64
    keys = values_of(name, count, rng)
    slots = rng.permutation(count).astype(np.uint32)  # distinct, < 2^31, unrelated to the order of arrival
    kinds = np.zeros(count, dtype=np.uint32)
    if flags:
        kinds = rng.choice(np.array([0, 0, 0, 1, 2, 2], dtype=np.uint32), size=count)
        kinds[-(limit + 8):] = 2  # … and drain the frontier at the end: every open member comes out, then none
    mixed = name.endswith("% nan")
    top = model.TopModel(limit, model.nan_first_insert if mixed else model.lower_bound_insert)
    records, cell_bits, cell_slots, size = ua.test_top(epl, flags, global_memory, kinds, keys, slots, limit)
    key_bits = keys.view(np.uint32)
    bits_by_slot = {int(s): int(b) for s, b in zip(slots, key_bits)}
    inserted = set()
    where = f"epl {epl} flags {flags} global {global_memory} limit {limit} values {name!r}"
    for i in range(count):
        got = [int(x) for x in records[i]]
        if kinds[i] <= 1:
            accepted = top.insert(float(keys[i]), int(slots[i]), closed=bool(flags and kinds[i] == 1))
            inserted.add(int(slots[i]))
            want = [int(accepted), len(top.buf), bits_of(top.radius), 0, NONE, NONE]
        else:
            popped = top.pop_open()
            want = [0, len(top.buf), bits_of(top.radius), 0, NONE, NONE]
            if popped is not None:
                cell, _, slot = popped
                want = [1, len(top.buf), bits_of(top.radius), bits_by_slot[slot], slot, cell]
        assert got == want, f"{where}: operation {i} (kind {kinds[i]}, {keys[i]!r}, slot {slots[i]}): device {got}, model {want}"
    # ---- the cells at the end, bit for bit (−0.0 and +0.0 tie, and each keeps its own bits with its slot)
    assert size == len(top.buf) == min(top.accepted, limit), where
    want_bits = [bits_by_slot[e[1]] for e in top.buf]
    want_words = [e[1] | (CLOSED if flags and e[2] else 0) for e in top.buf]
    held = cell_slots[:size].tolist()
    assert cell_bits[:size].tolist() == want_bits and held == want_words, where
    # ---- invariants, whatever the rule: no slot twice, only inserted slots, padding beyond the size
    plain = [word & ~CLOSED for word in held] if flags else held
    assert len(set(plain)) == len(plain) and set(plain) <= inserted, where
    if epl:
        assert len(cell_bits) == 64 * epl
        assert (cell_bits[size:] == INF_BITS).all() and (cell_slots[size:] == NONE).all(), where
    if flags:
        assert all(e[2] for e in top.buf), "the script's tail drains the frontier"
    return top


@pytest.mark.parametrize("name", VALUE_SETS)
@pytest.mark.parametrize("flags", [False, True])
@pytest.mark.parametrize("epl", [1, 2, 4, 8, 16])
def test_register_top_follows_the_model(epl, flags, name):
    for limit in limits_of(epl):
        replay(epl, flags, False, limit, name, seed=1000 * epl + limit)


@pytest.mark.parametrize("name", VALUE_SETS)
@pytest.mark.parametrize("global_memory", [False, True])
def test_scratch_top_follows_the_model(global_memory, name):
    for limit in limits_of(0):
        replay(0, False, global_memory, limit, name, seed=7000 + limit)


def test_limits_cover_the_lane_boundaries():
    assert limits_of(1) == [1, 2, 32, 63, 64]
    assert limits_of(4) == [1, 3, 4, 5, 128, 255, 256]
    assert limits_of(16) == [1, 15, 16, 17, 512, 608, 1023, 1024]
    top = replay(16, True, False, 608, "30% nan", seed=5)
    assert any(np.isnan(e[0]) for e in top.buf) and not all(np.isnan(e[0]) for e in top.buf)  # the mixed case really is mixed
